"""Properties of the operand declaration (models.Op rows; DESIGN.md, "The operand declaration") that the pack, the gradient struct, the gradient slots and the
transposed operands are derived from -- on CPU models, over the configurations of tools/operand_trace.py.  Nothing here restates the table."""
import collections
import ctypes as C

import pytest

from tokenreduction_amd import _lib
from tokenreduction_amd.training import TrainState
from tools.operand_trace import STAGE, RecordingPacker, configs, make

CONFIGS = {c[0]: c[1:] for c in configs()}
_built = {}


@pytest.fixture(params=list(CONFIGS))
def model(request):
    if request.param not in _built:
        _built[request.param] = make(*CONFIGS[request.param])
    m = _built[request.param]
    for p in m.parameters():
        p.requires_grad = True
    return m


def _struct_type(struct):
    return {"trunk": _lib.TrVitWeights, "blocks": _lib.TrBlockWeights, "stage": _lib.TrStageWeights}[struct if isinstance(struct, str) else struct[0]]


def test_every_parameter_takes_its_gradient_through_exactly_one_row(model):
    named = dict(model.named_parameters())
    seen = collections.Counter()
    for struct, name, row in model._operand_rows():
        if name is None or not row.grad:
            assert row.grad_rows == 0, (struct, row)          # nothing reserves a gradient slot without a parameter behind it
            continue
        seen[name] += 1
        gamma = row.gamma and f"blocks.{struct[1]}.{row.gamma}"
        if gamma in named:                                    # (a plain block has no gamma: the row's mention is idle)
            seen[gamma] += 1
    assert seen == collections.Counter(list(named)), (set(named) ^ set(seen), [n for n, k in seen.items() if k != 1])


def test_no_field_is_claimed_twice_within_a_struct(model):
    operands, grads = collections.Counter(), collections.Counter()
    for struct, name, row in model._operand_rows():
        assert (row.field, C.c_void_p) in _struct_type(struct)._fields_, (struct, row.field)
        if row.kind != "grad":
            operands[struct, row.field] += 1
        if row.grad:
            grads[struct, row.field] += 1
    assert max(operands.values()) == 1 and max(grads.values()) == 1


def test_a_gradient_lands_in_the_field_its_operand_is_packed_into(model):
    """Stage by stage: wherever G has a pointer, W has the operand -- but for SiT's `scale`, whose operand is the scalar member and whose gradient
    takes b2 -- and the pointer is the slot of the parameter the row names."""
    W = _lib.TrVitWeights()
    model._pack_stages(W, RecordingPacker())
    st = TrainState(model)
    G, discarded = st.grads_struct(model, want_dx=True)
    assert discarded == []
    flat0 = st.flat.data_ptr()
    grad_only = []
    for struct, name, row in model._operand_rows(blocks=False):
        if struct == "trunk" or not row.grad:
            continue
        loc = struct[1]
        assert getattr(G.stage[loc], row.field) == flat0 + 4 * st.offsets[name], (loc, row.field)
        if row.kind == "grad":
            grad_only.append((type(model).__name__, name.split(".")[-1], row.field))
            assert not getattr(W.stage[loc], row.field) and W.stage[loc].scale == pytest.approx(float(dict(model.named_parameters())[name]))
        else:
            assert getattr(W.stage[loc], row.field), (loc, row.field)
    assert set(grad_only) <= {("SelfSlimmedVisionTransformer", "scale", "b2")}
    assert bool(grad_only) == (type(model).__name__ == "SelfSlimmedVisionTransformer")
    for loc in range(model.depth):      # and nothing else in G's stages
        want = {r.field for s, n, r in model._operand_rows(blocks=False) if s == ("stage", loc) and r.grad}
        assert {f for f in STAGE if getattr(G.stage[loc], f)} == want


def test_gradient_slots_hold_the_declared_padding(model):
    padded = {name: row.grad_rows for _, name, row in model._operand_rows() if row.grad_rows}
    for n, p in model.named_parameters():
        slot = model._grad_slot_numel(n, p)
        assert slot >= p.numel(), n
        if n in padded:
            assert slot == padded[n] * (p.shape[-1] if p.dim() > 1 else 1) and padded[n] >= (p.shape[-2] if p.dim() > 1 else p.shape[0]), n
        else:
            assert slot == p.numel(), n


def test_a_family_without_transposed_stage_rows_may_have_all_operands_fused(model):
    """_pack_all_fused is open to a model exactly when no stage makes a dgrad operand of its own -- and a stage makes one for every matrix
    in the operand type that takes a gradient, for nothing else."""
    model._pack_stages(_lib.TrVitWeights(), RecordingPacker())          # (the stand-in wants transposed copies)
    assert model._stages_transposed() == bool(model._stage_t)
    for struct, name, row in model._operand_rows(blocks=False):
        if struct != "trunk":
            assert (row.t_rows is not None) == (row.kind == "w" and row.grad), (struct, row.field)
            assert ((struct[1], row.field) in model._stage_t) == (row.t_rows is not None)


def test_a_frozen_stage_below_the_floor_is_null(model):
    st = TrainState(model)
    if not st._stage_names:             # no reduction stage with parameters: nothing ever points into a stage
        G, _ = st.grads_struct(model, want_dx=True)
        assert not any(getattr(G.stage[loc], f) for loc in range(model.depth) for f in STAGE)
        return
    low = min(st._stage_names)
    above = tuple(f"blocks.{i}." for i in range(low + 1, model.depth)) + ("head.", "norm.") + tuple(n for loc, names in st._stage_names.items()
                                                                                                    if loc > low for n in names)
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith(above)
    G, _ = st.grads_struct(model)
    assert not any(getattr(G.stage[low], f) for f in STAGE)
    for loc in st._stage_names:
        if loc > low:
            assert any(getattr(G.stage[loc], f) for f in STAGE), loc
