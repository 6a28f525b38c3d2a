"""Multi-level dense feature maps in training at model level (model.forward_dense_train(x, blocks=...)), GPU tier, on the micro fixtures of
every family but DyViT.

Forward (blocks = every block, norm True and False): `out` is model(x)'s in train mode bit for bit; every level's index is the numpy
composition (tests/_dense_levels_ref.dense_index_levels) of the decisions read back from the TAPE (the soft families': the soft output the
forward wrote); every map is the restated gather of the slab the same forward wrote and `cls` its row 0; against
tests/_dense_train_levels_ref.streams_after_blocks with the device's decisions and bf16 rounding points the patch rows that have a row hold
the single-level test's bound (rel L2 < 3e-2; FORCED_TOL on `out`), the others are exactly `fill`.
Gradients (three spread levels -- one in front of the first stage, the stage's own block, the last block -- norm True and False): torch
autograd over streams_after_blocks, for cross_entropy(out) + sum_l (features[l] * G_l).sum() and for the map terms alone, under
tests/test_hip_train.py's bounds: grad_tol(case) on the whole vector, twice that on the worst parameter (floor 1e-3 of the whole norm),
twice that on x.grad.  G_l is seeded N(0, 1) / (B * P0), for tests/test_dense_train_gpu.py's reason."""
from collections import Counter

import numpy as np
import pytest
import torch

from tests import _decisions_ref as dref
from tests import _dense_levels_ref as lvl
from tests import _dense_ref as ref
from tests import _dense_train_levels_ref as lref
from tests import _launches
from tests._params import GOLDEN_CASES, grad_labels
from tests.test_avg_pool_gpu import _BlockRanges
from tests.test_dense_train_gpu import (CASES, DX_CASES, FILL, _bits, _check_grads, _grads, _head_loss, _image, _plain_step_labels, _tape_slabs,
                                        _train_model)
from tests.test_hip_model import FORCED_TOL
from tests.test_hip_train import _noise, _rel, grad_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def steps():
    return {}


def _spread(model):
    """Three levels: in front of the first stage, the stage's own block, the last block (a model without stages: blocks 0, 1, depth-1)."""
    stages = model._decision_stages()
    first = stages[0][0] if stages else 1
    blocks = (first - 1, first, model.depth - 1)
    assert 0 <= blocks[0] < blocks[1] < blocks[2], blocks
    return blocks


def _weights(case, model, L):
    B, D, P0 = case["batch"], model.embed_dim, model.patch_embed.num_patches
    return [torch.randn(B, D, P0, generator=torch.Generator().manual_seed(case["xseed"] + 23 + l)) / (B * P0) for l in range(L)]


def _map_loss(dense, Gs, only=None):
    terms = [(f.reshape(G.shape).float() * G.cuda()).sum() for l, (f, G) in enumerate(zip(dense["features"], Gs)) if only is None or l in only]
    return sum(terms[1:], terms[0])


def _step(case, model, x, blocks, norm, Gs, head=True, only=None, **kw):
    model.zero_grad(set_to_none=True)
    x.grad = None
    out, dense = model.forward_dense_train(x, blocks=blocks, norm=norm, fill=FILL, **kw)
    loss = _map_loss(dense, Gs, only)
    if head:
        loss = loss + _head_loss(case, out, None)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), dense, _grads(model), None if x.grad is None else x.grad.detach().clone()


def _slabs(model, B):
    """The rows of every level as the forward left them: ([tokens_l [B, N_l, D]], [stream_l] or None) on the host."""
    dn, D = model._train_state().levels, model.embed_dim
    rows = list(dn["rows"])
    cut = lambda buf: [buf[l * dn["stride"]: l * dn["stride"] + B * n * D].view(B, n, D).cpu().numpy() for l, n in enumerate(rows)]
    return rows, cut(dn["tokens"]), None if dn["stream"] is None else cut(dn["stream"])


def _forced(model):
    from tokenreduction_amd import training
    return {blk: (tuple(t.cpu() for t in d) if isinstance(d, tuple) else d.cpu()) for blk, d in training.train_decisions(model).items()} or None


def _forward_all(cache, name, norm, golden_dir):
    key = ("fwd", name, norm)
    if key not in cache:
        case = GOLDEN_CASES[name]
        noise = _noise(case, golden_dir) if case["family"] == "dpcknn" else None
        model, params, cfg = _train_model(case, noise)
        x = _image(case)
        plain = model(x).detach().clone()
        out, dense = model.forward_dense_train(x, blocks=range(model.depth), norm=norm, fill=FILL)
        torch.cuda.synchronize()
        rows, tokens, stream = _slabs(model, case["batch"])
        soft = model._train_state().levels["plan"]["soft"]
        kept, compl = _tape_slabs(model)
        with torch.no_grad():
            hs = lref.streams_after_blocks(params, x.cpu(), cfg, "bf16", _forced(model), noise)
            o_out = lref.logits_of(params, hs[-1], cfg, "bf16")
            o_rows = [lref.level_rows(h, params, cfg, norm) for h in hs]
        cache[key] = dict(case=case, model=model, plain=plain, out=out.detach(), dense=dense, rows=rows, tokens=tokens, stream=stream, kept=kept,
                          compl=compl, soft=None if soft is None else soft.cpu().numpy(), o_out=o_out, o_rows=o_rows)
    return cache[key]


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_forward_every_block_is_the_plain_forward_plus_the_restated_maps(steps, golden_dir, name, norm):
    s = _forward_all(steps, name, norm, golden_dir)
    case, model, dense = s["case"], s["model"], s["dense"]
    B, D, depth = case["batch"], model.embed_dim, model.depth
    h, w = model.patch_embed.grid_size
    P0 = h * w
    assert torch.equal(_bits(s["out"]), _bits(s["plain"]))
    assert dense["blocks"] == tuple(range(depth)) and dense["grid"] == (h, w) and len(dense["features"]) == len(dense["index"]) == depth
    assert s["rows"] == model._last_tokens
    stages = model._decision_stages()
    dec = dref.stage_decisions(s["kept"], s["compl"], s["soft"], stages, B, P0 + 1)
    index = lvl.dense_index_levels(dec, stages, B, P0, list(range(depth)), s["rows"])
    assert dense["cls"].shape == (B, depth, D) and dense["cls"].dtype == torch.float32 and not dense["cls"].requires_grad
    worst = 0.0
    for l in range(depth):
        f, i = dense["features"][l], dense["index"][l]
        assert f.shape == (B, D, h, w) and f.dtype == torch.float32 and f.requires_grad and f.grad_fn is dense["features"][0].grad_fn
        assert i.shape == (B, P0) and i.dtype == torch.int32 and not i.requires_grad
        np.testing.assert_array_equal(i.cpu().numpy(), index[l], err_msg=str(l))
        want = ref.dense_gather(s["tokens"][l], index[l], "NCHW", "fp32", FILL)
        np.testing.assert_array_equal(f.detach().cpu().numpy().reshape(B, D, P0).view(np.uint32), want.view(np.uint32), err_msg=str(l))
        np.testing.assert_array_equal(dense["cls"][:, l].cpu().numpy().view(np.uint32), s["tokens"][l][:, 0].view(np.uint32))
        if norm:      # the norm slab is the fp32 final norm of the stream slab (the arithmetic of the restated LayerNorm, to rounding)
            st = torch.from_numpy(s["stream"][l])
            ln = torch.nn.functional.layer_norm(st, (D,), model.norm.weight.detach().cpu(), model.norm.bias.detach().cpu(), model.norm.eps)
            assert _rel(torch.from_numpy(s["tokens"][l]), ln) < 1e-5, l
        got = f.detach().cpu().reshape(B, D, P0).permute(0, 2, 1)
        has = torch.from_numpy(index[l] >= 0)
        o = lref.level_map(s["o_rows"][l], index[l], FILL)
        r = _rel(got[has], o[has])
        worst = max(worst, r)
        assert r < 3e-2, (l, r)
        assert (got[~has] == FILL).all(), l
    assert out_close(s)
    family = case["family"]
    if family in ("deit",):
        assert all((index[l] == np.arange(1, P0 + 1)).all() for l in range(depth))
    else:
        assert (index[0] == np.arange(1, P0 + 1)).all() and not (index[-1] == np.arange(1, P0 + 1)).all()      # a level in front of every stage
    print(f"\n[{name} norm={norm}] out rel L2 {_rel(s['out'].cpu(), s['o_out']):.3e}; worst level's patch rows rel L2 {worst:.3e}")


def out_close(s):
    return _rel(s["out"].cpu(), s["o_out"]) < FORCED_TOL


@pytest.mark.parametrize("name", CASES)
def test_the_last_block_alone_is_the_single_level_call_bit_for_bit(golden_dir, name):
    case = GOLDEN_CASES[name]
    noise = _noise(case, golden_dir) if case["family"] == "dpcknn" else None
    model, _, _ = _train_model(case, noise)
    x = _image(case)
    G = _weights(case, model, 1)
    for head in (False, True):
        model.zero_grad(set_to_none=True)
        out1, d1 = model.forward_dense_train(x, fill=FILL)
        loss = (d1["features"].reshape(G[0].shape) * G[0].cuda()).sum()
        (loss + _head_loss(case, out1, None) if head else loss).backward()
        want = _grads(model)
        out2, d2, got, _ = _step(case, model, x, (model.depth - 1,), True, G, head=head)
        assert torch.equal(_bits(out1.detach()), _bits(out2))
        assert torch.equal(_bits(d1["features"].detach()), _bits(d2["features"][0].detach())) and torch.equal(d1["index"], d2["index"][0])
        for n in want:
            assert torch.equal(_bits(want[n]), _bits(got[n])), (head, n)


def _full(cache, name, norm, golden_dir):
    key = ("grad", name, norm)
    if key in cache:
        return cache[key]
    case = GOLDEN_CASES[name]
    noise = _noise(case, golden_dir) if case["family"] == "dpcknn" else None
    model, params, cfg = _train_model(case, noise)
    x = _image(case)
    if name in DX_CASES:
        x.requires_grad_(True)
    blocks = _spread(model)
    Gs = _weights(case, model, 3)
    out, dense, grads, dx = _step(case, model, x, blocks, norm, Gs)
    forced = _forced(model)
    index = [i.cpu() for i in dense["index"]]
    _, _, grads_map, dx_map = _step(case, model, x, blocks, norm, Gs, head=False)
    # torch autograd over the block composition, the device's decisions, bf16 rounding points
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    img = x.detach().cpu().to(torch.float32).clone().requires_grad_(True)
    with torch.enable_grad():
        hs = lref.streams_after_blocks(leaves, img, cfg, "bf16", forced, noise)
        o_out = lref.logits_of(leaves, hs[-1], cfg, "bf16")
        map_term = 0
        for l, b in enumerate(blocks):
            m = lref.level_map(lref.level_rows(hs[b], leaves, cfg, norm), index[l], FILL)
            map_term = map_term + (m.permute(0, 2, 1) * Gs[l]).sum()
        names, oracle = list(leaves), {"out": o_out.detach()}
        for what, loss in (("mixed", map_term + _head_loss(case, o_out, None)), ("map", map_term)):
            gs = torch.autograd.grad(loss, [leaves[n] for n in names] + [img], retain_graph=True, allow_unused=True)
            oracle[what] = ({n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, gs[:-1])}, gs[-1])
    cache[key] = dict(case=case, model=model, x=x, blocks=blocks, Gs=Gs, out=out, dense=dense, grads=grads, dx=dx, grads_map=grads_map, dx_map=dx_map,
                      oracle=oracle)
    return cache[key]


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_gradients_of_three_levels_match_autograd_over_the_block_composition(steps, golden_dir, name, norm):
    s = _full(steps, name, norm, golden_dir)
    o = s["oracle"]
    assert _rel(s["out"].cpu(), o["out"]) < FORCED_TOL
    _check_grads(f"{name} norm={norm} mixed", s["case"], s["grads"], s["dx"], *o["mixed"])
    _check_grads(f"{name} norm={norm} map", s["case"], s["grads_map"], s["dx_map"], *o["map"])
    assert (s["dx"] is not None) == (name in DX_CASES)
    assert float(s["grads_map"]["head.weight"].abs().max()) == 0 and float(s["grads"]["head.weight"].abs().max()) > 0
    if not norm:                                                 # the maps as they stand and no head term: the final norm takes no gradient
        assert float(s["grads_map"]["norm.weight"].abs().max()) == 0


@pytest.mark.parametrize("norm", [True, False])
def test_a_level_without_a_gradient_costs_nothing_and_out_alone_is_the_plain_step(steps, golden_dir, norm):
    s = _full(steps, "topk_micro", norm, golden_dir)
    case, blocks, Gs = s["case"], s["blocks"], s["Gs"]
    model, _, _ = _train_model(case)
    x = _image(case)
    plain_f, plain_b, plain_grads = _plain_step_labels(case, model, x)
    # levels 0 and 2 in the loss: autograd hands level 1's gradient over as None
    model.zero_grad(set_to_none=True)
    out, dense = model.forward_dense_train(x, blocks=blocks, norm=norm, fill=FILL)
    loss = _map_loss(dense, Gs, only=(0, 2)) + _head_loss(case, out, None)
    labels = _launches.labels(loss.backward)
    torch.cuda.synchronize()
    got = _grads(model)
    zero = [Gs[0], torch.zeros_like(Gs[1]), Gs[2]]
    _, _, want, _ = _step(case, model, x, blocks, norm, zero)
    total = _rel(torch.cat([got[n].reshape(-1) for n in got]), torch.cat([want[n].reshape(-1) for n in got]))
    print(f"\n[None level, norm={norm}] against a zero gradient for the level: whole-vector rel L2 {total:.3e}")
    assert total < grad_tol(case), total
    extra = Counter(labels) - Counter(plain_b)
    assert not Counter(plain_b) - Counter(labels)
    if norm:      # two injections: the last block's pass over every row and one level in front of its block -- not three
        assert extra == Counter({"tr_dense_scatter_levels": 1, "ln_bwd_kernel": 2, "tr_layernorm_bwd (reduce)": 2}), extra
    else:
        assert extra == Counter({"tr_dense_scatter_levels": 1, "tr_stream_grad_add": 2}), extra
    # a loss on `out` alone: model(x)'s step
    model.zero_grad(set_to_none=True)
    out, dense = model.forward_dense_train(x, blocks=blocks, norm=norm)
    labels = _launches.labels(_head_loss(case, out, None).backward)
    assert labels == plain_b and "tr_dense_scatter_levels" not in labels
    for n, g in _grads(model).items():
        assert torch.equal(_bits(g), _bits(plain_grads[n])), n


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", ["topk_micro", "tome_micro", "sit_micro"])
def test_launch_accounting_and_the_other_steps_keep_their_launches_and_bits(steps, golden_dir, name, norm):
    s = _full(steps, name, norm, golden_dir)
    case, blocks, Gs = s["case"], s["blocks"], s["Gs"]
    model, _, _ = _train_model(case)
    x = _image(case)
    G1 = Gs[0].cuda()

    def single_step():
        model.zero_grad(set_to_none=True)
        kept = []

        def fwd():
            out, dense = model.forward_dense_train(x)
            kept.append((dense["features"].reshape(G1.shape) * G1).sum() + _head_loss(case, out, None))
        fl = _launches.labels(fwd)
        return fl, _launches.labels(kept[0].backward), _grads(model)
    before, before1 = _plain_step_labels(case, model, x), single_step()
    kept = []

    def fwd():
        out, dense = model.forward_dense_train(x, blocks=blocks, norm=norm)
        kept.append(_map_loss(dense, Gs) + _head_loss(case, out, None))
    model.zero_grad(set_to_none=True)
    fl = _launches.labels(fwd)
    bl = _launches.labels(kept[0].backward)
    after, after1 = _plain_step_labels(case, model, x), single_step()
    for a, b in ((before, after), (before1, after1)):
        assert a[0] == b[0] and a[1] == b[1]
        for n in a[2]:
            assert torch.equal(_bits(a[2][n]), _bits(b[2][n])), n
    extra_f, extra_b = Counter(fl) - Counter(before[0]), Counter(bl) - Counter(before[1])
    assert not Counter(before[0]) - Counter(fl) and not Counter(before[1]) - Counter(bl)
    L = len(blocks)
    tail = ["tr_dense_index_levels", "tr_dense_gather_levels"]
    assert fl[-2:] == tail and bl[0] == "tr_dense_scatter_levels"
    want_f = Counter({"tr_level_tap_norm" if norm else "tr_cls_tap": L, "tr_dense_index_levels": 1, "tr_dense_gather_levels": 1})
    if model._decision_stages():
        want_f["tr_stage_decisions"] = 1
    assert extra_f == want_f, extra_f
    want_b = Counter({"tr_dense_scatter_levels": 1, "ln_bwd_kernel": L, "tr_layernorm_bwd (reduce)": L}) if norm else \
        Counter({"tr_dense_scatter_levels": 1, "tr_stream_grad_add": L})
    assert extra_b == want_b, extra_b


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", ["topk_micro", "tome_micro"])
def test_block_range_backward_is_the_single_call_bit_for_bit(steps, golden_dir, name, norm):
    s = _full(steps, name, norm, golden_dir)
    case = s["case"]
    model, _, _ = _train_model(case)
    model._grad_reducer = red = _BlockRanges()
    try:
        out, _, grads, dx = _step(case, model, _image(case).requires_grad_(True), s["blocks"], norm, s["Gs"])
    finally:
        model._grad_reducer = None
    assert len(red.launched) == case["depth"]
    assert torch.equal(_bits(out), _bits(s["out"])) and torch.equal(_bits(dx), _bits(s["dx"]))
    for n, g in grads.items():
        assert torch.equal(_bits(g), _bits(s["grads"][n])), n


def test_frozen_trunk_the_levels_still_reach_the_final_norm(steps, golden_dir):
    s = _full(steps, "topk_micro", True, golden_dir)
    case, blocks, Gs = s["case"], s["blocks"], s["Gs"]
    model, _, _ = _train_model(case)
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("norm.")
    x = _image(case)
    _, dense = model.forward_dense_train(x, blocks=blocks, fill=FILL)
    labels = _launches.labels(_map_loss(dense, Gs).backward)
    torch.cuda.synchronize()
    # the scatter, then the final norm's backward four times: the CLS rows' (zero here) and one pass per level, the last block's first
    assert labels.count("tr_dense_scatter_levels") == 1 and labels.count("ln_bwd_kernel") == 4, labels
    assert not [l for l in labels if "gemm" in l or "attention" in l or "linear_bwd" in l], labels      # no block kernel
    for n, p in model.named_parameters():
        if n.startswith("norm."):
            assert _rel(p.grad, s["grads_map"][n]) < 1e-5, n      # the trunk's gradient does not feed the norm's parameters
        else:
            assert p.grad is None, n


def test_frozen_below_a_block_a_level_below_it_changes_the_final_norm_only(steps, golden_dir):
    s = _full(steps, "topk_micro", True, golden_dir)
    case, blocks, Gs = s["case"], s["blocks"], s["Gs"]
    k = 2
    assert blocks[0] < k and blocks[1] < k <= blocks[2]
    model, _, _ = _train_model(case)
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith(("norm.", "head.")) or (n.startswith("blocks.") and int(n.split(".")[1]) >= k)
    x = _image(case)
    _, _, top, _ = _step(case, model, x, blocks, True, Gs, only=(2,))
    _, _, both, _ = _step(case, model, x, blocks, True, Gs, only=(0, 2))
    for n, p in model.named_parameters():
        if not p.requires_grad:
            assert both[n] is None, n
        elif n.startswith("norm."):
            assert not torch.equal(_bits(top[n]), _bits(both[n])), n
        else:
            assert torch.equal(_bits(top[n]), _bits(both[n])), n
    # a pass of range calls adds in the single call's order (the call that holds the stop block runs the levels below it): the same bits
    model._grad_reducer = _BlockRanges()
    try:
        _, _, ranged, _ = _step(case, model, x, blocks, True, Gs, only=(0, 2))
    finally:
        model._grad_reducer = None
    for n, g in both.items():
        assert (g is None and ranged[n] is None) or torch.equal(_bits(g), _bits(ranged[n])), n


def test_two_micro_steps_accumulate(steps, golden_dir):
    s = _full(steps, "tome_micro", True, golden_dir)
    case, blocks, Gs = s["case"], s["blocks"], s["Gs"]
    model, _, _ = _train_model(case)
    x = _image(case)

    def micro(shift, head):
        out, dense = model.forward_dense_train(x + shift, blocks=blocks, fill=FILL)
        loss = _map_loss(dense, Gs)
        (loss + _head_loss(case, out, None) if head else loss).backward()
    singles = []
    for shift, head in ((0.0, True), (0.25, False)):
        model.zero_grad(set_to_none=True)
        micro(shift, head)
        singles.append(_grads(model))
    model.zero_grad(set_to_none=True)
    micro(0.0, True)
    micro(0.25, False)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        want = singles[0][n] + singles[1][n]
        assert torch.allclose(p.grad, want, rtol=1e-5, atol=1e-7 + 2.0 ** -22 * float(want.abs().max())), n


def test_other_layout_and_other_dtype(steps, golden_dir):
    s = _full(steps, "tome_micro", True, golden_dir)
    case, blocks, Gs = s["case"], s["blocks"], s["Gs"]
    model, _, _ = _train_model(case)
    x = _image(case)
    f32 = [f.detach() for f in s["dense"]["features"]]
    want = None
    for fmt, dtype in (("NCHW", torch.float32), ("NHWC", torch.float32), ("NCHW", torch.bfloat16), ("NHWC", torch.bfloat16)):
        model.zero_grad(set_to_none=True)
        out, dense = model.forward_dense_train(x, blocks=blocks, output_fmt=fmt, dtype=dtype, fill=FILL)
        assert torch.equal(_bits(out), _bits(s["out"]))
        loss = 0
        for l, feat in enumerate(dense["features"]):
            assert feat.dtype == dtype and torch.equal(dense["index"][l], s["dense"]["index"][l])
            nchw = feat.detach() if fmt == "NCHW" else feat.detach().permute(0, 3, 1, 2)
            assert torch.equal(_bits(nchw), _bits(f32[l].to(dtype))), (fmt, dtype, l)
            Gf = Gs[l].cuda().reshape(f32[l].shape)
            loss = loss + (feat.float() * (Gf if fmt == "NCHW" else Gf.permute(0, 2, 3, 1))).sum()      # (bf16 map: the node gets a bf16 gradient)
        loss.backward()
        grads = _grads(model)
        if want is None:
            want = grads
            for n in grads:
                assert torch.equal(_bits(grads[n]), _bits(s["grads_map"][n])), n
        elif dtype == torch.float32:
            for n in grads:                                      # the same sums in the other layout: the same bits
                assert torch.equal(_bits(grads[n]), _bits(want[n])), (fmt, n)
        else:
            total = _rel(torch.cat([g.reshape(-1) for g in grads.values()]), torch.cat([want[n].reshape(-1) for n in grads]))
            assert total < 2.0 ** -7, (fmt, total)               # G rounded to bf16 on its way in: 2^-9 per element


def _maps_match_their_slabs(model, dense, B):
    rows, tokens, _ = _slabs(model, B)
    D, P0 = model.embed_dim, model.patch_embed.num_patches
    for l, f in enumerate(dense["features"]):
        want = ref.dense_gather(tokens[l], dense["index"][l].cpu().numpy(), "NCHW", "fp32", FILL)
        np.testing.assert_array_equal(f.detach().cpu().numpy().reshape(B, D, P0).view(np.uint32), want.view(np.uint32), err_msg=str(l))


@pytest.mark.parametrize("kind", ["uint8", "uint8_channels_last", "augmented"])
def test_uint8_and_augmented_input_go_through_the_same_entry(kind):
    from tokenreduction_amd import augment
    case = GOLDEN_CASES["tome_micro"]
    model, _, _ = _train_model(case)
    model.set_pixel_input()
    B, blocks = 4, _spread(model)
    u8 = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(9)).cuda()
    if kind == "uint8_channels_last":
        u8 = u8.contiguous(memory_format=torch.channels_last)
    x = u8
    if kind == "augmented":
        np.random.seed(3)
        torch.manual_seed(3)
        x, _ = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=case["num_classes"])(u8, torch.arange(B).cuda() % case["num_classes"])
    plain = model(x).detach().clone()
    out, dense = model.forward_dense_train(x, blocks=blocks, fill=FILL)
    assert torch.equal(_bits(out), _bits(plain))
    _maps_match_their_slabs(model, dense, B)
    model.zero_grad(set_to_none=True)
    sum((f * torch.randn(f.shape, generator=torch.Generator().manual_seed(2 + l)).cuda() / (B * 196)).sum()
        for l, f in enumerate(dense["features"])).backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        assert n.startswith("head.") or float(p.grad.abs().max()) > 0, n


def test_droppath_and_dropout_draw_as_for_the_plain_forward_and_the_map_path_stays_linear():
    case = dict(GOLDEN_CASES["topk_micro"], drop_path=0.1, drop_rate=0.1)
    model, _, _ = _train_model(case)
    x = _image(case)
    blocks, Gs = _spread(model), _weights(case, model, 3)

    def step(head, map_):
        torch.manual_seed(11)                                    # the same DropPath draws and dropout masks for every forward
        model.zero_grad(set_to_none=True)
        out, dense = model.forward_dense_train(x, blocks=blocks, fill=FILL)
        loss = 0
        if head:
            loss = loss + _head_loss(case, out, None)
        if map_:
            loss = loss + _map_loss(dense, Gs)
        loss.backward()
        return out.detach().clone(), dense, _grads(model)
    torch.manual_seed(11)
    model.zero_grad(set_to_none=True)
    plain = model(x)
    _head_loss(case, plain, None).backward()
    plain_grads = _grads(model)
    out, dense, head_only = step(True, False)
    assert torch.equal(_bits(out), _bits(plain.detach()))
    _maps_match_their_slabs(model, dense, case["batch"])
    for n in plain_grads:                                        # no gradient for the maps: model(x)'s step, bit for bit
        assert torch.equal(_bits(head_only[n]), _bits(plain_grads[n])), n
    _, _, map_only = step(False, True)
    _, _, both = step(True, True)
    total = _rel(torch.cat([both[n].reshape(-1) for n in both]), torch.cat([(head_only[n] + map_only[n]).reshape(-1) for n in both]))
    print(f"\n[droppath + dropout, three levels] mixed against head-only + map-only: whole-vector rel L2 {total:.3e}")
    assert total < grad_tol(case), total
    assert float(torch.cat([map_only[n].reshape(-1) for n in map_only if not n.startswith("head.")]).norm()) > 0


def test_refusals():
    case = GOLDEN_CASES["topk_micro"]
    model, _, _ = _train_model(case)
    x = _image(case)

    def refused(exc, match, fn):
        def call():
            with pytest.raises(exc, match=match):
                fn()
        assert _launches.labels(call) == []
    model.eval()
    refused(RuntimeError, r"model\.train\(\).*forward_dense", lambda: model.forward_dense_train(x, blocks=(1, 3)))
    model.train()
    with pytest.raises(RuntimeError, match="eval feature"):      # forward_dense and get_intermediate_layers stay eval entries
        model.forward_dense(x, blocks=(1, 3))
    with pytest.raises(RuntimeError, match="eval feature"):
        model.get_intermediate_layers(x, n=2)
    model.viz_mode = True
    refused(RuntimeError, "viz_mode", lambda: model.forward_dense_train(x, blocks=(1,)))
    model.viz_mode = False
    refused(RuntimeError, "no CPU path", lambda: model.forward_dense_train(x.cpu(), blocks=(1,)))
    refused(ValueError, "outside", lambda: model.forward_dense_train(x, blocks=(model.depth,)))
    refused(ValueError, "outside", lambda: model.forward_dense_train(x, blocks=(-model.depth - 1,)))
    refused(ValueError, "twice", lambda: model.forward_dense_train(x, blocks=(1, 1 - model.depth)))
    refused(ValueError, "empty", lambda: model.forward_dense_train(x, blocks=()))
    refused(ValueError, "output_fmt", lambda: model.forward_dense_train(x, blocks=(1,), output_fmt="CHW"))
    refused(ValueError, "dtype", lambda: model.forward_dense_train(x, blocks=(1,), dtype=torch.float16))
    model.precision = "fp32"
    refused(NotImplementedError, "bf16", lambda: model.forward_dense_train(x, blocks=(1,)))
    model.precision = "bf16"
    ats, _, _ = _train_model(GOLDEN_CASES["ats_micro"])
    ats.dynamic_width = True
    refused(RuntimeError, "dynamic_width", lambda: ats.forward_dense_train(x, blocks=(1,)))
    dyvit, _, _ = _train_model(GOLDEN_CASES["dyvit_micro_train"])
    refused(NotImplementedError, "DyViT", lambda: dyvit.forward_dense_train(x, blocks=(1,)))
    # results come in ascending block order whatever the order asked for
    _, dense = model.forward_dense_train(x, blocks=(-1, 2))
    assert dense["blocks"] == (2, model.depth - 1) and len(dense["features"]) == 2
    # one tape per model: a second forward makes the first one's backward stale
    Gs = _weights(case, model, 2)
    first = _map_loss(model.forward_dense_train(x, blocks=(0, 2))[1], Gs)
    second = _map_loss(model.forward_dense_train(x + 0.5, blocks=(0, 2))[1], Gs)
    with pytest.raises(RuntimeError, match="overwritten"):
        first.backward()
    second.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
