"""Decision taps, CPU tier: the numpy restatement of tr_stage_decisions (tests/_decisions_ref.py) on the decisions the committed fixtures
recorded, pushed through harness.decision_records, equals harness.image_records on the same fixture's viz_data -- the definition of the
record -- for every image and stage; and the C boundary of the new entry point (header, _lib, struct layout, host-side refusals)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _decisions_ref as ref
from tests._params import GOLDEN_CASES
from tokenreduction_amd import _lib, harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["topk_micro", "evit_micro", "tome_micro", "dyvit_micro", "sit_micro", "dpcknn_micro", "ats_micro", "kmedoids_micro",
            "sinkhorn_micro", "patchmerger_micro", "ats_micro_384", "sit_micro_384_kr07", "topk_micro_384"]


def _records_equal(got, want, what):
    assert list(got) == list(want), what
    for stage in want:
        assert sorted(got[stage]) == sorted(want[stage]), (what, stage)
        for key in want[stage]:
            np.testing.assert_array_equal(got[stage][key], want[stage][key], err_msg=f"{what} {stage} {key}")


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_decisions_are_the_reference_records(name):
    case = GOLDEN_CASES[name]
    kept, compl, soft, stages, B, N0, viz = ref.slabs_from_fixture(name, case)
    assert len(stages) >= 2 and B >= 2                                           # a composition happens, and more than one image
    dec = ref.stage_decisions(kept, compl, soft, stages, B, N0)
    if case["family"] == "ats":
        counts = dec["kept_count"]
        assert any((counts[blk] < stages[i][3] - 1).any() for i, blk in enumerate(dec["stages"]))       # an image with padding
        assert any(len(set(counts[blk].tolist())) > 1 for blk in counts)          # ... and rows of different valid widths
    model_name = case["family"] + "_micro"
    locs = list(case["reduction_loc"])
    for i in range(B):
        _records_equal(harness.decision_records(model_name, locs, dec, i), harness.image_records(model_name, locs, viz, i), f"{name}[{i}]")


def test_decision_records_takes_device_form_and_copies_each_buffer_once(monkeypatch):
    """The dec of forward_decisions holds int32 views of one buffer per kind: decisions_to_host copies a buffer once however many stages
    lie in it, and decision_records gives the same record from the tensor form as from the host form."""
    case = GOLDEN_CASES["dpcknn_micro"]
    kept, compl, soft, stages, B, N0, viz = ref.slabs_from_fixture("dpcknn_micro", case)
    dec = ref.stage_decisions(kept, compl, soft, stages, B, N0)

    def packed(d):
        flat = torch.from_numpy(np.concatenate([d[blk].reshape(-1) for blk in dec["stages"]]).astype(np.int32))
        out, off = {}, 0
        for blk in dec["stages"]:
            out[blk] = flat[off: off + d[blk].size].view(*d[blk].shape)
            off += d[blk].size
        return out
    tdec = {"stages": dec["stages"], "kept": packed(dec["kept"]), "kept_count": packed(dec["kept_count"]), "assign": packed(dec["assign"])}
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(self.numel()), real(self, *a, **k))[1])
    host = harness.decisions_to_host(tdec)
    assert len(copies) == 3, copies                                               # kept, kept_count, assign: one each
    locs = list(case["reduction_loc"])
    for i in range(B):
        want = harness.image_records("dpcknn_micro", locs, viz, i)
        _records_equal(harness.decision_records("dpcknn_micro", locs, host, i), want, f"host[{i}]")
    monkeypatch.undo()
    _records_equal(harness.decision_records("dpcknn_micro", locs, tdec, 1), harness.image_records("dpcknn_micro", locs, viz, 1), "tensor form")


def test_restatement_marks_what_it_cannot_index():
    B, N0 = 1, 9
    kept = np.zeros(4 * B * N0, dtype=np.int32)
    kept[1 * N0: 1 * N0 + 4] = [3, 8, -1, 0]                    # stage at block 1: 8 = P (one past the grid), -1
    kept[2 * N0: 2 * N0 + 2] = [4, 1]                           # block 2 indexes a list of 4: 4 is one past it
    dec = ref.stage_decisions(kept, kept, np.zeros(0, np.float32), [(1, ref.PRUNE, 9, 4), (2, ref.PRUNE, 5, 2)], B, N0)
    np.testing.assert_array_equal(dec["kept"][1], [[3, -2, -2, 0]])
    np.testing.assert_array_equal(dec["kept"][2], [[-2, -2]])
    dec = ref.stage_decisions(kept, kept, np.zeros(0, np.float32), [(1, ref.EVIT, 9, 4), (2, ref.EVIT, 6, 2)], B, N0)
    np.testing.assert_array_equal(dec["kept"][1], [[3, -2, -1, 0, -1]])
    np.testing.assert_array_equal(dec["kept"][2], [[-1, -2, -1]])                # index 4 is the trailing -1 of the list before


def test_header_declares_and_lib_types_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "tokenreduction_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+tr_stage_decisions\s*\(", code)
    assert "validate.py:199-229" in hdr                                            # the reference lines it replaces
    restype, argtypes = _lib.SIGNATURES["tr_stage_decisions"]
    assert restype is C.c_int and len(argtypes) == 15 and argtypes[5] == C.POINTER(_lib.TrDecisionStage)
    assert hasattr(_lib.load(), "tr_stage_decisions")
    body = re.search(r"typedef struct \{([^}]*)\}\s*tr_decision_stage;", code).group(1)
    fields = re.findall(r"(int32_t|int64_t)\s+(\w+);", body)
    assert [f for _, f in fields] == [f for f, _ in _lib.TrDecisionStage._fields_]
    off = 0
    for ctype, field in fields:
        size = 4 if ctype == "int32_t" else 8
        off = (off + size - 1) // size * size
        assert getattr(_lib.TrDecisionStage, field).offset == off and getattr(_lib.TrDecisionStage, field).size == size, field
        off += size
    assert C.sizeof(_lib.TrDecisionStage) == 40 == off
    for name in ("TR_MAX_DECISION_STAGES", "TR_DECISION_PRUNE", "TR_DECISION_EVIT", "TR_DECISION_ATS", "TR_DECISION_CENTRES", "TR_DECISION_TOME",
                 "TR_DECISION_SOFT"):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == getattr(_lib, name), name
    assert (ref.PRUNE, ref.EVIT, ref.ATS, ref.CENTRES, ref.TOME, ref.SOFT) == (
        _lib.TR_DECISION_PRUNE, _lib.TR_DECISION_EVIT, _lib.TR_DECISION_ATS, _lib.TR_DECISION_CENTRES, _lib.TR_DECISION_TOME, _lib.TR_DECISION_SOFT)


def test_entry_point_refuses_a_bad_table_before_any_launch():
    """Host-side checks only: nothing is dereferenced or launched, so no GPU is needed."""
    lib = _lib.load()
    p = 4096                                                    # any 16-byte aligned non-NULL address

    def call(stages, kept=p, compl=p, idx=1 << 20, soft=p, soft_n=1 << 20, B=2, N0=197, kept_out=p, kept_n=1 << 20, count=p, assign=p,
             assign_n=1 << 20, n=None):
        tab = (_lib.TrDecisionStage * max(1, len(stages)))(*[_lib.TrDecisionStage(*s) for s in stages])
        return lib.tr_stage_decisions(kept, compl, idx, soft, soft_n, tab, len(stages) if n is None else n, B, N0, kept_out, kept_n, count, assign,
                                      assign_n, None)
    ok = (1, _lib.TR_DECISION_PRUNE, 197, 137, 0, 0, 0)
    assert call([], kept=None, count=None) == 0                                   # no stage: nothing to do, nothing looked at
    assert call([ok] * 33) == -5 and b"stages" in lib.tr_last_error()
    assert call([ok], n=-1) == -5
    assert call([(1, 6, 197, 137, 0, 0, 0)]) == -5                                # unknown kind
    assert call([ok, ok]) == -5                                                   # blocks not ascending
    assert call([(32, 0, 197, 137, 0, 0, 0)]) == -5
    assert call([(1, 0, 197, 197, 0, 0, 0)]) == -1                                # k >= n_in
    assert call([(1, 0, 197, 0, 0, 0, 0)]) == -1                                  # k < 1
    assert call([(1, 0, 198, 137, 0, 0, 0)]) == -1                                # n_in > N0
    assert call([(1, _lib.TR_DECISION_ATS, 197, 1, 0, 0, 0)]) == -1
    assert call([ok], N0=1026) == -1 and call([ok], B=0) == -1
    assert call([ok], idx=2 * 2 * 197 - 1) == -1                                  # the slab of block 1 leaves the index buffer
    assert call([ok], kept_n=2 * 137 - 1) == -1                                   # offsets inside the buffers
    assert call([(1, 0, 197, 137, 1, 0, 0)], kept_n=2 * 137) == -1
    assert call([(1, 0, 197, 137, -1, 0, 0)]) == -1
    assert call([(1, _lib.TR_DECISION_TOME, 197, 16, 0, 1, 0)], assign_n=2 * 196) == -1
    assert call([(1, _lib.TR_DECISION_SOFT, 197, 8, 0, 0, 1)], soft_n=2 * 8 * 196) == -1
    assert call([ok], kept=None) == -3 and call([ok], count=None) == -3 and call([ok], kept_out=None) == -3
    assert call([(1, _lib.TR_DECISION_CENTRES, 197, 137, 0, 0, 0)], compl=None) == -3
    assert call([(1, _lib.TR_DECISION_SOFT, 197, 8, 0, 0, 0)], soft=None) == -3
    assert call([(1, _lib.TR_DECISION_TOME, 197, 16, 0, 0, 0)], assign=None) == -3
    for arg in ("kept", "compl", "soft", "kept_out", "count", "assign"):
        assert call([ok], **{arg: p + 4}) == -2, arg                              # misaligned pointer


class _StubModel:
    """forward_async(x, decisions=True) of a Top-K model whose decisions were recorded in a fixture: image id in the first pixel."""
    viz_mode = False

    def __init__(self, dec, locs):
        self.dec, self.locs, self.events, self.launched = dec, locs, [], 0

    def get_reduction_count(self):
        return self.locs

    def forward_async(self, x, decisions=False):
        ids = x[:, 0, 0, 0].long()
        k, self.launched = self.launched, self.launched + 1
        self.events.append(("launch", k, bool(decisions)))
        logits = torch.zeros(len(ids), 8)
        logits[torch.arange(len(ids)), ids % 8] = 1.0
        out = logits
        if decisions:
            take = lambda d: {blk: torch.from_numpy(a[ids.numpy()].astype(np.int32)) for blk, a in d.items()}
            out = (logits, {"stages": self.dec["stages"], "kept": take(self.dec["kept"]), "kept_count": take(self.dec["kept_count"]),
                            "assign": take(self.dec["assign"])})
        model = self

        class Handle:
            def result(self):
                model.events.append(("result", k))
                return out
        return Handle()

    def check_status(self):
        self.events.append(("status",))


def test_validate_fills_the_stage_records_with_one_batch_of_lookahead():
    case = GOLDEN_CASES["topk_micro"]
    kept, compl, soft, stages, B, N0, viz = ref.slabs_from_fixture("topk_micro", case)
    dec = ref.stage_decisions(kept, compl, soft, stages, B, N0)
    locs = list(case["reduction_loc"])
    order = [0, 1, 2, 2, 0]                                         # five images in batches of 2, 2, 1
    imgs = torch.zeros(len(order), 3, 2, 2)
    imgs[:, 0, 0, 0] = torch.tensor(order).float()
    loader = [(imgs[i: i + 2], torch.tensor(order[i: i + 2])) for i in range(0, len(order), 2)]
    names = [f"img_{i}" for i in range(len(order))]
    model = _StubModel(dec, locs)
    data = harness.validate(loader, model, torch.device("cpu"), "topk_micro", names, stage_records=True)
    assert model.events == [("launch", 0, True), ("launch", 1, True), ("result", 0), ("launch", 2, True), ("result", 1), ("result", 2),
                            ("status",)]
    for n, i in zip(names, order):
        assert sorted(data[n]) == ["Loss", "Predictions", "Stage-1", "Stage-2", "Stage-3", "Target"]
        _records_equal({k: v for k, v in data[n].items() if k.startswith("Stage-")}, harness.image_records("topk_micro", locs, viz, i), n)
    assert data["Top1-Acc"] == 100.0
    # the default: no decisions asked for, no stage keys
    model = _StubModel(dec, locs)
    data = harness.validate(loader, model, torch.device("cpu"), "topk_micro", names)
    assert [e[2] for e in model.events if e[0] == "launch"] == [False] * 3 and sorted(data[names[0]]) == ["Loss", "Predictions", "Target"]
