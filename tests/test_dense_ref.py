"""Dense feature maps, CPU tier: the C boundary of tr_dense_index / tr_dense_gather (header, _lib, Makefile, the pinned structs and
constants), their host-side refusals (no GPU: nothing is dereferenced or launched), and the numpy restatement (tests/_dense_ref.py) on
the decisions the committed fixtures recorded."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _decisions_ref as dref
from tests import _dense_ref as ref
from tests._params import GOLDEN_CASES
from tokenreduction_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["topk_micro", "evit_micro", "tome_micro", "dyvit_micro", "sit_micro", "dpcknn_micro", "ats_micro", "kmedoids_micro",
            "sinkhorn_micro", "patchmerger_micro", "ats_micro_384", "sit_micro_384_kr07", "topk_micro_384"]
NAMES = ("tr_dense_index", "tr_dense_gather")


def _header():
    hdr = open(os.path.join(ROOT, "include", "tokenreduction_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_lib_and_library_agree_on_the_entry_points():
    _, code = _header()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code)
        assert m, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(m.group(1).split(",")), name
        assert hasattr(lib, name)
    assert _lib.SIGNATURES["tr_dense_index"][1][4] == C.POINTER(_lib.TrDecisionStage)
    mk = open(os.path.join(ROOT, "tokenreduction_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\btr_dense\.hip\b", mk, flags=re.M)


def test_pinned_structs_and_constants_are_untouched():
    hdr, _ = _header()
    assert C.sizeof(_lib.TrDecisionStage) == 40
    assert C.sizeof(_lib.TrVitTaps) == 24
    assert C.sizeof(_lib.TrVitWeights) == 8 * 8 + 32 * 13 * 8 + 32 * 96
    assert C.sizeof(_lib.TrVitConfig) == (9 + 1 + 32 + 1 + 1 + 2 + 32 + 1 + 1) * 4
    assert sorted(re.findall(r"#define (TR_(?:LAYOUT|INPUT)_\w+)", hdr)) == ["TR_INPUT_F32", "TR_INPUT_U8_NCHW", "TR_INPUT_U8_NHWC", "TR_LAYOUT_NCHW",
                                                                             "TR_LAYOUT_NHWC"]
    assert (ref.PRUNE, ref.EVIT, ref.ATS, ref.CENTRES, ref.TOME, ref.SOFT) == (
        _lib.TR_DECISION_PRUNE, _lib.TR_DECISION_EVIT, _lib.TR_DECISION_ATS, _lib.TR_DECISION_CENTRES, _lib.TR_DECISION_TOME, _lib.TR_DECISION_SOFT)


def test_dense_gather_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    p = 4096                                                    # any 16-byte aligned non-NULL address

    def call(tokens=p, index=p, out=p, layout=_lib.TR_LAYOUT_NCHW, bf16=0, B=2, P=196, n_rows=138, D=384):
        return lib.tr_dense_gather(tokens, index, out, layout, bf16, 0.0, B, P, n_rows, D, None)
    assert call(tokens=None) == -3 and call(index=None) == -3 and call(out=None) == -3
    assert b"null" in lib.tr_last_error()
    assert call(D=382) == -1 and call(D=1028) == -1 and call(D=0) == -1           # D % 4, D > 1024
    assert call(P=1025) == -1 and call(P=0) == -1 and call(B=0) == -1 and call(n_rows=0) == -1
    assert call(layout=2) == -5 and call(layout=-1) == -5                         # unknown layout
    for arg in ("tokens", "index", "out"):
        assert call(**{arg: p + 4}) == -2, arg
        assert call(**{arg: p + 8}, bf16=1, layout=_lib.TR_LAYOUT_NHWC) == -2, arg


def test_dense_index_refuses_a_bad_table_before_any_launch():
    lib = _lib.load()
    p = 4096

    def call(stages, kept=p, kept_n=1 << 20, assign=p, assign_n=1 << 20, B=2, P0=196, n_last=None, out=p, n=None):
        tab = (_lib.TrDecisionStage * max(1, len(stages)))(*[_lib.TrDecisionStage(*s) for s in stages])
        if n_last is None:
            n_last = (ref.n_out(*stages[-1][1:4]) if stages else P0) + 1
        return lib.tr_dense_index(kept, kept_n, assign, assign_n, tab, len(stages) if n is None else n, B, P0, n_last, out, None)
    prune = (1, _lib.TR_DECISION_PRUNE, 197, 137, 0, 0, 0)
    tome = (1, _lib.TR_DECISION_TOME, 197, 16, 0, 0, 0)
    assert call([prune], out=None) == -3 and call([prune], kept=None) == -3 and call([tome], assign=None) == -3
    assert call([], out=None) == -3
    assert call([prune] * 33) == -5 and call([prune], n=-1) == -5
    assert call([(1, 6, 197, 137, 0, 0, 0)]) == -5                                # unknown kind
    assert call([prune, prune]) == -5                                             # blocks not ascending
    assert call([tome, (2, _lib.TR_DECISION_PRUNE, 181, 100, 0, 0, 0)]) == -5     # a kept-only stage behind a map stage
    assert b"kept list" in lib.tr_last_error()
    assert call([(1, _lib.TR_DECISION_SOFT, 197, 137, 0, 0, 0), (2, _lib.TR_DECISION_ATS, 138, 90, 0, 0, 0)]) == -5
    assert call([prune], P0=1025) == -1 and call([prune], B=0) == -1 and call([prune], P0=195) == -1      # n_in > P0 + 1
    assert call([(1, 0, 197, 197, 0, 0, 0)]) == -1 and call([(1, 0, 197, 0, 0, 0, 0)]) == -1              # k outside 1 ... n_in-1
    assert call([(1, _lib.TR_DECISION_ATS, 197, 1, 0, 0, 0)]) == -1
    # the chain must end at the last stream's patch rows
    assert call([prune], n_last=137) == -1 and call([prune], n_last=139) == -1    # (138 is right -- and would launch: never with these pointers)
    assert call([(1, _lib.TR_DECISION_EVIT, 197, 137, 0, 0, 0)], n_last=138) == -1                        # EViT leaves k + 1 patch rows
    assert call([(1, _lib.TR_DECISION_ATS, 197, 137, 0, 0, 0)], n_last=138) == -1                         # ATS k - 1
    assert call([tome], n_last=197 - 16 + 1) == -1
    assert call([], n_last=196) == -1                                             # no stage: every row stays
    # offsets inside their buffers
    assert call([prune], kept_n=2 * 137 - 1) == -1
    assert call([(1, 0, 197, 137, 1, 0, 0)], kept_n=2 * 137) == -1 and call([(1, 0, 197, 137, -1, 0, 0)]) == -1
    assert call([tome], assign_n=2 * 196 - 1) == -1
    assert call([(1, _lib.TR_DECISION_TOME, 197, 16, 0, 1, 0)], assign_n=2 * 196) == -1
    assert call([(1, _lib.TR_DECISION_CENTRES, 197, 137, 0, -1, 0)]) == -1
    for arg in ("kept", "assign", "out"):
        assert call([prune], **{arg: p + 4}) == -2, arg


def _fixture_index(name):
    case = GOLDEN_CASES[name]
    kept, compl, soft, stages, B, N0, _ = dref.slabs_from_fixture(name, case)
    dec = dref.stage_decisions(kept, compl, soft, stages, B, N0)
    n_last = ref.n_out(*stages[-1][1:]) + 1
    return case, dec, stages, B, N0 - 1, n_last, ref.dense_index(dec, stages, B, N0 - 1, n_last)


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_index_on_the_recorded_decisions(name):
    case, dec, stages, B, P0, n_last, index = _fixture_index(name)
    assert index.shape == (B, P0) and index.dtype == np.int32 and len(stages) >= 2
    assert ((index == -1) | ((index >= 1) & (index < n_last))).all()
    fam, last = case["family"], stages[-1][0]
    if fam in ("topk", "dyvit", "evit", "ats"):
        kept_last, count = dec["kept"][last], dec["kept_count"][last]
        for b in range(B):
            valid = [j for j in range(kept_last.shape[1]) if kept_last[b, j] >= 0]
            for j in valid:
                assert index[b, kept_last[b, j]] == j + 1, (b, j)
            owned = int((index[b] >= 0).sum())
            if fam == "evit":
                n_fused = int((kept_last[b] == -1).sum())       # this stage's fused token and those of the stages before that survived
                assert n_fused >= 1 and owned == kept_last.shape[1] - n_fused
            else:
                assert owned == count[b] == len(valid)
        assert (index == -1).any()                              # a pruning family drops patches
    elif fam == "tome":
        assert (index >= 1).all()
        for b in range(B):
            assert set(index[b].tolist()) == set(range(1, n_last))
    else:
        assert (index >= 1).all()                               # an assignment map sends every patch somewhere
    # the gather of the restatement: a patch shows its row, a lost patch the fill
    rng = np.random.default_rng(3)
    tokens = rng.standard_normal((B, n_last, 8)).astype(np.float32)
    feat = ref.dense_gather(tokens, index, "NCHW", "fp32", -7.5)
    for b in range(B):
        for p in (0, P0 // 2, P0 - 1):
            want = tokens[b, index[b, p]] if index[b, p] >= 0 else np.full(8, -7.5, np.float32)
            np.testing.assert_array_equal(feat[b, :, p], want)
    np.testing.assert_array_equal(ref.dense_gather(tokens, index, "NHWC", "fp32", -7.5), feat.transpose(0, 2, 1))


def test_no_stage_is_the_identity():
    index = ref.dense_index({"kept": {}, "assign": {}}, [], 2, 196, 197)           # DeiT, Heuristic: every row stays
    np.testing.assert_array_equal(index, np.tile(np.arange(1, 197, dtype=np.int32), (2, 1)))


def test_ats_valid_first_holds_on_the_fixture_and_catches_a_gap():
    for name in ("ats_micro", "ats_micro_384"):
        case = GOLDEN_CASES[name]
        kept, _, _, stages, B, N0, _ = dref.slabs_from_fixture(name, case)
        for blk, _, _, k in stages:
            assert ref.ats_valid_first(kept[blk * B * N0: blk * B * N0 + B * k].reshape(B, k))
    with pytest.raises(AssertionError):
        ref.ats_valid_first(np.array([[0, 3, 0, 5]]))
    with pytest.raises(AssertionError):
        ref.ats_valid_first(np.array([[0, 5, 3, 0]]))


def test_bf16_rounding_of_the_restatement_is_torchs():
    import torch
    vals = np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39, -1.0e-40, 1e-45, np.inf, -np.inf, 3.3895314e38, 65280.0,
                     0.1, -2.7], dtype=np.float32)
    want = torch.from_numpy(vals).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(ref.to_bf16_bits(vals), want)
