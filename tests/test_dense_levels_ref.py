"""Multi-level dense feature maps, CPU tier: the C boundary of tr_vit_forward_levels / tr_dense_index_levels / tr_dense_gather_levels (header,
_lib, Makefile, the pinned structs), their host-side refusals (no GPU: nothing is dereferenced or launched), and the numpy restatement
(tests/_dense_levels_ref.py) on the decisions the committed fixtures recorded."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _decisions_ref as dref
from tests import _dense_levels_ref as lref
from tests import _dense_ref as ref
from tests._params import GOLDEN_CASES
from tests.test_dense_ref import FIXTURES
from tokenreduction_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tr_vit_forward_levels", "tr_dense_index_levels", "tr_dense_gather_levels")
OK, SHAPE, ALIGN, NULL, CONFIG = 0, -1, -2, -3, -5
P = 4096                                                        # any 16-byte aligned non-NULL address


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
    assert _lib.SIGNATURES["tr_vit_forward_levels"][1][-2:] == [C.POINTER(_lib.TrVitTaps), C.POINTER(_lib.TrVitLevels)]
    assert _lib.SIGNATURES["tr_dense_index_levels"][1][4] == C.POINTER(_lib.TrDecisionStage)
    mk = open(os.path.join(ROOT, "tokenreduction_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\btr_dense\.hip\b", mk, flags=re.M) and re.search(r"^SRCS\s*=.*\btr_vit\.hip\b", mk, flags=re.M)


def test_the_new_struct_and_the_pinned_ones():
    _, code = _header()
    assert C.sizeof(_lib.TrVitLevels) == 24
    assert [f[0] for f in _lib.TrVitLevels._fields_] == ["blocks", "norm", "tokens_out", "tokens_elems"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*tr_vit_levels;", code)
    assert m and re.findall(r"(\w+);", m.group(1)) == ["blocks", "norm", "tokens_out", "tokens_elems"]
    assert (_lib.TrVitLevels.blocks.offset, _lib.TrVitLevels.norm.offset, _lib.TrVitLevels.tokens_out.offset,
            _lib.TrVitLevels.tokens_elems.offset) == (0, 4, 8, 16)
    assert C.sizeof(_lib.TrDecisionStage) == 40
    assert C.sizeof(_lib.TrVitTaps) == 24
    assert C.sizeof(_lib.TrVitWeights) == 8 * 8 + 32 * 13 * 8 + 32 * 96
    assert C.sizeof(_lib.TrVitConfig) == (9 + 1 + 32 + 1 + 1 + 2 + 32 + 1 + 1) * 4


# ---- tr_vit_forward_levels ---------------------------------------------------------------------------------------------------------------
def _micro_config(depth=4):
    cfg = _lib.TrVitConfig()
    cfg.family, cfg.img_size, cfg.patch, cfg.in_chans, cfg.embed_dim, cfg.depth = _lib.TR_FAMILY_DEIT, 224, 16, 3, 128, depth
    cfg.num_heads, cfg.mlp_hidden, cfg.num_classes, cfg.ln_eps, cfg.precision = 2, 512, 8, 1e-6, _lib.TR_PREC_BF16
    return cfg


def test_forward_levels_refuses_before_any_launch():
    """(The refusal of a training tape has no way in through this entry point: it takes no tape.  It guards the shared implementation.)"""
    lib = _lib.load()
    cfg, W = _micro_config(), _lib.TrVitWeights()
    B, slab = 2, 2 * 197 * 128
    nbytes = lib.tr_vit_workspace_bytes(C.byref(cfg), B)
    assert nbytes > 0
    tokens = (C.c_int * 4)()

    def call(blocks=0b0101, norm=0, out=P, elems=None, features=None, levels=True, taps=None, B=B):
        lv = _lib.TrVitLevels(blocks, norm, out, bin(blocks).count("1") * slab if elems is None else elems)
        return lib.tr_vit_forward_levels(C.byref(cfg), C.byref(W), P, _lib.TR_INPUT_F32, None, P, P, nbytes, None, None, None, None, features,
                                         tokens, B, None, taps, C.byref(lv) if levels else None)
    assert call(levels=False) == NULL and b"tr_vit_levels" in lib.tr_last_error()
    assert call(blocks=1 << 4) == CONFIG and b"outside" in lib.tr_last_error()            # a bit at depth
    assert call(blocks=1 << 31) == CONFIG and call(blocks=0b10001) == CONFIG
    assert call(out=None) == CONFIG and b"without tokens_out" in lib.tr_last_error()      # blocks without a buffer
    assert call(features=P) == CONFIG and b"features_out" in lib.tr_last_error()          # levels together with features_out
    assert call(norm=2) == CONFIG and call(norm=-1) == CONFIG
    assert call(elems=2 * slab - 1) == SHAPE and b"tokens_out holds" in lib.tr_last_error()
    assert call(blocks=0b1111, elems=3 * slab) == SHAPE and call(blocks=0b1000, elems=0) == SHAPE
    for off in (4, 8):
        assert call(out=P + off) == ALIGN
    # the tap struct rides along and keeps its own refusals
    assert call(taps=C.byref(_lib.TrVitTaps(1 << 4, P, None))) == CONFIG
    assert call(taps=C.byref(_lib.TrVitTaps(1, None, None))) == CONFIG
    assert call(B=0) == CONFIG                                                            # the executor's own checks come first


# ---- tr_dense_gather_levels --------------------------------------------------------------------------------------------------------------
def test_dense_gather_levels_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()

    def call(tokens=P, index=P, out=P, rows=(197, 138, 97), stride=2 * 197 * 384, layout=_lib.TR_LAYOUT_NCHW, bf16=0, B=2, Pn=196, D=384, L=None,
             no_rows=False):
        arr = (C.c_int32 * max(1, len(rows)))(*rows)
        return lib.tr_dense_gather_levels(tokens, stride, None if no_rows else arr, len(rows) if L is None else L, index, out, layout, bf16, 0.0,
                                          B, Pn, D, None)
    assert call(tokens=None) == NULL and call(index=None) == NULL and call(out=None) == NULL and call(no_rows=True) == NULL
    assert call(layout=2) == CONFIG and call(layout=-1) == CONFIG
    assert call(L=0) == CONFIG and call(L=33) == CONFIG and call(L=-1) == CONFIG
    assert call(D=382) == SHAPE and call(D=1028) == SHAPE and call(D=0) == SHAPE
    assert call(Pn=1025) == SHAPE and call(Pn=0) == SHAPE and call(B=0) == SHAPE
    assert call(rows=(197, 0, 97)) == SHAPE and call(rows=(197, -1)) == SHAPE
    assert call(rows=(198,)) == SHAPE and call(stride=2 * 197 * 384 - 4) == SHAPE         # a level's rows leave its slab
    assert b"does not fit" in lib.tr_last_error()
    assert call(rows=(1,), stride=2 * 384 + 2) == ALIGN                                   # slabs must start 16-byte aligned
    for arg in ("tokens", "index", "out"):
        assert call(**{arg: P + 4}) == ALIGN, arg
        assert call(**{arg: P + 8}, bf16=1, layout=_lib.TR_LAYOUT_NHWC) == ALIGN, arg


# ---- tr_dense_index_levels ---------------------------------------------------------------------------------------------------------------
def test_dense_index_levels_refuses_a_bad_table_or_bad_levels_before_any_launch():
    lib = _lib.load()
    prune = (1, _lib.TR_DECISION_PRUNE, 197, 137, 0, 0, 0)
    prune2 = (2, _lib.TR_DECISION_PRUNE, 138, 96, 2 * 137, 0, 0)
    tome = (1, _lib.TR_DECISION_TOME, 197, 16, 0, 0, 0)

    def call(stages, blocks=None, rows=None, kept=P, kept_n=1 << 20, assign=P, assign_n=1 << 20, B=2, P0=196, out=P, n=None, L=None,
             no_blocks=False, no_rows=False):
        tab = (_lib.TrDecisionStage * max(1, len(stages)))(*[_lib.TrDecisionStage(*s) for s in stages])
        if blocks is None:
            blocks = (stages[-1][0],) if stages else (0,)
        if rows is None:
            rows = [lref.level_rows([s[:4] for s in stages], P0, b) for b in blocks]
        ab, ar = (C.c_int32 * max(1, len(blocks)))(*blocks), (C.c_int32 * max(1, len(rows)))(*rows)
        return lib.tr_dense_index_levels(kept, kept_n, assign, assign_n, tab, len(stages) if n is None else n, B, P0, None if no_blocks else ab,
                                         None if no_rows else ar, len(blocks) if L is None else L, out, None)
    # the table: tr_dense_index's refusals
    assert call([prune], out=None) == NULL and call([prune], kept=None) == NULL and call([tome], assign=None) == NULL
    assert call([prune], no_blocks=True) == NULL and call([prune], no_rows=True) == NULL
    assert call([prune] * 33) == CONFIG and call([prune], n=-1) == CONFIG
    assert call([(1, 6, 197, 137, 0, 0, 0)]) == CONFIG and call([prune, prune]) == CONFIG
    assert call([tome, (2, _lib.TR_DECISION_PRUNE, 181, 100, 0, 0, 0)]) == CONFIG and b"kept list" in lib.tr_last_error()
    assert call([prune], P0=1025) == SHAPE and call([prune], B=0) == SHAPE and call([prune], P0=195) == SHAPE
    assert call([(1, 0, 197, 197, 0, 0, 0)]) == SHAPE and call([(1, _lib.TR_DECISION_ATS, 197, 1, 0, 0, 0)]) == SHAPE
    assert call([prune], kept_n=2 * 137 - 1) == SHAPE and call([tome], assign_n=2 * 196 - 1) == SHAPE
    for arg in ("kept", "assign", "out"):
        assert call([prune], **{arg: P + 4}) == ALIGN, arg
    # the levels: 1 ... 32 of them, strictly ascending blocks inside [0, TR_MAX_DEPTH)
    assert call([prune], L=0) == CONFIG and call([prune], L=33) == CONFIG
    assert call([prune], blocks=(1, 1), rows=(138, 138)) == CONFIG and call([prune], blocks=(2, 1), rows=(138, 138)) == CONFIG
    assert b"ascending" in lib.tr_last_error()
    assert call([prune], blocks=(-1,), rows=(197,)) == CONFIG and call([prune], blocks=(32,), rows=(138,)) == CONFIG
    # every level's prefix of the stages must leave the rows the caller saw there
    two = [prune, prune2]
    good = dict(blocks=(0, 1, 2, 3), rows=(197, 138, 97, 97))                             # (would launch: never with these pointers)
    for l, wrong in ((0, 196), (0, 138), (1, 197), (1, 137), (2, 138), (2, 96), (3, 138)):
        rows = list(good["rows"])
        rows[l] = wrong
        assert call(two, blocks=good["blocks"], rows=rows) == SHAPE, (l, wrong)
        assert b"level %d" % l in lib.tr_last_error()
    assert call([(1, _lib.TR_DECISION_EVIT, 197, 137, 0, 0, 0)], blocks=(1,), rows=(138,)) == SHAPE      # EViT leaves k + 1 patch rows
    assert call([tome], blocks=(0, 1), rows=(197, 197 - 16 + 1)) == SHAPE                 # (level 0 is right, level 1 one too many)
    assert call([], blocks=(0, 5), rows=(197, 196)) == SHAPE                              # no stage: every row stays at every level


# ---- the restatement on the recorded decisions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_restated_levels_on_the_recorded_decisions(name):
    case = GOLDEN_CASES[name]
    kept, compl, soft, stages, B, N0, _ = dref.slabs_from_fixture(name, case)
    dec = dref.stage_decisions(kept, compl, soft, stages, B, N0)
    P0, depth = N0 - 1, case["depth"]
    blocks = list(range(depth))
    levels = lref.dense_index_levels(dec, stages, B, P0, blocks)
    assert levels.shape == (depth, B, P0) and levels.dtype == np.int32
    # the last level is the single-level index of the whole table
    n_last = ref.n_out(*stages[-1][1:]) + 1
    np.testing.assert_array_equal(levels[depth - 1], ref.dense_index(dec, stages, B, P0, n_last))
    # a level before the first stage is the identity
    first = stages[0][0]
    for blk in range(first):
        np.testing.assert_array_equal(levels[blk], np.tile(np.arange(1, P0 + 1, dtype=np.int32), (B, 1)))
    assert first == 0 or lref.level_rows(stages, P0, first - 1) == N0
    # two levels between the same pair of stages agree, and every value names a row of its level
    stage_blocks = {st[0] for st in stages}
    for blk in range(1, depth):
        rows = lref.level_rows(stages, P0, blk)
        assert ((levels[blk] == -1) | ((levels[blk] >= 1) & (levels[blk] < rows))).all()
        if blk not in stage_blocks:
            np.testing.assert_array_equal(levels[blk], levels[blk - 1])
    # pruning families: a patch lost at a level is lost at every later level
    if case["family"] in ("topk", "dyvit", "evit", "ats"):
        lost = levels < 0
        assert lost[depth - 1].any()
        for blk in range(1, depth):
            assert (lost[blk] | ~lost[blk - 1]).all(), blk
    # the gather of the restatement is the single-level gather per level
    rng = np.random.default_rng(4)
    tokens = [rng.standard_normal((B, lref.level_rows(stages, P0, blk), 8)).astype(np.float32) for blk in blocks]
    feats = lref.dense_gather_levels(tokens, levels, "NHWC", "fp32", -7.5)
    assert feats.shape == (depth, B, P0, 8)
    for l in (0, depth - 1):
        np.testing.assert_array_equal(feats[l], ref.dense_gather(tokens[l], levels[l], "NHWC", "fp32", -7.5))


def test_level_rows_mismatch_is_caught_by_the_restatement():
    stages = [(1, ref.PRUNE, 197, 137)]
    dec = {"kept": {1: np.tile(np.arange(137, dtype=np.int32), (2, 1))}, "assign": {}}
    lref.dense_index_levels(dec, stages, 2, 196, [0, 1], rows=[197, 138])
    with pytest.raises(AssertionError):
        lref.dense_index_levels(dec, stages, 2, 196, [0, 1], rows=[197, 137])
    with pytest.raises(AssertionError):
        lref.dense_index_levels(dec, stages, 2, 196, [1, 0])
