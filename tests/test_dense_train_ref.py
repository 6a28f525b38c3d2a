"""Dense feature maps in training, CPU tier: the C boundary of tr_dense_scatter / tr_vit_forward_train_dense / tr_vit_backward_dense (header,
_lib, Makefile, the new struct and the pinned ones), their host-side refusals (no GPU: nothing is dereferenced or launched), and the numpy
restatement of the scatter (tests/_dense_train_ref.py) as the exact adjoint of tests/_dense_ref.dense_gather."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _dense_ref as ref
from tests import _dense_train_ref as tref
from tokenreduction_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tr_dense_scatter", "tr_vit_forward_train_dense", "tr_vit_backward_dense")
OK, SHAPE, ALIGN, NULL, CONFIG = 0, -1, -2, -3, -5
P = 4096                                                        # any 16-byte aligned non-NULL address
FIELDS = ["tokens_out", "stream_out", "rows_elems", "kept_idx", "compl_idx", "idx_elems", "soft_out", "soft_elems"]


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
    assert _lib.SIGNATURES["tr_vit_forward_train_dense"][1][-1] == C.POINTER(_lib.TrVitDenseTrain)
    # the backward entry is tr_vit_backward_dx's signature plus (dtokens, dtokens_is_bf16, stream)
    assert _lib.SIGNATURES["tr_vit_backward_dense"][1][:-3] == _lib.SIGNATURES["tr_vit_backward_dx"][1]
    # the scatter lives in tr_dense.hip, the executors where they were: no new file, the Makefile lists them
    mk = open(os.path.join(ROOT, "tokenreduction_amd", "csrc", "Makefile")).read()
    for src in ("tr_dense.hip", "tr_vit.hip", "tr_train.hip"):
        assert re.search(rf"^SRCS\s*=.*\b{re.escape(src)}\b", mk, flags=re.M), src
        assert os.path.exists(os.path.join(ROOT, "tokenreduction_amd", "csrc", src))


def test_the_new_struct_and_the_pinned_ones():
    _, code = _header()
    assert C.sizeof(_lib.TrVitDenseTrain) == 64
    assert [f[0] for f in _lib.TrVitDenseTrain._fields_] == FIELDS
    m = re.search(r"typedef struct \{([^}]*)\}\s*tr_vit_dense_train;", code)
    assert m and re.findall(r"(\w+);", m.group(1)) == FIELDS
    assert [getattr(_lib.TrVitDenseTrain, f).offset for f in FIELDS] == list(range(0, 64, 8))
    # nothing that existed changed its size
    assert C.sizeof(_lib.TrVitLevels) == 24
    assert C.sizeof(_lib.TrDecisionStage) == 40
    assert C.sizeof(_lib.TrVitTaps) == 24
    assert C.sizeof(_lib.TrVitWeights) == 8 * 8 + 32 * 13 * 8 + 32 * 96
    assert C.sizeof(_lib.TrVitConfig) == (9 + 1 + 32 + 1 + 1 + 2 + 32 + 1 + 1) * 4


# ---- tr_dense_scatter --------------------------------------------------------------------------------------------------------------------
def test_dense_scatter_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()

    def call(dmap=P, index=P, out=P, layout=_lib.TR_LAYOUT_NCHW, src_bf16=0, dst_bf16=0, B=2, Pn=196, n_rows=138, D=384):
        return lib.tr_dense_scatter(dmap, index, out, layout, src_bf16, dst_bf16, B, Pn, n_rows, D, None)
    assert call(dmap=None) == NULL and call(index=None) == NULL and call(out=None) == NULL
    assert call(layout=2) == CONFIG and call(layout=-1) == CONFIG and b"layout" in lib.tr_last_error()
    assert call(D=382) == SHAPE and call(D=1028) == SHAPE and call(D=0) == SHAPE
    assert call(Pn=1025) == SHAPE and call(Pn=0) == SHAPE and call(B=0) == SHAPE and call(n_rows=0) == SHAPE and call(n_rows=-3) == SHAPE
    for arg in ("dmap", "index", "out"):
        assert call(**{arg: P + 4}) == ALIGN, arg
        assert call(**{arg: P + 8}, src_bf16=1, dst_bf16=1, layout=_lib.TR_LAYOUT_NHWC) == ALIGN, arg


# ---- the two executor entries ------------------------------------------------------------------------------------------------------------
def _micro_config(family=_lib.TR_FAMILY_DEIT, depth=4):
    cfg = _lib.TrVitConfig()
    cfg.family, cfg.img_size, cfg.patch, cfg.in_chans, cfg.embed_dim, cfg.depth = family, 224, 16, 3, 128, depth
    cfg.num_heads, cfg.mlp_hidden, cfg.num_classes, cfg.ln_eps, cfg.precision = 2, 512, 8, 1e-6, _lib.TR_PREC_BF16
    return cfg


def test_forward_train_dense_refuses_before_any_launch():
    lib = _lib.load()
    cfg, W = _micro_config(), _lib.TrVitWeights()
    B, N0, D, depth = 2, 197, 128, 4
    ws_bytes, tape_bytes = lib.tr_vit_workspace_bytes(C.byref(cfg), B), lib.tr_vit_tape_bytes(C.byref(cfg), B)
    assert ws_bytes > 0 and tape_bytes > 0
    tokens = (C.c_int * depth)()
    rows, slabs = B * N0 * D, depth * B * N0

    def call(cfg=cfg, dense=True, fmt=_lib.TR_INPUT_F32, aug=None, B=B, tape=P, **over):
        fields = dict(tokens_out=P, stream_out=P, rows_elems=rows, kept_idx=P, compl_idx=P, idx_elems=slabs, soft_out=None, soft_elems=0)
        fields.update(over)
        dn = _lib.TrVitDenseTrain(*[fields[f] for f in FIELDS])
        return lib.tr_vit_forward_train_dense(C.byref(cfg), C.byref(W), P, fmt, None, aug, None, 0, P, P, lib.tr_vit_workspace_bytes(C.byref(cfg), max(B, 1)),
                                              tape, lib.tr_vit_tape_bytes(C.byref(cfg), max(B, 1)), None, None, tokens,
                                              B, None, None, 0.0, C.byref(dn) if dense else None)
    assert call(dense=False) == NULL and b"tr_vit_dense_train" in lib.tr_last_error()
    assert call(cfg=_micro_config(_lib.TR_FAMILY_DYVIT)) == CONFIG and b"DyViT" in lib.tr_last_error()      # before anything else is read
    assert call(tokens_out=None) == NULL and call(stream_out=None) == NULL
    assert call(kept_idx=None) == NULL and call(compl_idx=None) == NULL and b"both or neither" in lib.tr_last_error()
    assert call(rows_elems=rows - 1) == SHAPE and b"stream_out hold" in lib.tr_last_error()
    assert call(idx_elems=slabs - 1) == SHAPE and b"slabs" in lib.tr_last_error()
    for name in ("tokens_out", "stream_out", "kept_idx", "compl_idx", "soft_out"):
        for off in (4, 8):
            assert call(**{name: P + off}, soft_elems=1 << 20) == ALIGN, name
    # the training entry's own checks stay in front: the tape, the augmented input's format and batch
    assert call(tape=None) == NULL and call(tape=P + 8) == ALIGN
    assert call(aug=P) == CONFIG and b"uint8" in lib.tr_last_error()
    assert call(aug=P, fmt=_lib.TR_INPUT_U8_NCHW, B=3) == SHAPE and b"even" in lib.tr_last_error()
    # a soft family's stages need room in soft_out when it is given
    soft = _micro_config(_lib.TR_FAMILY_SIT)
    soft.keep[1] = 98
    assert call(cfg=soft, soft_out=P, soft_elems=B * 98 * 196 - 1) == SHAPE and b"soft stages" in lib.tr_last_error()


def test_backward_dense_refuses_before_any_launch():
    lib = _lib.load()
    cfg, W = _micro_config(), _lib.TrVitWeights()
    B = 2
    ws_bytes, tape_bytes = lib.tr_vit_backward_workspace_bytes(C.byref(cfg), B), lib.tr_vit_tape_bytes(C.byref(cfg), B)
    assert ws_bytes > 0

    def call(cfg=cfg, dtokens=P, stream=P, bf16=1, dlogits=P):
        return lib.tr_vit_backward_dense(C.byref(cfg), C.byref(W), C.byref(W), C.byref(W), dlogits, None, None, None, P, tape_bytes, P, ws_bytes, 0, 3, 0,
                                         B, None, None, 0.0, None, dtokens, bf16, stream)
    assert call(stream=None) == NULL and b"stream_out" in lib.tr_last_error()
    assert call(cfg=_micro_config(_lib.TR_FAMILY_DYVIT)) == CONFIG and b"dfeat" in lib.tr_last_error()
    for off in (4, 8):
        assert call(dtokens=P + off) == ALIGN and call(stream=P + off) == ALIGN and call(dtokens=P + off, bf16=0) == ALIGN
    assert call(dlogits=None) == NULL                            # tr_vit_backward's own checks are still there


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _indices(B, P0, n_rows, rng):
    yield "identity", np.tile(np.arange(1, P0 + 1, dtype=np.int32), (B, 1))
    yield "none", np.full((B, P0), -1, dtype=np.int32)
    merge = rng.integers(0, n_rows, size=(B, P0)).astype(np.int32)
    yield "merge", merge
    holes = merge.copy()
    holes[rng.random((B, P0)) < 0.4] = -1
    holes[0, 0], holes[-1, -1], holes[0, P0 // 2] = -2, n_rows, 2 ** 31 - 1
    yield "holes and entries that own nothing", holes
    yield "one row", np.full((B, P0), n_rows - 1, dtype=np.int32)
    yield "row 0", np.zeros((B, P0), dtype=np.int32)


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("P0,n_rows,D", [(1, 1, 4), (9, 2, 8), (65, 66, 12), (196, 120, 8)])
def test_scatter_is_the_exact_adjoint_of_the_gather(layout, P0, n_rows, D):
    """<gather(T), G> == <T, scatter(G)> on integer-valued arrays, where every product and every sum is exact (fill 0: a patch without a
    row contributes nothing on either side)."""
    rng = np.random.default_rng(P0 * 31 + D)
    B = 2
    for what, index in _indices(B, P0, n_rows, rng):
        T = rng.integers(-8, 9, size=(B, n_rows, D)).astype(np.float32)
        G = rng.integers(-8, 9, size=(B, D, P0) if layout == "NCHW" else (B, P0, D)).astype(np.float32)
        lhs = (ref.dense_gather(T, index, layout, "fp32", 0.0).astype(np.float64) * G).sum()
        S = tref.dense_scatter(G, index, n_rows, layout)
        assert S.shape == (B, n_rows, D) and S.dtype == np.float32, what
        assert lhs == (T.astype(np.float64) * S).sum(), what
        # a row nobody names is zero
        named = [set(int(r) for r in index[b] if 0 <= r < n_rows) for b in range(B)]
        for b in range(B):
            for r in set(range(n_rows)) - named[b]:
                assert not S[b, r].any(), (what, b, r)


def test_scatter_sums_in_fp32_in_ascending_patch_order_and_rounds_once():
    # 2^24 + 1 + 1 in fp32: ascending order loses both ones, the other order would not -- the restatement pins the order
    G = np.zeros((1, 3, 4), dtype=np.float32)
    G[0, :, 0] = [2.0 ** 24, 1.0, 1.0]
    G[0, :, 1] = [1.0, 1.0, 2.0 ** 24]
    index = np.zeros((1, 3), dtype=np.int32)
    S = tref.dense_scatter(G, index, 1, "NHWC")
    assert S[0, 0, 0] == 2.0 ** 24 and S[0, 0, 1] == 2.0 ** 24 + 2
    assert np.array_equal(tref.dense_scatter(G.transpose(0, 2, 1).copy(), index, 1, "NCHW"), S)
    # bf16 in: the bits are the values; bf16 out: the fp32 sum rounded once, to nearest even (1 + 2^-8 is a tie: down to even; 1 + 3 * 2^-8 up)
    bits = ref.to_bf16_bits(np.array([[[1.0, 2.0 ** -8, 1.0, 3 * 2.0 ** -8]]], dtype=np.float32).reshape(1, 2, 2))
    assert np.array_equal(tref.bf16_bits_to_f32(bits).reshape(-1), np.array([1.0, 2.0 ** -8, 1.0, 3 * 2.0 ** -8], dtype=np.float32))
    G2 = np.zeros((1, 2, 4), dtype=np.float32)
    G2[0, :, 0] = [1.0, 2.0 ** -8]
    G2[0, :, 1] = [1.0, 3 * 2.0 ** -8]
    out = tref.dense_scatter(G2, np.zeros((1, 2), dtype=np.int32), 1, "NHWC", "bf16")
    assert out.dtype == np.uint16 and out[0, 0, 0] == 0x3F80 and out[0, 0, 1] == 0x3F82
    # -0 + -0 from +0: the sum starts at +0
    Z = np.full((1, 2, 4), -0.0, dtype=np.float32)
    assert not np.signbit(tref.dense_scatter(Z, np.zeros((1, 2), dtype=np.int32), 1, "NHWC")).any()
