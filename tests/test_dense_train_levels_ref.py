"""Multi-level dense feature maps in training, CPU tier: the reference composition (tests/_dense_train_levels_ref.streams_after_blocks) pinned
bit for bit on the oracle's own forwards, the numpy restatement of tr_dense_scatter_levels as the per-level adjoint of the gather, the C
boundary of the three new entries with their host-side refusals (nothing is dereferenced or launched), and the interface's validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _dense_train_levels_ref as lref
from tests._params import GOLDEN_CASES, case_params, make_images
from tokenreduction_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["topk_micro", "evit_micro", "tome_micro", "dpcknn_micro", "ats_micro", "kmedoids_micro", "sit_micro", "sinkhorn_micro",
         "patchmerger_micro", "deit_micro"]
OK, SHAPE, ALIGN, NULL, CONFIG = 0, -1, -2, -3, -5
P = 4096                                                        # any 16-byte aligned non-NULL address


def _noise(case, name, golden_dir):
    if case["family"] != "dpcknn":
        return None
    import oracle
    from tests._params import case_config
    g = np.load(os.path.join(golden_dir, f"grad_{name}.npz"))
    return {blk: torch.from_numpy(g[f"rand_{n}"]) for n, blk in enumerate(sorted(oracle.dpcknn_cluster_counts(case_config(case))))}


# ---- the composition is the oracle's ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_streams_after_blocks_end_in_the_oracles_final_tokens_and_logits(golden_dir, name, precision):
    case = GOLDEN_CASES[name]
    cfg, params = case_params(case)
    x = make_images(case["batch"], case.get("img_size", 224), case["xseed"])
    noise = _noise(case, name, golden_dir)
    with torch.no_grad():
        logits, viz = lref.oracle_forward(params, x, cfg, precision, None, noise)
        hs = lref.streams_after_blocks(params, x, cfg, precision, None, noise)
        mine = lref.logits_of(params, hs[-1], cfg, precision)
    assert len(hs) == cfg.depth and [h.shape[1] for h in hs] == [viz["Tokens"][i] for i in range(cfg.depth)]
    assert torch.equal(hs[-1].view(torch.int32), viz["Final_Tokens"].view(torch.int32))
    assert torch.equal(mine.view(torch.int32), logits.view(torch.int32))
    assert len(set(lref.FAMILIES)) == 10 and case["family"] in lref.FAMILIES


def test_streams_after_blocks_is_differentiable_and_honours_forced_decisions():
    case = GOLDEN_CASES["topk_micro"]
    cfg, params = case_params(case)
    x = make_images(case["batch"], 224, case["xseed"])
    with torch.no_grad():
        _, viz = lref.oracle_forward(params, x, cfg, "bf16")
    blk = sorted(viz["Kept_Tokens"])[0]
    own = torch.from_numpy(viz["Kept_Tokens"][blk]).long()
    other = own.flip(1)                                          # the same rows in another order: another stream
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    with torch.enable_grad():
        hs = lref.streams_after_blocks(leaves, x, cfg, "bf16", {blk: other})
        assert not torch.equal(hs[blk], lref.streams_after_blocks(params, x, cfg, "bf16")[blk]) and hs[blk].shape[1] == own.shape[1] + 1
        rows = lref.level_rows(hs[0], leaves, cfg, True)
        index = torch.arange(1, 197).repeat(x.shape[0], 1)
        index[:, 5] = -1
        m = lref.level_map(rows, index, -7.5)
        assert (m[:, 5] == -7.5).all() and torch.equal(m[:, 6], rows[:, 7])
        (m.sum() + hs[-1].sum()).backward()
    assert leaves["norm.weight"].grad is not None and float(leaves["blocks.0.mlp.fc2.weight"].grad.abs().max()) > 0
    assert float(leaves[f"blocks.{cfg.depth - 1}.attn.qkv.weight"].grad.abs().max()) > 0


# ---- the restated scatter of L levels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
def test_scatter_levels_is_the_adjoint_of_the_gather_per_level(layout):
    """<gather_l(T), G> == <T, scatter_l(G)> per level in fp64, on integer-valued arrays where every product and sum is exact: indices with
    -1, with rows that several patches share and with rows nobody names; a NULL level is skipped."""
    rng = np.random.default_rng(5)
    B, P0, D = 2, 33, 8
    rows = [34, 1, 12, 20]
    index = np.stack([np.tile(np.arange(1, P0 + 1, dtype=np.int32), (B, 1)),
                      np.zeros((B, P0), dtype=np.int32),
                      rng.integers(-1, 12, size=(B, P0)).astype(np.int32),
                      rng.integers(0, 7, size=(B, P0)).astype(np.int32)])            # rows 7 ... 19 of the last level: nobody names them
    index[2, 0, 0], index[2, 1, 1] = -2, 12                       # entries that own nothing
    G = [rng.integers(-8, 9, size=(B, D, P0) if layout == "NCHW" else (B, P0, D)).astype(np.float32) for _ in rows]
    G[1] = None
    S = lref.dense_scatter_levels(G, index, rows, layout)
    assert S[1] is None
    for l, n in enumerate(rows):
        if G[l] is None:
            continue
        T = rng.integers(-8, 9, size=(B, n, D)).astype(np.float64)
        lhs = (lref.dense_gather_f64(T, index[l], layout) * G[l]).sum()
        assert S[l].shape == (B, n, D) and S[l].dtype == np.float32
        assert lhs == (T * S[l].astype(np.float64)).sum(), l
    assert not S[3][:, 7:].any() and S[3][:, :7].any()
    assert not S[2][0, 1:][~np.isin(np.arange(1, 12), index[2, 0])].any()


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------------
def _code():
    hdr = open(os.path.join(ROOT, "include", "tokenreduction_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_lib_and_library_agree_on_the_new_entry_points():
    code, lib = _code(), _lib.load()
    for name in ("tr_dense_scatter_levels", "tr_vit_forward_train_levels", "tr_vit_backward_levels", "tr_level_tap_norm", "tr_stream_grad_add"):
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code)
        assert m, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(m.group(1).split(",")), name
        assert hasattr(lib, name)
    # the new entries are the dense ones plus one struct pointer; no existing struct changed
    assert _lib.SIGNATURES["tr_vit_forward_train_levels"][1][:-1] == _lib.SIGNATURES["tr_vit_forward_train_dense"][1]
    assert _lib.SIGNATURES["tr_vit_backward_levels"][1][:-1] == _lib.SIGNATURES["tr_vit_backward_dense"][1]
    for struct, name, fields, size in ((_lib.TrVitTrainLevels, "tr_vit_train_levels", ["blocks", "norm", "tokens_out", "stream_out", "level_elems"], 32),
                                       (_lib.TrVitLevelGrads, "tr_vit_level_grads", ["blocks", "norm", "present", "dtokens", "stream", "level_stride"], 40)):
        m = re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", code)
        assert m and re.findall(r"(\w+);", m.group(1)) == fields == [f[0] for f in struct._fields_]
        assert C.sizeof(struct) == size
    assert C.sizeof(_lib.TrVitDenseTrain) == 64 and C.sizeof(_lib.TrVitLevels) == 24


def test_dense_scatter_levels_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    B, Pn, D = 2, 196, 384
    stride = B * (Pn + 1) * D

    def call(maps=(P, None, P), index=P, out=P, stride=stride, rows=(197, 138, 97), L=None, layout=_lib.TR_LAYOUT_NCHW, src_bf16=0, dst_bf16=0,
             B=B, Pn=Pn, D=D, null_maps=False, null_rows=False):
        L = len(maps) if L is None else L
        ptrs = (C.c_void_p * max(len(maps), 1))(*maps)
        r = (C.c_int32 * max(len(rows), 1))(*rows)
        return lib.tr_dense_scatter_levels(None if null_maps else ptrs, index, out, stride, None if null_rows else r, L, layout, src_bf16, dst_bf16,
                                           B, Pn, D, None)
    assert call(null_maps=True) == NULL and call(null_rows=True) == NULL and call(index=None) == NULL and call(out=None) == NULL
    assert call(L=0) == CONFIG and call(maps=(P,) * 33, rows=(5,) * 33) == CONFIG and b"levels" in lib.tr_last_error()
    assert call(layout=2) == CONFIG and call(layout=-1) == CONFIG and b"layout" in lib.tr_last_error()
    assert call(D=382) == SHAPE and call(D=1028) == SHAPE and call(Pn=1025) == SHAPE and call(Pn=0) == SHAPE and call(B=0) == SHAPE
    assert call(rows=(197, 0, 97)) == SHAPE and call(stride=B * 197 * D - 4) == SHAPE and b"does not fit a slab" in lib.tr_last_error()
    assert call(rows=(197, 198, 97)) == SHAPE                    # a level without a gradient is checked like the others
    assert call(stride=stride + 2) == ALIGN and call(stride=stride + 4, dst_bf16=1) == ALIGN
    for arg in ("index", "out"):
        assert call(**{arg: P + 4}) == ALIGN and call(**{arg: P + 8}, src_bf16=1, dst_bf16=1, layout=_lib.TR_LAYOUT_NHWC) == ALIGN, arg
    assert call(maps=(P, None, P + 8)) == ALIGN
    assert call(maps=(None, None, None)) == OK                   # no level has a gradient: nothing to launch, nothing dereferenced


def _micro_config(family=_lib.TR_FAMILY_DEIT, depth=4):
    cfg = _lib.TrVitConfig()
    cfg.family, cfg.img_size, cfg.patch, cfg.in_chans, cfg.embed_dim, cfg.depth = family, 224, 16, 3, 128, depth
    cfg.num_heads, cfg.mlp_hidden, cfg.num_classes, cfg.ln_eps, cfg.precision = 2, 512, 8, 1e-6, _lib.TR_PREC_BF16
    return cfg


def test_forward_train_levels_refuses_before_any_launch():
    lib = _lib.load()
    cfg, W = _micro_config(), _lib.TrVitWeights()
    B, N0, D, depth = 2, 197, 128, 4
    tokens = (C.c_int * depth)()
    slab, slabs = B * N0 * D, depth * B * N0

    def call(cfg=cfg, levels=True, dense=True, B=B, blocks=0b0101, norm=1, tokens_out=P, stream_out=P, elems=2 * slab, pair=(None, None), tape=P):
        dn = _lib.TrVitDenseTrain(pair[0], pair[1], slab, P, P, slabs, None, 0)
        lv = _lib.TrVitTrainLevels(blocks, norm, tokens_out, stream_out, elems)
        return lib.tr_vit_forward_train_levels(C.byref(cfg), C.byref(W), P, _lib.TR_INPUT_F32, None, None, None, 0, P, P,
                                               lib.tr_vit_workspace_bytes(C.byref(cfg), max(B, 1)), tape, lib.tr_vit_tape_bytes(C.byref(cfg), max(B, 1)),
                                               None, None, tokens, B, None, None, 0.0, C.byref(dn) if dense else None, C.byref(lv) if levels else None)
    assert call(levels=False) == NULL and call(dense=False) == NULL and b"tr_vit_train_levels" in lib.tr_last_error()
    assert call(cfg=_micro_config(_lib.TR_FAMILY_DYVIT)) == CONFIG and b"DyViT" in lib.tr_last_error()
    assert call(tokens_out=None) == NULL and call(stream_out=None) == NULL and call(pair=(P, None)) == NULL
    assert call(blocks=0) == CONFIG and call(blocks=1 << depth) == CONFIG and call(norm=2) == CONFIG
    assert call(elems=2 * slab - 1) == SHAPE and b"level buffers hold" in lib.tr_last_error()
    assert call(blocks=0b1111, elems=3 * slab) == SHAPE
    for off in (4, 8):
        assert call(tokens_out=P + off) == ALIGN and call(stream_out=P + off) == ALIGN
    assert call(tape=None) == NULL                               # the training entry's own checks stay
    # the eval entry keeps refusing a tape: the new entry is the one place where levels and a tape go together
    lv = _lib.TrVitLevels(0b0101, 1, P, 2 * slab)
    assert _lib.SIGNATURES["tr_vit_forward_levels"][1][-1] == C.POINTER(_lib.TrVitLevels) and C.sizeof(lv) == 24


def test_backward_levels_refuses_before_any_launch():
    lib = _lib.load()
    cfg, W = _micro_config(), _lib.TrVitWeights()
    B = 2
    ws_bytes, tape_bytes = lib.tr_vit_backward_workspace_bytes(C.byref(cfg), B), lib.tr_vit_tape_bytes(C.byref(cfg), B)
    slab = B * 197 * 128

    def call(cfg=cfg, blocks=0b1001, norm=1, present=0b11, dtokens=P, stream=P, stride=slab, dense_dtokens=None):
        lv = _lib.TrVitLevelGrads(blocks, norm, present, dtokens, stream, stride)
        return lib.tr_vit_backward_levels(C.byref(cfg), C.byref(W), C.byref(W), C.byref(W), P, None, None, None, P, tape_bytes, P, ws_bytes, 0, 3, 0,
                                          B, None, None, 0.0, None, dense_dtokens, 1, P if dense_dtokens else None, C.byref(lv))
    assert call(cfg=_micro_config(_lib.TR_FAMILY_DYVIT)) == CONFIG and b"dfeat" in lib.tr_last_error()
    assert call(blocks=1 << 4) == CONFIG and call(norm=3) == CONFIG and call(present=0b100) == CONFIG
    assert call(dtokens=None) == NULL and call(stream=None) == NULL
    assert call(stride=slab - 8) == SHAPE and b"level_stride" in lib.tr_last_error()
    assert call(dtokens=P + 8) == ALIGN and call(stream=P + 4) == ALIGN and call(stride=slab + 4) == ALIGN
    assert call(dense_dtokens=P) == CONFIG and b"AND dtokens" in lib.tr_last_error()      # the last block's level and dtokens: one or the other


# ---- the interface ----------------------------------------------------------------------------------------------------------------------
def _cpu_model():
    import types
    import tokenreduction_amd as tra
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[1, 2, 3], viz_mode=False)
    return tra.TopKVisionTransformer(patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4, qkv_bias=True, num_classes=16, args=args)


def test_blocks_are_validated_like_forward_dense_and_ordered_ascending():
    m = _cpu_model()
    dense, levels = m._dense_arguments(blocks=(-1, 2), norm=False)
    assert levels.blocks == (2, 3) and levels.norm is False and dense.fmt == "NCHW"
    assert m._dense_arguments(blocks=1)[1].blocks == (1,) and m._dense_arguments()[1] is None
    import inspect
    sig = inspect.signature(m.forward_dense_train)
    assert list(sig.parameters)[:3] == ["x", "blocks", "norm"] and sig.parameters["blocks"].default is None and sig.parameters["norm"].default is True
    # the refusals come in the documented order: the mode and the device first, then the arguments -- all before anything is launched
    x = torch.zeros(1, 3, 224, 224)
    m.train()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.forward_dense_train(x, blocks=(9,))
    m.eval()
    with pytest.raises(RuntimeError, match=r"model\.train\(\)"):
        m.forward_dense_train(x, blocks=(1,))

    class OnDevice(torch.Tensor):                                 # a tensor that says it is on the device: the argument checks come next
        is_cuda = True
    m.train()
    xd = torch.zeros(1, 3, 224, 224).as_subclass(OnDevice)
    for blocks, match in (((4,), "outside -4 ... 3"), ((-5,), "outside"), ((1, -3), "twice"), ((), "empty")):
        with pytest.raises(ValueError, match=match):
            m.forward_dense_train(xd, blocks=blocks)
    with pytest.raises(ValueError, match="output_fmt"):
        m.forward_dense_train(xd, blocks=(1,), output_fmt="CHW")


def test_the_not_built_lists_no_longer_name_multi_level_maps_in_training():
    for rel in ("README.md", "DESIGN.md", os.path.join("tokenreduction_amd", "models.py"), os.path.join("include", "tokenreduction_hip.h")):
        text = " ".join(open(os.path.join(ROOT, rel)).read().split())
        assert "Multi-level maps in training" not in text and "multi-level maps in training, a differentiable" not in text, rel
    doc = " ".join(_cpu_model().forward_dense_train.__doc__.split())
    for left in ("gradient through `cls`", "differentiable eval forward", "soft-weighted un-merge", "EViT's fused token"):
        assert left in doc, left
