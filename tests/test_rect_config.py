"""Rectangular inputs, img_size=(H, W), everything that needs no GPU: the config field's layout, the schedules and token counts of a
(64, 96) and a (96, 64) model of every family against the subclassed oracle (tests/_rect_params.py), the oracle itself against the
reference's vectors at those sizes, the position-table resize, and the host-side checks of the new *_hw entry points."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
import tokenreduction_amd as tra
from tokenreduction_amd import _lib, finetune
from tests import _rect_params as R
from tests.test_hip_model import FAM

TR_OK, TR_ERR_SHAPE, TR_ERR_NULL = 0, -1, -3


def _args(case):
    return types.SimpleNamespace(keep_rate=list(case["keep_rate"]), reduction_loc=list(case["reduction_loc"]), viz_mode=False,
                                 dyvit_distill=False, k_neighbors=5, equal_weight=False, sinkhorn_eps=1.0, cluster_iters=3,
                                 heuristic_pattern="l2", not_contiguous=False, min_radius=None)


def _model(case, **kw):
    k = dict(img_size=case["img_size"], patch_size=16, embed_dim=case["embed_dim"], depth=case["depth"], num_heads=case["num_heads"],
             mlp_ratio=4, qkv_bias=True, num_classes=case["num_classes"], args=_args(case))
    k.update(kw)
    return getattr(tra, FAM[case["family"]])(**k)


# ---- the config field -----------------------------------------------------------------------------------------------------------------
def test_config_keeps_its_size_and_offsets():
    T = _lib.TrVitConfig
    assert C.sizeof(T) == 80 * 4
    assert (T.family.offset, T.img_size.offset, T.img_width.offset, T.patch.offset, T.in_chans.offset) == (0, 4, 6, 8, 12)
    assert T.img_size.size == 2 and T.img_width.size == 2
    assert T.concurrent.offset == 79 * 4 and T.global_pool.offset == 79 * 4 + 2


class _ParentConfig(C.Structure):       # the layout before the split: one int
    _fields_ = [("family", C.c_int), ("img_size", C.c_int), ("rest", C.c_int * 78)]


def test_an_int_img_size_writes_the_bytes_it_wrote_before():
    cfg = _lib.TrVitConfig()
    cfg.img_size = 224
    assert cfg.img_width == 0 and cfg.image_hw == (224, 224)
    old = _ParentConfig()
    old.img_size = 224
    assert bytes(cfg) == bytes(old)
    cfg.img_width = 320
    assert cfg.image_hw == (224, 320)
    old.img_size = 224 | (320 << 16)
    assert bytes(cfg) == bytes(old)


@pytest.mark.parametrize("img_size,want", [(224, (224, 0)), ((224, 224), (224, 0)), (384, (384, 0)), ((64, 96), (64, 96)), ((96, 64), (96, 64))])
def test_model_fills_both_halves(img_size, want):
    """A square model, given an int or a pair, builds the bytes it built before the field was split; a rectangular one fills the width."""
    case = dict(R.RECT_CASES[R.case_name("deit", R.SIZES[0])], img_size=img_size)
    m = _model(case)
    cfg = m._cfg_geometry(_lib.TrVitConfig())
    assert (cfg.img_size, cfg.img_width, cfg.patch, cfg.in_chans) == (*want, 16, 3)
    if want[1] == 0:
        old = _ParentConfig()
        old.img_size = want[0]
        old.rest[0], old.rest[1] = 16, 3
        assert bytes(cfg) == bytes(old)


def _plan_config(case, model):
    """A tr_vit_config for the plans (no weights needed): geometry from the model, schedule from its keep list."""
    cfg = model._cfg_geometry(_lib.TrVitConfig())
    cfg.family = model._family
    cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden, cfg.num_classes = case["embed_dim"], case["depth"], case["num_heads"], 4 * case["embed_dim"], 16
    cfg.ln_eps, cfg.precision, cfg.knn_k, cfg.cluster_iters, cfg.sinkhorn_eps = 1e-6, _lib.TR_PREC_BF16, 5, 3, 1.0
    for i in range(case["depth"]):
        cfg.keep[i] = int(model._keep[i])
    return cfg


def test_plans_follow_gh_times_gw():
    lib = _lib.load()
    case = R.RECT_CASES[R.case_name("deit", R.SIZES[0])]
    cfg = _plan_config(case, _model(case))
    rect = lib.tr_vit_workspace_bytes(C.byref(cfg), 2)
    assert rect > 0
    # 24 patches either way round, and the same plan as any other 24-patch grid; a square of the same height has 16
    cfg.img_size, cfg.img_width = 96, 64
    assert lib.tr_vit_workspace_bytes(C.byref(cfg), 2) == rect
    cfg.img_size, cfg.img_width = 64, 0
    assert 0 < lib.tr_vit_workspace_bytes(C.byref(cfg), 2) < rect
    cfg.img_size, cfg.img_width = 64, 64
    square = lib.tr_vit_workspace_bytes(C.byref(cfg), 2)
    cfg.img_width = 0
    assert lib.tr_vit_workspace_bytes(C.byref(cfg), 2) == square
    for bad in (90, -16, 8):           # a width that is no positive multiple of the patch
        cfg.img_size, cfg.img_width = 64, bad
        assert lib.tr_vit_workspace_bytes(C.byref(cfg), 2) == 0
        assert lib.tr_vit_tape_bytes(C.byref(cfg), 2) == 0
    cfg.img_size, cfg.img_width = 60, 96
    assert lib.tr_vit_workspace_bytes(C.byref(cfg), 2) == 0


_ORACLE_SCHEDULE = {"topk": oracle.stage_keep_counts, "evit": oracle.stage_keep_counts, "tome": oracle.tome_schedule,
                    "dyvit": oracle.dyvit_keep_counts, "sit": oracle.sit_cluster_counts, "patchmerger": oracle.sit_cluster_counts,
                    "dpcknn": oracle.dpcknn_cluster_counts, "sinkhorn": oracle.dpcknn_cluster_counts, "kmedoids": oracle.dpcknn_cluster_counts}


@pytest.mark.parametrize("name", [n for n, c in R.RECT_CASES.items() if c["embed_dim"] == 384])
def test_schedule_and_token_counts_match_the_oracle(name):
    """pos_embed [1, gh*gw + 1, D], the keep schedule of every family and the token counts of the executor's plan, against the subclassed
    oracle's rules on num_patches = gh * gw = 24 (Top-K / EViT: int(ratio * 196), as the reference hard-codes it)."""
    case = R.RECT_CASES[name]
    fam, depth = case["family"], case["depth"]
    cfg = R.case_config(case)
    assert cfg.num_patches == 24 and cfg.grid_size == (case["img_size"][0] // 16, case["img_size"][1] // 16)
    m = _model(case)
    assert m.patch_embed.grid_size == cfg.grid_size and m.patch_embed.num_patches == 24
    assert tuple(m.pos_embed.shape) == (1, 25, 384) == tuple(R.case_params(case)[1]["pos_embed"].shape)
    m.load_state_dict(R.case_params(case)[1], strict=True)
    if fam == "deit":
        want = {}
    elif fam == "ats":
        counts = oracle.ats_sample_counts(cfg)
        assert [int(v) for v in m.sample_count] == [counts.get(i, 0) for i in range(depth)]
        want = {i: int(oracle.ats_sample_steps(k).numel()) + 1 for i, k in counts.items()}
    else:
        want = dict(_ORACLE_SCHEDULE[fam](cfg))
    assert [int(v) for v in m._keep] == [want.get(i, 0) for i in range(depth)]
    assert all(want[i] > 0 for i in case["reduction_loc"])          # every stage still reduces
    # the executor's token plan (tr_vit_tape_layout: tokens entering block i, inside its attention, inside its Mlp)
    lib, pc = _lib.load(), _plan_config(case, m)
    got = []
    for i in range(depth):
        out = (C.c_size_t * 18)()
        assert lib.tr_vit_tape_layout(C.byref(pc), 2, i, out) == TR_OK
        got.append(tuple(int(v) for v in out[14:17]))
    n, exp = 25, []
    for i in range(depth):
        k = want.get(i, 0)
        pre = n
        if fam in ("sit", "patchmerger", "dpcknn", "sinkhorn", "kmedoids") and k:
            n = k + 1
        att = n
        if fam == "topk" and k:
            n = k + 1
        elif fam == "evit" and k:
            n = k + 2
        elif fam == "tome":
            n -= min(k, (n - 1) // 2)
        elif fam == "ats" and k:
            n = k
        exp.append((pre, att, n))       # (DyViT trains under a mask: every block sees all 25 tokens)
    assert got == exp
    assert exp[0][0] == 25 and (fam in ("deit", "dyvit") or exp[-1][2] < 25)


def test_pos_embed_without_a_class_row():
    case = R.RECT_CASES[R.case_name("deit", R.SIZES[1])]
    assert tuple(_model(case, no_embed_class=True).pos_embed.shape) == (1, 24, 384)


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("name", sorted(n for n in tra.list_models() if "_tiny_" in n))
def test_every_factory_name_takes_a_pair(name, size):
    args = types.SimpleNamespace(keep_rate=[0.1, 0.05] if "topk" in name or "evit" in name else [0.7], reduction_loc=[3, 6], dyvit_distill=False,
                                 k_neighbors=5, equal_weight=False, cluster_iters=3, sinkhorn_eps=1.0, heuristic_pattern="l2",
                                 not_contiguous=False, min_radius=None, viz_mode=False)
    if "heuristic" in name:
        with pytest.raises(ValueError, match="square grid"):
            tra.create_model(name, pretrained=False, num_classes=10, img_size=size, args=args)
        return
    m = tra.create_model(name, pretrained=False, num_classes=10, img_size=size, args=args)
    assert m.patch_embed.img_size == size and m.patch_embed.grid_size == (size[0] // 16, size[1] // 16)
    assert m.pos_embed.shape[1] == 25


def test_heuristic_refuses_a_non_square_grid():
    case = dict(R.RECT_CASES[R.case_name("deit", R.SIZES[0])], family="heuristic", keep_rate=[0.7], reduction_loc=[1, 2])
    for contiguous in (False, True):
        a = _args(case)
        a.not_contiguous = not contiguous
        with pytest.raises(ValueError, match=r"4 x 6 patch grid.*sqrt\(num_patches\)"):
            _model(case, args=a)
    _model(dict(case, img_size=(64, 64)))         # a square pair is a square model


# ---- the oracle at these sizes, pinned on the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.GOLDEN_RECT)
def test_subclassed_oracle_matches_the_reference(golden_dir, name, monkeypatch):
    """tests/test_oracle_golden.py's checks and tolerances on the rectangular fixtures (tests/golden/gen_golden_rect.py)."""
    from tests import _params, test_oracle_golden
    monkeypatch.setitem(_params.GOLDEN_CASES, name, R.RECT_CASES[name])
    with R.patched(test_oracle_golden):
        test_oracle_golden.test_model_matches_reference(golden_dir, name)


# ---- position-table resize ---------------------------------------------------------------------------------------------------------------
def _pos_model(img_size, **kw):
    case = dict(R.RECT_CASES[R.case_name("deit", R.SIZES[0])], img_size=img_size, embed_dim=64, num_heads=1)
    return _model(case, **kw)


def test_position_resize_to_a_rectangular_grid():
    torch.manual_seed(3)
    src = torch.randn(1, 197, 64)
    m = _pos_model((64, 96))
    finetune.load_finetune_checkpoint(m, {"model": {"pos_embed": src.clone()}})
    grid = F.interpolate(src[:, 1:].reshape(1, 14, 14, 64).permute(0, 3, 1, 2), size=(4, 6), mode="bicubic", align_corners=False)
    want = torch.cat((src[:, :1], grid.permute(0, 2, 3, 1).reshape(1, 24, 64)), dim=1)
    assert torch.equal(m.pos_embed.detach(), want)
    t = _pos_model((96, 64))
    finetune.load_finetune_checkpoint(t, {"pos_embed": src.clone()})
    grid = F.interpolate(src[:, 1:].reshape(1, 14, 14, 64).permute(0, 3, 1, 2), size=(6, 4), mode="bicubic", align_corners=False)
    assert torch.equal(t.pos_embed.detach()[:, 1:], grid.permute(0, 2, 3, 1).reshape(1, 24, 64))
    assert not torch.equal(t.pos_embed.detach(), m.pos_embed.detach())


def test_position_resize_from_a_rectangular_source():
    torch.manual_seed(4)
    src = torch.randn(1, 1 + 24, 64)
    m = _pos_model((32, 48))
    with pytest.raises(ValueError, match="no square grid"):
        finetune.load_finetune_checkpoint(m, {"pos_embed": src.clone()})
    with pytest.raises(ValueError, match="src_grid"):
        finetune.load_finetune_checkpoint(m, {"pos_embed": src.clone()}, src_grid=(5, 5))
    finetune.load_finetune_checkpoint(m, {"pos_embed": src.clone()}, src_grid=(4, 6))
    grid = F.interpolate(src[:, 1:].reshape(1, 4, 6, 64).permute(0, 3, 1, 2), size=(2, 3), mode="bicubic", align_corners=False)
    assert torch.equal(m.pos_embed.detach()[:, 1:], grid.permute(0, 2, 3, 1).reshape(1, 6, 64))
    # the same number of rows on another grid: resized when src_grid says so, loaded as it is otherwise
    t = _pos_model((96, 64))
    finetune.load_finetune_checkpoint(t, {"pos_embed": src.clone()})
    assert torch.equal(t.pos_embed.detach(), src)
    finetune.load_finetune_checkpoint(t, {"pos_embed": src.clone()}, src_grid=(4, 6))
    grid = F.interpolate(src[:, 1:].reshape(1, 4, 6, 64).permute(0, 3, 1, 2), size=(6, 4), mode="bicubic", align_corners=False)
    assert torch.equal(t.pos_embed.detach()[:, 1:], grid.permute(0, 2, 3, 1).reshape(1, 24, 64))
    # no class row: all of the table is the grid
    n = _pos_model((64, 96), no_embed_class=True)
    finetune.load_finetune_checkpoint(n, {"pos_embed": src[:, 1:].clone()}, src_grid=(6, 4))
    grid = F.interpolate(src[:, 1:].reshape(1, 6, 4, 64).permute(0, 3, 1, 2), size=(4, 6), mode="bicubic", align_corners=False)
    assert torch.equal(n.pos_embed.detach(), grid.permute(0, 2, 3, 1).reshape(1, 24, 64))


# ---- the new entry points, host side -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,H,W,patch,D,want", [
    (3, 224, 320, 16, 384, 1), (3, 320, 224, 16, 768, 1), (3, 16, 640, 16, 384, 1), (3, 640, 16, 16, 384, 1), (1, 32, 48, 16, 384, 1),
    (4, 96, 240, 16, 1152, 1), (3, 224, 224, 16, 384, 1),
    (3, 224, 320, 16, 192, 0), (3, 224, 320, 16, 128, 0), (3, 224, 320, 32, 384, 0), (3, 224, 328, 16, 384, 0), (3, 230, 320, 16, 384, 0),
    (3, 0, 320, 16, 384, 0), (3, 224, 0, 16, 384, 0), (3, -16, 320, 16, 384, 0), (0, 224, 320, 16, 384, 0), (3, 224, 320, 16, 0, 0),
    (3, 16384, 16384, 16, 384, 1), (3, 16384, 32768, 16, 384, 0),        # C * H * W < 2^30: the kernel's 32-bit source offsets
])
def test_patch_embed_hw_supported(C_, H, W, patch, D, want):
    lib = _lib.load()
    assert lib.tr_patch_embed_hw_supported(C_, H, W, patch, D) == want
    if H == W and H > 0:
        assert lib.tr_patch_embed_supported(C_, H, patch, D) == want


@pytest.mark.parametrize("C_,H,W,patch,D,want", [
    (3, 48, 400, 16, 128, 1), (3, 80, 16, 16, 128, 1), (3, 16, 640, 16, 192, 1), (1, 16, 32, 16, 192, 1), (3, 32, 48, 16, 768, 1),
    (3, 4096, 16, 16, 384, 1), (3, 16, 4096, 16, 384, 1),
    (3, 4112, 16, 16, 384, 0), (3, 16, 4112, 16, 384, 0), (2, 64, 96, 16, 384, 0), (3, 64, 96, 16, 256, 0), (3, 64, 96, 8, 384, 0),
    (3, 64, 100, 16, 384, 0), (3, 60, 96, 16, 384, 0), (3, 0, 96, 16, 384, 0), (3, 64, 0, 16, 384, 0), (3, 64, -16, 16, 384, 0),
])
def test_patch_embed_dgrad_hw_supported(C_, H, W, patch, D, want):
    lib = _lib.load()
    assert lib.tr_patch_embed_dgrad_hw_supported(C_, H, W, patch, D) == want
    if H == W:
        assert lib.tr_patch_embed_dgrad_supported(C_, H, patch, D) == want


def test_hw_entries_refuse_null_and_bad_shapes_before_any_launch():
    """As tests/test_boundary.py holds the HW entries: every refusal is a host-side check (no GPU here), with the entry's own name in
    tr_last_error."""
    lib = _lib.load()
    buf = C.create_string_buffer(4096 + 16)
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)

    def err():
        return lib.tr_last_error().decode()

    assert lib.tr_patch_embed_hw_bf16(None, p, p, p, p, p, 1, 3, 64, 96, 16, 384, None) == TR_ERR_NULL and "tr_patch_embed_hw_bf16" in err()
    assert lib.tr_patch_embed_hw_bf16(p, p, p, p, p, None, 1, 3, 64, 96, 16, 384, None) == TR_ERR_NULL
    for shape in ((1, 3, 64, 96, 16, 128), (1, 3, 64, 100, 16, 384), (1, 3, 60, 96, 16, 384), (0, 3, 64, 96, 16, 384), (1, 3, 64, 96, 32, 384),
                  (1, 3, 64, 0, 16, 384)):
        assert lib.tr_patch_embed_hw_bf16(p, p, p, p, p, p, *shape, None) == TR_ERR_SHAPE, shape
        assert "tr_patch_embed_hw_bf16" in err() and "H and W multiples of 16" in err()
    assert lib.tr_patch_embed_u8_hw_bf16(p, None, 0, p, p, p, p, p, 1, 3, 64, 96, 16, 384, None) == TR_ERR_NULL and "tr_patch_embed_u8_hw_bf16" in err()
    assert lib.tr_patch_embed_u8_hw_bf16(p, p, 2, p, p, p, p, p, 1, 3, 64, 96, 16, 384, None) == TR_ERR_SHAPE and "layout 2" in err()
    assert lib.tr_patch_embed_u8_hw_bf16(p, p, 0, p, p, p, p, p, 1, 3, 64, 90, 16, 384, None) == TR_ERR_SHAPE and "W=90" in err()
    assert lib.tr_patch_embed_u8_hw_bf16(p, p, 1, p, p, p, p, p, 1, 4, 64, 96, 16, 384, None) == TR_ERR_SHAPE and "NHWC needs 1 or 3" in err()
    assert lib.tr_patch_embed_dgrad_hw(None, 384, p, p, 1, 3, 64, 96, 16, 384, None) == TR_ERR_NULL and "tr_patch_embed_dgrad_hw" in err()
    assert lib.tr_patch_embed_dgrad_hw(p, 384, p, None, 1, 3, 64, 96, 16, 384, None) == TR_ERR_NULL
    for shape, ldy in (((1, 3, 64, 100, 16, 384), 384), ((1, 2, 64, 96, 16, 384), 384), ((1, 3, 64, 96, 16, 256), 256), ((0, 3, 64, 96, 16, 384), 384),
                       ((1, 3, 64, 96, 16, 384), 128), ((1, 3, 4112, 96, 16, 384), 384)):
        assert lib.tr_patch_embed_dgrad_hw(p, ldy, p, p, *shape, None) == TR_ERR_SHAPE, shape
        assert "tr_patch_embed_dgrad_hw" in err() and "H and W multiples of 16" in err()
    # the HW entries keep their own messages
    assert lib.tr_patch_embed_bf16(p, p, p, p, p, p, 1, 3, 224, 16, 128, None) == TR_ERR_SHAPE and "tr_patch_embed_bf16: need patch 16, H = W" in err()
    assert lib.tr_patch_embed_dgrad(p, 384, p, p, 1, 2, 224, 16, 384, None) == TR_ERR_SHAPE and "tr_patch_embed_dgrad: need patch 16, H = W" in err()


def test_ops_wrappers_check_the_size_arguments():
    from tokenreduction_amd import ops
    dy, wt = torch.zeros(25, 128, dtype=torch.bfloat16), torch.zeros(768, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="once"):
        ops.patch_embed_dgrad(dy, wt, 1, 3, (64, 96), H=64, W=96)
    with pytest.raises(ValueError, match="either HW or both"):
        ops.patch_embed_dgrad(dy, wt, 1, 3, H=64)
    with pytest.raises(ValueError, match="either HW or both"):
        ops.patch_embed_dgrad(dy, wt, 1, 3, 64, W=96)
    with pytest.raises(ValueError, match="missing"):
        ops.patch_embed_dgrad(dy, wt, 1, 3)
