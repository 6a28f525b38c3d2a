"""CPU: LayerScale (init_values) and no_embed_class -- the Python surface, the fold / unfold identities in fp64, checkpoint ingest, parameter
groups, the flat gradient layout and the host-side checks of the two entry points.  (GPU: tests/test_hip_layerscale_ops.py for the kernels,
tests/test_layerscale_gpu.py for the models.)"""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

import tokenreduction_amd as tra
from tokenreduction_amd import _lib, finetune, models, ops, training
from tests._layerscale_ref import RefBlock, folded_block, make_model, twin_state_dict, unfold
from tests._params import GOLDEN_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_NAMES = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "ls1.gamma",
               "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma"]      # timm's order


def _args():
    return types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False)


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max())


def test_constructor_and_create_model_take_the_keywords():
    sig = inspect.signature(models.VisionTransformer.__init__)
    assert list(sig.parameters)[-2:] == ["init_values", "no_embed_class"]
    assert sig.parameters["init_values"].default is None and sig.parameters["no_embed_class"].default is False
    m = tra.create_model("topk_tiny_patch16_224", init_values=1e-6, no_embed_class=True, args=_args())
    assert tuple(m.pos_embed.shape) == (1, 196, 192) and m.num_tokens == 1
    assert m.no_weight_decay() == {"pos_embed", "cls_token", "dist_token"}
    for blk in m.blocks:
        assert [n for n, _ in blk.named_children()] == ["norm1", "attn", "ls1", "norm2", "mlp", "ls2"]
        for ls in (blk.ls1, blk.ls2):
            assert [n for n, _ in ls.named_parameters()] == ["gamma"] and tuple(ls.gamma.shape) == (192,)
            assert bool((ls.gamma == 1e-6).all())


@pytest.mark.parametrize("name", ["deit_micro", "topk_micro", "sit_micro"])
def test_state_dict_keys_and_parameter_order_are_timms(name):
    case = GOLDEN_CASES[name]
    m = make_model(case, init_values=1e-6)
    per_block = [n.split(".", 2)[2] for n, _ in m.named_parameters() if n.startswith("blocks.0.")]
    assert per_block == BLOCK_NAMES
    keys = set(m.state_dict())
    for i in range(case["depth"]):
        assert f"blocks.{i}.ls1.gamma" in keys and f"blocks.{i}.ls2.gamma" in keys
    # the same model without the options: exactly the keys and the order of today, nothing registered for ls1 / ls2
    plain, off = make_model(case), make_model(case, init_values=0, no_embed_class=False)
    for p in (plain, off):
        assert not any("ls1" in k or "ls2" in k or "gamma" in k for k in p.state_dict())
        assert not any(n in ("ls1", "ls2") for n, _ in p.blocks[0].named_children())
    assert list(plain.state_dict()) == list(off.state_dict()) == [k for k in m.state_dict() if not k.endswith(".gamma")]
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in m.named_parameters() if not n.endswith(".gamma")]
    assert tuple(plain.pos_embed.shape) == (1, 197, case["embed_dim"])


def test_fold_identity_fp64():
    """Block output of the LayerScale reference == the folded block's: two fp64 evaluations of one function that differ by a reassociated
    multiply (K * 2^-53 relative at most; 1e-9 is orders above)."""
    torch.manual_seed(0)
    blk = RefBlock(64, 1, seed=3).double()
    x = torch.randn(2, 9, 64, dtype=torch.float64)
    assert _rel(folded_block(blk)(x), blk(x)) <= 1e-9


def test_unfold_identity_fp64():
    """Autograd gradients of the LayerScale reference == unfold(gradients of the folded twin), every other gradient equal, to 1e-9 relative."""
    torch.manual_seed(1)
    blk = RefBlock(64, 1, seed=5).double()
    twin = folded_block(blk)
    x = torch.randn(2, 9, 64, dtype=torch.float64)
    t = torch.randn(2, 9, 64, dtype=torch.float64)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    (blk(xa) * t).sum().backward()
    (twin(xb) * t).sum().backward()
    assert _rel(xb.grad, xa.grad) <= 1e-9
    for lin, gamma in (("proj", blk.gamma_1), ("fc2", blk.gamma_2)):
        a, f = getattr(blk, lin), getattr(twin, lin)
        dw, db, dg = unfold(f.weight.grad, f.bias.grad, a.weight.detach(), a.bias.detach(), gamma.detach())
        assert _rel(dw, a.weight.grad) <= 1e-9 and _rel(db, a.bias.grad) <= 1e-9 and _rel(dg, gamma.grad) <= 1e-9
    for n, p in blk.named_parameters():
        if not n.startswith(("proj", "fc2", "gamma")):
            assert _rel(dict(twin.named_parameters())[n].grad, p.grad) <= 1e-9, n


def test_twin_state_dict():
    case = GOLDEN_CASES["deit_micro"]
    m = make_model(case, gamma_seed=7, init_values=1e-6, no_embed_class=True)
    sd = twin_state_dict(m)
    assert list(sd) == list(make_model(case).state_dict())
    assert tuple(sd["pos_embed"].shape) == (1, 197, 128) and bool((sd["pos_embed"][:, 0] == 0).all())
    assert torch.equal(sd["pos_embed"][:, 1:], m.pos_embed.detach())
    g, w = m.blocks[1].ls2.gamma.detach(), m.blocks[1].mlp.fc2.weight.detach()
    assert torch.equal(sd["blocks.1.mlp.fc2.weight"], g[:, None] * w) and torch.equal(sd["blocks.1.attn.qkv.weight"], m.blocks[1].attn.qkv.weight.detach())


def test_checkpoint_ingest_renames_gamma_and_resizes_a_classless_table():
    case = dict(GOLDEN_CASES["deit_micro"], img_size=384)
    m = make_model(case, init_values=1e-6, no_embed_class=True)
    D = case["embed_dim"]
    g = torch.Generator().manual_seed(0)
    ckpt = {k: torch.randn(v.shape, generator=g) for k, v in m.state_dict().items() if ".ls" not in k and k != "pos_embed"}
    ckpt["pos_embed"] = torch.randn(1, 196, D, generator=g)                 # a 224 x 224 DeiT-III table: no class row
    for i in range(case["depth"]):
        ckpt[f"blocks.{i}.gamma_1"] = torch.randn(D, generator=g)
        ckpt[f"blocks.{i}.gamma_2"] = torch.randn(D, generator=g)
    ckpt["blocks.0.ls1.gamma"] = torch.full((D,), 3.0)                       # both spellings: the new name wins
    before = {k: v.clone() for k, v in ckpt.items()}
    missing, unexpected = finetune.load_finetune_checkpoint(m, {"model": ckpt})
    assert not missing and not unexpected
    assert list(ckpt) == list(before) and all(torch.equal(ckpt[k], before[k]) for k in ckpt)          # the caller's dict is untouched
    assert bool((m.blocks[0].ls1.gamma == 3.0).all())
    assert torch.equal(m.blocks[0].ls2.gamma.detach(), ckpt["blocks.0.gamma_2"])
    assert torch.equal(m.blocks[2].ls1.gamma.detach(), ckpt["blocks.2.gamma_1"])
    assert tuple(m.pos_embed.shape) == (1, 576, D)
    want = torch.nn.functional.interpolate(ckpt["pos_embed"].reshape(1, 14, 14, D).permute(0, 3, 1, 2), size=(24, 24), mode="bicubic",
                                           align_corners=False).permute(0, 2, 3, 1).flatten(1, 2)
    assert torch.equal(m.pos_embed.detach(), want)                          # all 576 rows come from the grid: no prefix row
    # a model without LayerScale leaves the old names alone (unexpected, as before)
    plain = make_model(GOLDEN_CASES["deit_micro"])
    _, unexpected = finetune.load_finetune_checkpoint(plain, {"blocks.0.gamma_1": torch.zeros(D)})
    assert unexpected == ["blocks.0.gamma_1"]


def test_parameter_groups_put_gamma_in_a_no_decay_group():
    m = make_model(GOLDEN_CASES["topk_micro"], init_values=1e-6)
    groups = finetune.get_parameter_groups(m, 1e-3, weight_decay=0.05, with_names=True)
    where = {n: g for g in groups for n in g["params"]}
    for i in range(m.depth):
        for ls in ("ls1", "ls2"):
            assert where[f"blocks.{i}.{ls}.gamma"]["weight_decay"] == 0
    assert where["blocks.0.attn.proj.weight"]["weight_decay"] == 0.05


def test_freeze_attn_only_leaves_gamma_frozen_and_proj_trainable():
    m = make_model(GOLDEN_CASES["topk_micro"], init_values=1e-6)
    names = finetune.freeze_attn_only(m)
    assert "blocks.0.attn.proj.weight" in names and "blocks.0.attn.proj.bias" in names
    assert not any("gamma" in n for n in names)
    assert not m.blocks[0].ls1.gamma.requires_grad and not m.blocks[0].ls2.gamma.requires_grad and m.blocks[0].attn.proj.weight.requires_grad


@pytest.mark.parametrize("name", ["deit_micro", "topk_micro"])
def test_backward_order_keeps_gamma_in_its_blocks_slice(name):
    case = GOLDEN_CASES[name]
    m = make_model(case, init_values=1e-6, no_embed_class=True)
    names = [n for n, _ in training.backward_order(m)]
    assert sorted(names) == sorted(n for n, _ in m.named_parameters())
    for i in range(m.depth):
        idx = [k for k, n in enumerate(names) if n.startswith(f"blocks.{i}.")]
        assert idx == list(range(idx[0], idx[0] + 14)) and f"blocks.{i}.ls1.gamma" in names[idx[0]: idx[-1] + 1]
    st = training.TrainState(m)
    D, P = case["embed_dim"], m.patch_embed.num_patches
    for e, start, stop in st.block_slices:
        if e < m.depth:
            for ls in ("ls1", "ls2"):
                assert start <= st.offsets[f"blocks.{e}.{ls}.gamma"] < stop
    # the folded-gradient scratch, and the position gradient: a [(P + 1), D] slot whose rows 1 .. P are the parameter's view
    assert st.ls["scratch"].numel() == m.depth * (D * D + D * 4 * D + 2 * D) and st.ls["scratch"].dtype == torch.float32
    assert m._grad_slot_numel("pos_embed", m.pos_embed) == (P + 1) * D
    v = st.views["pos_embed"]
    assert tuple(v.shape) == (1, P, D) and v.is_contiguous()
    assert v.data_ptr() - st.flat.data_ptr() == 4 * (st.offsets["pos_embed"] + D) and (v.data_ptr() - st.flat.data_ptr()) % 256 == 0
    plain = training.TrainState(make_model(case))
    assert plain.ls is None and plain.view_off == {} and plain.views["pos_embed"].data_ptr() - plain.flat.data_ptr() == 4 * plain.offsets["pos_embed"]


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tokenreduction_hip.h")).read()
    lib = _lib.load()
    for name in ("tr_layerscale_fold", "tr_layerscale_unfold_grad"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == 5 == len(_lib.SIGNATURES[name][1])
        assert _lib.SIGNATURES[name][0] is ctypes.c_int and hasattr(lib, name)
    assert "tr_layerscale.hip" in open(os.path.join(ROOT, "tokenreduction_amd", "csrc", "Makefile")).read()
    assert callable(ops.layerscale_fold) and callable(ops.layerscale_unfold_grad)
    assert ops.LS_FOLD_ITEM.itemsize == 64 and ops.LS_UNFOLD_ITEM.itemsize == 80          # tr_ls_fold_item / tr_ls_unfold_item


def test_argument_validation_without_gpu():
    """rows / cols that are no multiples of 64, a null table, n <= 0: refused on the host, before any launch."""
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    ok, bad_r, bad_c, zero = ((ctypes.c_int * 2)(*v) for v in ((64, 64), (65, 64), (64, 96), (0, 64)))
    for fn, flag in ((lib.tr_layerscale_fold, 0), (lib.tr_layerscale_fold, 1), (lib.tr_layerscale_unfold_grad, 0), (lib.tr_layerscale_unfold_grad, 1)):
        assert fn(None, ok, 1, flag, None) == -3 and fn(p, None, 1, flag, None) == -3
        assert b"null" in lib.tr_last_error()
        assert fn(p, ok, 0, flag, None) == -1 and fn(p, ok, -2, flag, None) == -1
        assert fn(p, bad_r, 1, flag, None) == -1 and fn(p, bad_c, 1, flag, None) == -1 and fn(p, zero, 1, flag, None) == -1
        assert b"64" in lib.tr_last_error()
        assert fn(p + 8, ok, 1, flag, None) == -2
    with pytest.raises(ValueError, match="16-byte"):
        ops.layerscale_table([(8, 0, 16, 32, 0, 0, 64, 64)], ops.LS_FOLD_ITEM, "cpu")
