"""CPU: the Python surface of the average-pooled head (global_pool='avg') and its C boundary -- constructor / create_model /
reset_classifier plumbing, the values the argument takes, DyViT's train-mode refusal, the fc_norm.* -> norm.* checkpoint ingest, and the
header <-> _lib agreement for tr_token_pool, tr_token_pool_bwd and tr_vit_config.global_pool.  (GPU: tests/test_hip_token_pool.py for the
two kernels, tests/test_avg_pool_gpu.py for the models.)"""
import ctypes
import os
import re
import types

import pytest
import torch

import tokenreduction_amd as tra
from tokenreduction_amd import _lib, finetune
from tests import _pool_ref
from tests._params import make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["deit_tiny_patch16_224_local", "topk_tiny_patch16_224", "evit_tiny_patch16_224", "tome_tiny_patch16_224", "dyvit_tiny_patch16_224",
            "sit_tiny_patch16_224", "dpcknn_tiny_patch16_224", "ats_tiny_patch16_224", "sinkhorn_tiny_patch16_224", "kmedoids_tiny_patch16_224",
            "patchmerger_tiny_patch16_224", "heuristic_tiny_patch16_224", "dyvit_tiny_patch16_224_teacher"]


def _args():
    return types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], dyvit_distill=False, k_neighbors=5, equal_weight=False, cluster_iters=3,
                                 sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None)


@pytest.mark.parametrize("name", FAMILIES)
def test_every_family_constructor_takes_global_pool(name):
    m = tra.create_model(name, pretrained=False, num_classes=10, global_pool="avg", args=_args())
    assert m.global_pool == "avg" and m._pool_mode() == _lib.TR_POOL_AVG
    d = tra.create_model(name, pretrained=False, num_classes=10, args=_args())
    assert d.global_pool == "" and d._pool_mode() == _lib.TR_POOL_CLS
    assert set(m.state_dict()) == set(d.state_dict())              # the pooled head's norm is the model's norm: same keys
    assert not any(k.startswith("fc_norm") for k in m.state_dict())


def test_global_pool_values():
    mk = lambda **kw: tra.VisionTransformer(embed_dim=64, depth=1, num_heads=1, num_classes=4, **kw)
    assert mk().global_pool == "" and mk(global_pool="token")._pool_mode() == _lib.TR_POOL_CLS
    assert mk(global_pool="token").global_pool == "token"
    assert mk(global_pool="avg")._pool_mode() == _lib.TR_POOL_AVG
    for bad in ("max", "avgmax", "mean", None, 1):
        with pytest.raises(ValueError, match="global_pool"):
            mk(global_pool=bad)
    m = mk()
    m.global_pool = "max"                                           # written past the constructor: refused where it is read
    with pytest.raises(ValueError, match="global_pool"):
        m._pool_mode()
    assert tra.create_model("deit_tiny_patch16_224_local", global_pool=None).global_pool == ""       # create_model drops None kwargs


def test_reset_classifier_plumbing():
    m = tra.VisionTransformer(embed_dim=64, depth=1, num_heads=1, num_classes=4)
    m._packed = object()
    m.reset_classifier(7, global_pool="avg")
    assert m.global_pool == "avg" and m.head.out_features == 7 and m.num_classes == 7 and m._packed is None
    m.reset_classifier(3)                                           # without the argument: the pooling stays
    assert m.global_pool == "avg" and m.head.out_features == 3
    m.reset_classifier(0, "")                                       # headless, back on the CLS row (timm's positional form)
    assert m.global_pool == "" and isinstance(m.head, torch.nn.Identity)
    m.reset_classifier(0, global_pool="avg")
    assert m._pool_mode() == _lib.TR_POOL_AVG and m.num_classes == 0
    m.reset_classifier(5, global_pool="token")
    assert m._pool_mode() == _lib.TR_POOL_CLS
    with pytest.raises(ValueError, match="global_pool"):
        m.reset_classifier(5, global_pool="max")
    assert m.global_pool == "token" and m.head.out_features == 5    # a refused call changes nothing


def test_dyvit_refuses_average_pool_in_train_mode_only():
    m = tra.create_model("dyvit_tiny_patch16_224", pretrained=False, num_classes=10, global_pool="avg", args=_args())
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(NotImplementedError, match="DyViT in train mode"):
        m.train()(x)
    with pytest.raises(RuntimeError, match="no CPU path"):          # eval is built: on this machine it gets as far as the device check
        m.eval()(x)
    m.reset_classifier(10, global_pool="")
    with pytest.raises(RuntimeError, match="no CPU path"):          # ... as does training on the CLS row
        m.train()(x)
    t = tra.create_model("topk_tiny_patch16_224", pretrained=False, num_classes=10, global_pool="avg", args=_args())
    with pytest.raises(RuntimeError, match="no CPU path"):          # every other family trains pooled
        t.train()(x)


def _micro(**kw):
    cfg = types.SimpleNamespace(embed_dim=64, depth=2, num_heads=1, mlp_ratio=4, num_classes=5, img_size=224, patch_size=16, in_chans=3)
    m = tra.VisionTransformer(embed_dim=64, depth=2, num_heads=1, num_classes=5, **kw)
    return m, make_params(cfg, 5)


def test_fc_norm_checkpoint_ingest():
    m, sd = _micro(global_pool="avg")
    ck = dict(sd)
    ck["fc_norm.weight"], ck["fc_norm.bias"] = ck.pop("norm.weight"), ck.pop("norm.bias")          # timm's layout of a MAE fine-tuned model
    missing, unexpected = finetune.load_finetune_checkpoint(m, {"model": ck})
    assert not missing and not unexpected
    assert torch.equal(m.norm.weight, sd["norm.weight"]) and torch.equal(m.norm.bias, sd["norm.bias"])
    assert "fc_norm.weight" in ck and "norm.weight" not in ck       # the caller's dict is not rewritten


def test_fc_norm_does_not_overwrite_norm_and_needs_the_average_pool():
    m, sd = _micro(global_pool="avg")
    ck = dict(sd)
    ck["fc_norm.weight"], ck["fc_norm.bias"] = sd["norm.weight"] + 1.0, sd["norm.bias"] + 1.0        # both present: norm.* wins
    missing, unexpected = finetune.load_finetune_checkpoint(m, ck)
    assert not missing and sorted(unexpected) == ["fc_norm.bias", "fc_norm.weight"]
    assert torch.equal(m.norm.weight, sd["norm.weight"]) and torch.equal(m.norm.bias, sd["norm.bias"])
    c, sd = _micro()                                                # a CLS model does not take fc_norm for its norm
    ck = dict(sd)
    ck["fc_norm.weight"], ck["fc_norm.bias"] = ck.pop("norm.weight"), ck.pop("norm.bias")
    before = c.norm.weight.detach().clone()
    missing, unexpected = finetune.load_finetune_checkpoint(c, ck)
    assert sorted(missing) == ["norm.bias", "norm.weight"] and sorted(unexpected) == ["fc_norm.bias", "fc_norm.weight"]
    assert torch.equal(c.norm.weight, before)


def test_header_and_lib_agree_on_the_pool_symbols_and_the_config_field():
    hdr = open(os.path.join(ROOT, "include", "tokenreduction_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("tr_token_pool", 10), ("tr_token_pool_bwd", 7)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
        assert hasattr(_lib.load(), name)
    # global_pool is the LAST member of tr_vit_config and the mirrored struct ends with it: the upper 16 bits of the word that was
    # `int concurrent`, so the struct keeps its size and every other member its offset
    body = re.search(r"typedef struct \{([^}]*)\}\s*tr_vit_config;", code, flags=re.S).group(1)
    members = [d.strip() for d in body.split(";") if d.strip()]
    assert members[-2:] == ["short concurrent", "short global_pool"]
    assert _lib.TrVitConfig._fields_[-2:] == [("concurrent", ctypes.c_short), ("global_pool", ctypes.c_short)]
    assert ctypes.sizeof(_lib.TrVitConfig) == 80 * 4
    assert _lib.TrVitConfig.concurrent.offset == 79 * 4 and _lib.TrVitConfig.global_pool.offset == 79 * 4 + 2
    assert _lib.TrVitConfig.ats_dynamic.offset == 78 * 4
    cfg = _lib.TrVitConfig()
    ctypes.cast(ctypes.byref(cfg, 79 * 4), ctypes.POINTER(ctypes.c_int))[0] = 1          # a caller of the former layout: int concurrent = 1
    assert (cfg.concurrent, cfg.global_pool) == (1, 0)
    assert (_lib.TR_POOL_CLS, _lib.TR_POOL_AVG) == (0, 1)


def test_config_and_shape_checks_without_gpu():
    lib = _lib.load()
    cfg = _lib.TrVitConfig()
    cfg.family, cfg.img_size, cfg.patch, cfg.in_chans = 1, 224, 16, 3
    cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden, cfg.num_classes = 384, 12, 6, 1536, 1000
    base = lib.tr_vit_workspace_bytes(ctypes.byref(cfg), 8)
    cfg.global_pool = 1
    pooled = lib.tr_vit_workspace_bytes(ctypes.byref(cfg), 8)
    assert 0 < base < pooled <= base + 8 * 384 * 4 + 256           # one [B, D] fp32 slot more
    assert lib.tr_vit_tape_bytes(ctypes.byref(cfg), 8) > 0 and lib.tr_vit_backward_workspace_bytes(ctypes.byref(cfg), 8) > 0
    for bad in (2, -1):                                             # neither CLS nor avg: no plan
        cfg.global_pool = bad
        assert lib.tr_vit_workspace_bytes(ctypes.byref(cfg), 8) == 0
        assert lib.tr_vit_tape_bytes(ctypes.byref(cfg), 8) == 0 and lib.tr_vit_backward_workspace_bytes(ctypes.byref(cfg), 8) == 0
        buf = (ctypes.c_char * 512)()
        p = (ctypes.addressof(buf) + 255) // 256 * 256
        W = _lib.TrVitWeights()
        tokens = (ctypes.c_int * 12)()
        assert lib.tr_vit_forward(ctypes.byref(cfg), ctypes.byref(W), p, p, p, 1 << 40, None, None, None, None, None, tokens, 8, None) == -5
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    for B, N, D in ((1, 1, 64), (1, 0, 64), (1, 5, 32), (1, 5, 96), (0, 5, 64), (1, 5, 0)):          # N >= 2, D % 64 == 0, B >= 1
        assert lib.tr_token_pool(p, None, None, 0, None, p, B, N, D, None) == -1, (B, N, D)
        assert lib.tr_token_pool_bwd(p, None, p, B, N, D, None) == -1, (B, N, D)
    assert lib.tr_token_pool(None, None, None, 0, None, p, 1, 5, 64, None) == -3 and lib.tr_token_pool(p, None, p, 0, None, p, 1, 5, 64, None) == -3
    assert lib.tr_token_pool(p + 8, None, None, 0, None, p, 1, 5, 64, None) == -2 and lib.tr_token_pool_bwd(p, None, p + 4, 1, 5, 64, None) == -2
    assert lib.tr_token_pool_bwd(None, None, p, 1, 5, 64, None) == -3


def test_reference_helper_arithmetic():
    """tests/_pool_ref.py against itself on a case small enough to write out."""
    v = torch.tensor([[[9.0, 9.0], [1.0, 2.0], [3.0, 6.0]]])      # row 0 is the CLS token
    assert torch.equal(_pool_ref.pool(v), torch.tensor([[2.0, 4.0]], dtype=torch.float64))
    w = torch.tensor([[5.0, 3.0, 1.0]])
    assert torch.equal(_pool_ref.pool(v, w), torch.tensor([[1.5, 3.0]], dtype=torch.float64))
    assert torch.equal(_pool_ref.pool(v, torch.zeros(1, 3)), torch.zeros(1, 2, dtype=torch.float64))
    g = _pool_ref.pool_bwd(torch.tensor([[4.0, 8.0]]), 3, w)
    assert torch.equal(g, torch.tensor([[[0.0, 0.0], [3.0, 6.0], [1.0, 2.0]]], dtype=torch.float64))
    leaf = v.double().clone().requires_grad_(True)
    (_pool_ref.pool(leaf, w) * torch.tensor([[4.0, 8.0]])).sum().backward()
    assert torch.equal(leaf.grad, g)
