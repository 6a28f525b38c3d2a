"""Headless models (num_classes = 0: head = nn.Identity(), deit_viz.py:142,182), host-side checks: the C ABI sizes a headless
configuration in all three plans (eval workspace, training tape, backward workspace), every factory name builds at num_classes = 0 with
the reference's state_dict keys (tests/golden/headless_state_keys.json, written by tests/golden/gen_golden_headless.py), and
reset_classifier moves between a headless model and a classifier in both directions."""
import ctypes
import json
import os
import types

import pytest
import torch

import tokenreduction_amd as tra
from tokenreduction_amd import _lib

# The DyViT teachers' state_dict ORDER differs from the reference's for classifier models too (the reference builds their norm before the
# blocks; this package keeps timm's order for VisionTransformerTeacher) -- an order that predates headless models and that optimizer
# state_dicts of the teacher never address (the teacher is not trained).  For these three names the key SET is the reference's and the
# headless order is the classifier model's order without head.*; every other name matches the reference's list element by element.
_ORDER_AS_CLASSIFIER = {"dyvit_tiny_patch16_224_teacher", "dyvit_small_patch16_224_teacher", "dyvit_base_patch16_224_teacher"}


def _args(**kw):
    a = dict(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False, dyvit_distill=False, k_neighbors=5, equal_weight=False,
             sinkhorn_eps=1.0, cluster_iters=3, heuristic_pattern="l2", not_contiguous=False, min_radius=None)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _deit_s_config(num_classes, precision=_lib.TR_PREC_BF16):
    cfg = _lib.TrVitConfig()
    cfg.family, cfg.img_size, cfg.patch, cfg.in_chans = _lib.TR_FAMILY_TOPK, 224, 16, 3
    cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden, cfg.num_classes = 384, 12, 6, 1536, num_classes
    cfg.ln_eps, cfg.precision = 1e-6, precision
    cfg.keep[3], cfg.keep[6], cfg.keep[9] = 137, 96, 67
    return cfg


def test_headless_config_has_workspace_tape_and_backward_workspace():
    lib = _lib.load()
    cfg = _deit_s_config(0)
    ws = lib.tr_vit_workspace_bytes(ctypes.byref(cfg), 64)
    tape = lib.tr_vit_tape_bytes(ctypes.byref(cfg), 64)
    bws = lib.tr_vit_backward_workspace_bytes(ctypes.byref(cfg), 64)
    assert ws > 0 and tape > 0 and bws > 0, (ws, tape, bws)
    for prec in (_lib.TR_PREC_FP32, _lib.TR_PREC_BF16X3):
        assert lib.tr_vit_workspace_bytes(ctypes.byref(_deit_s_config(0, prec)), 64) > 0
    # the classifier's own scratch is all the headless plans may leave out
    cls = _deit_s_config(1000)
    assert ws == lib.tr_vit_workspace_bytes(ctypes.byref(cls), 64)
    assert tape == lib.tr_vit_tape_bytes(ctypes.byref(cls), 64)
    assert 0 < bws <= lib.tr_vit_backward_workspace_bytes(ctypes.byref(cls), 64)
    # still refused: a negative class count, and the all-zero configuration
    assert lib.tr_vit_workspace_bytes(ctypes.byref(_deit_s_config(-4)), 64) == 0
    assert lib.tr_vit_workspace_bytes(ctypes.byref(_lib.TrVitConfig()), 4) == 0


def test_every_factory_headless_state_keys_match_reference(golden_dir):
    with open(os.path.join(golden_dir, "headless_state_keys.json")) as f:
        ref = json.load(f)
    assert sorted(ref["models"]) == tra.list_models()
    for name in tra.list_models():
        torch.manual_seed(0)
        m = tra.create_model(name, pretrained=False, num_classes=0, img_size=224, args=_args())
        assert isinstance(m.head, torch.nn.Identity) and m.num_classes == 0, name
        keys, want = list(m.state_dict().keys()), ref["key_sets"][ref["models"][name]]
        assert not any(k.startswith("head.") for k in want), name
        if name in _ORDER_AS_CLASSIFIER:
            assert sorted(keys) == sorted(want), name
            c = tra.create_model(name, pretrained=False, num_classes=10, img_size=224, args=_args())
            assert keys == [k for k in c.state_dict().keys() if not k.startswith("head.")], name
        else:
            assert keys == want, name


@pytest.mark.parametrize("name", ["topk_tiny_patch16_224", "dyvit_tiny_patch16_224", "dyvit_tiny_patch16_224_teacher", "sit_tiny_patch16_224"])
def test_reset_classifier_round_trip_restores_keys_and_shapes(name):
    torch.manual_seed(0)
    m = tra.create_model(name, pretrained=False, num_classes=10, args=_args())
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    m.reset_classifier(0)
    assert m.num_classes == 0 and isinstance(m.head, torch.nn.Identity)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, s) for k, s in shapes if not k.startswith("head.")]
    assert m._out_width == m._out_cols == m.embed_dim
    m.reset_classifier(10)
    assert sorted((k, tuple(v.shape)) for k, v in m.state_dict().items()) == sorted(shapes)
    assert m._out_cols == 10 and m._out_width == 16
    m.reset_classifier(0)
    assert m._out_cols == m.embed_dim and not any(k.startswith("head.") for k in m.state_dict())


def test_classifier_checkpoint_loads_into_headless_model():
    """load_state_dict(classifier_state, strict=False): the head.* keys are the only unexpected ones and the trunk is loaded."""
    torch.manual_seed(0)
    src = tra.create_model("topk_tiny_patch16_224", pretrained=False, num_classes=10, args=_args())
    torch.manual_seed(1)
    dst = tra.create_model("topk_tiny_patch16_224", pretrained=False, num_classes=0, args=_args())
    res = dst.load_state_dict(src.state_dict(), strict=False)
    assert sorted(res.unexpected_keys) == ["head.bias", "head.weight"] and not res.missing_keys
    sd = dst.state_dict()
    for k, v in src.state_dict().items():
        if not k.startswith("head."):
            assert torch.equal(sd[k], v), k
