"""Raw uint8 image input (model.set_pixel_input), CPU tier: the C ABI surface, the normalization table, the model-level switch."""
import copy
import ctypes
import os
import re
import types

import pytest
import torch

import tokenreduction_amd as tra
from tokenreduction_amd import _lib, pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tr_im2col_u8_bf16", "tr_im2col_u8_f32", "tr_patch_embed_u8_bf16", "tr_vit_forward_pixels", "tr_vit_forward_train_pixels")


def _header():
    return open(os.path.join(ROOT, "include", "tokenreduction_hip.h")).read()


def _model(in_chans=3):
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[1, 2], viz_mode=False)
    return tra.TopKVisionTransformer(patch_size=16, embed_dim=128, depth=3, num_heads=2, mlp_ratio=4, qkv_bias=True, num_classes=8,
                                     in_chans=in_chans, args=args)


def test_new_symbols_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_format_constants_match_the_header():
    defs = dict(re.findall(r"#define (TR_(?:LAYOUT|INPUT)_\w+) (\d+)", _header()))
    assert {k: int(v) for k, v in defs.items()} == {n: getattr(_lib, n) for n in defs}
    assert set(defs) == {"TR_LAYOUT_NCHW", "TR_LAYOUT_NHWC", "TR_INPUT_F32", "TR_INPUT_U8_NCHW", "TR_INPUT_U8_NHWC"}
    # the structs keep their layout: the format and the table travel as arguments of the *_pixels entry points
    assert ctypes.sizeof(_lib.TrVitConfig) == 80 * 4 and ctypes.sizeof(_lib.TrVitWeights) == 8 * 8 + 32 * 13 * 8 + 32 * 96


def test_argument_checks_without_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.tr_patch_embed_u8_bf16(None, p, 0, p, p, p, p, p, 1, 3, 224, 16, 384, None) == -3          # TR_ERR_NULL: image
    assert lib.tr_patch_embed_u8_bf16(p, None, 0, p, p, p, p, p, 1, 3, 224, 16, 384, None) == -3          # ... and the LUT
    assert lib.tr_patch_embed_u8_bf16(p, p, 2, p, p, p, p, p, 1, 3, 224, 16, 384, None) == -1             # layout
    assert lib.tr_patch_embed_u8_bf16(p, p, 1, p, p, p, p, p, 1, 4, 224, 16, 384, None) == -1             # NHWC with 4 channels
    assert lib.tr_patch_embed_u8_bf16(p, p, 0, p, p, p, p, p, 1, 3, 224, 16, 192, None) == -1             # embed_dim % 384
    assert lib.tr_im2col_u8_bf16(p, None, 0, p, 1, 3, 224, 224, 16, None) == -3
    assert lib.tr_im2col_u8_f32(p, p, 5, p, 1, 3, 224, 224, 16, None) == -1
    cfg = _lib.TrVitConfig()
    W = _lib.TrVitWeights()
    for fmt, lut in ((3, p), (-1, p), (_lib.TR_INPUT_U8_NCHW, None)):       # unknown formats, a uint8 format without its table
        rc = lib.tr_vit_forward_pixels(ctypes.byref(cfg), ctypes.byref(W), p, fmt, lut, p, p, 1 << 40, None, None, None, None, None, None, 1,
                                       None)
        assert rc in (-5,), rc


def test_lut_is_torchvision_to_tensor_normalize_bit_for_bit():
    mean, std = pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD
    lut = pixels.pixel_lut(mean, std)
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    # ToTensor (uint8 -> float, / 255) + Normalize (per-channel fp32 tensors, [:, None, None]) on an image holding every value in every channel
    u8 = torch.arange(256, dtype=torch.uint8).repeat(3, 1).view(3, 16, 16)
    want = ((u8.float() / 255) - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]
    assert torch.equal(lut.view(torch.int32), want.reshape(3, 256).view(torch.int32))
    # any statistics, any channel count
    m, s = (0.5, 0.25, 0.1, 0.0), (0.5, 0.3, 1.7, 2.0)
    u = torch.arange(256, dtype=torch.uint8).repeat(4, 1).view(4, 16, 16)
    want = ((u.float() / 255) - torch.tensor(m)[:, None, None]) / torch.tensor(s)[:, None, None]
    assert torch.equal(pixels.pixel_lut(m, s).view(torch.int32), want.reshape(4, 256).view(torch.int32))


def test_set_pixel_input_arguments_and_round_trip():
    m = _model()
    assert m.pixel_input is None
    assert m.set_pixel_input() is m
    assert m.pixel_input == (pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD)
    m.set_pixel_input([0.5, 0.5, 0.5], [0.5, 0.5, 0.5])
    assert m.pixel_input == ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    for bad in (dict(mean=(0.5, 0.5), std=(0.5, 0.5)), dict(mean=(0.5,) * 4, std=(0.5,) * 4), dict(mean=(0.5,) * 3, std=(0.5, 0.5)),
                dict(mean=(0.5,) * 3, std=(0.5, 0.0, 0.5)), dict(mean=(float("nan"), 0.5, 0.5), std=(0.5,) * 3), dict(mean=0.5, std=0.5)):
        with pytest.raises(ValueError):
            m.set_pixel_input(**bad)
    assert m.pixel_input == ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))      # a refused call changes nothing
    m.set_pixel_input(None)
    assert m.pixel_input is None
    one = _model(in_chans=1)
    one.set_pixel_input((0.5,), (0.25,))
    with pytest.raises(ValueError):
        one.set_pixel_input()                                        # ImageNet statistics have three channels


def test_state_dict_keys_unchanged_and_deepcopy_keeps_the_setting():
    m = _model()
    keys = list(m.state_dict())
    m.set_pixel_input()
    assert list(m.state_dict()) == keys
    m._pixel_luts = {"cuda:0": object()}                             # per-device tables are executor state: the copy builds its own
    twin = copy.deepcopy(m)
    assert twin.pixel_input == m.pixel_input and twin._pixel_luts is None
    assert list(twin.state_dict()) == keys


def test_executor_input_formats():
    m = _model()
    x8 = torch.randint(0, 256, (2, 3, 224, 224), dtype=torch.uint8)
    xf = torch.randn(2, 3, 224, 224)
    # mode off: today's behaviour, a uint8 tensor is cast to fp32
    x, fmt, lut = m._executor_input(x8)
    assert fmt == _lib.TR_INPUT_F32 and lut is None and x.dtype == torch.float32 and torch.equal(x, x8.float())
    m.set_pixel_input()
    x, fmt, lut = m._executor_input(xf)                              # float inputs never change meaning
    assert fmt == _lib.TR_INPUT_F32 and lut is None and x.data_ptr() == xf.data_ptr()
    x, fmt, lut = m._executor_input(x8)                              # NCHW: in place
    assert fmt == _lib.TR_INPUT_U8_NCHW and x.data_ptr() == x8.data_ptr() and lut is not None
    cl = x8.contiguous(memory_format=torch.channels_last)
    x, fmt, _ = m._executor_input(cl)                                # NHWC: in place
    assert fmt == _lib.TR_INPUT_U8_NHWC and x.data_ptr() == cl.data_ptr()
    odd = x8.permute(0, 1, 3, 2)                                     # any other stride pattern: a contiguous copy
    x, fmt, _ = m._executor_input(odd)
    assert fmt == _lib.TR_INPUT_U8_NCHW and x.is_contiguous() and torch.equal(x, odd)
    m.set_pixel_input(None)
    assert m._executor_input(x8)[1] == _lib.TR_INPUT_F32
