"""Raw uint8 image input: the normalization table and the input formats of the executor.

A model switched on with `model.set_pixel_input(mean, std)` takes uint8 pixels [B, C, S, S] and normalizes them inside the kernels that
read the image.  The kernels never divide: they gather from a table the host builds here with torch's own CPU fp32 ops, in the order of
torchvision's ToTensor() + Normalize(mean, std) -- `(v / 255 - mean[c]) / std[c]` for every pixel value v -- so the normalized values are
bitwise the ones that transform produces, and everything downstream is bitwise what the fp32 input gives.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import torch

from . import _lib

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


def check_mean_std(mean: Sequence[float], std: Sequence[float], in_chans: int) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """(mean, std) as tuples of floats; ValueError unless both have `in_chans` finite entries and no std is zero."""
    try:
        mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    except TypeError as e:
        raise ValueError(f"mean and std must be sequences of {in_chans} numbers") from e
    if len(mean) != in_chans or len(std) != in_chans:
        raise ValueError(f"mean and std need {in_chans} entries (in_chans), got {len(mean)} and {len(std)}")
    if not all(math.isfinite(v) for v in mean + std) or any(v == 0.0 for v in std):
        raise ValueError(f"mean and std must be finite and std non-zero, got mean={mean} std={std}")
    return mean, std


def pixel_lut(mean: Sequence[float], std: Sequence[float]) -> torch.Tensor:
    """fp32 [C, 256] on the CPU: lut[c][v] = (v / 255 - mean[c]) / std[c], each step a torch fp32 op (ToTensor's div, Normalize's sub and
    div with per-channel fp32 tensors)."""
    m = torch.tensor(mean, dtype=torch.float32)[:, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None]
    return ((torch.arange(256).float().div(255)[None, :] - m) / s).contiguous()


def layout(img: torch.Tensor) -> int:
    """TR_LAYOUT_NCHW for a contiguous uint8 [B, C, H, W] tensor, TR_LAYOUT_NHWC for one in torch.channels_last; ValueError otherwise."""
    if img.is_contiguous():
        return _lib.TR_LAYOUT_NCHW
    if img.dim() == 4 and img.is_contiguous(memory_format=torch.channels_last):
        return _lib.TR_LAYOUT_NHWC
    raise ValueError("uint8 images must be contiguous (NCHW) or torch.channels_last (NHWC)")


def as_executor_input(x: torch.Tensor, in_chans: int) -> Tuple[torch.Tensor, int]:
    """(tensor, TR_INPUT_*) for uint8 pixels [B, C, S, S]: read in place when contiguous (NCHW) or channels_last (NHWC, 1 or 3 channels:
    what the fused patch embedding reads), otherwise -- other strides, an address off 16 bytes -- a contiguous copy."""
    x = x.detach()
    if x.is_contiguous():
        fmt = _lib.TR_INPUT_U8_NCHW
    elif in_chans in (1, 3) and x.is_contiguous(memory_format=torch.channels_last):
        fmt = _lib.TR_INPUT_U8_NHWC
    else:
        x, fmt = x.contiguous(), _lib.TR_INPUT_U8_NCHW
    if x.data_ptr() % 16:
        x, fmt = x.clone(memory_format=torch.contiguous_format), _lib.TR_INPUT_U8_NCHW
    return x, fmt
