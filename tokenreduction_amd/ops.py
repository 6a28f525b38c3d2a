"""Thin tensor-level wrappers over the C ABI (one per SURVEY.md section 8a row group).

PyTorch is plumbing here: it owns device memory and the stream; every byte of arithmetic happens
in the hand-written gfx950 kernels behind include/tokenreduction_hip.h.  All tensors must live
on a ROCm device -- there is no CPU path.

The soft-assignment backward wrappers (soft_merge_bwd, token_softmax_bwd, sinkhorn_bwd) ZERO the outputs they allocate; the kernels
write the patch rows of columns < K only (ds also a zero CLS row for those columns) and leave a caller's own output alone elsewhere.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import (TR_EPI_BF16, TR_EPI_F32, TR_EPI_GELU_BF16, TR_EPI_PATCH_F32,  # noqa: F401
                   TR_EPI_RESID_F32)


def _stream(t: torch.Tensor = None) -> int:
    """The launch stream: the current stream of the tensor's device (not of whatever device happens to be current)."""
    return torch.cuda.current_stream(None if t is None else t.device).cuda_stream


def _same_device(*tensors):
    devs = {t.device for t in tensors if t is not None}
    if len(devs) > 1:
        raise ValueError(f"operands live on different devices: {sorted(str(d) for d in devs)}")


def _dev(t: torch.Tensor, dtype, name: str) -> int:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; tokenreduction_amd has no CPU path (HIP kernels only)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _opt(t, dtype, name):
    return None if t is None else _dev(t, dtype, name)


def im2col(img: torch.Tensor, patch: int) -> torch.Tensor:
    """PatchEmbed unfold (topk.py:181): fp32 [B,C,H,W] -> bf16 [B*P, C*p*p]."""
    B, Cc, H, W = img.shape
    cols = torch.empty(B * (H // patch) * (W // patch), Cc * patch * patch, dtype=torch.bfloat16, device=img.device)
    _lib.check(_lib.load().tr_im2col_bf16(_dev(img, torch.float32, "img"), cols.data_ptr(), B, Cc, H, W, patch, _stream()),
               "tr_im2col_bf16")
    return cols


def cls_pos_rows(cls_token, pos_embed, x, B, N, D):
    _lib.check(_lib.load().tr_cls_pos_rows(_dev(cls_token, torch.float32, "cls_token"), _dev(pos_embed, torch.float32, "pos_embed"),
                                           _dev(x, torch.float32, "x"), B, N, D, _stream()), "tr_cls_pos_rows")


def patch_embed(img: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, cls_token: torch.Tensor, pos_embed: torch.Tensor, patch: int = 16) -> torch.Tensor:
    """PatchEmbed + cls_token + pos_embed in one launch (topk.py:181-186): img fp32 [B,C,H,W], w bf16 [D, C*p*p] -> x fp32 [B, P+1, D],
    P = (H/p)(W/p) row-major patches.  A square image goes through tr_patch_embed_bf16, any other through tr_patch_embed_hw_bf16."""
    B, Cc, H, W = img.shape
    D = w.shape[0]
    x = torch.empty(B, (H // patch) * (W // patch) + 1, D, dtype=torch.float32, device=img.device)
    args = (_dev(img, torch.float32, "img"), _dev(w, torch.bfloat16, "w"), _dev(bias, torch.float32, "bias"),
            _dev(cls_token, torch.float32, "cls_token"), _dev(pos_embed, torch.float32, "pos_embed"), x.data_ptr(), B, Cc)
    if H == W:
        _lib.check(_lib.load().tr_patch_embed_bf16(*args, H, patch, D, _stream()), "tr_patch_embed_bf16")
    else:
        _lib.check(_lib.load().tr_patch_embed_hw_bf16(*args, H, W, patch, D, _stream()), "tr_patch_embed_hw_bf16")
    return x


def _pixels(img: torch.Tensor, lut: torch.Tensor, C: int):
    """(image pointer, layout, LUT pointer) of uint8 pixels [B,C,H,W] (contiguous or channels_last) and their fp32 LUT [C,256]."""
    if not img.is_cuda:
        raise RuntimeError(f"img: tensor is on {img.device}; tokenreduction_amd has no CPU path (HIP kernels only)")
    if img.dtype != torch.uint8:
        raise TypeError(f"img: expected torch.uint8, got {img.dtype}")
    if tuple(lut.shape) != (C, 256):
        raise ValueError(f"lut: expected [{C}, 256], got {tuple(lut.shape)}")
    _same_device(img, lut)
    from .pixels import layout
    return img.data_ptr(), layout(img), _dev(lut, torch.float32, "lut")


def im2col_u8(img: torch.Tensor, lut: torch.Tensor, patch: int, f32: bool = False) -> torch.Tensor:
    """im2col of raw uint8 pixels (contiguous or channels_last) normalized through `lut` (pixels.pixel_lut): bf16 (f32=True: fp32)
    [B*P, C*p*p], bitwise the columns of the normalized fp32 image."""
    B, Cc, H, W = img.shape
    ptr, lay, lp = _pixels(img, lut, Cc)
    cols = torch.empty(B * (H // patch) * (W // patch), Cc * patch * patch, dtype=torch.float32 if f32 else torch.bfloat16, device=img.device)
    fn = _lib.load().tr_im2col_u8_f32 if f32 else _lib.load().tr_im2col_u8_bf16
    _lib.check(fn(ptr, lp, lay, cols.data_ptr(), B, Cc, H, W, patch, _stream(img)), "tr_im2col_u8")
    return cols


def _augment(img: torch.Tensor, table: torch.Tensor, noise: torch.Tensor):
    """(table pointer, noise pointer or None, noise length) of an augmentation table (uint8, 64 bytes per image: augment.REC_DTYPE) and
    its packed fp32 noise."""
    if table.numel() != 64 * img.shape[0]:
        raise ValueError(f"table: expected {64 * img.shape[0]} bytes (one 64-byte record per image), got {table.numel()}")
    _same_device(img, table, noise)
    return _dev(table, torch.uint8, "table"), (_dev(noise, torch.float32, "noise") if noise.numel() else None), noise.numel()


def im2col_u8_aug(img: torch.Tensor, lut: torch.Tensor, table: torch.Tensor, noise: torch.Tensor, patch: int, layout=None) -> torch.Tensor:
    """im2col_u8 with the device-side erase / mixup / cutmix of `table` (augment.py): bf16 [B*P, C*p*p], bitwise the columns of the
    augmented normalized image.  `layout` (TR_LAYOUT_*) overrides the one read off the strides (one channel: both describe the same bytes)."""
    B, Cc, H, W = img.shape
    ptr, lay, lp = _pixels(img, lut, Cc)
    lay = lay if layout is None else layout
    tp, npz, nl = _augment(img, table, noise)
    cols = torch.empty(B * (H // patch) * (W // patch), Cc * patch * patch, dtype=torch.bfloat16, device=img.device)
    _lib.check(_lib.load().tr_im2col_u8_aug_bf16(ptr, lp, lay, tp, npz, nl, cols.data_ptr(), B, Cc, H, W, patch, _stream(img)),
               "tr_im2col_u8_aug_bf16")
    return cols


def pixels_augment(img: torch.Tensor, lut: torch.Tensor, table: torch.Tensor, noise: torch.Tensor, patch: int = 8, layout=None) -> torch.Tensor:
    """The augmented, normalized image itself: uint8 pixels (contiguous or channels_last) -> fp32 [B,C,H,W] contiguous.  `patch` only
    shapes the launch (any multiple of 8 that divides H and W); `layout` as in im2col_u8_aug."""
    B, Cc, H, W = img.shape
    ptr, lay, lp = _pixels(img, lut, Cc)
    lay = lay if layout is None else layout
    tp, npz, nl = _augment(img, table, noise)
    out = torch.empty(B, Cc, H, W, dtype=torch.float32, device=img.device)
    _lib.check(_lib.load().tr_pixels_augment_f32(ptr, lp, lay, tp, npz, nl, out.data_ptr(), B, Cc, H, W, patch, _stream(img)),
               "tr_pixels_augment_f32")
    return out


def patch_embed_u8(img: torch.Tensor, lut: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, cls_token: torch.Tensor,
                   pos_embed: torch.Tensor, patch: int = 16) -> torch.Tensor:
    """patch_embed of raw uint8 pixels [B,C,H,W] (contiguous or channels_last) normalized through `lut`: bitwise patch_embed of the
    normalized image.  A square image goes through tr_patch_embed_u8_bf16, any other through tr_patch_embed_u8_hw_bf16."""
    B, Cc, H, W = img.shape
    D = w.shape[0]
    ptr, lay, lp = _pixels(img, lut, Cc)
    x = torch.empty(B, (H // patch) * (W // patch) + 1, D, dtype=torch.float32, device=img.device)
    args = (ptr, lp, lay, _dev(w, torch.bfloat16, "w"), _dev(bias, torch.float32, "bias"), _dev(cls_token, torch.float32, "cls_token"),
            _dev(pos_embed, torch.float32, "pos_embed"), x.data_ptr(), B, Cc)
    if H == W:
        _lib.check(_lib.load().tr_patch_embed_u8_bf16(*args, H, patch, D, _stream(img)), "tr_patch_embed_u8_bf16")
    else:
        _lib.check(_lib.load().tr_patch_embed_u8_hw_bf16(*args, H, W, patch, D, _stream(img)), "tr_patch_embed_u8_hw_bf16")
    return x


def gemm(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, epilogue: int, out: torch.Tensor = None,
         aux: torch.Tensor = None, aux_i: int = 0) -> torch.Tensor:
    """nn.Linear on MFMA: epilogue(a[M,K] @ w[N,K]^T + bias).  For RESID/PATCH `out` is required (updated in place)."""
    M, K = a.shape
    N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K:
        raise ValueError(f"gemm: weight is {tuple(w.shape)}, expected [N, {K}] for an activation of {tuple(a.shape)}")
    if bias.numel() != N:
        raise ValueError(f"gemm: bias has {bias.numel()} entries for {N} output columns")
    _same_device(a, w, bias, out, aux)
    if out is not None and epilogue not in (TR_EPI_PATCH_F32,) and tuple(out.shape) != (M, N):
        raise ValueError(f"gemm: out is {tuple(out.shape)}, expected {(M, N)}")
    if out is None:
        if epilogue in (TR_EPI_BF16, TR_EPI_GELU_BF16):
            out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
        elif epilogue == TR_EPI_F32:
            out = torch.empty(M, N, dtype=torch.float32, device=a.device)
        else:
            raise ValueError("this epilogue needs an explicit `out`")
    odt = torch.bfloat16 if epilogue in (TR_EPI_BF16, TR_EPI_GELU_BF16) else torch.float32
    _lib.check(_lib.load().tr_gemm_bf16(_dev(a, torch.bfloat16, "a"), _dev(w, torch.bfloat16, "w"), _dev(bias, torch.float32, "bias"),
                                        _dev(out, odt, "out"), _opt(aux, torch.float32, "aux"), aux_i, M, N, K, epilogue, _stream(a)),
               "tr_gemm_bf16")
    return out


def set_mlp_fused(mode: int) -> int:
    """Which Mlp the eval executor runs: 1 the fused launch wherever supported, 0 never, -1 (default) where its block schedule fills the chip
    (tr_set_mlp_fused; the two are bit-identical).  Process-wide, read when the launches are enqueued: a captured hipGraph keeps the mode it
    was captured with (drop `model._ws` to re-capture).  Returns the previous mode."""
    return int(_lib.load().tr_set_mlp_fused(int(mode)))


def mlp_pack(fc1_w: torch.Tensor, fc2_w: torch.Tensor, fc2_b: torch.Tensor) -> torch.Tensor:
    """Fragment-major copy of a block's Mlp weights (bf16 [Hd,D], [D,Hd]) and fc2's bias (fp32 [D]: the accumulators' start image) for
    mlp_fused; repack whenever they change."""
    Hd, D = fc1_w.shape
    if tuple(fc2_w.shape) != (D, Hd):
        raise ValueError(f"mlp_pack: fc2 weight is {tuple(fc2_w.shape)}, expected {(D, Hd)}")
    _same_device(fc1_w, fc2_w, fc2_b)
    if fc2_b.numel() != D:
        raise ValueError(f"mlp_pack: fc2 bias has {fc2_b.numel()} entries for {D} output columns")
    lib = _lib.load()
    n = lib.tr_mlp_pack_bytes(D, Hd)
    if n == 0 or not lib.tr_mlp_fused_supported(D, Hd):
        raise ValueError(f"mlp_pack: the fused Mlp kernel does not serve D={D}, Hd={Hd}")
    pk = torch.empty(n, dtype=torch.uint8, device=fc1_w.device)
    _lib.check(lib.tr_mlp_pack_bf16(_dev(fc1_w, torch.bfloat16, "fc1_w"), _dev(fc2_w, torch.bfloat16, "fc2_w"), _dev(fc2_b, torch.float32, "fc2_b"),
                                    pk.data_ptr(), D, Hd, _stream(fc1_w)), "tr_mlp_pack_bf16")
    return pk


_MLP_SCRATCH = {}


def _mlp_scratch(dev, D, Hd, streamk=True):
    """The stream-K hand-over scratch of a fused-Mlp launch on the CURRENT stream of `dev`: a scratch belongs to one launch at a time (its
    counters are zeroed in front of every launch), so launches that may overlap -- other streams -- must not share one: cached per
    (device, stream).  Returns (tensor | None, nbytes)."""
    if not streamk:
        return None, 0
    nbytes = int(_lib.load().tr_mlp_fused_scratch_bytes(D, Hd))
    if not nbytes:
        return None, 0
    with torch.cuda.device(dev):
        key = (dev, torch.cuda.current_stream().cuda_stream, nbytes)
    if key not in _MLP_SCRATCH:
        _MLP_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return _MLP_SCRATCH[key], nbytes


def mlp_fused(xn: torch.Tensor, packed: torch.Tensor, fc1_b: torch.Tensor, out: torch.Tensor = None, streamk: bool = True) -> torch.Tensor:
    """timm Mlp (fc1 -> GELU -> fc2, topk.py:95) of the eval forward in one launch: xn bf16 [M,D] -> bf16 [M,D]; bit-identical to
    gemm(GELU_BF16) followed by gemm(BF16).  streamk: give the launch its hand-over scratch (with more blocks of 128 rows than the device
    has compute units the steps are then dealt evenly over the workgroups); False: whole blocks round-robin.  Same bits."""
    M, D = xn.shape
    Hd = fc1_b.numel()
    _same_device(xn, packed, fc1_b, out)
    if out is None:
        out = torch.empty(M, D, dtype=torch.bfloat16, device=xn.device)
    scratch, nbytes = _mlp_scratch(xn.device, D, Hd, streamk)
    _lib.check(_lib.load().tr_mlp_fused_bf16(_dev(xn, torch.bfloat16, "xn"), _dev(packed, torch.uint8, "packed"), _dev(fc1_b, torch.float32, "fc1_b"),
                                             _dev(out, torch.bfloat16, "out"),
                                             None if scratch is None else scratch.data_ptr(), nbytes, M, D, Hd, _stream(xn)),
               "tr_mlp_fused_bf16")
    return out


def set_mlp_ln(mode: int) -> int:
    """Where the eval executor runs a lazy norm2 INSIDE the fused Mlp launch that follows it (mlp_fused_ln) instead of as its own LayerNorm
    launch -- the two are bit-identical: 1 (default) where that launch is one round of whole blocks and in every launch of a forward that
    runs beside others (model.forward_async: whole-block launches), 2 wherever the fused Mlp runs, 0 never.
    Process-wide, read when the launches are enqueued: a captured hipGraph keeps the form it was captured with (drop `model._ws` to
    re-capture).  Returns the previous setting."""
    return int(_lib.load().tr_set_mlp_ln(int(mode)))


def set_cls_tail(on: bool) -> bool:
    """Whether the eval executor (bf16) runs the LAST block's work after its attention -- proj, norm2, fc1, fc2 -- on the B CLS rows only, with
    the attention computing the CLS query alone (attention_cls): the only rows the final norm and the head read.  On by default; off: the
    full-width block.  Bit-identical.  Blocks that reduce from the attention onward, viz_mode and the fp32 / bf16x3 executors always run
    full width.  Process-wide, read when the launches are enqueued: a captured hipGraph keeps the form it was captured with (drop
    `model._ws` to re-capture).  Returns the previous setting."""
    return bool(_lib.load().tr_set_cls_tail(1 if on else 0))


def attention_cls(qkv: torch.Tensor, B: int, N: int, H: int, size: torch.Tensor = None) -> torch.Tensor:
    """Row 0 of every image of attention(qkv, B, N, H, size=size)[0], bit for bit, computing the first query block only -> bf16 [B, H*64]."""
    out = torch.empty(B, H * 64, dtype=torch.bfloat16, device=qkv.device)
    _lib.check(_lib.load().tr_attention_cls_bf16(_dev(qkv, torch.bfloat16, "qkv"), out.data_ptr(), _opt(size, torch.float32, "size"), B, N, H,
                                                 _stream()), "tr_attention_cls_bf16")
    return out


def mlp_fused_ln(x: torch.Tensor, delta: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, packed: torch.Tensor,
                 fc1_b: torch.Tensor, out: torch.Tensor = None, streamk: bool = True) -> torch.Tensor:
    """topk.py:95's `self.mlp(self.norm2(x))` in one launch: Mlp(LayerNorm(x + delta)) with x the fp32 stream [M,D] and delta the pending
    bf16 attention residual [M,D] (neither is written) -> bf16 [M,D].  Bit-identical to layernorm2 (no write-back) followed by mlp_fused."""
    M, D = x.shape
    Hd = fc1_b.numel()
    _same_device(x, delta, gamma, beta, packed, fc1_b, out)
    if tuple(delta.shape) != (M, D) or not x.is_contiguous() or not delta.is_contiguous():
        raise ValueError(f"mlp_fused_ln: x {tuple(x.shape)} and delta {tuple(delta.shape)} must be contiguous [M, D]")
    if out is None:
        out = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
    scratch, nbytes = _mlp_scratch(x.device, D, Hd, streamk)
    _lib.check(_lib.load().tr_mlp_fused_ln_bf16(_dev(x, torch.float32, "x"), _dev(delta, torch.bfloat16, "delta"), _dev(gamma, torch.float32, "gamma"),
                                                _dev(beta, torch.float32, "beta"), float(eps), _dev(packed, torch.uint8, "packed"),
                                                _dev(fc1_b, torch.float32, "fc1_b"), _dev(out, torch.bfloat16, "out"),
                                                None if scratch is None else scratch.data_ptr(), nbytes, M, D, Hd, _stream(x)),
               "tr_mlp_fused_ln_bf16")
    return out


def mlp_fused_status(dev=None, D: int = 384, Hd: int = 1536) -> None:
    """Status check of the fused-Mlp launches of the current stream of `dev` that went through this module's scratch: waits for the stream and
    raises if a stream-K hand-over poll ran out in one of them (tr_mlp_fused_status; the record is cleared)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    scratch, nbytes = _mlp_scratch(dev, D, Hd, True)
    if scratch is None:
        return
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tr_mlp_fused_status(scratch.data_ptr(), nbytes, D, Hd, torch.cuda.current_stream().cuda_stream),
                   "tr_mlp_fused_status")


def set_mlp_poll_max(iterations: int) -> int:
    """Bound of the stream-K hand-over poll (iterations of an 8-tick sleep; default 2^24: seconds).  Tests shorten it.  Returns the previous bound."""
    return int(_lib.load().tr_set_mlp_poll_max(int(iterations)))


_LNLIN_SCRATCH = {}


def lnlin_pack(w: torch.Tensor) -> torch.Tensor:
    """Fragment-major copy of an nn.Linear weight [N, 384] (bf16) for lnlin; repack whenever it changes."""
    N, D = w.shape
    lib = _lib.load()
    n = int(lib.tr_lnlin_pack_bytes(D, N))
    if n == 0:
        raise ValueError(f"lnlin_pack: the LayerNorm + Linear kernel does not serve D={D}, N={N}")
    pk = torch.empty(n, dtype=torch.uint8, device=w.device)
    _lib.check(lib.tr_lnlin_pack_bf16(_dev(w, torch.bfloat16, "w"), pk.data_ptr(), D, N, _stream(w)), "tr_lnlin_pack_bf16")
    return pk


def lnlin(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, packed: torch.Tensor, bias: torch.Tensor,
          d1: torch.Tensor = None, d2: torch.Tensor = None, out: torch.Tensor = None):
    """The start of a block in one launch (topk.py:86-87 norm1 + :44 qkv): v = (x [+ d1]) [+ d2]; returns (out bf16 [M,N] =
    LayerNorm(v) @ W^T + bias, x_out = v as a NEW fp32 tensor, or None when nothing was pending).  Bit-identical to layernorm / layernorm2
    followed by gemm(TR_EPI_BF16)."""
    M, D = x.shape
    N = bias.numel()
    _same_device(x, gamma, beta, packed, bias, d1, d2, out)
    if not x.is_contiguous() or (d1 is not None and not d1.is_contiguous()) or (d2 is not None and not d2.is_contiguous()):
        raise ValueError("lnlin: x, d1, d2 must be contiguous [M, D]")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    x_out = torch.empty_like(x) if d1 is not None else None
    lib = _lib.load()
    nbytes = int(lib.tr_lnlin_scratch_bytes(D, N))
    with torch.cuda.device(x.device):
        key = (x.device, torch.cuda.current_stream().cuda_stream, nbytes)
    if key not in _LNLIN_SCRATCH:
        _LNLIN_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    scratch = _LNLIN_SCRATCH[key]
    _lib.check(lib.tr_lnlin_bf16(_dev(x, torch.float32, "x"), _opt(d1, torch.bfloat16, "d1"), _opt(d2, torch.bfloat16, "d2"),
                                 None if x_out is None else x_out.data_ptr(), _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"),
                                 float(eps), _dev(packed, torch.uint8, "packed"), _dev(bias, torch.float32, "bias"), _dev(out, torch.bfloat16, "out"),
                                 scratch.data_ptr(), nbytes, M, D, N, _stream(x)), "tr_lnlin_bf16")
    return out, x_out


def set_mlp_resid_ln(on: bool) -> bool:
    """Whether the eval executor fuses the block tail (Mlp + residual add + the next block's norm1) into one launch where it can, or keeps
    the fused Mlp and the LayerNorm launch apart (default: the one-launch form measured 4 % slower in the model).  Process-wide, read when
    the launches are enqueued: a captured hipGraph keeps the form it was captured with (drop `model._ws` to re-capture).  Returns the
    previous setting."""
    return bool(_lib.load().tr_set_mlp_resid_ln(1 if on else 0))


def mlp_fused_resid_ln(xn: torch.Tensor, packed: torch.Tensor, fc1_b: torch.Tensor, fc2_b: torch.Tensor, x: torch.Tensor, next_g: torch.Tensor,
                       next_b: torch.Tensor, eps: float, xn_next: torch.Tensor = None, streamk: bool = True) -> torch.Tensor:
    """Block tail + next block's norm1 in one launch (topk.py:95, then :87): x (fp32 [M,D], updated IN PLACE) += Mlp(xn) and
    returns LayerNorm(x; next_g, next_b, eps) as bf16 [M,D]."""
    M, D = xn.shape
    Hd = fc1_b.numel()
    _same_device(xn, packed, fc1_b, fc2_b, x, next_g, next_b, xn_next)
    if tuple(x.shape) != (M, D) or not x.is_contiguous():
        raise ValueError(f"mlp_fused_resid_ln: x is {tuple(x.shape)}, expected contiguous {(M, D)}")
    if xn_next is None:
        xn_next = torch.empty(M, D, dtype=torch.bfloat16, device=xn.device)
    lib = _lib.load()
    scratch, nbytes = _mlp_scratch(xn.device, D, Hd, streamk)
    _lib.check(lib.tr_mlp_fused_resid_ln_bf16(_dev(xn, torch.bfloat16, "xn"), _dev(packed, torch.uint8, "packed"), _dev(fc1_b, torch.float32, "fc1_b"),
                                              _dev(fc2_b, torch.float32, "fc2_b"), _dev(x, torch.float32, "x"), _dev(next_g, torch.float32, "next_g"),
                                              _dev(next_b, torch.float32, "next_b"), float(eps), _dev(xn_next, torch.bfloat16, "xn_next"),
                                              None if scratch is None else scratch.data_ptr(), nbytes, M, D, Hd,
                                              _stream(xn)), "tr_mlp_fused_resid_ln_bf16")
    return xn_next


def _ln_out(y, shape, dtype, name: str, dev) -> torch.Tensor:
    """A forward LayerNorm's output: a fresh tensor, or the caller's own contiguous one (a slice of a larger buffer: what lies around it
    can be watched)."""
    if y is None:
        return torch.empty(*shape, dtype=dtype, device=dev)
    if tuple(y.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(y.shape)}")
    _dev(y, dtype, name)
    return y


def _ln_rows(t, dtype, name: str, ld: int = None):
    """(pointer, row stride) of a LayerNorm row operand, or (None, 0): contiguous, or a 2-D column slice of a wider tensor whose row stride is
    taken from the view; `ld` overrides the stride told to the C ABI."""
    if t is None:
        return None, 0 if ld is None else ld
    if t.dim() == 2 and t.stride(1) == 1 and t.is_cuda and t.dtype == dtype:
        p, s = t.data_ptr(), t.stride(0)
    else:
        p, s = _dev(t, dtype, name), t.shape[-1]
    return p, s if ld is None else ld


def layernorm(x: torch.Tensor, gamma, beta, eps: float, rows: int = None, ldx: int = None, delta: torch.Tensor = None,
              ldd: int = None, y: torch.Tensor = None) -> torch.Tensor:
    """[x += delta (bf16, written back);] nn.LayerNorm over the last dim of fp32 x -> bf16 [M,D]
    (optionally only `rows` rows at stride ldx / ldd).  y: the caller's own bf16 [M,D] output."""
    D = x.shape[-1]
    M = rows if rows is not None else x.numel() // D
    ld = ldx if ldx is not None else D
    y = _ln_out(y, (M, D), torch.bfloat16, "y", x.device)
    _lib.check(_lib.load().tr_layernorm_bf16(_dev(x, torch.float32, "x"), ld, _opt(delta, torch.bfloat16, "delta"),
                                             ldd if ldd is not None else D, _dev(gamma, torch.float32, "gamma"),
                                             _dev(beta, torch.float32, "beta"), y.data_ptr(), M, D, eps, _stream()),
               "tr_layernorm_bf16")
    return y


def attention(qkv: torch.Tensor, B: int, N: int, H: int, want_cls: bool = False, size: torch.Tensor = None,
              colsum_part: torch.Tensor = None):
    """softmax(q k^T / 8) v per (image, head) (topk.py:44-51).  qkv bf16 [B*N, 3*H*64] -> (out bf16 [B*N, H*64], cls_rows|None)."""
    out = torch.empty(B * N, H * 64, dtype=torch.bfloat16, device=qkv.device)
    cls_rows = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device) if want_cls else None
    _lib.check(_lib.load().tr_attention_bf16(_dev(qkv, torch.bfloat16, "qkv"), out.data_ptr(),
                                             None if cls_rows is None else cls_rows.data_ptr(), _opt(size, torch.float32, "size"),
                                             _opt(colsum_part, torch.float32, "colsum_part"), B, N, H, _stream()),
               "tr_attention_bf16")
    return out, cls_rows


def cls_topk(cls_rows: torch.Tensor, K: int, want_compl: bool = False):
    """Top-K over head-mean CLS attention (topk.py:59-61) -> (idx int32 [B,K], compl int32 [B,P-K]|None, scores fp32 [B,P])."""
    B, H, N = cls_rows.shape
    P = N - 1
    idx = torch.empty(B, K, dtype=torch.int32, device=cls_rows.device)
    compl = torch.empty(B, P - K, dtype=torch.int32, device=cls_rows.device) if want_compl else None
    scores = torch.empty(B, P, dtype=torch.float32, device=cls_rows.device)
    _lib.check(_lib.load().tr_cls_topk(_dev(cls_rows, torch.float32, "cls_rows"), idx.data_ptr(),
                                       None if compl is None else compl.data_ptr(), scores.data_ptr(), B, H, N, K, _stream()),
               "tr_cls_topk")
    return idx, compl, scores


def gather_layernorm(x: torch.Tensor, idx, compl, scores, gamma, beta, eps: float, delta: torch.Tensor = None, x_out: torch.Tensor = None,
                     y: torch.Tensor = None, f32: bool = False):
    """Top-K gather/compact (topk.py:89-93) [+ EViT fused token evit.py:111-123] fused with norm2.
    With delta (bf16 [B,N,D], pending attn.proj output) the gather reads x + delta.
    x fp32 [B,N,D] -> (x_out fp32 [B,N_out,D], y bf16 [B,N_out,D]).  idx None: the plain LayerNorm of all N rows through the gather kernel
    (x_out None unless the caller passes one).  x_out / y: the caller's own outputs.  f32: tr_gather_layernorm_f32 (fp32 delta and y).
    compl of shape [B, 0] (everything kept, K = N - 1) still asks for the fused row: an empty weighted sum, exactly zero."""
    B, N, D = x.shape
    ydt, ddt = (torch.float32, torch.float32) if f32 else (torch.bfloat16, torch.bfloat16)
    if idx is None:
        if compl is not None:
            raise ValueError("gather_layernorm: compl without idx")
        K, N_out, pidx, pcompl = 0, N, None, None
        if x_out is not None:
            x_out = _ln_out(x_out, (B, N_out, D), torch.float32, "x_out", x.device)
    else:
        K = idx.shape[1]
        N_out = K + 1 + (1 if compl is not None else 0)
        pidx, pcompl = _dev(idx, torch.int32, "idx"), None
        if compl is not None:
            if tuple(compl.shape) != (B, N - 1 - K):
                raise ValueError(f"gather_layernorm: compl is {tuple(compl.shape)}, expected {(B, N - 1 - K)}")
            # the C ABI reads "fuse" from compl_idx != NULL, and an empty tensor has no storage (data_ptr() == 0): hand over idx's pointer,
            # of which the kernel reads no element when the complement is empty
            pcompl = _dev(compl, torch.int32, "compl") if compl.numel() else pidx
        x_out = _ln_out(x_out, (B, N_out, D), torch.float32, "x_out", x.device)
    y = _ln_out(y, (B, N_out, D), ydt, "y", x.device)
    lib = _lib.load()
    fn, what = (lib.tr_gather_layernorm_f32, "tr_gather_layernorm_f32") if f32 else (lib.tr_gather_layernorm_bf16, "tr_gather_layernorm_bf16")
    _lib.check(fn(_dev(x, torch.float32, "x"), _opt(delta, ddt, "delta"), pidx, pcompl,
                  _opt(scores, torch.float32, "scores"), _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"),
                  None if x_out is None else x_out.data_ptr(), y.data_ptr(), B, N, K, D, eps, _stream()), what)
    return x_out, y


# ---------------------------------------------------------------------------------------- fp32 validation path
def gemm_f32(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, epilogue: int = TR_EPI_F32, out: torch.Tensor = None,
             aux: torch.Tensor = None, aux_i: int = 0, split: bool = False) -> torch.Tensor:
    """nn.Linear in the reference's arithmetic (fp32 operands): epilogue TR_EPI_F32 | TR_EPI_GELU_BF16 (GELU, fp32 out) | PATCH.
    split=True: the same Linear as split-bf16 (hi/lo) products on the matrix cores (TR_PREC_BF16X3)."""
    M, K = a.shape
    N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K:
        raise ValueError(f"gemm: weight is {tuple(w.shape)}, expected [N, {K}] for an activation of {tuple(a.shape)}")
    if bias.numel() != N:
        raise ValueError(f"gemm: bias has {bias.numel()} entries for {N} output columns")
    _same_device(a, w, bias, out, aux)
    if out is not None and epilogue not in (TR_EPI_PATCH_F32,) and tuple(out.shape) != (M, N):
        raise ValueError(f"gemm: out is {tuple(out.shape)}, expected {(M, N)}")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    fn = _lib.load().tr_gemm_split if split else _lib.load().tr_gemm_f32
    _lib.check(fn(_dev(a, torch.float32, "a"), _dev(w, torch.float32, "w"), _dev(bias, torch.float32, "bias"),
                  _dev(out, torch.float32, "out"), _opt(aux, torch.float32, "aux"), aux_i, M, N, K, epilogue, _stream()),
               "tr_gemm_split" if split else "tr_gemm_f32")
    return out


def layernorm2(x: torch.Tensor, gamma, beta, eps: float, delta: torch.Tensor, delta2: torch.Tensor = None, write_x: bool = True,
               y: torch.Tensor = None, x_out: torch.Tensor = None, rows: int = None, ldx: int = None, ldxo: int = None, ldd: int = None,
               ldd2: int = None) -> torch.Tensor:
    """y = LayerNorm((x + delta) + delta2) -> bf16 [M,D]; the sum is written back to x unless write_x is False (tr_layernorm2_bf16:
    the eval executor's norm2 without a stream write, and the norm1 that absorbs both pending residuals after it).
    y: the caller's own output; x_out: the sum goes there and x is not written; x, x_out, delta and delta2 may be 2-D column slices
    (their row stride is told to the C ABI; ldx / ldxo / ldd / ldd2 override it); rows: only that many rows."""
    D = x.shape[-1]
    M = rows if rows is not None else x.numel() // D
    y = _ln_out(y, (M, D), torch.bfloat16, "y", x.device)
    xp, sx = _ln_rows(x, torch.float32, "x", ldx)
    if x_out is not None:
        if not write_x:
            raise ValueError("layernorm2: x_out together with write_x=False")
        po, so = _ln_rows(x_out, torch.float32, "x_out", ldxo)
    else:
        po, so = (xp, sx if ldxo is None else ldxo) if write_x else (None, D if ldxo is None else ldxo)
    pd, sd = _ln_rows(delta, torch.bfloat16, "delta", ldd)
    pd2, sd2 = _ln_rows(delta2, torch.bfloat16, "delta2", ldd2) if delta2 is not None else (None, D if ldd2 is None else ldd2)
    _lib.check(_lib.load().tr_layernorm2_bf16(xp, sx, po, so, pd, sd, pd2, sd2, _dev(gamma, torch.float32, "gamma"),
                                              _dev(beta, torch.float32, "beta"), y.data_ptr(), M, D, eps, _stream()), "tr_layernorm2_bf16")
    return y


def layernorm_f32(x: torch.Tensor, gamma, beta, eps: float, delta: torch.Tensor = None, y: torch.Tensor = None, rows: int = None,
                  ldx: int = None, ldd: int = None) -> torch.Tensor:
    """tr_layernorm_f32: [x += delta (fp32, written back);] LayerNorm in the reference's arithmetic -> fp32 [M,D].  y: the caller's own
    output; x and delta may be 2-D column slices (ldx / ldd override the row stride); rows: only that many rows."""
    D = x.shape[-1]
    M = rows if rows is not None else x.numel() // D
    y = _ln_out(y, (M, D), torch.float32, "y", x.device)
    xp, sx = _ln_rows(x, torch.float32, "x", ldx)
    pd, sd = _ln_rows(delta, torch.float32, "delta", ldd) if delta is not None else (None, D if ldd is None else ldd)
    _lib.check(_lib.load().tr_layernorm_f32(xp, sx, pd, sd, _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"),
                                            y.data_ptr(), M, D, eps, _stream()), "tr_layernorm_f32")
    return y


def _pending(d, name):
    """Pointer of a pending residual operand (bf16 or fp32 rows) or None."""
    if d is None:
        return None
    if d.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"{name}: expected bf16 or fp32, got {d.dtype}")
    return _dev(d, d.dtype, name)


def _pending_f32(d1, d2):
    if d1 is not None and d2 is not None and d1.dtype != d2.dtype:
        raise TypeError("the two pending operands must have one dtype")
    return int(d1 is not None and d1.dtype == torch.float32)


def cls_tap(x: torch.Tensor, ldx: int, B: int, D: int, d1: torch.Tensor = None, ld1: int = 0, d2: torch.Tensor = None, ld2: int = 0,
            out: torch.Tensor = None, ldo: int = None, offset: int = 0) -> torch.Tensor:
    """out[b] = (x[b] + d1[b]) + d2[b] for B rows of D at their own strides (tr_cls_tap): x fp32 rows at ldx, the pending operands (bf16 or
    fp32, both nullable) at ld1 / ld2, the destination rows at ldo starting `offset` elements into `out` (fp32; allocated [B, D] if None)."""
    _same_device(x, d1, d2, out)
    if out is None:
        out, ldo, offset = torch.empty(B, D, dtype=torch.float32, device=x.device), D, 0
    _lib.check(_lib.load().tr_cls_tap(_dev(x, torch.float32, "x"), ldx, _pending(d1, "d1"), ld1, _pending(d2, "d2"), ld2, _pending_f32(d1, d2),
                                      _dev(out, torch.float32, "out") + 4 * offset, D if ldo is None else ldo, B, D, _stream(x)), "tr_cls_tap")
    return out


def final_tokens_f32(x: torch.Tensor, gamma, beta, eps: float, d1: torch.Tensor = None, d2: torch.Tensor = None) -> torch.Tensor:
    """y = LayerNorm((x + d1) + d2) over fp32 rows [M, D] in fp32 arithmetic, one pass (tr_final_tokens_f32): d1 / d2 bf16 or fp32 rows
    [M, D], both nullable; x is not written.  Bit for bit layernorm_f32 of the fp32 sums."""
    _same_device(x, d1, d2, gamma, beta)
    D = x.shape[-1]
    M = x.numel() // D
    y = torch.empty(M, D, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().tr_final_tokens_f32(_dev(x, torch.float32, "x"), _pending(d1, "d1"), _pending(d2, "d2"), _pending_f32(d1, d2),
                                               _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"), y.data_ptr(), M, D, eps,
                                               _stream(x)), "tr_final_tokens_f32")
    return y


def _pool_weight(weight, B, N):
    if weight is not None and tuple(weight.shape) != (B, N):
        raise ValueError(f"weight must be [B, N] = [{B}, {N}] (entry 0, the CLS token's, is not read), got {tuple(weight.shape)}")
    return _opt(weight, torch.float32, "weight")


def token_pool(x: torch.Tensor, d1: torch.Tensor = None, d2: torch.Tensor = None, weight: torch.Tensor = None) -> torch.Tensor:
    """out fp32 [B, D] = sum_n w[b,n] v[b,n] / sum_n w[b,n] over the patch rows n = 1 .. N-1 of v = (x + d1) + d2 (tr_token_pool): x fp32
    [B, N, D], the pending operands bf16 or fp32 [B, N, D] (both nullable), weight fp32 [B, N] or None (all ones).  Row 0 (CLS) is left out;
    an image whose weights sum to 0 pools to zeros.  Deterministic: the same bits on every launch and in any batch."""
    _same_device(x, d1, d2, weight)
    B, N, D = x.shape
    for d, name in ((d1, "d1"), (d2, "d2")):
        if d is not None and d.shape != x.shape:
            raise ValueError(f"{name} must have x's shape {tuple(x.shape)}, got {tuple(d.shape)}")
    out = torch.empty(B, D, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().tr_token_pool(_dev(x, torch.float32, "x"), _pending(d1, "d1"), _pending(d2, "d2"), _pending_f32(d1, d2),
                                         _pool_weight(weight, B, N), out.data_ptr(), B, N, D, _stream(x)), "tr_token_pool")
    return out


def token_pool_bwd(gpool: torch.Tensor, N: int, weight: torch.Tensor = None, out: torch.Tensor = None) -> torch.Tensor:
    """g fp32 [B, N, D]: g[b,0] = 0, g[b,n] = gpool[b] * (w[b,n] / sum_n w[b,n]) (tr_token_pool_bwd), the gradient of token_pool with
    respect to x (and to each pending operand) for gpool fp32 [B, D]; every element of g is written (out: a buffer to write into)."""
    _same_device(gpool, weight, out)
    B, D = gpool.shape
    g = torch.empty(B, N, D, dtype=torch.float32, device=gpool.device) if out is None else out
    if tuple(g.shape) != (B, N, D):
        raise ValueError(f"out must be [B, N, D] = [{B}, {N}, {D}], got {tuple(g.shape)}")
    _lib.check(_lib.load().tr_token_pool_bwd(_dev(gpool, torch.float32, "gpool"), _pool_weight(weight, B, N), _dev(g, torch.float32, "out"),
                                             B, N, D, _stream(gpool)), "tr_token_pool_bwd")
    return g


def decision_table(stages, B: int):
    """tr_stage_decisions' host table for `stages` [(blk, _lib.TR_DECISION_* kind, n_in, k)] at batch size B, its outputs laid out back to
    back: (ctypes table, [(blk, n_in, W, kept_off, A, assign_off)], kept elements, assign elements, soft elements) -- W / A: width of the
    stage's kept rows / assignment rows, 0 where it has none."""
    table = (_lib.TrDecisionStage * max(1, len(stages)))()
    layout, kept_n, assign_n, soft_n = [], 0, 0, 0
    for i, (blk, kind, n_in, k) in enumerate(stages):
        W = max(0, {_lib.TR_DECISION_PRUNE: k, _lib.TR_DECISION_CENTRES: k, _lib.TR_DECISION_EVIT: k + 1, _lib.TR_DECISION_ATS: k - 1}.get(kind, 0))
        A = max(0, n_in - 1) if kind in (_lib.TR_DECISION_CENTRES, _lib.TR_DECISION_TOME, _lib.TR_DECISION_SOFT) else 0
        table[i] = _lib.TrDecisionStage(blk, kind, n_in, k, kept_n, assign_n, soft_n)
        layout.append((blk, n_in, W, kept_n, A, assign_n))
        kept_n += B * W
        assign_n += B * A
        if kind == _lib.TR_DECISION_SOFT:
            soft_n += B * max(0, k) * max(0, n_in - 1)
    return table, layout, kept_n, assign_n, soft_n


def stage_decisions(kept_idx: torch.Tensor, compl_idx: torch.Tensor, soft: torch.Tensor, stages, B: int, N0: int) -> dict:
    """The raw stage slabs of an eval forward -> record-form decisions (tr_stage_decisions, one launch): kept_idx / compl_idx int32 slabs
    (block blk at blk * B * N0; compl_idx nullable), soft fp32 (the SOFT stages' [B, k, P] blocks back to back; nullable), stages
    [(blk, _lib.TR_DECISION_* kind, n_in, k)] in block order.  Returns {"stages", "kept": {blk: int32 [B, W]}, "kept_count": {blk: int32 [B]},
    "assign": {blk: int32 [B, P]}} -- what VisionTransformer.forward_decisions returns."""
    _same_device(kept_idx, compl_idx, soft)
    if compl_idx is not None and compl_idx.numel() != kept_idx.numel():
        raise ValueError("kept_idx and compl_idx are slabs of one shape")
    dev = kept_idx.device
    table, layout, kept_n, assign_n, _ = decision_table(stages, B)
    kept = torch.empty(max(1, kept_n), dtype=torch.int32, device=dev)
    assign = torch.empty(max(1, assign_n), dtype=torch.int32, device=dev)
    count = torch.empty(max(1, len(stages) * B), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tr_stage_decisions(_dev(kept_idx, torch.int32, "kept_idx"), _opt(compl_idx, torch.int32, "compl_idx"), kept_idx.numel(),
                                              _opt(soft, torch.float32, "soft"), 0 if soft is None else soft.numel(), table, len(stages), B, N0,
                                              kept.data_ptr(), kept_n, count.data_ptr(), assign.data_ptr(), assign_n, _stream(kept_idx)),
               "tr_stage_decisions")
    out = {"stages": tuple(lay[0] for lay in layout), "kept": {}, "kept_count": {}, "assign": {}}
    for i, (blk, _, W, koff, A, aoff) in enumerate(layout):
        if W:
            out["kept"][blk] = kept[koff: koff + B * W].view(B, W)
            out["kept_count"][blk] = count[i * B: (i + 1) * B]
        if A:
            out["assign"][blk] = assign[aoff: aoff + B * A].view(B, A)
    return out


def dense_index(kept: torch.Tensor, assign: torch.Tensor, stages, B: int, P0: int, n_last: int, table=None, out: torch.Tensor = None) -> torch.Tensor:
    """index int32 [B, P0]: the row of the last stream (1 ... n_last-1) that stands for grid patch p, -1 where none does (tr_dense_index, one
    launch).  kept / assign: the flat int32 buffers tr_stage_decisions wrote for `stages` [(blk, _lib.TR_DECISION_* kind, n_in, k)] laid out
    by decision_table (either may be None where no stage has one); `table`: that ctypes table, built here when None.  No stage: the identity."""
    _same_device(kept, assign, out)
    if table is None:
        table = decision_table(stages, B)[0]
    if out is None:
        dev = next((t.device for t in (kept, assign) if t is not None), torch.device("cuda", torch.cuda.current_device()))
        out = torch.empty(B, P0, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tr_dense_index(_opt(kept, torch.int32, "kept"), 0 if kept is None else kept.numel(), _opt(assign, torch.int32, "assign"),
                                          0 if assign is None else assign.numel(), table, len(stages), B, P0, n_last,
                                          _dev(out, torch.int32, "out"), _stream(out)), "tr_dense_index")
    return out


DENSE_LAYOUTS = {"NCHW": _lib.TR_LAYOUT_NCHW, "NHWC": _lib.TR_LAYOUT_NHWC}


def dense_gather(tokens: torch.Tensor, index: torch.Tensor, layout: str = "NCHW", dtype=torch.float32, fill: float = 0.0,
                 out: torch.Tensor = None) -> torch.Tensor:
    """features[b, :, p] = tokens[b, index[b, p], :] where 0 <= index < n_rows, `fill` elsewhere (tr_dense_gather, one launch): tokens fp32
    [B, n_rows, D], index int32 [B, P]; the result is [B, D, P] (layout "NCHW") or [B, P, D] ("NHWC"), fp32 or bf16 (round to nearest even).
    Every element of the result is written once."""
    _same_device(tokens, index, out)
    if layout not in DENSE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(DENSE_LAYOUTS)}, got {layout!r}")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, got {dtype}")
    B, n_rows, D = tokens.shape
    P = index.shape[1]
    if index.shape[0] != B:
        raise ValueError(f"index must be [B, P] with B = {B}, got {tuple(index.shape)}")
    shape = (B, D, P) if layout == "NCHW" else (B, P, D)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=tokens.device)
    elif out.numel() != B * D * P:
        raise ValueError(f"out must hold {B * D * P} elements, got {out.numel()}")
    _lib.check(_lib.load().tr_dense_gather(_dev(tokens, torch.float32, "tokens"), _dev(index, torch.int32, "index"), _dev(out, dtype, "out"),
                                           DENSE_LAYOUTS[layout], int(dtype == torch.bfloat16), float(fill), B, P, n_rows, D, _stream(tokens)),
               "tr_dense_gather")
    return out.view(shape)


def dense_scatter(dmap: torch.Tensor, index: torch.Tensor, n_rows: int, layout: str = "NCHW", dtype=torch.float32,
                  out: torch.Tensor = None) -> torch.Tensor:
    """The adjoint of dense_gather (tr_dense_scatter, one launch): dtokens[b, r, :] = the sum of dmap[b, :, p] over the patches p with
    index[b, p] == r, 0 <= r < n_rows.  dmap [B, D, P] (layout "NCHW") or [B, P, D] ("NHWC"), fp32 or bf16; index int32 [B, P]; the result is
    [B, n_rows, D], fp32 or bf16 (`dtype`: the fp32 sum rounded once, to nearest even).  The sum is in fp32, in ascending p; a row no patch
    names is zero; an index entry outside [0, n_rows) owns nothing.  Every element of the result is written once, the same bits every time."""
    _same_device(dmap, index, out)
    if layout not in DENSE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(DENSE_LAYOUTS)}, got {layout!r}")
    if dtype not in (torch.float32, torch.bfloat16) or dmap.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"dmap and dtype must be torch.float32 or torch.bfloat16, got {dmap.dtype} and {dtype}")
    if dmap.dim() != 3 or index.dim() != 2 or index.shape[0] != dmap.shape[0]:
        raise ValueError(f"dmap must be [B, D, P] / [B, P, D] and index [B, P], got {tuple(dmap.shape)} and {tuple(index.shape)}")
    B, P = index.shape
    D = dmap.shape[1] if layout == "NCHW" else dmap.shape[2]
    if dmap.numel() != B * D * P:
        raise ValueError(f"dmap {tuple(dmap.shape)} does not hold [B, D, P] = [{B}, {D}, {P}] in layout {layout}")
    if out is None:
        out = torch.empty(B, n_rows, D, dtype=dtype, device=dmap.device)
    elif out.numel() != B * n_rows * D:
        raise ValueError(f"out must hold {B * n_rows * D} elements, got {out.numel()}")
    _lib.check(_lib.load().tr_dense_scatter(_dev(dmap, dmap.dtype, "dmap"), _dev(index, torch.int32, "index"), _dev(out, dtype, "out"),
                                            DENSE_LAYOUTS[layout], int(dmap.dtype == torch.bfloat16), int(dtype == torch.bfloat16), B, P,
                                            int(n_rows), D, _stream(dmap)), "tr_dense_scatter")
    return out.view(B, n_rows, D)


def _level_array(values, what):
    vals = [int(v) for v in values]
    if not 1 <= len(vals) <= _lib.TR_MAX_DEPTH:
        raise ValueError(f"{what}: {len(vals)} levels (1 ... {_lib.TR_MAX_DEPTH})")
    return (ctypes.c_int32 * len(vals))(*vals)


def dense_index_levels(kept: torch.Tensor, assign: torch.Tensor, stages, B: int, P0: int, level_blocks, level_rows, table=None,
                       out: torch.Tensor = None) -> torch.Tensor:
    """index int32 [L, B, P0]: per level l -- the stream after block level_blocks[l], level_rows[l] tokens with the CLS token -- the row
    (1 ... level_rows[l]-1) that stands for grid patch p, -1 where none does (tr_dense_index_levels, one launch for all levels).  Level l sits
    behind the stages with block <= level_blocks[l]; a level in front of every stage is the identity.  kept / assign / stages / table as
    dense_index; level_blocks strictly ascending."""
    _same_device(kept, assign, out)
    if len(level_blocks) != len(level_rows):
        raise ValueError(f"{len(level_blocks)} level blocks, {len(level_rows)} level rows")
    blocks, rows = _level_array(level_blocks, "level_blocks"), _level_array(level_rows, "level_rows")
    L = len(blocks)
    if table is None:
        table = decision_table(stages, B)[0]
    if out is None:
        dev = next((t.device for t in (kept, assign) if t is not None), torch.device("cuda", torch.cuda.current_device()))
        out = torch.empty(L, B, P0, dtype=torch.int32, device=dev)
    elif out.numel() != L * B * P0:
        raise ValueError(f"out must hold {L * B * P0} elements, got {out.numel()}")
    _lib.check(_lib.load().tr_dense_index_levels(_opt(kept, torch.int32, "kept"), 0 if kept is None else kept.numel(),
                                                 _opt(assign, torch.int32, "assign"), 0 if assign is None else assign.numel(), table, len(stages),
                                                 B, P0, blocks, rows, L, _dev(out, torch.int32, "out"), _stream(out)), "tr_dense_index_levels")
    return out.view(L, B, P0)


def dense_gather_levels(tokens: torch.Tensor, level_stride: int, level_rows, index: torch.Tensor, D: int, layout: str = "NCHW",
                        dtype=torch.float32, fill: float = 0.0, out: torch.Tensor = None) -> torch.Tensor:
    """features[l][b, :, p] = the row index[l, b, p] of level l's tokens where 0 <= index < level_rows[l], `fill` elsewhere
    (tr_dense_gather_levels, one launch for all levels): tokens fp32, flat, level l's rows [B, level_rows[l], D] at l * level_stride; index
    int32 [L, B, P]; the result is [L, B, D, P] (layout "NCHW") or [L, B, P, D] ("NHWC"), fp32 or bf16.  Per level the bits of dense_gather."""
    _same_device(tokens, index, out)
    if layout not in DENSE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(DENSE_LAYOUTS)}, got {layout!r}")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, got {dtype}")
    rows = _level_array(level_rows, "level_rows")
    L = len(rows)
    if index.dim() != 3 or index.shape[0] != L:
        raise ValueError(f"index must be [L, B, P] with L = {L}, got {tuple(index.shape)}")
    _, B, P = index.shape
    need = max(l * level_stride + B * rows[l] * D for l in range(L))
    if tokens.numel() < need:
        raise ValueError(f"tokens holds {tokens.numel()} elements, {L} levels at stride {level_stride} need {need}")
    shape = (L, B, D, P) if layout == "NCHW" else (L, B, P, D)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=tokens.device)
    elif out.numel() != L * B * D * P:
        raise ValueError(f"out must hold {L * B * D * P} elements, got {out.numel()}")
    _lib.check(_lib.load().tr_dense_gather_levels(_dev(tokens, torch.float32, "tokens"), level_stride, rows, L, _dev(index, torch.int32, "index"),
                                                  _dev(out, dtype, "out"), DENSE_LAYOUTS[layout], int(dtype == torch.bfloat16), float(fill), B, P, D,
                                                  _stream(tokens)), "tr_dense_gather_levels")
    return out.view(shape)


def dense_scatter_levels(dmaps, index: torch.Tensor, level_rows, level_stride: int, layout: str = "NCHW", dtype=torch.float32,
                         out: torch.Tensor = None) -> torch.Tensor:
    """The adjoint of dense_gather_levels (tr_dense_scatter_levels, one launch for all levels): dmaps is a sequence of L map gradients, each
    [B, D, P] (layout "NCHW") or [B, P, D] ("NHWC"), all fp32 or all bf16 -- or None for a level without a gradient, whose slab of the result is
    not touched and which costs no workgroup.  index int32 [L, B, P]; the result is flat, level l's rows [B, level_rows[l], D] at
    l * level_stride elements, fp32 or bf16 (`dtype`).  Per level the bits of dense_scatter.  With every entry None nothing is launched."""
    dmaps = list(dmaps)
    _same_device(index, out, *dmaps)
    if layout not in DENSE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(DENSE_LAYOUTS)}, got {layout!r}")
    rows = _level_array(level_rows, "level_rows")
    L = len(rows)
    if len(dmaps) != L or index.dim() != 3 or index.shape[0] != L:
        raise ValueError(f"{L} level rows need {L} maps (or None) and an index [L, B, P], got {len(dmaps)} maps and index {tuple(index.shape)}")
    _, B, P = index.shape
    present = [m for m in dmaps if m is not None]
    in_dtype = present[0].dtype if present else torch.float32
    if dtype not in (torch.float32, torch.bfloat16) or in_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"the maps and dtype must be torch.float32 or torch.bfloat16, got {in_dtype} and {dtype}")
    if not present:
        D = 4
    else:
        D = present[0].shape[1] if layout == "NCHW" else present[0].shape[2]
        for m in present:
            if m.dim() != 3 or m.dtype != in_dtype or tuple(m.shape) != ((B, D, P) if layout == "NCHW" else (B, P, D)):
                raise ValueError(f"every map must be {in_dtype} {(B, D, P) if layout == 'NCHW' else (B, P, D)}, got {m.dtype} {tuple(m.shape)}")
    if out is None:
        out = torch.empty(L * level_stride, dtype=dtype, device=index.device)
    elif out.numel() < L * level_stride:
        raise ValueError(f"out must hold {L * level_stride} elements, got {out.numel()}")
    ptrs = (ctypes.c_void_p * L)(*[None if m is None else _dev(m, in_dtype, "dmap") for m in dmaps])
    _lib.check(_lib.load().tr_dense_scatter_levels(ptrs, _dev(index, torch.int32, "index"), _dev(out, dtype, "out"), level_stride, rows, L,
                                                   DENSE_LAYOUTS[layout], int(in_dtype == torch.bfloat16), int(dtype == torch.bfloat16), B, P, D,
                                                   _stream(index)), "tr_dense_scatter_levels")
    return out


def level_tap_norm(x: torch.Tensor, gamma, beta, eps: float, d1: torch.Tensor = None, d2: torch.Tensor = None):
    """(sum, y) of fp32 rows [M, D] in one launch (tr_level_tap_norm): sum = (x + d1) + d2 -- cls_tap's bits at row stride D -- and y its fp32
    LayerNorm -- final_tokens_f32's bits.  d1 / d2 bf16 or fp32 rows [M, D], both nullable; x is not written."""
    _same_device(x, d1, d2, gamma, beta)
    D = x.shape[-1]
    M = x.numel() // D
    total, y = torch.empty(M, D, dtype=torch.float32, device=x.device), torch.empty(M, D, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().tr_level_tap_norm(_dev(x, torch.float32, "x"), _pending(d1, "d1"), _pending(d2, "d2"), _pending_f32(d1, d2),
                                             _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"), total.data_ptr(),
                                             y.data_ptr(), M, D, eps, _stream(x)), "tr_level_tap_norm")
    return total, y


def stream_grad_add(d: torch.Tensor, g: torch.Tensor, gb: torch.Tensor = None):
    """g += d in fp32 and gb = bf16(g), in place (tr_stream_grad_add): d, g fp32 and gb bf16 (nullable) of one element count, a multiple of 4."""
    _same_device(d, g, gb)
    if d.numel() != g.numel() or (gb is not None and gb.numel() != g.numel()):
        raise ValueError(f"d, g and gb must hold the same number of elements, got {d.numel()}, {g.numel()}, {None if gb is None else gb.numel()}")
    _lib.check(_lib.load().tr_stream_grad_add(_dev(d, torch.float32, "d"), _dev(g, torch.float32, "g"), _opt(gb, torch.bfloat16, "gb"),
                                              g.numel(), _stream(g)), "tr_stream_grad_add")
    return g, gb


def attention_f32(qkv: torch.Tensor, B: int, N: int, H: int, want_cls: bool = False, size: torch.Tensor = None,
                  colsum_part: torch.Tensor = None, split: bool = False):
    out = torch.empty(B * N, H * 64, dtype=torch.float32, device=qkv.device)
    cls_rows = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device) if want_cls else None
    fn = _lib.load().tr_attention_split if split else _lib.load().tr_attention_f32
    _lib.check(fn(_dev(qkv, torch.float32, "qkv"), out.data_ptr(), None if cls_rows is None else cls_rows.data_ptr(),
                  _opt(size, torch.float32, "size"), _opt(colsum_part, torch.float32, "colsum_part"), B, N, H, _stream()),
               "tr_attention_split" if split else "tr_attention_f32")
    return out, cls_rows


# ---------------------------------------------------------------------------------------- ToMe (models/tome.py)
def ats_width(new_mask: torch.Tensor) -> int:
    """ats.py:77-78: the token count the reference keeps after a sampling block = the batch maximum of valid ids (row sums of new_mask)."""
    B, K = new_mask.shape
    w = torch.zeros(1, dtype=torch.int32, device=new_mask.device)
    _lib.check(_lib.load().tr_ats_width(_dev(new_mask, torch.float32, "new_mask"), w.data_ptr(), B, K, _stream(new_mask)), "tr_ats_width")
    return int(w.item())


def ats_narrow(ids: torch.Tensor, new_mask: torch.Tensor, Kw: int):
    """The first Kw columns of ids / new_mask [B,K] as contiguous [B,Kw] tensors (what ats_gather and the next block's key mask take)."""
    B, K = ids.shape
    ids_out = torch.empty(B, Kw, dtype=torch.int32, device=ids.device)
    mask_out = torch.empty(B, Kw, dtype=torch.float32, device=ids.device)
    _lib.check(_lib.load().tr_ats_narrow(_dev(ids, torch.int32, "ids"), _dev(new_mask, torch.float32, "new_mask"), ids_out.data_ptr(),
                                         mask_out.data_ptr(), B, K, int(Kw), _stream(ids)), "tr_ats_narrow")
    return ids_out, mask_out


def tome_match(qkv: torch.Tensor, B: int, N: int, H: int, r: int):
    """bipartite_soft_matching (tome.py:230-277) on metric = k.mean(1): qkv bf16|fp32 [B*N, 3*H*64] ->
    (unm_idx [B, ceil(N/2)-r], src_idx [B,r], dst_idx [B,r]) int32."""
    if qkv.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("qkv must be bf16 or fp32")
    na = (N + 1) // 2
    unm = torch.empty(B, na - r, dtype=torch.int32, device=qkv.device)
    src = torch.empty(B, r, dtype=torch.int32, device=qkv.device)
    dst = torch.empty(B, r, dtype=torch.int32, device=qkv.device)
    _lib.check(_lib.load().tr_tome_match(_dev(qkv, qkv.dtype, "qkv"), int(qkv.dtype == torch.float32), unm.data_ptr(), src.data_ptr(),
                                         dst.data_ptr(), B, N, H, r, _stream()), "tr_tome_match")
    return unm, src, dst


def tome_merge_layernorm(x: torch.Tensor, delta, size, unm, src, dst, gamma, beta, eps: float, f32: bool = False):
    """merge_wavg (tome.py:309-323) of x (+ delta) with norm2 fused: -> (x_out fp32 [B,N-r,D], size_out fp32 [B,N-r], y)."""
    B, N, D = x.shape
    r = src.shape[1]
    x_out = torch.empty(B, N - r, D, dtype=torch.float32, device=x.device)
    size_out = torch.empty(B, N - r, dtype=torch.float32, device=x.device)
    y = torch.empty(B, N - r, D, dtype=torch.float32 if f32 else torch.bfloat16, device=x.device)
    ddt = torch.float32 if f32 else torch.bfloat16
    _lib.check(_lib.load().tr_tome_merge_layernorm(
        _dev(x, torch.float32, "x"), _opt(delta, ddt, "delta"), int(f32), _opt(size, torch.float32, "size"), _dev(unm, torch.int32, "unm"),
        _dev(src, torch.int32, "src"), _dev(dst, torch.int32, "dst"), _dev(gamma, torch.float32, "gamma"),
        _dev(beta, torch.float32, "beta"), x_out.data_ptr(), size_out.data_ptr(), y.data_ptr(), B, N, r, D, eps, _stream()),
        "tr_tome_merge_layernorm")
    return x_out, size_out, y


# ---------------------------------------------------------------------------------------- DyViT / SiT (reduce before the block)
def pool_broadcast(h: torch.Tensor, B: int, N: int, eps: float = 1e-6):
    """PredictorLG global feature (dyvit.py:115-118, policy == 1): in place on h bf16|fp32 [B*N, C]."""
    if h.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("h must be bf16 or fp32")
    C_ = h.shape[-1]
    _lib.check(_lib.load().tr_pool_broadcast(_dev(h, h.dtype, "h"), int(h.dtype == torch.float32), B, N, C_, eps, _stream()),
               "tr_pool_broadcast")
    return h


def dyvit_score(h: torch.Tensor, w: torch.Tensor, b: torch.Tensor):
    """out_conv.4 + LogSoftmax + [..., 0] (dyvit.py:108-109, 231): h bf16|fp32 [M, C], w fp32 [2, C] -> scores fp32 [M]."""
    M, C_ = h.shape
    scores = torch.empty(M, dtype=torch.float32, device=h.device)
    _lib.check(_lib.load().tr_dyvit_score(_dev(h, h.dtype, "h"), int(h.dtype == torch.float32), _dev(w, torch.float32, "w"),
                                          _dev(b, torch.float32, "b"), scores.data_ptr(), M, C_, _stream()), "tr_dyvit_score")
    return scores


def softassign_merge_fast(logits: torch.Tensor, scale: float, x: torch.Tensor, K: int, apply_softmax: bool = True,
                          want_soft: bool = False, src: torch.Tensor = None):
    """MFMA version of sit_merge / weighted_merge (bf16 executor; `logits` is overwritten by the weights when apply_softmax):
    -> (x_out fp32 [B,K+1,D], soft fp32 [B,K,N-1] | None)."""
    B, N, D = x.shape
    ldl = logits.shape[-1]
    x_out = torch.empty(B, K + 1, D, dtype=torch.float32, device=x.device)
    soft = torch.empty(B, K, N - 1, dtype=torch.float32, device=x.device) if (want_soft and apply_softmax) else None
    _lib.check(_lib.load().tr_softassign_merge_fast(_dev(logits, torch.float32, "logits"), ldl, float(scale), int(apply_softmax),
                                                    _dev(x, torch.float32, "x"), _dev(x if src is None else src, torch.float32, "src"),
                                                    x_out.data_ptr(), None if soft is None else soft.data_ptr(), B, N, K, D, _stream()),
               "tr_softassign_merge_fast")
    return x_out, soft


def sit_merge(logits: torch.Tensor, scale: float, x: torch.Tensor, K: int, want_soft: bool = False, src: torch.Tensor = None):
    """TokenSlimmingModule tail (sit.py:38-39): logits fp32 [B,N,ldl] (first K columns), x fp32 [B,N,D] ->
    (x_out fp32 [B,K+1,D], soft fp32 [B,K,N-1] | None)."""
    B, N, D = x.shape
    ldl = logits.shape[-1]
    x_out = torch.empty(B, K + 1, D, dtype=torch.float32, device=x.device)
    soft = torch.empty(B, K, N - 1, dtype=torch.float32, device=x.device) if want_soft else None
    _lib.check(_lib.load().tr_softassign_merge(_dev(logits, torch.float32, "logits"), ldl, float(scale), _dev(x, torch.float32, "x"),
                                               _dev(x if src is None else src, torch.float32, "src"), x_out.data_ptr(),
                                               None if soft is None else soft.data_ptr(), B, N, K, D, _stream()),
               "tr_softassign_merge")
    return x_out, soft


# ---------------------------------------------------------------------------------------- DPC-KNN (models/dpcknn.py)
def cluster_workspace_floats(B: int, N: int) -> int:
    """fp32 elements of the workspace dpcknn_cluster, kmedoids and kmedoids_equal need for B images of N tokens."""
    return int(_lib.load().tr_dpcknn_workspace_floats(B, N))


def _cluster_ws(ws, B: int, N: int, device) -> torch.Tensor:
    """The clustering workspace: a fresh one, or the caller's (whose stage intermediates the caller can then read back)."""
    need = cluster_workspace_floats(B, N)
    if ws is None:
        return torch.empty(need, dtype=torch.float32, device=device)
    if not (isinstance(ws, torch.Tensor) and ws.dtype == torch.float32 and ws.is_contiguous() and ws.device == device and ws.numel() >= need):
        raise ValueError(f"ws must be a contiguous fp32 tensor on {device} with at least {need} elements")
    return ws


def dpcknn_cluster(x: torch.Tensor, K: int, noise: torch.Tensor = None, k: int = 5, fast_dist=False, ws: torch.Tensor = None):
    """cluster_dpc_knn (dpcknn.py:44-100) on the patch rows of x fp32 [B,N,D] ->
    (centers int32 [B,K] in descending-score order, idx_cluster int32 [B,N-1], scores fp32 [B,N-1]).
    fast_dist: False / 0 = fp32 distances; True / 1 = split-bf16 MFMA distances, in ONE launch where the kernel applies; 2 = the same
    distances through the staged launches.  ws: caller-owned workspace (cluster_workspace_floats), None = a fresh one."""
    B, N, D = x.shape
    lib = _lib.load()
    ws = _cluster_ws(ws, B, N, x.device)
    centers = torch.empty(B, K, dtype=torch.int32, device=x.device)
    idx_cluster = torch.empty(B, N - 1, dtype=torch.int32, device=x.device)
    scores = torch.empty(B, N - 1, dtype=torch.float32, device=x.device)
    _lib.check(lib.tr_dpcknn_cluster(_dev(x, torch.float32, "x"), _opt(noise, torch.float32, "noise"), ws.data_ptr(),
                                     centers.data_ptr(), idx_cluster.data_ptr(), scores.data_ptr(), B, N, D, K, k, int(fast_dist),
                                     _stream()),
               "tr_dpcknn_cluster")
    return centers, idx_cluster, scores


def cluster_merge_layernorm(x: torch.Tensor, idx_cluster: torch.Tensor, K: int, gamma, beta, eps: float, score_w=None, score_b=None,
                            f32: bool = False):
    """merge_tokens (dpcknn.py:103-132) with token_weight = exp(Linear(D,1)(x)) (None = equal weights) + the next LayerNorm:
    x fp32 [B,N,D] -> (x_out fp32 [B,K+1,D], y [B,K+1,D])."""
    B, N, D = x.shape
    x_out = torch.empty(B, K + 1, D, dtype=torch.float32, device=x.device)
    y = torch.empty(B, K + 1, D, dtype=torch.float32 if f32 else torch.bfloat16, device=x.device)
    wws = torch.empty(B, N - 1, dtype=torch.float32, device=x.device) if score_w is not None else None
    _lib.check(_lib.load().tr_cluster_merge_layernorm(
        _dev(x, torch.float32, "x"), _opt(score_w, torch.float32, "score_w"), _opt(score_b, torch.float32, "score_b"),
        None if wws is None else wws.data_ptr(), _dev(idx_cluster, torch.int32, "idx_cluster"), _dev(gamma, torch.float32, "gamma"),
        _dev(beta, torch.float32, "beta"), x_out.data_ptr(), y.data_ptr(), int(f32), B, N, K, D, eps, _stream()),
        "tr_cluster_merge_layernorm")
    return x_out, y


# ---------------------------------------------------------------------------------------- ATS (models/ats.py)
def ats_sample(cls_rows: torch.Tensor, qkv: torch.Tensor, mask, steps: torch.Tensor, K: int, want_cdf: bool = False):
    """AdaptiveTokenSampling (ats.py:52-84): cls_rows fp32 [B,H,N], qkv bf16|fp32 [B*N, 3*H*64], mask fp32 [B,N] of 1/0 or None
    -> (ids int32 [B,K] (CLS 0 first, 1-based ids, 0 padding), new_mask fp32 [B,K], cdf fp32 [B,N-1] | None)."""
    B, H, N = cls_rows.shape
    ids = torch.empty(B, K, dtype=torch.int32, device=qkv.device)
    new_mask = torch.empty(B, K, dtype=torch.float32, device=qkv.device)
    cdf = torch.empty(B, N - 1, dtype=torch.float32, device=qkv.device) if want_cdf else None
    _lib.check(_lib.load().tr_ats_sample(_dev(cls_rows, torch.float32, "cls_rows"), _dev(qkv, qkv.dtype, "qkv"),
                                         int(qkv.dtype == torch.float32), _opt(mask, torch.float32, "mask"),
                                         _dev(steps, torch.float32, "steps"), steps.numel(), ids.data_ptr(), new_mask.data_ptr(),
                                         None if cdf is None else cdf.data_ptr(), B, N, H, K, _stream()), "tr_ats_sample")
    return ids, new_mask, cdf


def ats_gather(x: torch.Tensor, ao: torch.Tensor, ids: torch.Tensor):
    """x fp32 [B,N,D], ao bf16|fp32 [B*N, D], ids int32 [B,K] -> (x_out fp32 [B,K,D], ao_out [B*K, D]) rows ids (ats.py:86,157)."""
    B, N, D = x.shape
    K = ids.shape[1]
    x_out = torch.empty(B, K, D, dtype=torch.float32, device=x.device)
    ao_out = torch.empty(B * K, D, dtype=ao.dtype, device=x.device)
    _lib.check(_lib.load().tr_ats_gather(_dev(x, torch.float32, "x"), _dev(ao, ao.dtype, "ao"), int(ao.dtype == torch.float32),
                                         _dev(ids, torch.int32, "ids"), x_out.data_ptr(), ao_out.data_ptr(), B, N, K, D, _stream()),
               "tr_ats_gather")
    return x_out, ao_out


# ---------------------------------------------------------------------------------------- Sinkhorn (models/sinkhorn.py)
def rownorm(x: torch.Tensor, f32: bool = False):
    """F.normalize(x, dim=-1): x fp32 [M,D] -> (xh fp32 [M,D], xh as GEMM operand bf16|fp32)."""
    M, D = x.shape
    xh = torch.empty_like(x)
    lp = torch.empty(M, D, dtype=torch.float32 if f32 else torch.bfloat16, device=x.device)
    _lib.check(_lib.load().tr_rownorm(_dev(x, torch.float32, "x"), xh.data_ptr(), lp.data_ptr(), int(f32), M, D, _stream()), "tr_rownorm")
    return xh, lp


def sinkhorn(scores: torch.Tensor, K: int, eps: float, iters: int, want_soft: bool = False):
    """log_optimal_transport (sinkhorn.py:41-56): scores fp32 [B,N,ldl] -> (wt fp32 [B,N,ldl] token-major plan, soft [B,K,N-1]|None)."""
    B, N, ldl = scores.shape
    wt = torch.zeros_like(scores)
    soft = torch.empty(B, K, N - 1, dtype=torch.float32, device=scores.device) if want_soft else None
    _lib.check(_lib.load().tr_sinkhorn(_dev(scores, torch.float32, "scores"), ldl, float(eps), int(iters), wt.data_ptr(),
                                       None if soft is None else soft.data_ptr(), B, N, K, _stream()), "tr_sinkhorn")
    return wt, soft


def weighted_merge(wt: torch.Tensor, x: torch.Tensor, src: torch.Tensor, K: int):
    """x_out[b,1+k] = sum_p wt[b,1+p,k] * src[b,1+p]; x_out[b,0] = x[b,0]  (sinkhorn.py:83)."""
    B, N, D = x.shape
    x_out = torch.empty(B, K + 1, D, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().tr_weighted_merge(_dev(wt, torch.float32, "wt"), wt.shape[-1], _dev(x, torch.float32, "x"),
                                             _dev(src, torch.float32, "src"), x_out.data_ptr(), B, N, K, D, _stream()),
               "tr_weighted_merge")
    return x_out


# ---------------------------------------------------------------------------------------- K-Medoids (models/kmedoids.py)
def kmedoids(x: torch.Tensor, colsum_part: torch.Tensor, K: int, iters: int, fast_dist: bool = False, ws: torch.Tensor = None):
    """k_medoids_fit (kmedoids.py:40-85, weighted branch): x fp32 [B,N,D], colsum_part fp32 [B,H,4,N] (previous block's attention)
    -> (centers int32 [B,K], assignment int32 [B,N-1]).  ws: caller-owned workspace (cluster_workspace_floats), None = a fresh one."""
    B, N, D = x.shape
    H = colsum_part.shape[1]
    lib = _lib.load()
    ws = _cluster_ws(ws, B, N, x.device)
    centers = torch.empty(B, K, dtype=torch.int32, device=x.device)
    assign = torch.empty(B, N - 1, dtype=torch.int32, device=x.device)
    _lib.check(lib.tr_kmedoids(_dev(x, torch.float32, "x"), _dev(colsum_part, torch.float32, "colsum_part"), ws.data_ptr(),
                               centers.data_ptr(), assign.data_ptr(), B, N, D, H, K, iters, int(fast_dist), _stream()), "tr_kmedoids")
    return centers, assign


def kmedoids_equal(x: torch.Tensor, first: int, K: int, iters: int, fast_dist: bool = False, ws: torch.Tensor = None):
    """k_medoids_fit with token_weight None (args.equal_weight, kmedoids.py:43-58): `first` = the np.random.choice draw."""
    B, N, D = x.shape
    lib = _lib.load()
    ws = _cluster_ws(ws, B, N, x.device)
    centers = torch.empty(B, K, dtype=torch.int32, device=x.device)
    assign = torch.empty(B, N - 1, dtype=torch.int32, device=x.device)
    _lib.check(lib.tr_kmedoids_equal(_dev(x, torch.float32, "x"), int(first), ws.data_ptr(), centers.data_ptr(), assign.data_ptr(), B, N, D, K,
                                     iters, int(fast_dist), _stream()), "tr_kmedoids_equal")
    return centers, assign


# ---------------------------------------------------------------------------------------- DyViT training attention (forward)
def attention_policy(qkv: torch.Tensor, policy: torch.Tensor, B: int, N: int, H: int) -> torch.Tensor:
    """Policy_Attention with softmax_with_policy (dyvit.py:39-67): qkv bf16|fp32 [B*N, 3*H*64], policy fp32 [B,N] of 1/0 ->
    out [B*N, H*64] in qkv's dtype."""
    out = torch.empty(B * N, H * 64, dtype=qkv.dtype, device=qkv.device)
    lib = _lib.load()
    fn = lib.tr_attention_policy_f32 if qkv.dtype == torch.float32 else lib.tr_attention_policy_bf16
    _lib.check(fn(_dev(qkv, qkv.dtype, "qkv"), out.data_ptr(), _dev(policy, torch.float32, "policy"), B, N, H, _stream()),
               "tr_attention_policy")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# backward kernels (csrc/tr_backward.hip, csrc/tr_attention_bwd.hip): gradients of the ops above
def _ws(n_floats: int, dev) -> torch.Tensor:
    return torch.empty(max(int(n_floats), 4), dtype=torch.float32, device=dev)


def _ws_arg(ws, ws_floats, need: int, dev):
    """(workspace pointer, floats told to the C ABI).  Default: a fresh workspace of the size the library recommends.  ws: the caller's own
    fp32 buffer (a slice of a larger one: what lies around it can be watched); ws_floats: what the kernels may use of it -- fewer floats
    than recommended make the launch re-plan its token ranges, as the executor's shared workspace does."""
    if ws is None:
        ws = _ws(need if ws_floats is None else ws_floats, dev)
        return ws, ws.data_ptr(), ws.numel() if ws_floats is None else int(ws_floats)
    n = ws.numel() if ws_floats is None else int(ws_floats)
    if n > ws.numel():
        raise ValueError(f"ws: {n} floats asked of a workspace of {ws.numel()}")
    return ws, _dev(ws, torch.float32, "ws"), n


def _rows(t: torch.Tensor, dtype, name: str):
    """(pointer, row stride): 2-D operands may be column slices of a wider tensor (unit column stride, any row stride) -- the C ABI takes
    a leading dimension; everything else must be contiguous."""
    if t.dim() == 2 and t.stride(1) == 1 and t.is_cuda and t.dtype == dtype:
        return t.data_ptr(), t.stride(0)
    return _dev(t, dtype, name), t.shape[-1]


def wgrad(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor = None, accumulate: bool = False, yskip: int = 0,
          rows: int = None, ws: torch.Tensor = None, ws_floats: int = None) -> torch.Tensor:
    """nn.Linear weight gradient dW[N,K] (+)= dy[M,N]^T x[M,K] (bf16 operands, fp32 result)."""
    M = rows if rows is not None else x.shape[0]
    N, K = dy.shape[-1], x.shape[-1]
    lib = _lib.load()
    if out is None:
        out = torch.empty(N, K, dtype=torch.float32, device=x.device)
    ws, pws, nws = _ws_arg(ws, ws_floats, lib.tr_wgrad_workspace_floats(M, N, K), x.device)
    (py, ldy), (px, ldx) = _rows(dy, torch.bfloat16, "dy"), _rows(x, torch.bfloat16, "x")
    _lib.check(lib.tr_wgrad_bf16(py, ldy, yskip, px, ldx, _dev(out, torch.float32, "out"), int(accumulate), pws, nws, M, N, K, _stream()),
               "tr_wgrad_bf16")
    return out


def patch_embed_dgrad(dy: torch.Tensor, wt: torch.Tensor, B: int, C: int, HW=None, patch: int = 16, out: torch.Tensor = None, *, H: int = None,
                      W: int = None) -> torch.Tensor:
    """PatchEmbed's data gradient folded back into the image (tr_patch_embed_dgrad): dy bf16 token rows [B * (P + 1), D] (or a column slice
    of a wider tensor; the CLS row of every image is never read), wt bf16 [C*patch*patch, D] = the patch weight transposed -> dx fp32
    [B, C, HW, HW], every element written exactly once.  An unsupported shape raises.  A rectangular image: HW = (H, W) or the keywords
    H and W -> dx [B, C, H, W] through tr_patch_embed_dgrad_hw (also when H == W); an int HW keeps the square entry."""
    if H is not None or W is not None or isinstance(HW, (tuple, list)):
        if isinstance(HW, (tuple, list)):
            if H is not None or W is not None or len(HW) != 2:
                raise ValueError(f"patch_embed_dgrad: give the image size once, as HW = (H, W) or as H and W (got HW = {HW}, H = {H}, W = {W})")
            H, W = HW
        elif HW is not None or H is None or W is None:
            raise ValueError(f"patch_embed_dgrad: give either HW or both H and W (got HW = {HW}, H = {H}, W = {W})")
        return _patch_embed_dgrad_hw(dy, wt, B, C, int(H), int(W), patch, out)
    if HW is None:
        raise ValueError("patch_embed_dgrad: the image size is missing (HW, or H and W)")
    D = wt.shape[-1]
    if out is None:
        out = torch.empty(B, C, HW, HW, dtype=torch.float32, device=dy.device)
    _same_device(dy, wt, out)
    pdy, ldy = _rows(dy, torch.bfloat16, "dy")
    if wt.dim() != 2 or wt.shape[0] != C * patch * patch:
        raise ValueError(f"wt: expected [{C * patch * patch}, D] (the patch weight transposed), got {tuple(wt.shape)}")
    if dy.dim() != 2 or dy.shape[1] != D or patch <= 0 or HW % patch or dy.shape[0] != B * ((HW // patch) ** 2 + 1):
        raise ValueError(f"dy: expected token rows [B * (P + 1), {D}] for B = {B}, HW = {HW}, patch = {patch}, got {tuple(dy.shape)}")
    if out.shape != (B, C, HW, HW):
        raise ValueError(f"out: expected {(B, C, HW, HW)}, got {tuple(out.shape)}")
    _lib.check(_lib.load().tr_patch_embed_dgrad(pdy, ldy, _dev(wt, torch.bfloat16, "wt"), _dev(out, torch.float32, "out"), B, C, HW, patch, D,
                                                _stream(dy)), "tr_patch_embed_dgrad")
    return out


def _patch_embed_dgrad_hw(dy, wt, B, C, H, W, patch, out):
    """patch_embed_dgrad on [B, C, H, W] (tr_patch_embed_dgrad_hw), the same checks."""
    D = wt.shape[-1]
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=dy.device)
    _same_device(dy, wt, out)
    pdy, ldy = _rows(dy, torch.bfloat16, "dy")
    if wt.dim() != 2 or wt.shape[0] != C * patch * patch:
        raise ValueError(f"wt: expected [{C * patch * patch}, D] (the patch weight transposed), got {tuple(wt.shape)}")
    if dy.dim() != 2 or dy.shape[1] != D or patch <= 0 or H % patch or W % patch or dy.shape[0] != B * ((H // patch) * (W // patch) + 1):
        raise ValueError(f"dy: expected token rows [B * (P + 1), {D}] for B = {B}, H = {H}, W = {W}, patch = {patch}, got {tuple(dy.shape)}")
    if out.shape != (B, C, H, W):
        raise ValueError(f"out: expected {(B, C, H, W)}, got {tuple(out.shape)}")
    _lib.check(_lib.load().tr_patch_embed_dgrad_hw(pdy, ldy, _dev(wt, torch.bfloat16, "wt"), _dev(out, torch.float32, "out"), B, C, H, W, patch,
                                                   D, _stream(dy)), "tr_patch_embed_dgrad_hw")
    return out


def linear_bwd_params(dy: torch.Tensor, x: torch.Tensor, accumulate: bool = False, dw: torch.Tensor = None, db: torch.Tensor = None,
                      yskip: int = 0, ws: torch.Tensor = None, ws_floats: int = None):
    """Weight and bias gradient of an nn.Linear in one pass (tr_linear_bwd_params): (dW fp32 [N,K], db fp32 [N]).  yskip > 0: dy holds one
    extra leading row per `yskip` rows (the CLS row of [B, P + 1, D]) that the layer never saw (PatchEmbed)."""
    M, N, K = x.shape[0], dy.shape[-1], x.shape[-1]
    lib = _lib.load()
    dw = torch.empty(N, K, dtype=torch.float32, device=x.device) if dw is None else dw
    db = torch.empty(N, dtype=torch.float32, device=x.device) if db is None else db
    ws, pws, nws = _ws_arg(ws, ws_floats, lib.tr_wgrad_workspace_floats(M, N, K), x.device)
    (py, ldy), (px, ldx) = _rows(dy, torch.bfloat16, "dy"), _rows(x, torch.bfloat16, "x")
    _lib.check(lib.tr_linear_bwd_params(py, ldy, yskip, px, ldx, _dev(dw, torch.float32, "dw"),
                                        _dev(db, torch.float32, "db"), int(accumulate), pws, nws, M, N, K, _stream()),
               "tr_linear_bwd_params")
    return dw, db


def colsum(dy: torch.Tensor, out: torch.Tensor = None, accumulate: bool = False, yskip: int = 0, rows: int = None, ws: torch.Tensor = None,
           ws_floats: int = None) -> torch.Tensor:
    """nn.Linear bias gradient db[N] (+)= sum_m dy[m,n]."""
    N = dy.shape[-1]
    M = rows if rows is not None else (dy.shape[0] if dy.dim() == 2 else dy.numel() // N)
    lib = _lib.load()
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=dy.device)
    ws, pws, nws = _ws_arg(ws, ws_floats, lib.tr_colsum_workspace_floats(M, N), dy.device)
    py, ldy = _rows(dy, torch.bfloat16, "dy")
    _lib.check(lib.tr_colsum_bf16(py, ldy, yskip, _dev(out, torch.float32, "out"), int(accumulate), pws, nws, M, N, _stream()), "tr_colsum_bf16")
    return out


def gelu(pre: torch.Tensor) -> torch.Tensor:
    h = torch.empty_like(pre)
    _lib.check(_lib.load().tr_gelu_bf16(_dev(pre, torch.bfloat16, "pre"), h.data_ptr(), pre.numel(), _stream()), "tr_gelu_bf16")
    return h


def gelu_bwd(pre: torch.Tensor, dh: torch.Tensor) -> torch.Tensor:
    """dh := dh * gelu'(pre) in place."""
    _lib.check(_lib.load().tr_gelu_bwd_bf16(_dev(pre, torch.bfloat16, "pre"), _dev(dh, torch.bfloat16, "dh"), pre.numel(), _stream()),
               "tr_gelu_bwd_bf16")
    return dh


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, eps: float, g_in: torch.Tensor = None, idx: torch.Tensor = None,
                  n_out: int = None, fused: bool = False, g_out: torch.Tensor = None, ldx: int = None, ldgi: int = None, gb: bool = True,
                  accumulate: bool = False, dgamma: torch.Tensor = None, dbeta: torch.Tensor = None, params: bool = True, add: bool = False,
                  ws: torch.Tensor = None, ws_floats: int = None):
    """LayerNorm backward fused with the residual gradient.  dy bf16 [M,D], x fp32 [M,D] (LayerNorm input), g_in fp32 [M,D]|None.
    Plain: returns (g fp32 [M,D], gb bf16 [M,D], dgamma, dbeta).  With idx int32 [B,K] (Top-K gather backward): rows are
    [B, K+1(+1 fused)], results scattered into zero-filled [B, n_out, D]; also returns g_fused [B,D] when fused.
    The forms the backward executor uses: x, g_in and g_out may be row-strided 2-D views (ldx / ldgi override the stride taken from the
    view); g_out: the caller's destination (g_in itself: in place; with idx: zero-filled by the caller); gb=False: no bf16 copy (None
    returned); accumulate: ADD to the given dgamma / dbeta; params=False: a frozen norm, no parameter gradients (None returned);
    add=True (needs idx): tr_layernorm_bwd_scatter_add -- repeated ids are summed with float atomics, no bf16 copy."""
    M, D = dy.shape
    lib = _lib.load()
    dev = dy.device
    if params:
        dgamma = _grad_out(dgamma, (D,), "dgamma", accumulate, dev)
        dbeta = _grad_out(dbeta, (D,), "dbeta", accumulate, dev)
        ws, pws, nws = _ws_arg(ws, ws_floats, lib.tr_layernorm_bwd_workspace_floats(M, D), dev)
        pdg, pdb = dgamma.data_ptr(), dbeta.data_ptr()
    else:
        dgamma = dbeta = pws = pdg = pdb = None
        nws = 0
    g_fused = gbuf = None
    if idx is None:
        if add:
            raise ValueError("layernorm_bwd: add=True is the scatter of repeated ids and needs idx")
        g = torch.empty(M, D, dtype=torch.float32, device=dev) if g_out is None else g_out
        if gb:
            gbuf = torch.empty(M, D, dtype=torch.bfloat16, device=dev)
        K = n_in = no = 0
    else:
        B, K = idx.shape
        n_in = K + 1 + (1 if fused else 0)
        no = n_out
        g = torch.zeros(B * n_out, D, dtype=torch.float32, device=dev) if g_out is None else g_out
        if gb and not add:
            gbuf = torch.zeros(B * n_out, D, dtype=torch.bfloat16, device=dev)
        if fused:
            g_fused = torch.empty(B, D, dtype=torch.float32, device=dev)
    px, sx = _rows(x, torch.float32, "x")
    pgi, sgi = (None, D) if g_in is None else _rows(g_in, torch.float32, "g_in")
    pgo, sgo = _rows(g, torch.float32, "g_out")
    ldx, ldgi = sx if ldx is None else ldx, sgi if ldgi is None else ldgi
    if add:
        if fused or ldx != D or ldgi != D or sgo != D:
            raise ValueError("layernorm_bwd: add=True takes contiguous rows and no fused row")
        _lib.check(lib.tr_layernorm_bwd_scatter_add(_dev(dy, torch.bfloat16, "dy"), px, _dev(gamma, torch.float32, "gamma"), pgi, pgo,
                                                    _dev(idx, torch.int32, "idx"), K, no, pdg, pdb, int(accumulate), pws, nws, M, D, eps,
                                                    _stream()), "tr_layernorm_bwd_scatter_add")
        return g, None, dgamma, dbeta
    _lib.check(lib.tr_layernorm_bwd(_dev(dy, torch.bfloat16, "dy"), px, ldx, _dev(gamma, torch.float32, "gamma"), pgi, ldgi, pgo, sgo,
                                    None if gbuf is None else gbuf.data_ptr(), _opt(idx, torch.int32, "idx"), K, n_in,
                                    no, None if g_fused is None else g_fused.data_ptr(), pdg, pdb, int(accumulate),
                                    pws, nws, M, D, eps, _stream()), "tr_layernorm_bwd")
    if idx is not None and fused:
        return g, gbuf, dgamma, dbeta, g_fused
    return g, gbuf, dgamma, dbeta


def attention_bwd(qkv: torch.Tensor, dout: torch.Tensor, B: int, N: int, H: int, size: torch.Tensor = None, dcls: torch.Tensor = None):
    """d qkv (bf16 [B*N, 3*H*64]) of softmax(q k^T / 8 [+ log size]) v given d out (bf16 [B*N, H*64])."""
    dqkv = torch.empty_like(qkv)
    _lib.check(_lib.load().tr_attention_bwd_bf16(_dev(qkv, torch.bfloat16, "qkv"), _dev(dout, torch.bfloat16, "dout"),
                                                 _opt(size, torch.float32, "size"), _opt(dcls, torch.float32, "dcls"), dqkv.data_ptr(), B, N,
                                                 H, _stream()), "tr_attention_bwd_bf16")
    return dqkv


def _grad_out(t, shape, name: str, accumulate: bool, dev) -> torch.Tensor:
    """A gradient destination: the caller's preallocated fp32 tensor (required when accumulating: the kernel adds to it), or a fresh one."""
    if t is None:
        if accumulate:
            raise ValueError(f"{name}: accumulate=True adds to a destination the caller must pass")
        return torch.empty(*shape, dtype=torch.float32, device=dev)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    _dev(t, torch.float32, name)
    return t


def head_bwd(dlogits: torch.Tensor, w: torch.Tensor, xn: torch.Tensor, accumulate: bool = False, dw: torch.Tensor = None,
             db: torch.Tensor = None):
    """Classifier backward on the CLS rows: (dxn bf16 [B,D], dW fp32 [C,D], db fp32 [C]); dW / db (+)= with accumulate (into the given dw, db)."""
    B, Cc = dlogits.shape
    D = w.shape[1]
    dxn = torch.empty(B, D, dtype=torch.bfloat16, device=w.device)
    dw = _grad_out(dw, (Cc, D), "dw", accumulate, w.device)
    db = _grad_out(db, (Cc,), "db", accumulate, w.device)
    lib = _lib.load()
    dl16 = torch.empty(B, Cc, dtype=torch.bfloat16, device=w.device)
    ws = _ws(lib.tr_wgrad_workspace_floats(B, Cc, D), w.device)
    _lib.check(lib.tr_head_bwd(_dev(dlogits, torch.float32, "dlogits"), _dev(w, torch.bfloat16, "w"), _dev(xn, torch.bfloat16, "xn"),
                               dxn.data_ptr(), dw.data_ptr(), db.data_ptr(), int(accumulate), dl16.data_ptr(), ws.data_ptr(), ws.numel(), B, Cc, D,
                               _stream()),
               "tr_head_bwd")
    return dxn, dw, db


def embed_bwd(g: torch.Tensor, accumulate: bool = False, dpos: torch.Tensor = None, dcls: torch.Tensor = None):
    """(d pos_embed fp32 [N,D], d cls_token fp32 [D]) = sums of g fp32 [B,N,D] over the batch; (+)= with accumulate (into the given dpos, dcls)."""
    B, N, D = g.shape
    dpos = _grad_out(dpos, (N, D), "dpos", accumulate, g.device)
    dcls = _grad_out(dcls, (D,), "dcls", accumulate, g.device)
    _lib.check(_lib.load().tr_embed_bwd(_dev(g, torch.float32, "g"), dpos.data_ptr(), dcls.data_ptr(), int(accumulate), B, N, D, _stream()),
               "tr_embed_bwd")
    return dpos, dcls


def evit_fuse_bwd(x, delta, compl, scores, g_fused, g_out, gb_out):
    """In place on g_out / gb_out ([B,N,D]); returns dscore fp32 [B,N] (gradient wrt the head-mean CLS attention, entry 1+token)."""
    B, N, D = x.shape
    K = N - 1 - compl.shape[1]
    dscore = torch.zeros(B, N, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().tr_evit_fuse_bwd(_dev(x, torch.float32, "x"), _opt(delta, torch.bfloat16, "delta"), _dev(compl, torch.int32, "compl"),
                                            _dev(scores, torch.float32, "scores"), _dev(g_fused, torch.float32, "g_fused"),
                                            _dev(g_out, torch.float32, "g_out"), _dev(gb_out, torch.bfloat16, "gb_out"), dscore.data_ptr(),
                                            B, N, K, D, _stream()), "tr_evit_fuse_bwd")
    return dscore


def tome_merge_bwd(g_merged, size_in, size_out, unm, src, dst, N: int):
    B, N_out, D = g_merged.shape
    r = N - N_out
    g = torch.empty(B, N, D, dtype=torch.float32, device=g_merged.device)
    gb = torch.empty(B, N, D, dtype=torch.bfloat16, device=g_merged.device)
    inv = torch.empty(B, N, dtype=torch.int32, device=g_merged.device)
    _lib.check(_lib.load().tr_tome_merge_bwd(_dev(g_merged, torch.float32, "g_merged"), _opt(size_in, torch.float32, "size_in"),
                                             _dev(size_out, torch.float32, "size_out"), _dev(unm, torch.int32, "unm"), _dev(src, torch.int32, "src"),
                                             _dev(dst, torch.int32, "dst"), inv.data_ptr(), g.data_ptr(), gb.data_ptr(), B, N, r, D, _stream()),
               "tr_tome_merge_bwd")
    return g, gb


def cluster_merge_bwd(g_in, x0, x1, wtok, assign, score_w, accumulate: bool = False, dsw: torch.Tensor = None, dsb: torch.Tensor = None):
    """DPC-KNN CTM backward.  Returns (g fp32 [B,N,D], gb bf16, d_sw [D]|None, d_sb [1]|None); d_sw / d_sb (+)= with accumulate (into the
    given dsw, dsb; weighted merge only)."""
    B, N, D = x0.shape
    K = x1.shape[1] - 1
    lib = _lib.load()
    g = torch.empty(B, N, D, dtype=torch.float32, device=x0.device)
    gb = torch.empty(B, N, D, dtype=torch.bfloat16, device=x0.device)
    if score_w is not None:
        dsw = _grad_out(dsw, (D,), "dsw", accumulate, x0.device)
        dsb = _grad_out(dsb, (1,), "dsb", accumulate, x0.device)
    elif accumulate or dsw is not None or dsb is not None:
        raise ValueError("cluster_merge_bwd: accumulate / dsw / dsb need score_w (the equal-weight merge has no score gradient)")
    ws = _ws((8 * B + 1) * (D + 4), x0.device)
    _lib.check(lib.tr_cluster_merge_bwd(_dev(g_in, torch.float32, "g_in"), _dev(x0, torch.float32, "x0"), _dev(x1, torch.float32, "x1"),
                                        _opt(wtok, torch.float32, "wtok"), _dev(assign, torch.int32, "assign"), _opt(score_w, torch.float32, "score_w"),
                                        g.data_ptr(), gb.data_ptr(), None if dsw is None else dsw.data_ptr(), None if dsb is None else dsb.data_ptr(),
                                        int(accumulate), ws.data_ptr(), ws.numel(), B, N, K, D, _stream()), "tr_cluster_merge_bwd")
    return g, gb, dsw, dsb


def ats_scatter(g, dao_s, ids, N: int):
    B, Ks, D = g.shape
    g_full = torch.zeros(B, N, D, dtype=torch.float32, device=g.device)
    dao_full = torch.zeros(B, N, D, dtype=torch.bfloat16, device=g.device)
    _lib.check(_lib.load().tr_ats_scatter(_dev(g, torch.float32, "g"), _dev(dao_s, torch.bfloat16, "dao_s"), _dev(ids, torch.int32, "ids"),
                                          g_full.data_ptr(), dao_full.data_ptr(), B, N, Ks, D, _stream()), "tr_ats_scatter")
    return g_full, dao_full


# ---------------------------------------------------------------------------------------- soft-assignment reducers, backward (csrc/tr_soft_bwd.hip)
def _soft_out(t, shape, dtype, name: str, dev) -> torch.Tensor:
    """An output of the soft-assignment backward: a fresh ZEROED tensor, or the caller's (contiguous, of this shape; NOT zeroed here -- the
    kernels write the patch rows of columns < K only, and `ds` a zero CLS row for those columns)."""
    if t is None:
        return torch.zeros(*shape, dtype=dtype, device=dev)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    _dev(t, dtype, name)
    return t


def _soft_ldo(ds, ldo, K: int) -> int:
    if ldo is None:
        return (K + 63) // 64 * 64 if ds is None else ds.shape[-1]
    return int(ldo)


def soft_merge_bwd(g: torch.Tensor, wt: torch.Tensor, src: torch.Tensor, dwt: torch.Tensor = None, dsrc: torch.Tensor = None):
    """out[b,1+k] = sum_p wt[b,1+p,k] src[b,1+p] backwards: g fp32 [B,K+1,D], wt fp32 [B,N,ldl], src fp32 [B,N,D] ->
    (dwt fp32 [B,N,ldl] (CLS rows / columns >= K zero), dsrc fp32 [B,N,D] (CLS rows zero)).  A given dwt / dsrc is written on the patch
    rows (dwt: columns < K) and keeps what it held everywhere else."""
    B, N, D = src.shape
    K, ldl = g.shape[1] - 1, wt.shape[2]
    lib = _lib.load()
    dwt = _soft_out(dwt, (B, N, ldl), torch.float32, "dwt", src.device)
    dsrc = _soft_out(dsrc, (B, N, D), torch.float32, "dsrc", src.device)
    _lib.check(lib.tr_soft_dweights(_dev(g, torch.float32, "g"), _dev(src, torch.float32, "src"), dwt.data_ptr(), ldl, B, N, K, D, _stream()),
               "tr_soft_dweights")
    _lib.check(lib.tr_soft_dsrc(_dev(g, torch.float32, "g"), _dev(wt, torch.float32, "wt"), ldl, dsrc.data_ptr(), B, N, K, D, _stream()), "tr_soft_dsrc")
    return dwt, dsrc


def token_softmax_bwd(wt: torch.Tensor, dwt: torch.Tensor, logits: torch.Tensor, scale: float, K: int, want_dscale: bool = False,
                      ds: torch.Tensor = None, ldo: int = None, dscale: torch.Tensor = None, accumulate: bool = False):
    """-> (ds bf16 [B,N,ldo], dscale fp32[1] | None); ldo = the given one, else the given ds's, else K rounded up to 64.  A given ds keeps
    what it held in columns >= K.  d scale goes to the given `dscale` ((+)= with accumulate) or, with want_dscale, to a fresh one;
    `logits` may be None when no d scale is asked for."""
    B, N, ldl = wt.shape
    ldo = _soft_ldo(ds, ldo, K)
    lib = _lib.load()
    ds = _soft_out(ds, (B, N, ldo), torch.bfloat16, "ds", wt.device)
    if dscale is not None or accumulate:
        dscale = _grad_out(dscale, (1,), "dscale", accumulate, wt.device)
    elif want_dscale:
        dscale = torch.zeros(1, dtype=torch.float32, device=wt.device)
    ws = _ws(lib.tr_token_softmax_bwd_workspace_floats(B, K), wt.device)
    _lib.check(lib.tr_token_softmax_bwd(_dev(wt, torch.float32, "wt"), _dev(dwt, torch.float32, "dwt"), _opt(logits, torch.float32, "logits"), ldl,
                                        float(scale), ds.data_ptr(), ldo, None if dscale is None else dscale.data_ptr(), int(accumulate),
                                        ws.data_ptr(), ws.numel(), B, N, K, _stream()), "tr_token_softmax_bwd")
    return ds, dscale


def sinkhorn_bwd(scores: torch.Tensor, dplan: torch.Tensor, K: int, eps: float, iters: int, ds: torch.Tensor = None,
                 ldo: int = None) -> torch.Tensor:
    """-> ds bf16 [B,N,ldo] (ldo as token_softmax_bwd's); a given ds keeps what it held in columns >= K."""
    B, N, ldl = scores.shape
    ldo = _soft_ldo(ds, ldo, K)
    ds = _soft_out(ds, (B, N, ldo), torch.bfloat16, "ds", scores.device)
    _lib.check(_lib.load().tr_sinkhorn_bwd(_dev(scores, torch.float32, "scores"), _dev(dplan, torch.float32, "dplan"), ldl, float(eps), iters,
                                           ds.data_ptr(), ldo, B, N, K, _stream()), "tr_sinkhorn_bwd")
    return ds


def rownorm_bwd(x: torch.Tensor, da: torch.Tensor, db: torch.Tensor = None) -> torch.Tensor:
    M, D = x.shape
    dx = torch.empty(M, D, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().tr_rownorm_bwd(_dev(x, torch.float32, "x"), _dev(da, torch.float32, "da"), _opt(db, torch.bfloat16, "db"), dx.data_ptr(), M, D,
                                          _stream()), "tr_rownorm_bwd")
    return dx


def add_into_bf16(a: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    _lib.check(_lib.load().tr_add_into_bf16(_dev(a, torch.float32, "a"), _dev(y, torch.bfloat16, "y"), a.numel(), _stream()), "tr_add_into_bf16")
    return y


def attention_policy_bwd(qkv: torch.Tensor, dout: torch.Tensor, policy: torch.Tensor, B: int, N: int, H: int):
    """Backward of attention_policy (bf16): -> (dqkv bf16 [B*N, 3*H*64], d policy fp32 [B,H,N] per head).  Beyond 224 tokens the
    key-blocked kernels (tr_attention_policy_bwd_long_bf16), as in the training executor."""
    lib = _lib.load()
    dqkv = torch.empty_like(qkv)
    dpart = torch.zeros(B, H, N, dtype=torch.float32, device=qkv.device)
    args = (_dev(qkv, torch.bfloat16, "qkv"), _dev(dout, torch.bfloat16, "dout"), _dev(policy, torch.float32, "policy"), dqkv.data_ptr(), dpart.data_ptr())
    if N > 224:
        ws = _ws(lib.tr_attention_bwd_long_workspace_floats(B, N, H), qkv.device)
        _lib.check(lib.tr_attention_policy_bwd_long_bf16(*args, ws.data_ptr(), ws.numel(), B, N, H, _stream()), "tr_attention_policy_bwd_long_bf16")
    else:
        _lib.check(lib.tr_attention_policy_bwd_bf16(*args, B, N, H, _stream()), "tr_attention_policy_bwd_bf16")
    return dqkv, dpart


def attention_bwd_long(qkv: torch.Tensor, dout: torch.Tensor, B: int, N: int, H: int, size: torch.Tensor = None, dcls: torch.Tensor = None):
    """tr_attention_bwd_bf16's gradient for any sequence length (key-blocked kernels; what the training executor runs beyond 224 tokens)."""
    lib = _lib.load()
    dqkv = torch.empty_like(qkv)
    ws = _ws(lib.tr_attention_bwd_long_workspace_floats(B, N, H), qkv.device)
    _lib.check(lib.tr_attention_bwd_long_bf16(_dev(qkv, torch.bfloat16, "qkv"), _dev(dout, torch.bfloat16, "dout"), _opt(size, torch.float32, "size"),
                                              _opt(dcls, torch.float32, "dcls"), dqkv.data_ptr(), ws.data_ptr(), ws.numel(), B, N, H, _stream()),
               "tr_attention_bwd_long_bf16")
    return dqkv


def gemm_gelu_keep(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor):
    """Training forward of Linear + GELU in one launch: (pre bf16 [M,N], h = gelu(pre) bf16 [M,N])."""
    M, K = a.shape
    N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K or bias.numel() != N:
        raise ValueError(f"gemm_gelu_keep: a {tuple(a.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)} do not form a Linear")
    _same_device(a, w, bias)
    pre = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    h = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    _lib.check(_lib.load().tr_gemm_gelu_keep_bf16(_dev(a, torch.bfloat16, "a"), _dev(w, torch.bfloat16, "w"), _dev(bias, torch.float32, "bias"),
                                                  pre.data_ptr(), h.data_ptr(), M, N, K, _stream(a)), "tr_gemm_gelu_keep_bf16")
    return pre, h


def gemm_dgelu(a: torch.Tensor, w: torch.Tensor, pre: torch.Tensor) -> torch.Tensor:
    """Data gradient of a Linear with the GELU backward of the layer below folded in: bf16(a w^T) * gelu'(pre), bf16 [M,N]."""
    M, K = a.shape
    N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K or tuple(pre.shape) != (M, N):
        raise ValueError(f"gemm_dgelu: a {tuple(a.shape)}, w {tuple(w.shape)}, pre {tuple(pre.shape)} do not fit")
    _same_device(a, w, pre)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    _lib.check(_lib.load().tr_gemm_dgelu_bf16(_dev(a, torch.bfloat16, "a"), _dev(w, torch.bfloat16, "w"), _dev(pre, torch.bfloat16, "pre"),
                                              out.data_ptr(), M, N, K, _stream(a)), "tr_gemm_dgelu_bf16")
    return out


def linear_bwd_params2(dy0: torch.Tensor, x0: torch.Tensor, dy1: torch.Tensor, x1: torch.Tensor, accumulate: bool = False, outs=None):
    """Weight and bias gradients of TWO Linear layers in one weight-gradient launch + one reduce (tr_linear_bwd_params2):
    ((dW0, db0), (dW1, db1)).  outs: the four destination tensors when accumulating."""
    lib = _lib.load()
    (M0, N0), K0 = dy0.shape, x0.shape[-1]
    (M1, N1), K1 = dy1.shape, x1.shape[-1]
    dev = x0.device
    if outs is None:
        outs = (torch.empty(N0, K0, device=dev), torch.empty(N0, device=dev), torch.empty(N1, K1, device=dev), torch.empty(N1, device=dev))
    ws = _ws(lib.tr_linear_bwd_params2_workspace_floats(M0, N0, K0, M1, N1, K1), dev)
    _lib.check(lib.tr_linear_bwd_params2(_dev(dy0, torch.bfloat16, "dy0"), N0, _dev(x0, torch.bfloat16, "x0"), K0, _dev(outs[0], torch.float32, "dw0"),
                                         _dev(outs[1], torch.float32, "db0"), M0, N0, K0, _dev(dy1, torch.bfloat16, "dy1"), N1,
                                         _dev(x1, torch.bfloat16, "x1"), K1, _dev(outs[2], torch.float32, "dw1"), _dev(outs[3], torch.float32, "db1"),
                                         M1, N1, K1, int(accumulate), ws.data_ptr(), ws.numel(), _stream()), "tr_linear_bwd_params2")
    return (outs[0], outs[1]), (outs[2], outs[3])


def linear_bwd_group_workspace_floats(shapes) -> int:
    """Workspace floats tr_linear_bwd_group wants for layers of the given (M, N, K)."""
    arr = (_lib.TrLinearGrad * len(shapes))(*[_lib.TrLinearGrad(None, N, None, K, None, None, M, N, K) for M, N, K in shapes])
    return int(_lib.load().tr_linear_bwd_group_workspace_floats(ctypes.cast(arr, ctypes.c_void_p), len(shapes)))


def linear_bwd_group(layers, accumulate: bool = False, outs=None, ws: torch.Tensor = None, ws_floats: int = None):
    """Weight and bias gradients of up to four Linear layers in ONE weight-gradient launch + one reduce (tr_linear_bwd_group).
    layers: [(dy bf16 [M_i, N_i], x bf16 [M_i, K_i]), ...] (row-strided column slices allowed); returns [(dW_i fp32 [N_i, K_i],
    db_i fp32 [N_i]), ...]; outs: the same list of destination tensors when accumulating."""
    lib = _lib.load()
    n = len(layers)
    if not 1 <= n <= 4:
        raise ValueError("linear_bwd_group: 1..4 layers")
    dev = layers[0][0].device
    if outs is None:
        outs = [(torch.empty(dy.shape[1], x.shape[1], device=dev), torch.empty(dy.shape[1], device=dev)) for dy, x in layers]
    arr = (_lib.TrLinearGrad * n)()
    for i, ((dy, x), (dw, db)) in enumerate(zip(layers, outs)):
        if dy.shape[0] != x.shape[0] or tuple(dw.shape) != (dy.shape[1], x.shape[1]) or db.numel() != dy.shape[1]:
            raise ValueError(f"linear_bwd_group: layer {i}: dy {tuple(dy.shape)}, x {tuple(x.shape)}, dw {tuple(dw.shape)}, db {tuple(db.shape)} do not fit")
        (py, ldy), (px, ldx) = _rows(dy, torch.bfloat16, "dy"), _rows(x, torch.bfloat16, "x")
        arr[i] = _lib.TrLinearGrad(py, ldy, px, ldx, _dev(dw, torch.float32, "dw"), _dev(db, torch.float32, "db"), dy.shape[0], dy.shape[1], x.shape[1])
    ws, pws, nws = _ws_arg(ws, ws_floats, lib.tr_linear_bwd_group_workspace_floats(ctypes.cast(arr, ctypes.c_void_p), n), dev)
    _lib.check(lib.tr_linear_bwd_group(ctypes.cast(arr, ctypes.c_void_p), n, int(accumulate), pws, nws, _stream()), "tr_linear_bwd_group")
    return outs


# ---------------------------------------------------------------------------------------- DyViT training pieces (csrc/tr_dyvit_train.hip)
def pool_policy(h: torch.Tensor, policy: torch.Tensor, B: int, N: int, eps: float = 1e-6) -> torch.Tensor:
    """PredictorLG global feature under a policy (dyvit.py:115-118), in place on h bf16 [B*N, C]: channels C/2.. of every row :=
    sum_p h[p] policy[p] / sum_p policy[p] + eps over the image's patch rows.  policy fp32 [B,N] (entry 0 = CLS, not read)."""
    C_ = h.shape[-1]
    _same_device(h, policy)
    _lib.check(_lib.load().tr_pool_policy(_dev(h, torch.bfloat16, "h"), _dev(policy, torch.float32, "policy"), B, N, C_, float(eps), _stream(h)),
               "tr_pool_policy")
    return h


def _view_ptr(t: torch.Tensor, dtype, name: str) -> int:
    """Pointer of a dense tensor that may start anywhere inside a larger buffer (a view): for the entry points that choose a kernel by
    the alignment of their operands."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; tokenreduction_amd has no CPU path (HIP kernels only)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def pool_policy_bwd(dcat: torch.Tensor, pre0: torch.Tensor, cat: torch.Tensor, policy: torch.Tensor, dpolicy: torch.Tensor, B: int, N: int,
                    dh: torch.Tensor = None) -> torch.Tensor:
    """Backward of pool_policy: dcat bf16 [B*N, C] (gradient wrt [local | global]), pre0 the saved pre-activation, cat the forward's
    output -> dh bf16 [B*N, C] (wrt the GELU output); dpolicy fp32 [B,N] += (entry 0 untouched)."""
    C_ = dcat.shape[-1]
    _same_device(dcat, pre0, cat, policy, dpolicy, dh)
    if dh is None:
        dh = torch.empty(B * N, C_, dtype=torch.bfloat16, device=dcat.device)
    _lib.check(_lib.load().tr_pool_policy_bwd(_view_ptr(dcat, torch.bfloat16, "dcat"), _view_ptr(pre0, torch.bfloat16, "pre0"),
                                              _view_ptr(cat, torch.bfloat16, "cat"), _dev(policy, torch.float32, "policy"),
                                              _view_ptr(dh, torch.bfloat16, "dh"), _dev(dpolicy, torch.float32, "dpolicy"), B, N, C_, _stream(dcat)),
               "tr_pool_policy_bwd")
    return dh


def dyvit_decide(h2: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, gumbel: torch.Tensor, prev: torch.Tensor, B: int, N: int, C: int,
                 outs=None):
    """out_conv.4 + LogSoftmax + F.gumbel_softmax(hard=True)[..., 0] * prev_decision (dyvit.py:108-109, 223-224): h2 bf16 [B*N, ldh]
    (first C columns), w fp32 [2,C], gumbel fp32 [B,N-1,2], prev fp32 [B,N] -> (policy_out, ysoft0, sm0, hard0) fp32 [B,N]; CLS entries:
    policy_out 1, the others not written.  outs: the four destinations (tests prefill them)."""
    ldh = h2.shape[-1]
    _same_device(h2, w, bias, gumbel, prev)
    if outs is None:
        outs = tuple(torch.zeros(B, N, dtype=torch.float32, device=h2.device) for _ in range(4))
    _lib.check(_lib.load().tr_dyvit_decide(_dev(h2, torch.bfloat16, "h2"), ldh, _dev(w, torch.float32, "w"), _dev(bias, torch.float32, "bias"),
                                           _dev(gumbel, torch.float32, "gumbel"), _dev(prev, torch.float32, "prev"),
                                           *(_dev(t, torch.float32, "out") for t in outs), B, N, C, _stream(h2)), "tr_dyvit_decide")
    return outs


def dyvit_decide_bwd(dkeep, prev, hard0, ysoft0, sm0, h2, w, dprev, B: int, N: int, C: int, dw=None, db=None, accumulate: bool = False,
                     ws: torch.Tensor = None):
    """Backward of dyvit_decide: dkeep fp32 [B,N] -> (dh2 bf16 [B*N, ldh], dW3 fp32 [2,C], db3 fp32 [2]); dprev fp32 [B,N] += dkeep * hard0
    (CLS entries untouched).  ws: the workspace (tr_dyvit_decide_bwd_workspace_floats), allocated when None."""
    ldh = h2.shape[-1]
    _same_device(dkeep, prev, hard0, ysoft0, sm0, h2, w, dprev, dw, db, ws)
    lib = _lib.load()
    dev = h2.device
    dh2 = torch.empty(B * N, ldh, dtype=torch.bfloat16, device=dev)
    dw = torch.empty(2, C, dtype=torch.float32, device=dev) if dw is None else dw
    db = torch.empty(2, dtype=torch.float32, device=dev) if db is None else db
    if ws is None:
        ws = torch.empty(lib.tr_dyvit_decide_bwd_workspace_floats(B, N, C), dtype=torch.float32, device=dev)
    _lib.check(lib.tr_dyvit_decide_bwd(_dev(dkeep, torch.float32, "dkeep"), _dev(prev, torch.float32, "prev"), _dev(hard0, torch.float32, "hard0"),
                                       _dev(ysoft0, torch.float32, "ysoft0"), _dev(sm0, torch.float32, "sm0"), _dev(h2, torch.bfloat16, "h2"), ldh,
                                       _dev(w, torch.float32, "w"), dh2.data_ptr(), _dev(dprev, torch.float32, "dprev"),
                                       _dev(dw, torch.float32, "dw"), _dev(db, torch.float32, "db"), int(accumulate), ws.data_ptr(), ws.numel(),
                                       B, N, C, _stream(h2)), "tr_dyvit_decide_bwd")
    return dh2, dw, db


def head_sum(part: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst fp32 [B,N] += sum over the heads (in index order) of part fp32 [B,H,N]."""
    B, H, N = part.shape
    _same_device(part, dst)
    _lib.check(_lib.load().tr_head_sum(_dev(part, torch.float32, "part"), _dev(dst, torch.float32, "dst"), B, H, N, _stream(part)), "tr_head_sum")
    return dst


def add_patch_rows(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """dst fp32 [B,N][:, 1:] += src fp32 [B,N-1]; column 0 (the CLS entry) untouched."""
    B, N = dst.shape
    _same_device(dst, src)
    _lib.check(_lib.load().tr_add_patch_rows(_dev(dst, torch.float32, "dst"), _dev(src, torch.float32, "src"), B, N, _stream(dst)),
               "tr_add_patch_rows")
    return dst


def fill_f32(t: torch.Tensor, value: float, n: int = None) -> torch.Tensor:
    """The first n (default: all) elements of fp32 t := value."""
    _lib.check(_lib.load().tr_fill_f32(_dev(t, torch.float32, "t"), float(value), t.numel() if n is None else int(n), _stream(t)), "tr_fill_f32")
    return t


# ---------------------------------------------------------------------------------------- training glue (csrc/tr_backward.hip, csrc/tr_norm.hip)
def dropout(src: torch.Tensor, keep: torch.Tensor, mul: float, dst: torch.Tensor = None, n: int = None) -> torch.Tensor:
    """nn.Dropout with the caller's keep mask (uint8, non-zero = keep): dst = keep ? src * mul : 0 on the first n elements; bf16 or fp32;
    dst may be src (the executor's form)."""
    if src.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("src must be bf16 or fp32")
    dst = torch.empty_like(src) if dst is None else dst
    _same_device(src, keep, dst)
    lib = _lib.load()
    fn = lib.tr_dropout_f32 if src.dtype == torch.float32 else lib.tr_dropout_bf16
    _lib.check(fn(_view_ptr(src, src.dtype, "src"), _view_ptr(dst, src.dtype, "dst"), _view_ptr(keep, torch.uint8, "keep"), float(mul),
                  src.numel() if n is None else int(n), _stream(src)), "tr_dropout")
    return dst


def rowscale(src: torch.Tensor, scale: torch.Tensor, dst: torch.Tensor = None) -> torch.Tensor:
    """DropPath's per-image scaling: dst[b, r, :] = src[b, r, :] * scale[b], bf16 [B, rows, D]; dst may be src."""
    B, rows, D = src.shape
    dst = torch.empty_like(src) if dst is None else dst
    _same_device(src, dst, scale)
    _lib.check(_lib.load().tr_rowscale_bf16(_dev(src, torch.bfloat16, "src"), _dev(dst, torch.bfloat16, "dst"), _dev(scale, torch.float32, "scale"),
                                            B, rows, D, _stream(src)), "tr_rowscale_bf16")
    return dst


def f32_to_bf16(src: torch.Tensor) -> torch.Tensor:
    dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    _lib.check(_lib.load().tr_f32_to_bf16(_dev(src, torch.float32, "src"), dst.data_ptr(), src.numel(), _stream(src)), "tr_f32_to_bf16")
    return dst


def reduce_partials(part: torch.Tensor, dst: torch.Tensor = None, accumulate: bool = False) -> torch.Tensor:
    """dst fp32 [count] (+)= sum_s part fp32 [S, count], in the kernel's fixed order."""
    S, count = part.shape
    dst = torch.empty(count, dtype=torch.float32, device=part.device) if dst is None else dst
    _same_device(part, dst)
    _lib.check(_lib.load().tr_reduce_partials_f32(_dev(part, torch.float32, "part"), S, count, _dev(dst, torch.float32, "dst"), int(accumulate),
                                                  _stream(part)), "tr_reduce_partials_f32")
    return dst


def _rows2d(t, dtype, name):
    """(pointer, row stride) of a 2-D operand that may be a column slice of a wider tensor (unit column stride)."""
    if t.dim() != 2 or t.stride(1) != 1 or not t.is_cuda or t.dtype != dtype:
        raise ValueError(f"{name}: expected a 2-D {dtype} device tensor with unit column stride")
    return t.data_ptr(), t.stride(0)


def layernorm_to(x: torch.Tensor, x_out: torch.Tensor, gamma, beta, eps: float, delta: torch.Tensor = None, y: torch.Tensor = None,
                 ldxo: int = None, ldd: int = None) -> torch.Tensor:
    """layernorm out of place (tr_layernorm_bf16_to): x_out = x + delta, y = LayerNorm(x_out) -> bf16 [M,D]; x is not written.  x, x_out
    (fp32) and delta (bf16) are [M,D] rows, possibly column slices of wider tensors.  y: the caller's own output; ldxo / ldd override the
    row strides taken from the views."""
    M, D = x.shape
    _same_device(x, x_out, gamma, beta, delta)
    (px, ldx), (po, ldo) = _rows2d(x, torch.float32, "x"), _rows2d(x_out, torch.float32, "x_out")
    pd, sd = _rows2d(delta, torch.bfloat16, "delta") if delta is not None else (None, D)
    ldo, sd = ldo if ldxo is None else ldxo, sd if ldd is None else ldd
    y = _ln_out(y, (M, D), torch.bfloat16, "y", x.device)
    _lib.check(_lib.load().tr_layernorm_bf16_to(px, ldx, po, ldo, pd, sd, _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"),
                                                y.data_ptr(), M, D, eps, _stream(x)), "tr_layernorm_bf16_to")
    return y


def layernorm_bf16_f32(x: torch.Tensor, gamma, beta, eps: float, delta: torch.Tensor = None, delta2: torch.Tensor = None,
                       x_out: torch.Tensor = None, y: torch.Tensor = None, rows: int = None, ldx: int = None, ldxo: int = None,
                       ldd: int = None, ldd2: int = None) -> torch.Tensor:
    """The bf16 path's LayerNorm with fp32 output (tr_layernorm_bf16_f32): y fp32 [M,D] = LayerNorm((x + delta) + delta2); the sum goes to
    x_out (x itself: in place; None: not written).  y: the caller's own output; x, x_out, delta and delta2 may be 2-D column slices (their
    row stride is told to the C ABI; ldx / ldxo / ldd / ldd2 override it); rows: only that many rows."""
    D = x.shape[-1]
    M = rows if rows is not None else x.numel() // D
    _same_device(x, gamma, beta, delta, delta2, x_out)
    y = _ln_out(y, (M, D), torch.float32, "y", x.device)
    xp, sx = _ln_rows(x, torch.float32, "x", ldx)
    po, so = _ln_rows(x_out, torch.float32, "x_out", ldxo) if x_out is not None else (None, D if ldxo is None else ldxo)
    pd, sd = _ln_rows(delta, torch.bfloat16, "delta", ldd) if delta is not None else (None, D if ldd is None else ldd)
    pd2, sd2 = _ln_rows(delta2, torch.bfloat16, "delta2", ldd2) if delta2 is not None else (None, D if ldd2 is None else ldd2)
    _lib.check(_lib.load().tr_layernorm_bf16_f32(xp, sx, po, so, pd, sd, pd2, sd2, _dev(gamma, torch.float32, "gamma"),
                                                 _dev(beta, torch.float32, "beta"), y.data_ptr(), M, D, eps, _stream(x)), "tr_layernorm_bf16_f32")
    return y


def residual_snapshot(x: torch.Tensor, delta: torch.Tensor = None) -> torch.Tensor:
    """out fp32 = x + delta (bf16 or fp32, or None: a copy)."""
    out = torch.empty_like(x)
    _same_device(x, delta)
    if delta is not None and delta.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("delta must be bf16 or fp32")
    _lib.check(_lib.load().tr_residual_snapshot(_dev(x, torch.float32, "x"), None if delta is None else _dev(delta, delta.dtype, "delta"),
                                                int(delta is not None and delta.dtype == torch.float32), out.data_ptr(), x.numel(), _stream(x)),
               "tr_residual_snapshot")
    return out


def broadcast_rows(src: torch.Tensor, B: int) -> torch.Tensor:
    """dst fp32 [B,N] = src fp32 [N] in every row."""
    N = src.numel()
    dst = torch.empty(B, N, dtype=torch.float32, device=src.device)
    _lib.check(_lib.load().tr_broadcast_rows(_dev(src, torch.float32, "src"), dst.data_ptr(), B, N, _stream(src)), "tr_broadcast_rows")
    return dst


class _CastItem(ctypes.Structure):          # tr_cast_item
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("dst_t", ctypes.c_void_p), ("rows", ctypes.c_int), ("cols", ctypes.c_int)]


def cast_pack(items) -> None:
    """fp32 master weights -> bf16 operand copies, every item in ONE launch (tr_cast_pack_bf16).  items: [(src fp32 [rows, cols],
    dst bf16 [rows, cols] | None, dst_t bf16 [cols, rows] | None), ...]; the tensors may be views that start anywhere in a buffer.
    For tests: the item table is built and uploaded per call and the stream is synchronised before it is freed (the models keep a
    persistent table, models.py)."""
    n = len(items)
    arr = (_CastItem * n)()
    first = [0]
    for i, (src, dst, dst_t) in enumerate(items):
        rows, cols = src.shape
        _same_device(src, dst, dst_t, items[0][0])
        if dst is not None and tuple(dst.shape) != (rows, cols) or dst_t is not None and tuple(dst_t.shape) != (cols, rows):
            raise ValueError(f"cast_pack: item {i}: destinations do not fit a [{rows}, {cols}] source")
        arr[i] = _CastItem(_view_ptr(src, torch.float32, "src"), None if dst is None else _view_ptr(dst, torch.bfloat16, "dst"),
                           None if dst_t is None else _view_ptr(dst_t, torch.bfloat16, "dst_t"), rows, cols)
        first.append(first[-1] + ((rows + 63) // 64) * ((cols + 63) // 64))
    dev = items[0][0].device
    d_items = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    d_first = torch.tensor(first, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tr_cast_pack_bf16(d_items.data_ptr(), d_first.data_ptr(), n, first[-1], _stream(items[0][0])), "tr_cast_pack_bf16")
    torch.cuda.current_stream(dev).synchronize()          # the item table must outlive the launch


class _AdamwItem(ctypes.Structure):          # tr_adamw_item
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("dst", ctypes.c_void_p),
                ("dst_t", ctypes.c_void_p), ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("group", ctypes.c_int), ("pad_", ctypes.c_int)]


def adamw_step(items, lrs, wds, betas, eps: float, step: int, zero_grads: bool = False) -> None:
    """One AdamW step of every item in ONE launch (tr_adamw_step, csrc/tr_optim.hip).  items: [(p, g, exp_avg, exp_avg_sq fp32 of one
    shape, dst bf16 [rows, cols] | None, dst_t bf16 [cols, rows] | None, group), ...] with rows, cols as optim.FusedAdamW derives them
    (shape[0] x the rest from two dimensions on, one row below); the tensors may be views that start anywhere in a buffer.  lrs / wds: up
    to 8 learning rates / weight decays, indexed by an item's group.  step: the 1-based count of this step; the bias corrections are
    formed in double and rounded to float as optim.FusedAdamW forms them.
    For tests: the item table is built and uploaded per call and the stream is synchronised before it is freed (optim.FusedAdamW keeps a
    persistent table)."""
    import math
    n = len(items)
    if n == 0:
        raise ValueError("adamw_step: no items")
    if not 0 < len(lrs) <= 8 or len(wds) != len(lrs):
        raise ValueError(f"adamw_step: 1 to 8 learning rates and as many weight decays, got {len(lrs)} and {len(wds)}")
    if step < 1:
        raise ValueError(f"adamw_step: step counts from 1, got {step}")
    arr = (_AdamwItem * n)()
    first = [0]
    for i, (p, g, m, v, dst, dst_t, group) in enumerate(items):
        rows, cols = (p.shape[0], p.numel() // p.shape[0]) if p.dim() >= 2 else (1, p.numel())
        _same_device(p, g, m, v, dst, dst_t, items[0][0])
        if not (g.shape == p.shape and m.shape == p.shape and v.shape == p.shape) or rows * cols == 0:
            raise ValueError(f"adamw_step: item {i}: p, g, exp_avg, exp_avg_sq must share one non-empty shape")
        if dst is not None and tuple(dst.shape) != (rows, cols) or dst_t is not None and tuple(dst_t.shape) != (cols, rows):
            raise ValueError(f"adamw_step: item {i}: destinations do not fit a [{rows}, {cols}] parameter")
        if not 0 <= group < len(lrs):
            raise ValueError(f"adamw_step: item {i}: group {group} of {len(lrs)}")
        arr[i] = _AdamwItem(_view_ptr(p, torch.float32, "p"), _view_ptr(g, torch.float32, "g"), _view_ptr(m, torch.float32, "exp_avg"),
                            _view_ptr(v, torch.float32, "exp_avg_sq"), None if dst is None else _view_ptr(dst, torch.bfloat16, "dst"),
                            None if dst_t is None else _view_ptr(dst_t, torch.bfloat16, "dst_t"), rows, cols, group, 0)
        first.append(first[-1] + ((rows + 63) // 64) * ((cols + 63) // 64))
    beta1, beta2 = betas
    bc1 = 1.0 - math.pow(beta1, step)
    bc2_sqrt = math.sqrt(1.0 - math.pow(beta2, step))
    lr8 = (ctypes.c_double * 8)(*([float(x) for x in lrs] + [0.0] * (8 - len(lrs))))
    wd8 = (ctypes.c_double * 8)(*([float(x) for x in wds] + [0.0] * (8 - len(wds))))
    dev = items[0][0].device
    d_items = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    d_first = torch.tensor(first, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tr_adamw_step(d_items.data_ptr(), d_first.data_ptr(), n, first[-1], float(beta1), float(beta2), float(eps), bc1,
                                             bc2_sqrt, lr8, wd8, 1 if zero_grads else 0, _stream(items[0][0])), "tr_adamw_step")
    torch.cuda.current_stream(dev).synchronize()          # the item table must outlive the launch


LS_FOLD_ITEM = np.dtype([("w", "<u8"), ("b", "<u8"), ("gamma", "<u8"), ("dst", "<u8"), ("dst_t", "<u8"), ("b_dst", "<u8"), ("rows", "<i4"),
                         ("cols", "<i4"), ("first", "<i4"), ("pad", "<i4")])                                      # tr_ls_fold_item
LS_UNFOLD_ITEM = np.dtype([("dw_f", "<u8"), ("db_f", "<u8"), ("w", "<u8"), ("b", "<u8"), ("gamma", "<u8"), ("dw", "<u8"), ("db", "<u8"),
                           ("dgamma", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("first", "<i4"), ("pad", "<i4")])  # tr_ls_unfold_item


def layerscale_table(rows, dtype, dev):
    """The two halves of a tr_layerscale_fold / tr_layerscale_unfold_grad item table from `rows` = [(address, ..., rows, cols)] (the item's
    fields up to `cols`; 0 = NULL): dict(items = the device array, shapes = the host (rows, cols) pairs, n).  `first` is filled in here:
    the workgroups before the item, (rows/64) * (cols/64) each for the fold, rows/4 for the unfold.  Every address must be 16-byte aligned."""
    arr = np.zeros(len(rows), dtype=dtype)
    shapes = (ctypes.c_int * (2 * len(rows)))()
    first = 0
    for i, it in enumerate(rows):
        r, c = int(it[-2]), int(it[-1])
        if any(int(a) % 16 for a in it[:-2]):
            raise ValueError(f"layerscale item {i}: every operand must start on a 16-byte boundary")
        arr[i] = tuple(int(a) for a in it[:-2]) + (r, c, first, 0)
        shapes[2 * i], shapes[2 * i + 1] = r, c
        first += (r // 64) * (c // 64) if dtype is LS_FOLD_ITEM else r // 4
    return dict(items=torch.from_numpy(arr.view(np.uint8).copy()).to(dev), shapes=shapes, n=len(rows))


def layerscale_fold(items, dst_f32: bool = False) -> None:
    """LayerScale folded into the Linear that ends a branch, every item in ONE launch (tr_layerscale_fold, csrc/tr_layerscale.hip).  items:
    [(w fp32 [rows, cols], b fp32 [rows] | None, gamma fp32 [rows], dst [rows, cols] bf16 (fp32 with dst_f32) | None, dst_t bf16 [cols, rows]
    | None, b_dst fp32 [rows] | None), ...]: dst = fl32(gamma[d] * w[d, k]) (rounded to nearest-even to bf16), dst_t its transpose, b_dst =
    fl32(gamma o b).  rows and cols are multiples of 64; the tensors may be views that start on any 16-byte boundary of a buffer.
    For tests and tools: the item table is built and uploaded per call and the stream is synchronised before it is freed (the models keep
    persistent tables)."""
    rows = []
    ddt = torch.float32 if dst_f32 else torch.bfloat16
    for i, (w, b, gamma, dst, dst_t, b_dst) in enumerate(items):
        r, c = w.shape
        _same_device(w, b, gamma, dst, dst_t, b_dst, items[0][0])
        if gamma.shape != (r,) or (b is not None and b.shape != (r,)) or (b_dst is not None and (b is None or b_dst.shape != (r,))):
            raise ValueError(f"layerscale_fold: item {i}: b, gamma and b_dst must have {r} entries (b_dst needs b)")
        if dst is not None and tuple(dst.shape) != (r, c) or dst_t is not None and tuple(dst_t.shape) != (c, r):
            raise ValueError(f"layerscale_fold: item {i}: destinations do not fit a [{r}, {c}] source")
        rows.append((_view_ptr(w, torch.float32, "w"), 0 if b is None else _view_ptr(b, torch.float32, "b"), _view_ptr(gamma, torch.float32, "gamma"),
                     0 if dst is None else _view_ptr(dst, ddt, "dst"), 0 if dst_t is None else _view_ptr(dst_t, torch.bfloat16, "dst_t"),
                     0 if b_dst is None else _view_ptr(b_dst, torch.float32, "b_dst"), r, c))
    dev = items[0][0].device
    tab = layerscale_table(rows, LS_FOLD_ITEM, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tr_layerscale_fold(tab["items"].data_ptr(), tab["shapes"], tab["n"], 1 if dst_f32 else 0, _stream(items[0][0])),
                   "tr_layerscale_fold")
    torch.cuda.current_stream(dev).synchronize()          # the item table must outlive the launch


def layerscale_unfold_grad(items, accumulate: bool = False) -> None:
    """Gradients of W, b and gamma from the gradients of the folded operands, every item in ONE launch (tr_layerscale_unfold_grad).  items:
    [(dw_f fp32 [rows, cols], db_f fp32 [rows], w, b, gamma (the fp32 parameters), dw | None, db | None, dgamma | None), ...]: dw = fl(gamma
    * dw_f), db = fl(gamma * db_f), dgamma[d] = sum_k dw_f[d,k] w[d,k] + db_f[d] b[d]; with `accumulate` each is added to what the output
    holds (dw, db: fl(old + fl(gamma * x))).  A None output is not written.  Same table handling as layerscale_fold."""
    rows = []
    for i, (dw_f, db_f, w, b, gamma, dw, db, dgamma) in enumerate(items):
        r, c = dw_f.shape
        _same_device(dw_f, db_f, w, b, gamma, dw, db, dgamma, items[0][0])
        if w.shape != (r, c) or (dw is not None and dw.shape != (r, c)) or any(t is not None and t.shape != (r,) for t in (db_f, b, gamma, db, dgamma)):
            raise ValueError(f"layerscale_unfold_grad: item {i}: operands do not fit a [{r}, {c}] folded gradient")
        rows.append(tuple(0 if t is None else _view_ptr(t, torch.float32, n)
                          for t, n in zip((dw_f, db_f, w, b, gamma, dw, db, dgamma), ("dw_f", "db_f", "w", "b", "gamma", "dw", "db", "dgamma"))) + (r, c))
    dev = items[0][0].device
    tab = layerscale_table(rows, LS_UNFOLD_ITEM, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tr_layerscale_unfold_grad(tab["items"].data_ptr(), tab["shapes"], tab["n"], 1 if accumulate else 0,
                                                         _stream(items[0][0])), "tr_layerscale_unfold_grad")
    torch.cuda.current_stream(dev).synchronize()          # the item table must outlive the launch
