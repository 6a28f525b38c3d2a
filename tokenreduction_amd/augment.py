"""Device-side mixup, cutmix and random erasing for uint8 training batches.

The reference's default recipe (train.py:120-141: --reprob 0.25 --remode pixel --mixup 0.8 --cutmix 1.0 --mixup-mode batch --smoothing 0.1)
erases in the loader after normalization (datasets.py:93-95, timm RandomErasing) and mixes in the loop (train.py:313-319 builds
timm.data.Mixup, engine.py:47-48 applies it to the normalized batch).  Both act on normalized floats, so a loader that ships raw uint8
pixels (model.set_pixel_input) cannot run them itself.  `DeviceAugment` is the replacement for both: called as `mixup_fn(samples, targets)`
it draws every parameter on the host, writes them into a table of one 64-byte record per image (tr_augment_rec,
include/tokenreduction_hip.h), draws the erase noise on the device in one torch.randn, and returns an `AugmentedBatch` -- the untouched
uint8 pixels plus the table -- and the soft targets.  A model with set_pixel_input on, in train mode, unfolds that batch through
tr_im2col_u8_aug_bf16, which erases, blends and pastes while it normalizes; everything else materializes the fp32 image with
`AugmentedBatch.float()` (tr_pixels_augment_f32).

The arithmetic (bit for bit what the kernels compute; partner of image b in an even batch B is j = B - 1 - b, timm's x.flip(0)):

    src(i) = the normalized image i with its erase box overwritten by its noise block          (erasing happens before mixing)
    kind 0: out = src(b)     kind 1: out = rn(rn(src(b) * lam) + rn(src(j) * oml))     kind 2: out = src(j) inside the box, src(b) outside

The host draws restate timm 0.4.12 from its source (timm/data/mixup.py: Mixup._params_per_batch / _params_per_elem, rand_bbox,
rand_bbox_minmax, cutmix_bbox_and_lam, mixup_target; timm/data/random_erasing.py: RandomErasing._erase with its ten attempts) in the same
order of numpy / `random` calls.  timm is not a dependency of this package and is not installed where its tests run, so the draw order
is restated, not pinned against timm itself.  One erase box per image (--recount 1).

Given a float batch (already normalized: the float loader, or a CPU tensor) the same drawn parameters are applied with plain torch ops,
so one training loop serves both loaders.
"""
from __future__ import annotations

import ctypes as C
import math
import random
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, pixels

KIND_NONE, KIND_BLEND, KIND_PASTE = 0, 1, 2

# tr_augment_rec, field for field (natural alignment puts noise_off at byte 48; 64 bytes per record)
REC_DTYPE = np.dtype([("kind", "<i4"), ("lam", "<f4"), ("oml", "<f4"), ("yl", "<i4"), ("yh", "<i4"), ("xl", "<i4"), ("xh", "<i4"),
                      ("erased", "<i4"), ("ey", "<i4"), ("eh", "<i4"), ("ex", "<i4"), ("ew", "<i4"), ("noise_off", "<i8"),
                      ("reserved_", "<i4", (2,))])
assert REC_DTYPE.itemsize == C.sizeof(_lib.TrAugmentRec) == 64


def empty_table(B: int) -> np.ndarray:
    """B all-zero records: nothing erased, nothing mixed (the bits of the plain uint8 path)."""
    return np.zeros(B, dtype=REC_DTYPE)


def validate_table(table: np.ndarray, C_: int, H: int, W: int, noise_len: int) -> None:
    """ValueError unless the batch is even, every kind is known, every box lies inside the image and every erased image's [C, eh, ew]
    noise block lies inside the noise buffer.  (The kernels clamp all of this themselves; this is what turns a wrong table into an
    error instead of wrong pixels.)"""
    if table.dtype != REC_DTYPE or table.ndim != 1:
        raise ValueError("the augmentation table must be a 1-D array of augment.REC_DTYPE records")
    B = table.shape[0]
    if B == 0 or B % 2:
        raise ValueError(f"the batch must be even (image b mixes with image B - 1 - b), got {B} images")
    for b, r in enumerate(table):
        kind = int(r["kind"])
        if kind not in (KIND_NONE, KIND_BLEND, KIND_PASTE):
            raise ValueError(f"image {b}: unknown kind {kind}")
        if kind == KIND_BLEND and not (math.isfinite(float(r["lam"])) and math.isfinite(float(r["oml"]))):
            raise ValueError(f"image {b}: blend factors {float(r['lam'])}, {float(r['oml'])} are not finite")
        if kind == KIND_PASTE and not (0 <= r["yl"] <= r["yh"] <= H and 0 <= r["xl"] <= r["xh"] <= W):
            raise ValueError(f"image {b}: paste box y [{r['yl']}, {r['yh']}) x [{r['xl']}, {r['xh']}) is outside the {H} x {W} image")
        if r["erased"]:
            ey, eh, ex, ew, off = (int(r[k]) for k in ("ey", "eh", "ex", "ew", "noise_off"))
            if not (eh > 0 and ew > 0 and 0 <= ey and ey + eh <= H and 0 <= ex and ex + ew <= W):
                raise ValueError(f"image {b}: erase box y [{ey}, {ey + eh}) x [{ex}, {ex + ew}) is empty or outside the {H} x {W} image")
            if off < 0 or off + C_ * eh * ew > noise_len:
                raise ValueError(f"image {b}: noise block [{off}, {off + C_ * eh * ew}) is outside the noise buffer of {noise_len} floats")


class AugmentedBatch:
    """A uint8 batch [B, C, H, W] (contiguous or channels_last) with the augmentation still to be applied: `table` (device, B records as
    bytes), `noise` (device, packed fp32) and `host_table` (the records as a numpy array).  Quacks like the tensor where a training loop
    touches its samples: .shape, .device, .is_cuda, .to(); .float() is the augmented, normalized fp32 image [B, C, H, W] (HIP)."""

    def __init__(self, pixels_u8: torch.Tensor, host_table: np.ndarray, noise: Optional[torch.Tensor] = None,
                 mean: Sequence[float] = pixels.IMAGENET_DEFAULT_MEAN, std: Sequence[float] = pixels.IMAGENET_DEFAULT_STD):
        if pixels_u8.dtype != torch.uint8 or pixels_u8.dim() != 4:
            raise TypeError(f"expected uint8 pixels [B, C, H, W], got {pixels_u8.dtype} {tuple(pixels_u8.shape)}")
        B, Cc, H, W = pixels_u8.shape
        if noise is None:
            noise = torch.zeros(0, dtype=torch.float32, device=pixels_u8.device)
        if noise.dtype != torch.float32 or noise.dim() != 1:
            raise TypeError("noise must be a 1-D fp32 tensor")
        host_table = np.ascontiguousarray(host_table)
        if host_table.shape != (B,):
            raise ValueError(f"{host_table.shape[0] if host_table.ndim else 0} records for {B} images")
        validate_table(host_table, Cc, H, W, noise.numel())
        self.mean_std = pixels.check_mean_std(mean, std, Cc)
        self.pixels = pixels_u8
        self.host_table = host_table
        self.noise = noise.contiguous().to(pixels_u8.device)
        self.table = torch.from_numpy(host_table.view(np.uint8).reshape(-1).copy()).to(pixels_u8.device)
        self._lut = None
        self._float = None

    shape = property(lambda self: self.pixels.shape)
    device = property(lambda self: self.pixels.device)
    is_cuda = property(lambda self: self.pixels.is_cuda)
    dtype = property(lambda self: self.pixels.dtype)

    def __len__(self):
        return self.pixels.shape[0]

    def size(self, dim=None):
        return self.pixels.size() if dim is None else self.pixels.size(dim)

    def to(self, *args, **kwargs):
        """The batch on another device (device arguments only: the pixels stay uint8)."""
        moved = self.pixels.to(*args, **kwargs)
        if moved.dtype != torch.uint8:
            raise TypeError("AugmentedBatch.to() moves the batch between devices; use .float() for the augmented fp32 image")
        if moved.device == self.pixels.device:
            return self
        new = object.__new__(AugmentedBatch)
        new.__dict__.update(self.__dict__)
        new.pixels, new.noise, new.table = moved, self.noise.to(moved.device), self.table.to(moved.device)
        new._lut = new._float = None
        return new

    def cuda(self, device=None):
        return self.to(torch.device("cuda") if device is None else device)

    def lut(self) -> torch.Tensor:
        if self._lut is None:
            self._lut = pixels.pixel_lut(*self.mean_std).to(self.device)
        return self._lut

    def float(self) -> torch.Tensor:
        """The augmented, normalized image, fp32 [B, C, H, W] contiguous -- what the float pipeline would hold (tr_pixels_augment_f32;
        computed once per batch)."""
        if self._float is None:
            from . import ops
            px = self.pixels
            if not (px.is_contiguous() or px.is_contiguous(memory_format=torch.channels_last)) or px.data_ptr() % 16:
                px = px.clone(memory_format=torch.contiguous_format)
            self._float = ops.pixels_augment(px, self.lut(), self.table, self.noise)
        return self._float


def _one_hot(target: torch.Tensor, num_classes: int, on: float, off: float) -> torch.Tensor:
    t = target.long().view(-1, 1)
    return torch.full((t.shape[0], num_classes), off, device=target.device).scatter_(1, t, on)


def soft_targets(target: torch.Tensor, num_classes: int, lam, smoothing: float) -> torch.Tensor:
    """timm mixup_target: smoothed one-hot rows of the batch and of the flipped batch, mixed with lam (a float, or an fp32 column [B, 1])."""
    off = smoothing / num_classes
    on = 1.0 - smoothing + off
    y1 = _one_hot(target, num_classes, on, off)
    y2 = _one_hot(target.flip(0), num_classes, on, off)
    return y1 * lam + y2 * (1.0 - lam)


def _rand_bbox(H: int, W: int, lam: float) -> Tuple[int, int, int, int]:
    """timm rand_bbox (margin 0): a box of sqrt(1 - lam) of each side around a uniform centre, clipped to the image."""
    ratio = np.sqrt(1 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    cy = np.random.randint(0, H)
    cx = np.random.randint(0, W)
    yl, yh = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
    xl, xh = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
    return int(yl), int(yh), int(xl), int(xh)


def _rand_bbox_minmax(H: int, W: int, minmax) -> Tuple[int, int, int, int]:
    """timm rand_bbox_minmax: side lengths uniform in [min, max) of the image's, placed uniformly inside it."""
    cut_h = np.random.randint(int(H * minmax[0]), int(H * minmax[1]))
    cut_w = np.random.randint(int(W * minmax[0]), int(W * minmax[1]))
    yl = np.random.randint(0, H - cut_h)
    xl = np.random.randint(0, W - cut_w)
    return int(yl), int(yl + cut_h), int(xl), int(xl + cut_w)


class DeviceAugment:
    """timm.data.Mixup's arguments plus RandomErasing's (re_prob, re_mode in pixel | rand | const, re_min_area, re_max_area,
    re_min_aspect; one box per image), and the (mean, std) a uint8 batch is normalized with.  `mixup_fn(samples, targets)` returns
    (AugmentedBatch, soft targets) for a uint8 batch and (augmented fp32 tensor, soft targets) for a float batch (see the module text)."""

    def __init__(self, mixup_alpha: float = 1.0, cutmix_alpha: float = 0.0, cutmix_minmax=None, prob: float = 1.0, switch_prob: float = 0.5,
                 mode: str = "batch", correct_lam: bool = True, label_smoothing: float = 0.1, num_classes: int = 1000,
                 re_prob: float = 0.0, re_mode: str = "pixel", re_min_area: float = 0.02, re_max_area: float = 1 / 3,
                 re_min_aspect: float = 0.3, mean: Sequence[float] = pixels.IMAGENET_DEFAULT_MEAN,
                 std: Sequence[float] = pixels.IMAGENET_DEFAULT_STD):
        if mode not in ("batch", "pair", "elem"):
            raise ValueError(f"mode must be batch, pair or elem, got {mode!r}")
        if re_mode not in ("pixel", "rand", "const"):
            raise ValueError(f"re_mode must be pixel, rand or const, got {re_mode!r}")
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = mixup_alpha, cutmix_alpha, cutmix_minmax
        if cutmix_minmax is not None:
            if len(cutmix_minmax) != 2:
                raise ValueError("cutmix_minmax needs two entries")
            self.cutmix_alpha = 1.0          # timm: minmax forces cutmix on with alpha 1
        self.mix_prob, self.switch_prob, self.mode, self.correct_lam = prob, switch_prob, mode, correct_lam
        self.label_smoothing, self.num_classes = label_smoothing, num_classes
        self.mixup_enabled = (self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0)
        self.re_prob, self.re_mode = re_prob, re_mode
        self.re_min_area, self.re_max_area = re_min_area, re_max_area
        self.re_log_aspect = (math.log(re_min_aspect), math.log(1 / re_min_aspect))
        self.mean, self.std = tuple(mean), tuple(std)

    # ---- host draws -----------------------------------------------------------------------------------------------------------------
    def _params_per_elem(self, n: int):
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = np.random.rand(n) < self.switch_prob
                lam_mix = np.where(use_cutmix, np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n),
                                   np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n))
            elif self.mixup_alpha > 0.0:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            else:
                use_cutmix = np.ones(n, dtype=bool)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            lam = np.where(np.random.rand(n) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _params_per_batch(self):
        lam, use_cutmix = 1.0, False
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = bool(np.random.rand() < self.switch_prob)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else \
                    np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.0:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha)
            else:
                use_cutmix = True
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha)
            lam = float(lam_mix)
        return lam, use_cutmix

    def _cutmix_box_and_lam(self, H: int, W: int, lam):
        """timm cutmix_bbox_and_lam: the box, and lam corrected to the area the (clipped) box really covers."""
        if self.cutmix_minmax is not None:
            yl, yh, xl, xh = _rand_bbox_minmax(H, W, self.cutmix_minmax)
        else:
            yl, yh, xl, xh = _rand_bbox(H, W, lam)
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1.0 - (yh - yl) * (xh - xl) / float(H * W)
        return (yl, yh, xl, xh), lam

    def _draw_erase(self, table: np.ndarray, Cc: int, H: int, W: int) -> int:
        """RandomErasing._erase per image (count 1): up to ten attempts at a box with h < H and w < W.  Returns the packed noise length."""
        n = 0
        if self.re_prob <= 0.0:
            return n
        area = H * W
        for r in table:
            if random.random() > self.re_prob:
                continue
            for _ in range(10):
                target_area = random.uniform(self.re_min_area, self.re_max_area) * area
                aspect = math.exp(random.uniform(*self.re_log_aspect))
                h = int(round(math.sqrt(target_area * aspect)))
                w = int(round(math.sqrt(target_area / aspect)))
                if w < W and h < H:
                    top = random.randint(0, H - h)
                    left = random.randint(0, W - w)
                    if h > 0 and w > 0:                 # (a box of no pixels erases nothing)
                        r["erased"], r["ey"], r["eh"], r["ex"], r["ew"], r["noise_off"] = 1, top, h, left, w, n
                        n += Cc * h * w
                    break
        return n

    def _draw_mix(self, table: np.ndarray, H: int, W: int):
        """Mixup._mix_batch / _mix_pair / _mix_elem without the pixels: fills kind, factors and boxes; returns lam for the targets (a float
        in batch mode, an fp32 array per image otherwise)."""
        B = table.shape[0]
        one = np.float32(1.0)
        if self.mode == "batch":
            lam, use_cutmix = self._params_per_batch()
            if lam == 1.0:
                return 1.0
            if use_cutmix:
                (yl, yh, xl, xh), lam = self._cutmix_box_and_lam(H, W, lam)
                table["kind"] = KIND_PASTE
                table["yl"], table["yh"], table["xl"], table["xh"] = yl, yh, xl, xh
            else:
                table["kind"] = KIND_BLEND
                table["lam"], table["oml"] = np.float32(lam), np.float32(1.0 - lam)      # x.mul_(lam), x.flip(0).mul_(1. - lam): 1 - lam in double
            return lam
        n = B // 2 if self.mode == "pair" else B
        lam_batch, use_cutmix = self._params_per_elem(n)
        for i in range(n):
            j = B - i - 1
            lam = lam_batch[i]
            if lam != 1.0:
                rows = (i, j) if self.mode == "pair" else (i,)
                if use_cutmix[i]:
                    (yl, yh, xl, xh), lam = self._cutmix_box_and_lam(H, W, lam)
                    for r in rows:
                        table[r]["kind"] = KIND_PASTE
                        table[r]["yl"], table[r]["yh"], table[r]["xl"], table[r]["xh"] = yl, yh, xl, xh
                    lam_batch[i] = lam
                else:
                    for r in rows:
                        table[r]["kind"] = KIND_BLEND
                        table[r]["lam"], table[r]["oml"] = lam, one - lam             # x[i] * lam + x_orig[j] * (1 - lam) with lam an np.float32
        if self.mode == "pair":
            lam_batch = np.concatenate((lam_batch, lam_batch[::-1]))
        return lam_batch

    def draw(self, B: int, Cc: int, H: int, W: int):
        """(table, noise_len, lam): the erase draws of the B images first (the loader's step), then the mix draws (the loop's step)."""
        if B % 2:
            raise ValueError(f"the batch must be even (image b mixes with image B - 1 - b), got {B} images")
        table = empty_table(B)
        noise_len = self._draw_erase(table, Cc, H, W)
        lam = self._draw_mix(table, H, W)
        return table, noise_len, lam

    def _draw_noise(self, table: np.ndarray, Cc: int, noise_len: int, device) -> torch.Tensor:
        if self.re_mode == "const" or noise_len == 0:
            return torch.zeros(noise_len, dtype=torch.float32, device=device)
        if self.re_mode == "pixel":
            return torch.randn(noise_len, dtype=torch.float32, device=device)
        er = table[table["erased"] != 0]                                      # rand: one normal per channel, over the channel's box
        counts = torch.as_tensor(np.repeat(er["eh"].astype(np.int64) * er["ew"].astype(np.int64), Cc), device=device)
        return torch.repeat_interleave(torch.randn(er.shape[0] * Cc, dtype=torch.float32, device=device), counts)

    # ---- the call -------------------------------------------------------------------------------------------------------------------
    def __call__(self, samples, targets: torch.Tensor):
        B, Cc, H, W = samples.shape
        table, noise_len, lam = self.draw(B, Cc, H, W)
        noise = self._draw_noise(table, Cc, noise_len, samples.device)
        if not isinstance(lam, float):
            lam = torch.tensor(lam, device=targets.device, dtype=torch.float32).unsqueeze(1)
        soft = soft_targets(targets, self.num_classes, lam, self.label_smoothing)
        if samples.dtype == torch.uint8:
            return AugmentedBatch(samples, table, noise, self.mean, self.std), soft
        return apply_to_float(samples, table, noise), soft


def apply_to_float(x: torch.Tensor, table: np.ndarray, noise: torch.Tensor) -> torch.Tensor:
    """The table applied to an already normalized float batch [B, C, H, W] with plain torch ops (any device): the float loader's path.
    Erases in place (as the loader would have), returns the mixed batch."""
    B, Cc, H, W = x.shape
    validate_table(table, Cc, H, W, noise.numel())
    for b, r in enumerate(table):
        if r["erased"]:
            ey, eh, ex, ew, off = (int(r[k]) for k in ("ey", "eh", "ex", "ew", "noise_off"))
            x[b, :, ey:ey + eh, ex:ex + ew] = noise[off: off + Cc * eh * ew].view(Cc, eh, ew).to(x.dtype)
    kinds = table["kind"]
    if not kinds.any():
        return x
    partner = x.flip(0)
    out = x.clone()
    blend = np.flatnonzero(kinds == KIND_BLEND)
    if blend.size:
        idx = torch.as_tensor(blend, device=x.device)
        lam = torch.as_tensor(table["lam"][blend].copy(), device=x.device).to(x.dtype).view(-1, 1, 1, 1)
        oml = torch.as_tensor(table["oml"][blend].copy(), device=x.device).to(x.dtype).view(-1, 1, 1, 1)
        out[idx] = (x[idx] * lam).add_(partner[idx] * oml)
    for b in np.flatnonzero(kinds == KIND_PASTE):
        yl, yh, xl, xh = (int(table[b][k]) for k in ("yl", "yh", "xl", "xh"))
        out[b, :, yl:yh, xl:xh] = partner[b, :, yl:yh, xl:xh]
    return out
