"""Device-side mixup / cutmix / random erasing (tokenreduction_amd.augment), CPU tier: the C boundary, the table's validation, the host
draws and the float fallback.  The reference side of every pixel comparison is `restate` below, a torch restatement of the arithmetic
the kernels are specified by (LUT gather, slice-assigned noise, timm's flip / mul_ / add_ or slice assignment from the flipped batch); it
uses neither augment.py's fallback nor the library.  tests/test_device_augment_gpu.py imports it."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from tokenreduction_amd import _lib, augment, pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD
FIELDS = ("kind", "lam", "oml", "yl", "yh", "xl", "xh", "erased", "ey", "eh", "ex", "ew", "noise_off")


def make_table(rows):
    """list of dicts (missing fields zero) -> the record array"""
    t = augment.empty_table(len(rows))
    for i, r in enumerate(rows):
        for k, v in r.items():
            assert k in FIELDS, k
            t[i][k] = v
    return t


def restate(u8, lut, table, noise):
    """The specification in torch, on u8's device: fp32 [B, C, H, W]."""
    B, C, H, W = u8.shape
    x = torch.stack([lut[c][u8[:, c].long()] for c in range(C)], dim=1).contiguous()      # lut[c][img[i,c,y,x]]
    for i in range(B):                                                                     # erasing: per image, before mixing
        r = table[i]
        if r["erased"]:
            ey, eh, ex, ew, off = int(r["ey"]), int(r["eh"]), int(r["ex"]), int(r["ew"]), int(r["noise_off"])
            x[i, :, ey:ey + eh, ex:ex + ew] = noise[off: off + C * eh * ew].view(C, eh, ew)
    x_orig = x.clone()
    for b in range(B):
        r = table[b]
        if r["kind"] == 1:
            flipped = x_orig.flip(0)[b].clone().mul_(float(r["oml"]))
            x[b].mul_(float(r["lam"])).add_(flipped)
        elif r["kind"] == 2:
            yl, yh, xl, xh = int(r["yl"]), int(r["yh"]), int(r["xl"]), int(r["xh"])
            x[b, :, yl:yh, xl:xh] = x_orig.flip(0)[b, :, yl:yh, xl:xh]
    return x


def u8_batch(B, C, S, seed):
    return torch.randint(0, 256, (B, C, S, S), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("tr_im2col_u8_aug_bf16", "tr_pixels_augment_f32", "tr_vit_forward_train_aug")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tokenreduction_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the old uint8 entry points are still there, with their signatures
    assert len(_lib.SIGNATURES["tr_im2col_u8_bf16"][1]) == 10 and len(_lib.SIGNATURES["tr_vit_forward_train_pixels"][1]) == 18
    assert len(_lib.SIGNATURES["tr_vit_forward_train_aug"][1]) == 21


def test_record_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "tokenreduction_hip.h")).read()
    body = re.search(r"typedef struct tr_augment_rec \{(.*?)\} tr_augment_rec;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.TrAugmentRec._fields_] == list(augment.REC_DTYPE.names)
    assert ctypes.sizeof(_lib.TrAugmentRec) == augment.REC_DTYPE.itemsize == 64
    for n in names:
        assert getattr(_lib.TrAugmentRec, n).offset == augment.REC_DTYPE.fields[n][1], n
    assert _lib.TrAugmentRec.noise_off.offset == 48 and _lib.TrAugmentRec.erased.offset == 28


def test_entry_points_check_their_arguments():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    for fn in (lib.tr_im2col_u8_aug_bf16, lib.tr_pixels_augment_f32):
        assert fn(p, p, 0, p, p, 16, p, 3, 3, 32, 32, 16, None) == -1 and b"even" in lib.tr_last_error()      # an odd batch
        assert fn(None, p, 0, p, p, 16, p, 4, 3, 32, 32, 16, None) == -3
        assert fn(p, None, 0, p, p, 16, p, 4, 3, 32, 32, 16, None) == -3
        assert fn(p, p, 0, None, p, 16, p, 4, 3, 32, 32, 16, None) == -3                                      # no table
        assert fn(p, p, 0, p, None, 16, p, 4, 3, 32, 32, 16, None) == -3                                      # noise_len > 0 without noise
        assert fn(p, p, 0, p, p, 16, None, 4, 3, 32, 32, 16, None) == -3
        assert fn(p + 8, p, 0, p, p, 16, p, 4, 3, 32, 32, 16, None) == -2 and fn(p, p, 0, p + 8, p, 16, p, 4, 3, 32, 32, 16, None) == -2
        assert fn(p, p, 0, p, p, 16, p + 8, 4, 3, 32, 32, 16, None) == -2 and fn(p, p, 0, p, p + 2, 16, p, 4, 3, 32, 32, 16, None) == -2
        assert fn(p, p, 2, p, p, 16, p, 4, 3, 32, 32, 16, None) == -1                                         # layout
        assert fn(p, p, 0, p, p, 16, p, 4, 3, 32, 32, 12, None) == -1 and fn(p, p, 0, p, p, 16, p, 4, 3, 40, 32, 16, None) == -1      # patch % 8, H % patch
        assert fn(p, p, 0, p, p, -1, p, 4, 3, 32, 32, 16, None) == -1
    cfg, w = _lib.TrVitConfig(), _lib.TrVitWeights()
    tokens = (ctypes.c_int * 32)()
    rest = (p, p, 4096, p, 4096, None, None, None, tokens, 4, None, None, 0.0)
    assert lib.tr_vit_forward_train_aug(ctypes.byref(cfg), ctypes.byref(w), p, 1, p, None, p, 16, *rest) == -3                        # no table
    assert lib.tr_vit_forward_train_aug(ctypes.byref(cfg), ctypes.byref(w), p, 0, p, p, p, 16, *rest) == -5                           # a float input
    odd = rest[:9] + (3,) + rest[10:]
    assert lib.tr_vit_forward_train_aug(ctypes.byref(cfg), ctypes.byref(w), p, 1, p, p, p, 16, *odd) == -1


def test_augmented_batch_validates_the_table():
    u8 = u8_batch(4, 3, 32, 0)
    noise = torch.zeros(3 * 8 * 8)
    ok = [dict(kind=2, yl=5, yh=29, xl=3, xh=21), dict(erased=1, ey=24, eh=8, ex=24, ew=8, noise_off=0), dict(kind=1, lam=0.3, oml=0.7), {}]
    batch = augment.AugmentedBatch(u8, make_table(ok), noise)
    assert tuple(batch.shape) == (4, 3, 32, 32) and batch.device == u8.device and not batch.is_cuda and batch.to("cpu") is batch
    assert batch.table.dtype == torch.uint8 and batch.table.numel() == 4 * 64 and batch.host_table.shape == (4,)
    with pytest.raises(ValueError, match="even"):
        augment.AugmentedBatch(u8[:3], make_table(ok[:3]), noise)
    bad = [dict(kind=2, yl=5, yh=33, xl=3, xh=21), dict(kind=2, yl=-1, yh=3, xl=3, xh=21), dict(kind=2, yl=9, yh=5, xl=3, xh=21),
           dict(erased=1, ey=25, eh=8, ex=24, ew=8, noise_off=0), dict(erased=1, ey=0, eh=8, ex=-1, ew=8, noise_off=0),
           dict(erased=1, ey=24, eh=8, ex=24, ew=8, noise_off=1), dict(erased=1, ey=24, eh=8, ex=24, ew=8, noise_off=-1),
           dict(erased=1, ey=0, eh=9, ex=0, ew=8, noise_off=0), dict(kind=3)]
    for r in bad:
        with pytest.raises(ValueError):
            augment.AugmentedBatch(u8, make_table([r, {}, {}, {}]), noise)
    with pytest.raises(ValueError):
        augment.AugmentedBatch(u8, make_table(ok)[:2], noise)
    with pytest.raises(ValueError, match="even"):
        augment.DeviceAugment().draw(3, 3, 32, 32)


# ---- host draws -------------------------------------------------------------------------------------------------------------------

def _one_hot(t, n, on, off):
    y = torch.full((t.shape[0], n), off)
    y[torch.arange(t.shape[0]), t] = on
    return y


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_soft_targets_equal_the_formula(mode):
    n, smoothing, B = 10, 0.1, 8
    aug = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, label_smoothing=smoothing, num_classes=n)
    targets = torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(1))
    for seed in range(6):
        _seed(seed)
        _, soft = aug(torch.zeros(B, 3, 32, 32), targets)
        _seed(seed)
        _, _, lam = aug.draw(B, 3, 32, 32)
        off = smoothing / n
        on = 1.0 - smoothing + off
        if mode == "batch":
            assert isinstance(lam, float)
        else:
            assert lam.dtype == np.float32 and lam.shape == (B,)
            if mode == "pair":
                assert np.array_equal(lam, lam[::-1])
            lam = torch.tensor(lam).unsqueeze(1)
        want = _one_hot(targets, n, on, off) * lam + _one_hot(targets.flip(0), n, on, off) * (1.0 - lam)
        assert soft.shape == (B, n) and torch.equal(soft, want), (mode, seed)
        assert torch.allclose(soft.sum(1), torch.ones(B), atol=1e-6)


def test_lam_is_corrected_for_a_box_clipped_at_the_border(monkeypatch):
    """32 x 32, lam 0.75: cut = int(32 * sqrt(0.25)) = 16.  Centre (cy, cx) = (2, 30): y [2 - 8, 2 + 8) clips to [0, 10), x [22, 38) to
    [22, 32): 10 x 10 = 100 pixels, lam = 1 - 100 / 1024."""
    aug = augment.DeviceAugment(mixup_alpha=0.0, cutmix_alpha=1.0, mode="batch")
    centres = iter([2, 30])
    monkeypatch.setattr(np.random, "rand", lambda *a: 0.0)
    monkeypatch.setattr(np.random, "beta", lambda a, b, size=None: 0.75)
    monkeypatch.setattr(np.random, "randint", lambda lo, hi=None, size=None: next(centres))
    table, noise_len, lam = aug.draw(4, 3, 32, 32)
    assert noise_len == 0 and lam == 1.0 - 100 / 1024 == 0.90234375
    assert all((r["kind"], r["yl"], r["yh"], r["xl"], r["xh"]) == (2, 0, 10, 22, 32) for r in table)
    centres = iter([2, 30])
    unc = augment.DeviceAugment(mixup_alpha=0.0, cutmix_alpha=1.0, mode="batch", correct_lam=False)
    assert unc.draw(4, 3, 32, 32)[2] == 0.75


def test_lam_one_gives_kind_zero():
    _seed(0)
    table, _, lam = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0).draw(6, 3, 32, 32)
    assert lam == 1.0 and not table["kind"].any()
    for mode in ("pair", "elem"):
        aug = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5, mode=mode, correct_lam=False)
        seen = set()
        for seed in range(20):
            _seed(seed)
            table, _, lam = aug.draw(8, 3, 32, 32)
            for b in range(8):
                assert (table[b]["kind"] == 0) == (lam[b] == 1.0), (mode, seed, b)
                seen.add(int(table[b]["kind"]))
        assert seen == {0, 1, 2}
    targets = torch.arange(6)
    _seed(0)
    _, soft = augment.DeviceAugment(prob=0.0, label_smoothing=0.1, num_classes=6)(torch.zeros(6, 3, 32, 32), targets)
    assert torch.equal(soft, _one_hot(targets, 6, 1.0 - 0.1 + 0.1 / 6, 0.1 / 6))


def test_blend_factors_follow_each_mode():
    """batch: float32(lam) and float32(1.0 - lam) with the subtraction in double; pair / elem: lam is an fp32 number and 1 - lam an fp32
    subtraction.  The two roundings of 1 - lam differ for some draws, which is why the table carries both factors."""
    differ = 0
    for seed in range(200):
        _seed(seed)
        table, _, lam = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=0.0, mode="batch").draw(4, 3, 32, 32)
        assert isinstance(lam, float) and (table["kind"] == 1).all()
        assert (table["lam"] == np.float32(lam)).all() and (table["oml"] == np.float32(1.0 - lam)).all()
        differ += np.float32(1.0 - lam) != np.float32(1) - np.float32(lam)
    assert differ > 0
    for mode in ("pair", "elem"):
        _seed(3)
        table, _, lam = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=0.0, mode=mode).draw(8, 3, 32, 32)
        assert lam.dtype == np.float32 and (table["kind"] == 1).all()
        assert np.array_equal(table["lam"], lam) and np.array_equal(table["oml"], np.float32(1) - lam)
        if mode == "pair":
            assert np.array_equal(table["lam"], table["lam"][::-1])


def test_erase_boxes_stay_inside_the_image():
    H, W, C = 48, 32, 3
    aug = augment.DeviceAugment(mixup_alpha=0.0, cutmix_alpha=0.0, re_prob=1.0)
    _seed(11)
    n_erased = 0
    for _ in range(250):                              # 250 batches of 4: 1,000 images
        table, noise_len, _ = aug.draw(4, C, H, W)
        off = 0
        for r in table:
            if not r["erased"]:
                continue
            n_erased += 1
            assert 0 < r["eh"] < H and 0 < r["ew"] < W
            assert 0 <= r["ey"] and r["ey"] + r["eh"] <= H and 0 <= r["ex"] and r["ex"] + r["ew"] <= W
            assert r["noise_off"] == off
            off += C * int(r["eh"]) * int(r["ew"])
        assert off == noise_len
        augment.validate_table(table, C, H, W, noise_len)
    assert n_erased > 900                             # re_prob 1: only ten failed attempts in a row leave an image alone
    _seed(11)
    assert not augment.DeviceAugment(re_prob=0.0).draw(4, C, H, W)[0]["erased"].any()


def test_same_seeds_give_the_same_table():
    aug = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", re_prob=0.5)
    _seed(5)
    a = aug.draw(8, 3, 48, 48)
    _seed(5)
    b = aug.draw(8, 3, 48, 48)
    _seed(6)
    c = aug.draw(8, 3, 48, 48)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert a[0].tobytes() != c[0].tobytes()


# ---- the float fallback -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("re_mode", ["pixel", "rand", "const"])
@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_float_fallback_equals_the_restatement(mode, re_mode):
    B, C, S = 6, 3, 32
    lut = pixels.pixel_lut(MEAN, STD)
    aug = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, re_prob=0.6, re_mode=re_mode, num_classes=10)
    targets = torch.arange(B)
    kinds = set()
    for seed in range(8):
        u8 = u8_batch(B, C, S, seed)
        xf = torch.stack([lut[c][u8[:, c].long()] for c in range(C)], dim=1)
        _seed(seed)
        got, _ = aug(xf.clone(), targets)
        _seed(seed)
        table, noise_len, _ = aug.draw(B, C, S, S)
        noise = aug._draw_noise(table, C, noise_len, "cpu")
        assert noise.shape == (noise_len,)
        if re_mode == "const":
            assert not noise.any()
        elif re_mode == "rand" and noise_len:
            r = table[table["erased"] != 0][0]
            blk = noise[int(r["noise_off"]): int(r["noise_off"]) + C * int(r["eh"]) * int(r["ew"])].view(C, -1)
            assert (blk == blk[:, :1]).all() and blk[:, 0].unique().numel() == C
        assert got.dtype == torch.float32 and torch.equal(got, restate(u8, lut, table, noise)), (mode, re_mode, seed)
        kinds |= set(table["kind"].tolist())
        # ... and a uint8 batch gets the same table, untouched pixels and the same noise
        _seed(seed)
        batch, _ = aug(u8, targets)
        assert isinstance(batch, augment.AugmentedBatch) and batch.host_table.tobytes() == table.tobytes()
        assert torch.equal(batch.noise, noise) and batch.pixels is u8
    assert kinds >= {1, 2}
