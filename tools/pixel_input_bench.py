"""Raw uint8 image input (model.set_pixel_input): what it does to the patch embedding and to a data loop.

    python tools/pixel_input_bench.py kernels [--shape deit_s_224|deit_b_224|deit_s_448]
        fp32 / uint8 NCHW / uint8 NHWC patch embedding at batch 256, 50 launches each (checks that the three give the same bits).
        Kernel times: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/pixel_input_bench.py kernels --shape ...`
        (patch_embed_kernel<0> = fp32, <1> = uint8 NCHW, <2> = uint8 NHWC); the event times it prints include the launch gaps.
    python tools/pixel_input_bench.py e2e
        DeiT-S Top-K kr 0.7, batch 256, forward_async with one batch of lookahead: every batch goes from pinned host memory through an
        H2D copy on a copy stream into a ring of three device buffers, overlapped with the forwards.  images/s for fp32 (normalized on the
        host), uint8 NCHW and uint8 NHWC, and the bandwidth of the H2D copy alone.  Prints one JSON line per leg.
    python tools/pixel_input_bench.py train
        DeiT-S Top-K kr 0.7, batch 128, forward + backward + FusedAdamW with the reference's default recipe (mixup 0.8, cutmix 1.0, batch
        mode, reprob 0.25 pixel), every batch copied from pinned host memory: (a) an fp32 loader with torch mixup / cutmix and erasing on the
        device, (b) the uint8 loader with augment.DeviceAugment.  images/s and ms per step, one JSON line per side.
    python tools/pixel_input_bench.py kernels --aug
        The training unfold at batch 128: im2col_u8_kernel against im2col_u8_aug_kernel with a none table, a blend table and a paste +
        erase table, 50 launches each (event times; kernel medians from `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tokenreduction_amd as tra  # noqa: E402
from tokenreduction_amd import ops, pixels  # noqa: E402

SHAPES = {"deit_s_224": (384, 224), "deit_b_224": (768, 224), "deit_s_448": (384, 448)}
MEAN, STD = pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD


def normalized(u8):
    return ((u8.float() / 255) - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]


def kernels(shape, B=256, reps=50):
    D, S = SHAPES[shape]
    g = torch.Generator().manual_seed(0)
    P = (S // 16) ** 2
    w = (0.02 * torch.randn(D, 768, generator=g)).bfloat16().cuda()
    b, cls = (0.02 * torch.randn(D, generator=g)).cuda(), (0.02 * torch.randn(D, generator=g)).cuda()
    pos = (0.02 * torch.randn(P + 1, D, generator=g)).cuda()
    u8 = torch.randint(0, 256, (B, 3, S, S), generator=g, dtype=torch.uint8)
    xf = normalized(u8).cuda()
    nchw = u8.cuda()
    nhwc = nchw.contiguous(memory_format=torch.channels_last)
    lut = pixels.pixel_lut(MEAN, STD).cuda()
    legs = {"fp32": lambda: ops.patch_embed(xf, w, b, cls, pos), "u8_nchw": lambda: ops.patch_embed_u8(nchw, lut, w, b, cls, pos),
            "u8_nhwc": lambda: ops.patch_embed_u8(nhwc, lut, w, b, cls, pos)}
    ref = legs["fp32"]()
    for name, fn in legs.items():
        assert torch.equal(fn(), ref), f"{name} differs from fp32"
    out = {"shape": shape, "B": B, "D": D, "S": S}
    for name, fn in legs.items():
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[f"{name}_event_us"] = round(1000.0 * e0.elapsed_time(e1) / reps, 2)
    print(json.dumps(out), flush=True)


def e2e(steps=60, warmup=10, B=256):
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False)
    torch.manual_seed(0)
    m = tra.create_model("topk_small_patch16_224", pretrained=False, num_classes=1000, args=args).cuda().eval()
    m.set_pixel_input(MEAN, STD)
    g = torch.Generator().manual_seed(1)
    host_u8 = [torch.randint(0, 256, (B, 3, 224, 224), generator=g, dtype=torch.uint8) for _ in range(2)]
    legs = {"fp32": [normalized(h).pin_memory() for h in host_u8],
            "u8_nchw": [h.pin_memory() for h in host_u8],
            "u8_nhwc": [h.contiguous(memory_format=torch.channels_last).pin_memory() for h in host_u8]}
    # the three legs compute the same logits
    want = m(legs["fp32"][0].cuda()).clone()
    for name in ("u8_nchw", "u8_nhwc"):
        assert torch.equal(m(legs[name][0].cuda()), want), name
    cs = torch.cuda.Stream()
    cur = torch.cuda.current_stream()
    for name, host in legs.items():
        ring = [torch.empty_like(host[0], device="cuda") for _ in range(3)]
        # H2D copy alone
        for _ in range(3):
            ring[0].copy_(host[0], non_blocking=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(20):
            ring[i % 3].copy_(host[i % 2], non_blocking=True)
        torch.cuda.synchronize()
        copy_gbs = 20 * host[0].numel() * host[0].element_size() / (time.perf_counter() - t0) / 1e9
        free = [None] * 3

        def run(n):
            pending = None
            for i in range(n):
                k = i % 3
                with torch.cuda.stream(cs):
                    if free[k] is not None:
                        cs.wait_event(free[k])             # the forward that read this buffer is done
                    ring[k].copy_(host[i % 2], non_blocking=True)
                    ready = torch.cuda.Event()
                    ready.record(cs)
                cur.wait_event(ready)
                h = m.forward_async(ring[k])
                if pending is not None:
                    pending[0].result().argmax(-1)
                    ev = torch.cuda.Event()
                    ev.record(cur)
                    free[pending[1]] = ev
                pending = (h, k)
            pending[0].result()
            torch.cuda.synchronize()
        run(warmup)
        t0 = time.perf_counter()
        run(steps)
        dt = time.perf_counter() - t0
        print(json.dumps({"leg": name, "B": B, "steps": steps, "images_per_s": round(steps * B / dt, 1), "ms_per_batch": round(1e3 * dt / steps, 3),
                          "bytes_per_batch": host[0].numel() * host[0].element_size(), "h2d_copy_alone_GBps": round(copy_gbs, 2)}), flush=True)
    m.check_status()


def _event_us(fn, reps=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(1000.0 * e0.elapsed_time(e1) / reps, 2)


def kernels_aug(B=128, S=224):
    from tokenreduction_amd import augment
    g = torch.Generator().manual_seed(0)
    nchw = torch.randint(0, 256, (B, 3, S, S), generator=g, dtype=torch.uint8).cuda()
    lut = pixels.pixel_lut(MEAN, STD).cuda()
    none = augment.empty_table(B)
    blend = augment.empty_table(B)
    blend["kind"], blend["lam"], blend["oml"] = 1, 0.3, 0.7
    paste = augment.empty_table(B)                        # a cutmix box of half the image's area; every fourth image erased (15 % of its area)
    paste["kind"], paste["yl"], paste["yh"], paste["xl"], paste["xh"] = 2, 33, 191, 29, 187
    n = 0
    for r in paste[::4]:
        r["erased"], r["ey"], r["eh"], r["ex"], r["ew"], r["noise_off"] = 1, 40, 77, 50, 98, n
        n += 3 * 77 * 98
    noise = torch.randn(n, device="cuda")
    up = lambda t: torch.from_numpy(t.view("u1").copy()).cuda()      # noqa: E731
    tabs = {"aug_none": (up(none), noise[:0]), "aug_blend": (up(blend), noise[:0]), "aug_paste_erase": (up(paste), noise)}
    assert torch.equal(ops.im2col_u8_aug(nchw, lut, *tabs["aug_none"], 16).view(torch.int16), ops.im2col_u8(nchw, lut, 16).view(torch.int16))
    out = {"B": B, "S": S}
    for lay, img in (("nchw", nchw), ("nhwc", nchw.contiguous(memory_format=torch.channels_last))):
        out[f"{lay}_im2col_u8_event_us"] = _event_us(lambda: ops.im2col_u8(img, lut, 16))
        for name, (tab, nz) in tabs.items():
            out[f"{lay}_{name}_event_us"] = _event_us(lambda: ops.im2col_u8_aug(img, lut, tab, nz, 16))
    print(json.dumps(out), flush=True)


class _TorchRecipe:
    """The float side of the `train` leg: timm's RandomErasing (pixel mode, per image) and Mixup (batch mode) written with torch ops on the
    normalized device batch -- what a loop started from the reference's command line runs today.  Same draws as DeviceAugment."""

    def __init__(self, aug):
        self.aug = aug

    def __call__(self, x, target):
        from tokenreduction_amd import augment
        B, Cc, H, W = x.shape
        table, noise_len, lam = self.aug.draw(B, Cc, H, W)
        for b, r in enumerate(table):
            if r["erased"]:
                ey, eh, ex, ew = int(r["ey"]), int(r["eh"]), int(r["ex"]), int(r["ew"])
                x[b, :, ey:ey + eh, ex:ex + ew] = torch.empty((Cc, eh, ew), dtype=x.dtype, device=x.device).normal_()
        k = int(table["kind"][0])
        if k == augment.KIND_PASTE:
            yl, yh, xl, xh = (int(table[0][f]) for f in ("yl", "yh", "xl", "xh"))
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        elif k == augment.KIND_BLEND:
            x_flipped = x.flip(0).mul_(1.0 - lam)
            x.mul_(lam).add_(x_flipped)
        return x, augment.soft_targets(target, self.aug.num_classes, lam, self.aug.label_smoothing)


def train(steps=40, warmup=8, B=128):
    import random
    import numpy as np
    from tokenreduction_amd import augment
    from tokenreduction_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(1)
    host_u8 = [torch.randint(0, 256, (B, 3, 224, 224), generator=g, dtype=torch.uint8) for _ in range(2)]
    host_y = [torch.randint(0, 1000, (B,), generator=g).pin_memory() for _ in range(2)]
    aug = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1,
                                num_classes=1000, re_prob=0.25, re_mode="pixel")
    sides = {"a_fp32_torch_mixup": ([normalized(h).pin_memory() for h in host_u8], _TorchRecipe(aug)),
             "b_uint8_device_augment": ([h.pin_memory() for h in host_u8], aug)}
    for name, (host, mix) in sides.items():
        args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False)
        torch.manual_seed(0)
        random.seed(0)
        np.random.seed(0)
        m = tra.create_model("topk_small_patch16_224", pretrained=False, num_classes=1000, args=args).cuda().train()
        m.set_pixel_input(MEAN, STD)
        opt = FusedAdamW(list(m.parameters()), lr=1e-4, weight_decay=0.05, model=m)

        def run(n):
            for i in range(n):
                x = host[i % 2].to("cuda", non_blocking=True)
                y = host_y[i % 2].to("cuda", non_blocking=True)
                x, soft = mix(x, y)
                loss = torch.sum(-soft * torch.nn.functional.log_softmax(m(x).float(), dim=-1), dim=-1).mean()
                loss.backward()
                opt.step()
                opt.zero_grad()
            torch.cuda.synchronize()
            return loss.item()
        run(warmup)
        t0 = time.perf_counter()
        last = run(steps)
        dt = time.perf_counter() - t0
        print(json.dumps({"side": name, "B": B, "steps": steps, "images_per_s": round(steps * B / dt, 1), "ms_per_step": round(1e3 * dt / steps, 3),
                          "h2d_bytes_per_step": host[0].numel() * host[0].element_size(), "last_loss": round(last, 4)}), flush=True)
        del m, opt


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "e2e", "train"])
    ap.add_argument("--shape", default="deit_s_224", choices=list(SHAPES))
    ap.add_argument("--aug", action="store_true", help="kernels: the training unfold with and without the augmentation table")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.what == "kernels":
        kernels_aug() if a.aug else kernels(a.shape)
    elif a.what == "e2e":
        e2e()
    else:
        train()
