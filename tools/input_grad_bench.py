"""The input gradient: what `x.requires_grad` costs a training step, and what it leaves alone (profiles/input_grad_lab.md).

    python tools/input_grad_bench.py step --leg finetune|finetune_dx|attack [--batch 256] [--steps 150] [--warmup 20]
        One workload in this process on DeiT-S Top-K kr 0.7, one JSON line with ms per step:
          finetune     forward + cross-entropy + backward + FusedAdamW, the input takes no gradient (runs on any build: the leg to compare
                       with the parent commit)
          finetune_dx  the same step with x.requires_grad set: the backward also writes dx [B, 3, 224, 224]
          attack       every weight frozen, x.requires_grad set: forward + backward to the image + a signed-gradient step on x (torch)
    python tools/input_grad_bench.py table [--rounds 3]
        The three legs, each in a fresh process, taken in turn within a round; the JSON lines and a summary line per leg.
    python tools/input_grad_bench.py kernel [--batch 256]
        tr_patch_embed_dgrad alone at DeiT-S width: microseconds per launch (HIP events around 50 launches) and the bytes it writes.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("finetune", "finetune_dx", "attack")


def step(leg, batch, steps, warmup):
    import torch
    import tokenreduction_amd as tra
    from tokenreduction_amd import finetune
    from tokenreduction_amd.optim import FusedAdamW
    assert torch.cuda.is_available(), "needs a GPU"
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False, dyvit_distill=False, k_neighbors=5, equal_weight=False,
                                 cluster_iters=3, sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None)
    torch.manual_seed(0)
    m = tra.create_model("topk_small_patch16_224", pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None,
                         img_size=224, args=args).cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 1000, (batch,), generator=g).cuda()
    opt = None
    if leg == "attack":
        for p in m.parameters():
            p.requires_grad = False
    else:
        opt = FusedAdamW(finetune.get_parameter_groups(m, 1e-4, 0.05, 1.0, 0), model=m)
    if leg != "finetune":
        x.requires_grad_(True)

    def run(n):
        for _ in range(n):
            loss = torch.nn.functional.cross_entropy(m(x), y)
            loss.backward()
            if opt is not None:
                opt.step()
                opt.zero_grad()
            if leg == "attack":
                with torch.no_grad():
                    x.add_(x.grad.sign(), alpha=1e-3)
            if x.grad is not None:
                x.grad = None
        torch.cuda.synchronize()
        return loss.item()
    run(warmup)
    t0 = time.perf_counter()
    last = run(steps)
    dt = time.perf_counter() - t0
    print(json.dumps({"leg": leg, "B": batch, "steps": steps, "ms_per_step": round(1e3 * dt / steps, 3), "images_per_s": round(steps * batch / dt, 1),
                      "last_loss": round(last, 4)}), flush=True)


def table(rounds, batch, steps, warmup):
    ms = {leg: [] for leg in LEGS}
    for _ in range(rounds):
        for leg in LEGS:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "step", "--leg", leg, "--batch", str(batch), "--steps", str(steps),
                                  "--warmup", str(warmup)], capture_output=True, text=True, timeout=600, cwd=ROOT)
            if out.returncode != 0:
                sys.exit(f"{leg}: exit {out.returncode}\n{out.stdout[-2000:]}{out.stderr[-2000:]}")
            line = out.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            ms[leg].append(json.loads(line)["ms_per_step"])
    for leg in LEGS:
        med, base = statistics.median(ms[leg]), statistics.median(ms["finetune"])
        print(json.dumps({"leg": leg, "ms_per_step": ms[leg], "median_ms": round(med, 3), "minus_finetune_ms": round(med - base, 3)}), flush=True)


def kernel(batch):
    import torch
    from tokenreduction_amd import ops
    assert torch.cuda.is_available(), "needs a GPU"
    D, HW, C = 384, 224, 3
    P = (HW // 16) ** 2
    g = torch.Generator().manual_seed(2)
    dy = torch.randn(batch * (P + 1), D, generator=g).bfloat16().cuda()
    wt = (0.05 * torch.randn(C * 256, D, generator=g)).bfloat16().cuda()
    dx = torch.empty(batch, C, HW, HW, device="cuda")
    for _ in range(5):
        ops.patch_embed_dgrad(dy, wt, batch, C, HW, out=dx)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 50
    a.record()
    for _ in range(n):
        ops.patch_embed_dgrad(dy, wt, batch, C, HW, out=dx)
    b.record()
    torch.cuda.synchronize()
    us = 1e3 * a.elapsed_time(b) / n
    print(json.dumps({"kernel": "tr_patch_embed_dgrad", "B": batch, "D": D, "us_per_launch": round(us, 1), "dx_MB": round(dx.numel() * 4 / 1e6, 1),
                      "write_GB_per_s": round(dx.numel() * 4 / us / 1e3, 1), "TFLOP_per_s": round(2.0 * batch * P * D * C * 256 / us / 1e6, 1)}),
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "table", "kernel"])
    ap.add_argument("--leg", default="finetune", choices=LEGS)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.what == "step":
        step(a.leg, a.batch, a.steps, a.warmup)
    elif a.what == "table":
        table(a.rounds, a.batch, a.steps, a.warmup)
    else:
        kernel(a.batch)
