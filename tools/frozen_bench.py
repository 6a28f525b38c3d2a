"""Fine-tuning with frozen parameters: what skipping their gradient work in the HIP backward buys (profiles/frozen_lab.md).

    python tools/frozen_bench.py step --model topk_small --mask attn_only [--batch 256] [--steps 150] [--warmup 20]
        One fine-tune workload in this process: forward + loss + backward + FusedAdamW over the trainable parameter groups
        (finetune.get_parameter_groups), one JSON line with ms per step.  For kernel times put it after
        `rocprofv3 --kernel-trace --stats -d DIR --` (a run of its own: tracing slows the host).
    python tools/frozen_bench.py table [--rounds 3]
        Every row of the lab note, each in a fresh process, the rows of a model alternating within a round so that a drift of the box
        shows as spread between rounds rather than as a difference between rows: DeiT-S Top-K kr 0.7 at batch 256 with four masks
        (all trainable, attn-only, head + the top two blocks, head only), DeiT-B ATS kr 0.5 at batch 128 (all trainable, attn-only).
        Prints the JSON lines of the children and a summary line per row (median ms per step, ratio to the all-trainable row).
    python tools/frozen_bench.py wgrad-share DIR
        The weight-gradient kernels' share of the kernel time in a rocprofv3 kernel-stats directory.
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {"topk_small": ("topk_small_patch16_224", [0.7], 256), "ats_base": ("ats_base_patch16_224", [0.5], 128)}
MASKS = ("all", "attn_only", "top2", "head")
TABLE = [("topk_small", m) for m in MASKS] + [("ats_base", "all"), ("ats_base", "attn_only")]


def apply_mask(model, mask):
    from tokenreduction_amd import finetune
    if mask == "attn_only":
        finetune.freeze_attn_only(model)
    elif mask == "top2":          # head + the top two blocks
        top = tuple(f"blocks.{i}." for i in (model.depth - 2, model.depth - 1))
        for n, p in model.named_parameters():
            p.requires_grad = n.startswith(("head.",) + top)
    elif mask == "head":          # linear probe
        for n, p in model.named_parameters():
            p.requires_grad = n.startswith("head.")
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def step(model_key, mask, batch, steps, warmup):
    import torch
    import tokenreduction_amd as tra
    from tokenreduction_amd import finetune
    from tokenreduction_amd.optim import FusedAdamW
    assert torch.cuda.is_available(), "needs a GPU"
    factory, keep, default_batch = MODELS[model_key]
    B = batch or default_batch
    args = types.SimpleNamespace(keep_rate=keep, reduction_loc=[3, 6, 9], viz_mode=False, dyvit_distill=False, k_neighbors=5, equal_weight=False,
                                 cluster_iters=3, sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None)
    torch.manual_seed(0)
    m = tra.create_model(factory, pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None, img_size=224,
                         args=args).cuda().train()
    trainable = apply_mask(m, mask)
    opt = FusedAdamW(finetune.get_parameter_groups(m, 1e-4, 0.05, 1.0, 0), model=m)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 1000, (B,), generator=g).cuda()

    def run(n):
        for _ in range(n):
            loss = torch.nn.functional.cross_entropy(m(x), y)
            loss.backward()
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        return loss.item()
    run(warmup)
    t0 = time.perf_counter()
    last = run(steps)
    dt = time.perf_counter() - t0
    print(json.dumps({"model": model_key, "mask": mask, "B": B, "steps": steps, "trainable_elements": trainable,
                      "ms_per_step": round(1e3 * dt / steps, 3), "images_per_s": round(steps * B / dt, 1), "last_loss": round(last, 4)}), flush=True)


def table(rounds, steps, warmup):
    ms = {row: [] for row in TABLE}
    for _ in range(rounds):
        for row in TABLE:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "step", "--model", row[0], "--mask", row[1], "--steps", str(steps),
                                  "--warmup", str(warmup)], capture_output=True, text=True, timeout=600, cwd=ROOT)
            if out.returncode != 0:
                sys.exit(f"{row}: exit {out.returncode}\n{out.stdout[-2000:]}{out.stderr[-2000:]}")
            line = out.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            ms[row].append(json.loads(line)["ms_per_step"])
    for row in TABLE:
        med, base = statistics.median(ms[row]), statistics.median(ms[(row[0], "all")])
        print(json.dumps({"row": f"{row[0]}/{row[1]}", "ms_per_step": ms[row], "median_ms": round(med, 3), "ratio_to_all": round(med / base, 4)}),
              flush=True)


def wgrad_share(directory):
    f = glob.glob(directory + "/**/*kernel_stats.csv", recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    wg = [r for r in rows if "wgrad" in r["Name"]]
    short = lambda name: re.sub(r"\(.*", "", re.sub(r"^void |\(anonymous namespace\)::", "", name))          # noqa: E731
    print(json.dumps({"stats": f, "kernel_ms_total": round(total / 1e6, 3),
                      "wgrad": {short(r["Name"]): {"calls": int(r["Calls"]), "ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                                                   "share": round(float(r["TotalDurationNs"]) / total, 4)} for r in wg},
                      "wgrad_share": round(sum(float(r["TotalDurationNs"]) for r in wg) / total, 4)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "table", "wgrad-share"])
    ap.add_argument("directory", nargs="?")
    ap.add_argument("--model", default="topk_small", choices=list(MODELS))
    ap.add_argument("--mask", default="all", choices=MASKS)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.what == "step":
        step(a.model, a.mask, a.batch, a.steps, a.warmup)
    elif a.what == "table":
        table(a.rounds, a.steps, a.warmup)
    else:
        wgrad_share(a.directory)
