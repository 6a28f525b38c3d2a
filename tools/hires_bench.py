#!/usr/bin/env python3
"""Eval throughput at high resolution: DeiT-S dense, Top-K (keep_rate 0.7), ToMe and DPC-KNN at 224^2, 384^2, 448^2 and 512^2 inputs,
bf16 by default (--precision), batch 64, one forward at a time (each timed window ends in a device synchronise).  Prints one JSON line: per (model, size)
images/s and ms per forward, and the speed-up of each reduction model over the dense model at the same size.  Random weights and
images (seeded): throughput does not depend on the values, only on the token schedule, which the keep rates fix."""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tokenreduction_amd as tra  # noqa: E402

MODELS = {"dense": "deit_small_patch16_224_local", "topk": "topk_small_patch16_224", "tome": "tome_small_patch16_224",
          "dpcknn": "dpcknn_small_patch16_224", "sinkhorn": "sinkhorn_small_patch16_224"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[224, 384, 448, 512])
    ap.add_argument("--models", nargs="+", default=["dense", "topk", "tome", "dpcknn"], choices=list(MODELS))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep-rate", type=float, default=0.7)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3", "fp32"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hires_bench.py needs a GPU")
    args = types.SimpleNamespace(keep_rate=[a.keep_rate], reduction_loc=[3, 6, 9], dyvit_distill=False, k_neighbors=5, equal_weight=False,
                                 cluster_iters=3, sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None)
    res = {}
    for S in a.sizes:
        x = torch.randn(a.batch, 3, S, S, generator=torch.Generator().manual_seed(S)).cuda()
        for key in a.models:
            torch.manual_seed(0)
            m = tra.create_model(MODELS[key], pretrained=False, num_classes=1000, img_size=S, args=args).cuda().eval()
            m.precision = a.precision
            for _ in range(a.warmup):
                m(x)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for _ in range(a.steps):
                t0.record()
                out = m(x)
                t1.record()
                torch.cuda.synchronize()
                ms.append(t0.elapsed_time(t1))
            assert bool(torch.isfinite(out).all()), f"{key} at {S}: non-finite logits"
            ms.sort()
            med = ms[len(ms) // 2]
            res[f"{key}_{S}"] = {"ms_per_forward": round(med, 3), "ms_min": round(ms[0], 3), "images_per_s": round(a.batch * 1e3 / med, 1),
                                 "tokens": (S // 16) ** 2 + 1}
            del m
    for S in a.sizes:
        d = res.get(f"dense_{S}")
        for key in a.models:
            if key != "dense" and d and f"{key}_{S}" in res:
                res[f"{key}_{S}"]["speedup_vs_dense"] = round(d["ms_per_forward"] / res[f"{key}_{S}"]["ms_per_forward"], 3)
    print(json.dumps({"tool": "hires_bench", "batch": a.batch, "steps": a.steps, "precision": a.precision, "keep_rate": a.keep_rate, "device": torch.cuda.get_device_name(),
                      "results": res}))


if __name__ == "__main__":
    main()
