"""LayerScale (init_values) on the hot path: what the fold and the unfold cost (profiles/layerscale_lab.md).

    python tools/layerscale_bench.py table [--rounds 3] [--steps 60] [--warmup 15]
        DeiT-S at batch 256 and DeiT-B at batch 128 (dense, deit_*_patch16_224_local), each built twice in ONE process -- plain and with
        init_values=1e-6 + no_embed_class -- the two taking turns within a round so that a drift of the box shows as spread between rounds
        and not as a difference between them.  Per model and variant: eval images/s (hipGraph replay, static input) and the fine-tune
        step (forward + loss + backward + optim.FusedAdamW) in ms.  One JSON line per measurement and a summary line per row.
    python tools/layerscale_bench.py launches [--reps 20]
        The two new launches of the LayerScale variants, timed by the library's launch profiler (HIP events around every launch: the
        kernel plus its dependent-launch boundary) inside real steps: median ms and the achieved bytes/s over the bytes the operation
        needs (fold: W read, the bf16 copy and its transposed copy written; unfold: dW' and W read, dW written).
    python tools/layerscale_bench.py step --model small --ls 1 [--steps 60]
        One variant's fine-tune steps alone, for `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/layerscale_bench.py step ...`
        (a run of its own: tracing slows the host).
    python tools/layerscale_bench.py kernels DIR --model small
        The two kernels' rows of a rocprofv3 kernel-stats directory: calls, mean us, bytes/s over the same byte counts.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {"small": ("deit_small_patch16_224_local", 256, 384), "base": ("deit_base_patch16_224_local", 128, 768)}
FOLD, UNFOLD = "tr_layerscale_fold", "tr_layerscale_unfold_grad"


def op_bytes(D, depth=12):
    """Bytes the two operations need for a whole model (training, bf16): the matrices dominate, the [D] vectors are counted too."""
    elems = depth * (D * D + D * 4 * D)
    vec = depth * 2 * D * 4
    return {FOLD: elems * (4 + 2 + 2) + 3 * vec, UNFOLD: elems * (4 + 4 + 4) + 6 * vec}


def build(key, ls):
    import torch
    import tokenreduction_amd as tra
    factory, B, _D = MODELS[key]
    torch.manual_seed(0)
    extra = dict(init_values=1e-6, no_embed_class=True) if ls else {}
    m = tra.create_model(factory, pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0, img_size=224, **extra).cuda()
    if ls:                  # gammas of a trained DeiT-III are O(0.1 .. 1): values do not change the work, but keep the loss alive
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith(".gamma"):
                    p.fill_(0.3)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 1000, (B,), generator=g).cuda()
    return m, x, y


def trainer(m, x, y):
    import torch
    from tokenreduction_amd import finetune
    from tokenreduction_amd.optim import FusedAdamW
    opt = FusedAdamW(finetune.get_parameter_groups(m, 1e-4, 0.05, 1.0, 0), model=m)

    def run(n):
        m.train()
        for _ in range(n):
            loss = torch.nn.functional.cross_entropy(m(x), y)
            loss.backward()
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        return loss.item()
    return run


def evaluator(m, x):
    import torch

    def run(n):
        m.eval()
        with torch.no_grad():
            for _ in range(n):
                out = m(x)
        torch.cuda.synchronize()
        return out
    return run


def table(rounds, steps, warmup):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    for key, (_f, B, _D) in MODELS.items():
        sides = {}
        for ls in (0, 1):
            m, x, y = build(key, ls)
            sides[ls] = (evaluator(m, x), trainer(m, x, y))
        res = {(ls, what): [] for ls in (0, 1) for what in ("eval", "train")}
        for ls in (0, 1):           # warm every shape the timed windows use
            sides[ls][1](warmup)
            sides[ls][0](warmup)
        for _ in range(rounds):
            for what, idx, n in (("eval", 0, 4 * steps), ("train", 1, steps)):
                for ls in (0, 1):
                    sides[ls][idx](3)
                    t0 = time.perf_counter()
                    sides[ls][idx](n)
                    dt = time.perf_counter() - t0
                    val = n * B / dt if what == "eval" else 1e3 * dt / n
                    res[(ls, what)].append(val)
                    print(json.dumps({"model": key, "B": B, "layerscale": ls, "what": what, "n": n,
                                      "images_per_s" if what == "eval" else "ms_per_step": round(val, 3)}), flush=True)
        med = {k: statistics.median(v) for k, v in res.items()}
        print(json.dumps({"row": key, "B": B, "eval_images_per_s": {"plain": round(med[(0, "eval")], 1), "layerscale": round(med[(1, "eval")], 1)},
                          "train_ms_per_step": {"plain": round(med[(0, "train")], 3), "layerscale": round(med[(1, "train")], 3)},
                          "train_step_ratio": round(med[(1, "train")] / med[(0, "train")], 4),
                          "spread_train_ms": {"plain": [round(v, 3) for v in res[(0, "train")]], "layerscale": [round(v, 3) for v in res[(1, "train")]]}}),
              flush=True)
        del sides
        torch.cuda.empty_cache()


def launches(reps, warmup):
    import numpy as np
    import torch
    from tokenreduction_amd import _lib
    assert torch.cuda.is_available(), "needs a GPU"
    lib = _lib.load()
    cap = 8192
    for key, (_f, B, D) in MODELS.items():
        m, x, y = build(key, 1)
        run = trainer(m, x, y)
        run(warmup)
        ms = {FOLD: [], UNFOLD: []}
        labels, t = np.zeros(cap * 48, dtype=np.uint8), np.zeros(cap, dtype=np.float32)
        for _ in range(reps):
            _lib.check(lib.tr_profile_begin(torch.cuda.current_stream().cuda_stream), "tr_profile_begin")
            run(1)
            n = lib.tr_profile_end(cap, labels.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), None, None)
            assert 0 < n <= cap
            names = [bytes(labels[48 * i: 48 * (i + 1)]).split(b"\0")[0].decode() for i in range(n)]
            for name in ms:
                hits = [float(t[i]) for i, s in enumerate(names) if s == name]
                assert len(hits) == 1, (name, len(hits))
                ms[name].append(hits[0])
        need = op_bytes(D)
        for name, v in ms.items():
            med = statistics.median(v)
            print(json.dumps({"model": key, "B": B, "launch": name, "median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                              "bytes": need[name], "GB_per_s": round(need[name] / (med * 1e-3) / 1e9, 1), "clock": "HIP events around the launch"}),
                  flush=True)
        del m, run
        torch.cuda.empty_cache()


def step(key, ls, steps, warmup):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    m, x, y = build(key, ls)
    run = trainer(m, x, y)
    run(warmup)
    t0 = time.perf_counter()
    last = run(steps)
    dt = time.perf_counter() - t0
    print(json.dumps({"model": key, "layerscale": ls, "steps": steps, "ms_per_step": round(1e3 * dt / steps, 3), "last_loss": round(last, 4)}), flush=True)


def kernels(directory, key):
    f = glob.glob(directory + "/**/*kernel_stats.csv", recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    D = MODELS[key][2]
    need = op_bytes(D)
    for kern, name in (("ls_fold_kernel", FOLD), ("ls_unfold_kernel", UNFOLD)):
        for r in rows:
            if kern in r["Name"]:
                mean_ns = float(r["TotalDurationNs"]) / int(r["Calls"])
                print(json.dumps({"stats": f, "kernel": kern, "calls": int(r["Calls"]), "mean_us": round(mean_ns / 1e3, 2),
                                  "bytes": need[name], "GB_per_s": round(need[name] / mean_ns, 1), "model": key}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["table", "launches", "step", "kernels"])
    ap.add_argument("directory", nargs="?")
    ap.add_argument("--model", default="small", choices=list(MODELS))
    ap.add_argument("--ls", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.what == "table":
        table(a.rounds, a.steps, a.warmup)
    elif a.what == "launches":
        launches(a.reps, a.warmup)
    elif a.what == "step":
        step(a.model, a.ls, a.steps, a.warmup)
    else:
        kernels(a.directory, a.model)
