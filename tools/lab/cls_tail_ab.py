"""Lab: CLS tail of the eval forward's last block (tr_set_cls_tail) off / on, round-robin on one box, hipGraph replay.
Two models per workload (one captured with the tail off, one with it on) take turns, so drift of the box hits both alike.
(1) images/s, one forward at a time and two in flight: headline (Top-K kr 0.7), Top-K kr 0.5, dense DeiT-S, dense DeiT-B (batch 64);
(2) per-launch HIP-event us of the last block's launches, tail off and on (plain launches, tr_profile_begin / tr_profile_end)."""
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import bench
from tokenreduction_amd import _lib, ops

ROUNDS = int(os.environ.get("CLS_TAIL_AB_ROUNDS", "6"))
WORK = (("topk kr0.7", lambda: bench.build_model(keep_rate=[0.7]), bench.BATCH),
        ("topk kr0.5", lambda: bench.build_model(keep_rate=[0.5]), bench.BATCH),
        ("dense deit-s", lambda: bench.build_model("deit_small_patch16_224_local", [1.0], []), bench.BATCH),
        ("dense deit-b", lambda: bench.build_model("deit_base_patch16_224_local", [1.0], []), 64))


def last_block_launches(model, x, reps=5):
    """[(label, best us)] of the launches from the last attention of a plain-launch forward on."""
    lib = _lib.load()
    model.use_graph = False
    cap = 1024
    labels, ms = np.zeros(cap * 48, dtype=np.uint8), np.zeros(cap, dtype=np.float32)
    best = None
    for _ in range(reps + 1):
        _lib.check(lib.tr_profile_begin(torch.cuda.current_stream().cuda_stream), "tr_profile_begin")
        model(x)
        n = lib.tr_profile_end(cap, labels.ctypes.data, ms.ctypes.data, None, None)
        names = [bytes(labels[i * 48:(i + 1) * 48]).split(b"\0")[0].decode() for i in range(n)]
        best = ms[:n].copy() if best is None else np.minimum(best, ms[:n])
    model.use_graph = True
    first = max(i for i, nm in enumerate(names) if nm.startswith("attention"))
    return [(names[i], 1e3 * float(best[i])) for i in range(first, n)]


for name, make, batch in WORK:
    x = torch.randn(batch, 3, 224, 224, generator=torch.Generator().manual_seed(0)).cuda()
    models = {}
    for on in (0, 1):
        ops.set_cls_tail(on)
        models[on] = make()
        models[on](x)                                   # captured in this form
        models[on].forward_async(x).result()
        models[on].forward_async(x).result()
    assert torch.equal(models[0](x), models[1](x))
    for k in (1, 2):
        runs = {0: [], 1: []}
        for _ in range(ROUNDS):
            for on in (0, 1):
                runs[on].append(bench.quick_images_per_s(models[on], x, iters=40, reps=3, in_flight=k))
        for on in (0, 1):
            r = sorted(runs[on])
            print(f"{name:13s} in flight {k}  tail {on}: median {r[len(r) // 2]:9.1f} images/s  range {r[0]:9.1f} .. {r[-1]:9.1f}  "
                  f"({batch / r[len(r) // 2] * 1e3:.3f} ms)  runs {' '.join(f'{v:.0f}' for v in runs[on])}", flush=True)
        print(f"{name:13s} in flight {k}  every tail-on run above every tail-off run: {min(runs[1]) > max(runs[0])}", flush=True)
    for on in (0, 1):
        ops.set_cls_tail(on)
        rows = last_block_launches(models[on], x)
        print(f"{name:13s} tail {on}: last block from its attention on, {sum(u for _, u in rows):6.1f} us: " +
              ", ".join(f"{nm} {u:.1f}" for nm, u in rows), flush=True)
    del models
ops.set_cls_tail(1)
