"""What every kind of eval request launches, returns and captures, as text -- to compare two commits (profiles/eval_requests_lab.md).

    python tools/request_trace.py
        On the device.  The micro cases of tests/_params.GOLDEN_CASES at their recorded batch sizes (plus topk_micro once more with uint8
        pixel input) x nine request kinds (plain, CLS taps, taps + final_tokens, decisions, decisions + taps, dense NCHW fp32, dense NHWC
        bf16, two levels with and without the final norm) x {synchronous entry, forward_async}.  One JSON line per combination:
          launches  [label, flops, bytes] of one plain-launch forward (hipGraph replay off; the synchronous entry only: the profiler
                    follows the caller's stream),
          tensors   the sha256 (16 hex digits) of every tensor a replayed call returns, by its path in the result,
          keys      the sorted repr of the workspace's graph keys after that call, with the three addresses in a key (input, pixel LUT,
                    noise) replaced by "x" / "lut" / "noise" so that two processes print the same text.
        Two trees that print the same bytes enqueue the same launches, return the same bits and capture under the same keys.
    python tools/request_trace.py --summary TRACE
        No GPU.  A saved trace as one short line per combination (counts and digests), and the sha256 of the file.
    python tools/request_trace.py --host-time
        Host cost of the hot enqueue path on the headline model (topk_small_patch16_224): wall time of 1000 replayed forward_async(x)
        calls before a single synchronise, 5 repeats, in microseconds per call -- at batch 1 and at the headline's batch 256.  Once the
        queue is full the host waits for the device, so a figure is an upper bound on the host's own cost per call (batch 1 is the
        tighter one); a host path that got slower than the device's pace would show as a rise.
"""
import argparse
import hashlib
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

CASES = ["deit_micro", "topk_micro", "evit_micro", "tome_micro", "ats_micro", "sit_micro", "dpcknn_micro", "kmedoids_micro", "heuristic_micro_l2"]


def kinds(depth):
    """(label, synchronous call, forward_async keywords) of every request kind, on a model of `depth` blocks"""
    two = (1, depth - 1)
    dense = lambda **kw: (lambda m, x: m.forward_dense(x, **kw), dict(dense=kw))
    return [("plain", lambda m, x: m(x), {}),
            ("taps", lambda m, x: m.forward_taps(x, cls_blocks=two), dict(cls_blocks=two)),
            ("taps+final", lambda m, x: m.forward_taps(x, cls_blocks=two, final_tokens=True), dict(cls_blocks=two, final_tokens=True)),
            ("decisions", lambda m, x: m.forward_decisions(x), dict(decisions=True)),
            ("decisions+taps", lambda m, x: m.forward_decisions(x, cls_blocks=two), dict(decisions=True, cls_blocks=two)),
            ("dense NCHW fp32",) + dense(),
            ("dense NHWC bf16",) + dense(output_fmt="NHWC", dtype=torch.bfloat16, fill=-1.0),
            ("levels norm",) + dense(blocks=two, norm=True),
            ("levels raw",) + dense(blocks=two, norm=False)]


def sha(t):
    t = t.detach().contiguous()
    return hashlib.sha256(t.view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b"").hexdigest()[:16]


def digests(out, path="out"):
    """{path: sha} of every tensor in a result (tuples, lists and dicts walked in order)"""
    if isinstance(out, torch.Tensor):
        return {path: sha(out)}
    if isinstance(out, dict):
        out = list(out.items())
    elif isinstance(out, (tuple, list)):
        out = list(enumerate(out))
    else:
        return {}
    found = {}
    for k, v in out:
        found.update(digests(v, f"{path}.{k}"))
    return found


def key_text(key, x):
    """repr of a graph key with its addresses named: (input address, dtype, format, LUT address, ..., noise address, ...)"""
    key = list(key)
    assert key[0] == x.data_ptr(), "the key does not begin with the input's address"
    key[0], key[3], key[6] = "x", key[3] and "lut", key[6] and "noise"
    return repr(tuple(key))


def model_and_input(name, pixels):
    from tests._params import GOLDEN_CASES, make_images
    from tests.test_hip_model import build_model
    case = GOLDEN_CASES[name]
    model, _, _ = build_model(case)
    model.viz_mode = False
    model.pipeline_depth = 1              # forward_async on one side stream: its second call replays what its first captured
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    noise = {int(k.split("_")[1]): torch.from_numpy(g[k]) for k in g.files if k.startswith("noise_")}
    if noise:
        model.density_noise = noise
    if pixels:
        model.set_pixel_input()
        x = torch.randint(0, 256, (case["batch"], 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(case["xseed"]))
    else:
        x = make_images(case["batch"], 224, case["xseed"])
    return model, x.cuda(), case["xseed"]


def trace():
    from tests import _launches
    for name, pixels in [(n, False) for n in CASES] + [("topk_micro", True)]:
        model, x, seed = model_and_input(name, pixels)

        def run(call):
            np.random.seed(seed)          # K-Medoids draws its first medoids from numpy's global generator
            return call()

        for kind, sync, kw in kinds(model.depth):
            for mode, call in (("sync", lambda: sync(model, x)), ("async", lambda: model.forward_async(x, **kw).result())):
                rec = dict(case=name + ("+uint8" if pixels else ""), kind=kind, mode=mode)
                if mode == "sync":
                    model.use_graph = False
                    run(call)
                    torch.cuda.synchronize()
                    rec["launches"] = _launches.record(lambda: run(call))
                model.use_graph = True
                run(call)                 # captures
                out = run(call)           # replays
                torch.cuda.synchronize()
                rec["tensors"] = digests(out)
                rec["keys"] = sorted(key_text(k, x) for k in model._last_ws["graphs"])
                print(json.dumps(rec), flush=True)
        model.check_status()


def host_time(batch, calls=1000, repeats=5):
    import tokenreduction_amd as tra
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False)
    torch.manual_seed(0)
    model = tra.create_model("topk_small_patch16_224", pretrained=False, num_classes=1000, img_size=224, args=args).cuda().eval()
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    for _ in range(8):                    # both pipeline slots captured and replayed
        model.forward_async(x).result()
    torch.cuda.synchronize()
    reps = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            model.forward_async(x)
        reps.append((time.perf_counter() - t0) / calls * 1e6)
        torch.cuda.synchronize()
    model.check_status()
    print(f"forward_async(x), replayed, topk_small batch {batch}: us per call over {calls} calls before one synchronise, {repeats} repeats: "
          f"{' '.join(f'{r:.1f}' for r in reps)}  median {sorted(reps)[repeats // 2]:.1f} min {min(reps):.1f} max {max(reps):.1f}", flush=True)


def summary(path):
    """One short line per line of a saved trace: the launch count and 12-digit digests of its launches, tensors and keys; then the file's own."""
    short = lambda v: hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest()[:12]
    with open(path, "rb") as f:
        raw = f.read()
    for line in raw.decode().splitlines():
        r = json.loads(line)
        launches = f"{len(r['launches']):3d} launches {short(r['launches'])}" if "launches" in r else " " * 25
        print(f"{r['case']:18s} {r['kind']:15s} {r['mode']:5s} {launches}  {len(r['tensors']):2d} tensors {short(r['tensors'])}  "
              f"{len(r['keys']):2d} keys {short(r['keys'])}")
    print(f"sha256 of the whole trace ({len(raw)} bytes): {hashlib.sha256(raw).hexdigest()}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-time", action="store_true")
    ap.add_argument("--summary", metavar="TRACE", help="no GPU: the digest listing of a trace saved to a file")
    a = ap.parse_args()
    if a.summary:
        sys.exit(summary(a.summary))
    assert torch.cuda.is_available(), "needs a GPU"
    if a.host_time:
        host_time(1)
        host_time(256)
    else:
        trace()
