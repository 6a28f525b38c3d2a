"""Decision taps against the viz_mode path they replace, both sides in one process on one box (profiles/decisions_lab.md).

    python tools/decisions_bench.py [--batch 256] [--steps 20] [--rounds 3] [--loop-batches 4] [--models topk tome dpcknn sit]

Per model (DeiT-S width: Top-K kr 0.7, ToMe, DPC-KNN, SiT; reduction at blocks 3 / 6 / 9) two legs, each with its own JSON line:
  forward   ms per batch of the forward alone, model(x) against model.forward_decisions(x), device events around `steps` forwards: the
            difference is what the one tr_stage_decisions launch (and, for the soft families, writing the soft matrix) costs
  validate  images/s of harness.validate over a loader of `loop_batches` batches: model.viz_mode = True (the only way to the stage records
            before the taps) against stage_records=True.  This is the whole loop, host work included: the per-image dictionaries, top-5
            and loss are the same Python on both sides and may well bound it.
The records of the two validate runs are compared value for value before anything is timed.  The two sides alternate within a round, so a
drift of the box shows as spread between rounds."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {"topk": "topk_small_patch16_224", "tome": "tome_small_patch16_224", "dpcknn": "dpcknn_small_patch16_224", "sit": "sit_small_patch16_224"}


def _args(**kw):
    base = dict(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False, dyvit_distill=False, k_neighbors=5, equal_weight=False, cluster_iters=3,
                sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _create(name):
    import torch
    import tokenreduction_amd as tra
    torch.manual_seed(0)
    return tra.create_model(name, pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None, img_size=224,
                            args=_args()).cuda().eval()


def _event_ms(fn, steps):
    """ms per call of `steps` calls between two device events on the current stream."""
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(sides, measure, rounds, warmup=2):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(measure(fn))
    return out


def _same_records(a, b):
    import numpy as np
    if sorted(a) != sorted(b):
        return False
    for key in a:
        if isinstance(a[key], dict):
            if not _same_records(a[key], b[key]):
                return False
        elif not np.array_equal(np.asarray(a[key]), np.asarray(b[key])):
            return False
    return True


def run(tag, batch, steps, rounds, loop_batches):
    import torch
    from tokenreduction_amd import harness
    name = MODELS[tag]
    m = _create(name)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 1000, (batch,), generator=g).cuda()
    if tag == "dpcknn":                                        # the same density noise on both sides, or the clusterings differ
        m.density_noise = {blk: torch.rand(batch, P, generator=g).cuda() for blk, _, P in m._stage_shapes()}
    loader = [(x, y)] * loop_batches
    names = [f"img_{i}" for i in range(batch * loop_batches)]
    dev = torch.device("cuda")

    def validate_viz():
        m.viz_mode = True
        try:
            return harness.validate(loader, m, dev, name, names)
        finally:
            m.viz_mode = False

    def validate_taps():
        return harness.validate(loader, m, dev, name, names, stage_records=True)

    same = _same_records(validate_viz(), validate_taps())
    plain = m(x)
    logits, dec = m.forward_decisions(x)
    same_logits = bool(torch.equal(plain, logits))
    fwd = _alternate({"plain": lambda: m(x), "decisions": lambda: m.forward_decisions(x)}, lambda fn: _event_ms(fn, steps), rounds)
    ms = {k: [round(v, 4) for v in vals] for k, vals in fwd.items()}
    print(json.dumps({"leg": "forward", "model": name, "B": batch, "steps": steps, "logits_bitwise_equal": same_logits, "ms_per_batch": ms,
                      "median_ms_per_batch": {k: statistics.median(v) for k, v in ms.items()}}), flush=True)
    secs = _alternate({"viz_mode": validate_viz, "stage_records": validate_taps}, _wall, rounds, warmup=1)
    ips = {k: [round(batch * loop_batches / s, 1) for s in v] for k, v in secs.items()}
    print(json.dumps({"leg": "validate", "model": name, "B": batch, "batches": loop_batches, "records_equal": bool(same), "images_per_s": ips,
                      "median_images_per_s": {k: statistics.median(v) for k, v in ips.items()}}), flush=True)
    assert same and same_logits, "the decision taps and viz_mode disagree"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-batches", type=int, default=4)
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    for tag in a.models:
        run(tag, a.batch, a.steps, a.rounds, a.loop_batches)
