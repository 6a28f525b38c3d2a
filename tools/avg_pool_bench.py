"""The average-pooled head (global_pool='avg') against the CLS head, both sides in one process on one box (profiles/avg_pool_lab.md).

    python tools/avg_pool_bench.py op [--steps 2000] [--rounds 3]
        tr_token_pool alone, microseconds and achieved GB/s at (B, N, D) = (256, 197, 384), (256, 138, 384), (128, 197, 768) -- the stream
        of the last block of DeiT-S, of Top-K kr 0.7 after its first stage, of DeiT-B -- with both pending residuals as bf16 (what the bf16
        executor hands it), and at B = 8 where the launch has to spread over narrow slabs.  The operands (150 MB at the first shape) are
        rotated over four buffer sets so that no launch finds its input in the last-level cache.
    python tools/avg_pool_bench.py eval [--batch 256] [--steps 20] [--rounds 3]
        The headline eval forward (DeiT-S Top-K, keep_rate 0.7 at blocks 3, 6, 9): pooled against CLS and against CLS with the CLS tail
        off (tr_set_cls_tail(0): the full-width last block the pool needs), one forward at a time and two in flight (forward_async).  The
        models are built in this process from the same weights.
    python tools/avg_pool_bench.py train [--batch 128] [--steps 10] [--rounds 3]
        One fine-tune step (forward, cross-entropy, backward, FusedAdamW), pooled against CLS.
The sides alternate within a round, so a drift of the box shows as spread between rounds.  One JSON line per leg."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args():
    return types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False)


def _create(**kw):
    import torch
    import tokenreduction_amd as tra
    torch.manual_seed(0)
    return tra.create_model("topk_small_patch16_224", pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None,
                            img_size=224, args=_args(), **kw).cuda()


def _timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(sides, steps, rounds, warmup=2):
    """{name: [seconds per round]} with the sides taking turns inside every round."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(_timed(fn, steps))
    return out


def op(steps, rounds):
    import torch
    from tokenreduction_amd import ops
    for B, N, D in ((256, 197, 384), (256, 138, 384), (128, 197, 768), (8, 197, 384), (1, 197, 384)):
        g = torch.Generator().manual_seed(1)
        sets = [(torch.randn(B, N, D, generator=g).cuda(), torch.randn(B, N, D, generator=g).bfloat16().cuda(),
                 torch.randn(B, N, D, generator=g).bfloat16().cuda()) for _ in range(4)]
        nbytes = B * (N - 1) * D * 8 + B * D * 4
        i = [0]

        def launch():
            x, d1, d2 = sets[i[0] % 4]
            i[0] += 1
            ops.token_pool(x, d1, d2)

        secs = _alternate({"tr_token_pool": launch}, steps, rounds)["tr_token_pool"]
        us = [round(1e6 * s / steps, 2) for s in secs]
        print(json.dumps({"leg": "op", "B": B, "N": N, "D": D, "pending": "2 x bf16", "bytes": nbytes, "us": us, "median_us": statistics.median(us),
                          "GB_per_s": round(nbytes / (statistics.median(us) * 1e-6) / 1e9, 1),
                          "note": "host clock around back-to-back launches and a synchronise: at the small shapes this is the enqueue rate, not the kernel"}), flush=True)


def eval_forward(batch, steps, rounds):
    import torch
    from tokenreduction_amd import ops
    cls = _create().eval()
    avg = _create(global_pool="avg").eval()
    avg.load_state_dict(cls.state_dict())
    full = _create().eval()                        # CLS pooling with the CLS tail off: captured while the switch is off
    full.load_state_dict(cls.state_dict())
    x = torch.randn(batch, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    models = {"cls": cls, "cls_tail_off": full, "avg": avg}
    # at this batch the forward takes the fused Mlp and the norm inside it: an image must still pool to the bits it has in a batch of two
    same = bool(torch.equal(avg(x)[:2], avg(x[:2].contiguous())))

    def run(name, in_flight):
        m = models[name]
        was = ops.set_cls_tail(name != "cls_tail_off")
        try:
            if in_flight == 1:
                m(x)
            else:
                a, b = m.forward_async(x), m.forward_async(x)
                a.result()
                b.result()
        finally:
            ops.set_cls_tail(was)

    res = {}
    for in_flight in (1, 2):
        secs = _alternate({k: (lambda k=k: run(k, in_flight)) for k in models}, steps, rounds)
        res[in_flight] = {k: [round(1e3 * s / (steps * in_flight), 4) for s in v] for k, v in secs.items()}
    for m in models.values():
        m.check_status()
    print(json.dumps({"leg": "eval", "model": "topk_small kr 0.7", "B": batch, "steps": steps, "pooled_bits_independent_of_batch": same,
                      "ms_per_forward": {f"in_flight_{k}": v for k, v in res.items()},
                      "median_ms_per_forward": {f"in_flight_{k}": {n: statistics.median(t) for n, t in v.items()} for k, v in res.items()}}), flush=True)
    assert same, "the pooled output of an image depends on its batch"


def train_step(batch, steps, rounds):
    import torch
    from tokenreduction_amd import finetune
    from tokenreduction_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 1000, (batch,), generator=g).cuda()
    sides = {}
    for name, kw in (("cls", {}), ("avg", {"global_pool": "avg"})):
        m = _create(**kw).train()
        opt = FusedAdamW(finetune.get_parameter_groups(m, 1e-4, 0.05, 1.0, 0), model=m)

        def step(m=m, opt=opt):
            torch.nn.functional.cross_entropy(m(x), y).backward()
            opt.step()
            opt.zero_grad()
        sides[name] = step
    secs = _alternate(sides, steps, rounds)
    ms = {k: [round(1e3 * s / steps, 3) for s in v] for k, v in secs.items()}
    print(json.dumps({"leg": "train_step", "model": "topk_small kr 0.7", "B": batch, "steps": steps, "ms_per_step": ms,
                      "median_ms_per_step": {k: statistics.median(v) for k, v in ms.items()}}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["op", "eval", "train"])
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    if a.leg == "op":
        op(a.steps or 2000, a.rounds)
    elif a.leg == "eval":
        eval_forward(a.batch or 256, a.steps or 20, a.rounds)
    else:
        train_step(a.batch or 128, a.steps or 10, a.rounds)
