"""Dense feature maps in training against the plain training step, both in one process on one box (profiles/dense_train_lab.md).

    python tools/dense_train_bench.py [--batch 256] [--steps 10] [--rounds 3] [--models topk tome deit] [--fmt NCHW] [--dtype fp32]
                                       [--levels 2 5 8 11] [--no-norm]

Per model (DeiT-S width, 224 x 224: Top-K kr 0.7, ToMe, dense DeiT-S; reduction at blocks 3 / 6 / 9) one JSON line with ms per step, device
events around `steps` steps, the two sides alternating within a round (median, min and max over the rounds):
  plain    model(x) + cross-entropy + backward
  dense    model.forward_dense_train(x) + a sum loss on the map + backward
then the launches the dense step has and the plain step has not, by label, with the library profiler's time per launch (one profiled step
of each side: the milliseconds since the previous launch's event, so a launch's own time plus its launch gap), and one JSON line per
(layout, input dtype) of tr_dense_scatter alone on the model's own index: its time (device events around `steps` launches, bf16 out as the
backward asks for it) and the bytes it must move -- the map once, the token gradient once, the index -- per second, against the rate a
float4 copy reaches on this part.
With --levels b0 b1 ... (profiles/dense_train_levels_lab.md) a third side joins the rounds, all three alternating within a round:
  levels   model.forward_dense_train(x, blocks=(b0, b1, ...)) + a sum loss on every map + backward
and the scatter section compares ONE tr_dense_scatter_levels launch for all levels with one tr_dense_scatter launch per level on the same
slabs and indices (the levels step's own), alternating within a round, in time and in bytes per second of the kernel's own traffic."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {"deit": "deit_small_patch16_224_local", "topk": "topk_small_patch16_224", "tome": "tome_small_patch16_224"}
HBM_COPY_TBS = 6.29          # measured float4 copy on MI355X (tools/dense_bench.py)


def _create(tag):
    import torch
    import tokenreduction_amd as tra
    torch.manual_seed(0)
    reduce = tag != "deit"
    args = types.SimpleNamespace(keep_rate=[0.7] if reduce else [1.0], reduction_loc=[3, 6, 9] if reduce else [], viz_mode=False, dyvit_distill=False,
                                 k_neighbors=5, equal_weight=False, cluster_iters=3, sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False,
                                 min_radius=None)
    return tra.create_model(MODELS[tag], pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None, img_size=224,
                            args=args).cuda().train()


def _event_ms(fn, steps):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def _profile(fn, cap=8192):
    """[(label, ms)] of the launches fn() enqueues through the library."""
    import torch
    from tokenreduction_amd import _lib
    lib = _lib.load()
    labels, ms, flops, nbytes = C.create_string_buffer(48 * cap), (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    assert lib.tr_profile_begin(torch.cuda.current_stream().cuda_stream) == 0
    try:
        fn()
    finally:
        n = lib.tr_profile_end(cap, labels, ms, flops, nbytes)
    return [(labels.raw[48 * i:48 * (i + 1)].split(b"\0")[0].decode(), float(ms[i])) for i in range(min(n, cap))]


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def run(tag, batch, steps, rounds, fmt, dtype, levels=None, norm=True):
    import torch
    from tokenreduction_amd import ops
    model = _create(tag)
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    y = torch.randint(0, 1000, (batch,), device="cuda")

    def plain():
        model.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(model(x), y).backward()

    def dense():
        model.zero_grad(set_to_none=True)
        _, d = model.forward_dense_train(x, output_fmt=fmt, dtype=dtype)
        d["features"].sum().backward()

    def multi():
        model.zero_grad(set_to_none=True)
        _, d = model.forward_dense_train(x, blocks=levels, norm=norm, output_fmt=fmt, dtype=dtype)
        sum(f.sum() for f in d["features"]).backward()

    sides = {"plain": plain, "dense": dense}
    if levels:
        sides["levels"] = multi
    for _ in range(2):
        for fn in sides.values():
            fn()
    t = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            t[k].append(_event_ms(fn, steps))
    line = {"model": tag, "batch": batch, "fmt": fmt, "dtype": str(dtype), "steps": steps, "rounds": rounds,
            "plain_ms": _stats(t["plain"]), "dense_ms": _stats(t["dense"]),
            "dense_minus_plain_ms": round(statistics.median(t["dense"]) - statistics.median(t["plain"]), 4)}
    if levels:
        line.update(levels=list(levels), norm=norm, levels_ms=_stats(t["levels"]),
                    levels_minus_plain_ms=round(statistics.median(t["levels"]) - statistics.median(t["plain"]), 4))
    print(json.dumps(line), flush=True)
    # the launches only the dense step has, with their times
    p, d = _profile(plain), _profile(dense)
    left = {}
    for label, _ in p:
        left[label] = left.get(label, 0) + 1
    extra = {}
    for label, ms in d:
        if left.get(label, 0) > 0:
            left[label] -= 1
        else:
            e = extra.setdefault(label, [0, 0.0])
            e[0] += 1
            e[1] += ms
    print(json.dumps({"model": tag, "launches_plain": len(p), "launches_dense": len(d), "profiled_ms_plain": round(sum(m for _, m in p), 4),
                      "profiled_ms_dense": round(sum(m for _, m in d), 4),
                      "extra_launches": {k: {"count": c, "ms": round(m, 4)} for k, (c, m) in extra.items()}}), flush=True)
    if levels:
        _scatter_levels(model, tag, batch, steps, rounds, multi)
    # the scatter alone, on the index of the last dense forward
    dense()
    st = model._train_state()
    P0, D, n_rows = model.patch_embed.num_patches, model.embed_dim, st.dense["rows"]
    index = st.dense["index"].view(batch, P0)
    for layout in ("NCHW", "NHWC"):
        for src in (torch.float32, torch.bfloat16):
            g = torch.randn((batch, D, P0) if layout == "NCHW" else (batch, P0, D), device="cuda").to(src)
            out = torch.empty(batch, n_rows, D, dtype=torch.bfloat16, device="cuda")
            fn = lambda: ops.dense_scatter(g, index, n_rows, layout=layout, dtype=torch.bfloat16, out=out)
            fn()
            ms = [_event_ms(fn, steps) for _ in range(rounds)]
            need = batch * P0 * D * g.element_size() + batch * n_rows * D * 2 + 4 * batch * P0
            med = statistics.median(ms)
            print(json.dumps({"model": tag, "scatter": layout, "dmap": str(src), "n_rows": n_rows, "ms": _stats(ms), "required_bytes": need,
                              "tb_per_s": round(need / med / 1e9, 3), "of_float4_copy": round(need / med / 1e9 / HBM_COPY_TBS, 3)}), flush=True)


def _scatter_levels(model, tag, batch, steps, rounds, multi):
    """One tr_dense_scatter_levels launch against one tr_dense_scatter launch per level, on the levels step's own indices and rows."""
    import torch
    from tokenreduction_amd import ops
    multi()
    dn = model._train_state().levels
    P0, D, rows, stride = model.patch_embed.num_patches, model.embed_dim, list(dn["rows"]), dn["stride"]
    L = len(rows)
    index = dn["index"].view(L, batch, P0)
    per_level = [index[l].clone() for l in range(L)]
    for layout in ("NCHW", "NHWC"):
        for src in (torch.float32, torch.bfloat16):
            maps = [torch.randn((batch, D, P0) if layout == "NCHW" else (batch, P0, D), device="cuda").to(src) for _ in range(L)]
            out = torch.empty(L * stride, dtype=torch.bfloat16, device="cuda")
            outs = [out[l * stride: l * stride + batch * rows[l] * D] for l in range(L)]
            one = lambda: ops.dense_scatter_levels(maps, index, rows, stride, layout=layout, dtype=torch.bfloat16, out=out)

            def each():
                for l in range(L):
                    ops.dense_scatter(maps[l], per_level[l], rows[l], layout=layout, dtype=torch.bfloat16, out=outs[l])
            one()
            each()
            ms = {"one_launch": [], "per_level": []}
            for _ in range(rounds):
                ms["one_launch"].append(_event_ms(one, steps))
                ms["per_level"].append(_event_ms(each, steps))
            need = sum(batch * P0 * D * maps[0].element_size() + batch * r * D * 2 + 4 * batch * P0 for r in rows)
            m1, mL = statistics.median(ms["one_launch"]), statistics.median(ms["per_level"])
            print(json.dumps({"model": tag, "scatter_levels": layout, "dmap": str(src), "rows": rows, "one_launch_ms": _stats(ms["one_launch"]),
                              "per_level_ms": _stats(ms["per_level"]), "required_bytes": need, "one_launch_tb_per_s": round(need / m1 / 1e9, 3),
                              "per_level_tb_per_s": round(need / mL / 1e9, 3), "of_float4_copy": round(need / m1 / 1e9 / HBM_COPY_TBS, 3)}),
                  flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", nargs="+", default=["topk", "tome", "deit"], choices=sorted(MODELS))
    ap.add_argument("--fmt", default="NCHW", choices=["NCHW", "NHWC"])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--levels", type=int, nargs="+", default=None, help="blocks of a multi-level step, e.g. 2 5 8 11")
    ap.add_argument("--no-norm", action="store_true", help="the levels as they stand (norm=False)")
    a = ap.parse_args()
    dtype = torch.float32 if a.dtype == "fp32" else torch.bfloat16
    for tag in a.models:
        run(tag, a.batch, a.steps, a.rounds, a.fmt, dtype, tuple(a.levels) if a.levels else None, not a.no_norm)


if __name__ == "__main__":
    main()
