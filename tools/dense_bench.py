"""Dense feature maps against the torch restatement they replace, both sides in one process on one box (profiles/dense_lab.md).

    python tools/dense_bench.py [--batch 256] [--steps 20] [--rounds 3] [--models deit topk tome sit dpcknn] [--fmt NCHW] [--dtype fp32]
    python tools/dense_bench.py --kernels          # the same forwards under rocprofv3 --kernel-trace --stats: the gather's bytes/s
    python tools/dense_bench.py --levels [2 5 8 11] [--no-norm] [--models deit topk tome dpcknn] [--kernels]     # profiles/dense_levels_lab.md
    python tools/dense_bench.py --size 384 640 --levels 2 5 8 11 --models deit topk      # a rectangular input (profiles/rect_input_lab.md)

Per model (DeiT-S width, 224 x 224: dense DeiT as the identity case, Top-K kr 0.7, ToMe, SiT, DPC-KNN; reduction at blocks 3 / 6 / 9) one
JSON line with ms per batch, device events around `steps` forwards, the sides alternating within a round:
  plain    model(x)
  torch    model.forward_decisions(x, final_tokens=True), then the map on the device in torch: the decisions composed stage by stage with
           torch.gather / scatter, the rows gathered per patch, masked with the fill, and permute().contiguous() for NCHW
  dense    model.forward_dense(x)
(gather_required_bytes: the upper bound of one fp32 row per patch; gather_distinct_bytes: the map plus every row of the last stream once.)
The two maps are compared bit for bit before anything is timed.  --kernels runs a child process of this tool (leg `dense` only) under
rocprofv3 and divides the bytes tr_dense_gather HAS to move -- every output element once, the rows it reads at most once per patch, the
index: computed from the shapes here -- by the kernel's average duration, against the HBM rate a float4 copy reaches on this part.

--levels: the multi-level maps of forward_dense(blocks=...).  Three sides, alternating within a round:
  plain    model(x)
  viz      the only other route to the same tensors: a viz_mode forward (every row of every block, lazy norms, graph replay and the CLS tail
           off), tr_stage_decisions on the slabs it left, and per level the torch composition above on that block's rows (norm: through
           tr_final_tokens_f32) -- the rows are taken from the device buffer, not from the host copies viz_mode returns
  levels   model.forward_dense(x, blocks=...)
The maps of the two routes are compared bit for bit before anything is timed.  With --kernels the child also runs L single-level
tr_dense_gather launches on the same slabs and indices per step: the batched gather's average duration against their sum."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {"deit": "deit_small_patch16_224_local", "topk": "topk_small_patch16_224", "tome": "tome_small_patch16_224", "sit": "sit_small_patch16_224",
          "dpcknn": "dpcknn_small_patch16_224"}
HBM_COPY_TBS = 6.29          # measured float4 copy on MI355X (8.0 TB/s on paper)
SIZE = (224, 224)            # --size H W: the input; the factories take a pair (Top-K keeps int(ratio * 196) whatever the grid, topk.py:56)


def _args(**kw):
    base = dict(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False, dyvit_distill=False, k_neighbors=5, equal_weight=False, cluster_iters=3,
                sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _create(tag):
    import torch
    import tokenreduction_amd as tra
    torch.manual_seed(0)
    args = _args(keep_rate=[1.0], reduction_loc=[]) if tag == "deit" else _args()
    return tra.create_model(MODELS[tag], pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None,
                            img_size=SIZE[0] if SIZE[0] == SIZE[1] else SIZE, args=args).cuda().eval()


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


def torch_index(dec, stages, B, P0, dev):
    """The record-form decisions of `stages` composed with torch ops on the device (the semantics of tr_dense_index)."""
    import torch
    from tokenreduction_amd import _lib
    cur = torch.arange(P0, device=dev).expand(B, P0)
    for blk, kind, n_in, k in stages:
        if kind in (_lib.TR_DECISION_CENTRES, _lib.TR_DECISION_TOME, _lib.TR_DECISION_SOFT):
            n_out = n_in - 1 - min(k, (n_in - 1) // 2) if kind == _lib.TR_DECISION_TOME else k
            ok = (cur >= 0) & (cur < n_in - 1)
            nxt = torch.gather(dec["assign"][blk].long(), 1, cur.clamp(0, n_in - 2))
            cur = torch.where(ok & (nxt >= 0) & (nxt < n_out), nxt, torch.full_like(nxt, -1))
        else:
            kept = dec["kept"][blk].long()
            W = kept.shape[1]
            valid = (kept >= 0) & (kept < P0)
            inv = torch.full((B, P0 + 1), W, dtype=torch.long, device=dev)
            inv.scatter_reduce_(1, torch.where(valid, kept, torch.full_like(kept, P0)), torch.arange(W, device=dev).expand(B, W), "amin")
            cur = torch.where(inv[:, :P0] < W, inv[:, :P0], torch.full_like(inv[:, :P0], -1))
    return torch.where(cur >= 0, cur + 1, cur)


def torch_gather(tokens, index, grid, fmt, dtype, fill):
    """... and the rows gathered per patch, masked with the fill (the semantics of tr_dense_gather)."""
    import torch
    B, n_rows, D = tokens.shape
    (h, w), P0 = grid, index.shape[1]
    rows = torch.gather(tokens, 1, index.clamp(0, n_rows - 1)[:, :, None].expand(B, P0, D))
    feat = torch.where((index >= 0)[:, :, None], rows, torch.full_like(rows, fill)).to(dtype)
    return feat.permute(0, 2, 1).contiguous().view(B, D, h, w) if fmt == "NCHW" else feat.view(B, h, w, D)


def torch_dense(model, x, fmt, dtype, fill):
    """The map through forward_decisions and torch ops on the device."""
    logits, taps, dec = model.forward_decisions(x, final_tokens=True)
    tokens = taps["final_tokens"]
    index = torch_index(dec, model._decision_stages(), tokens.shape[0], model.patch_embed.num_patches, x.device)
    return logits, torch_gather(tokens, index, model.patch_embed.grid_size, fmt, dtype, fill), index.int()


def viz_levels(model, x, blocks, norm, fmt, dtype, fill):
    """The level maps through a viz_mode forward: its rows of every block (the device buffer), its slabs through tr_stage_decisions, and the
    torch composition per level."""
    from tokenreduction_amd import ops
    model.viz_mode = True
    try:
        logits, _ = model(x)
    finally:
        model.viz_mode = False
    ws, tokens, B, D, P0 = model._last_ws, model._last_tokens, x.shape[0], model.embed_dim, model.patch_embed.num_patches
    stages = model._decision_stages()
    dec = ops.stage_decisions(ws["kept"], ws["compl"], ws.get("soft"), stages, B, P0 + 1) if stages else {"kept": {}, "assign": {}}
    off = [0]
    for t in tokens:
        off.append(off[-1] + B * t * D)
    feats, indices = [], []
    for blk in blocks:
        rows = ws["feat"][off[blk]: off[blk + 1]].view(B, tokens[blk], D)
        if norm:
            rows = ops.final_tokens_f32(rows, model.norm.weight.detach(), model.norm.bias.detach(), float(model.norm.eps)).view(B, tokens[blk], D)
        index = torch_index(dec, [st for st in stages if st[0] <= blk], B, P0, x.device)
        feats.append(torch_gather(rows, index, model.patch_embed.grid_size, fmt, dtype, fill))
        indices.append(index.int())
    return logits, feats, indices


def run_levels(tag, batch, steps, rounds, fmt, dtype, blocks, norm, child=False):
    import torch
    from tokenreduction_amd import ops
    m = _create(tag)
    tdtype = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, *SIZE, generator=g).cuda()
    if tag == "dpcknn":
        m.density_noise = {blk: torch.rand(batch, P, generator=g).cuda() for blk, _, P in m._stage_shapes()}
    blocks = tuple(sorted(blocks))
    levels = lambda: m.forward_dense(x, blocks=blocks, norm=norm, output_fmt=fmt, dtype=tdtype, fill=0.0)
    P0, D, L = m.patch_embed.num_patches, m.embed_dim, len(blocks)
    if child:
        m.use_graph = False                                    # plain launches: every kernel shows under its own name in the trace
        for _ in range(steps + 2):
            levels()
        # the same un-reduce as L single-level launches, on the slabs and indices the last forward left in its static buffers
        lv, tokens, slab = m._last_ws["levels"][L], m._last_tokens, batch * (P0 + 1) * D
        index = lv["index"].view(L, batch, P0)
        for _ in range(steps + 2):
            for l, blk in enumerate(blocks):
                ops.dense_gather(lv["tokens"][l * slab: l * slab + batch * tokens[blk] * D].view(batch, tokens[blk], D), index[l], layout=fmt,
                                 dtype=tdtype, fill=0.0)
        torch.cuda.synchronize()
        m.check_status()
        return
    la, fa, ia = viz_levels(m, x, blocks, norm, fmt, tdtype, 0.0)
    lb, db = levels()
    bits = torch.int16 if tdtype == torch.bfloat16 else torch.int32
    same = bool(torch.equal(la, lb) and all(torch.equal(ia[l], db["index"][l]) and torch.equal(fa[l].view(bits), db["features"][l].view(bits))
                                            for l in range(L)))
    sides = {"plain": lambda: m(x), "viz": lambda: viz_levels(m, x, blocks, norm, fmt, tdtype, 0.0), "levels": levels}
    for fn in sides.values():
        for _ in range(2):
            fn()
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            for _ in range(3):                                 # untimed: the viz side leaves the device idle behind its host copies
                fn()
            ms[k].append(round(_event_ms(fn, steps), 4))
    m.check_status()
    med = {k: statistics.median(v) for k, v in ms.items()}
    out_bytes = 2 if dtype == "bf16" else 4
    tokens = [int(m._last_tokens[b]) for b in blocks]
    print(json.dumps({"leg": "levels", "model": MODELS[tag], "B": batch, "size": list(SIZE), "blocks": blocks, "norm": norm, "fmt": fmt, "dtype": dtype, "steps": steps,
                      "bitwise_equal": same, "level_tokens": tokens, "ms_per_batch": ms, "median_ms_per_batch": med,
                      "images_per_s": {k: round(batch / med[k] * 1e3, 1) for k in med},
                      "extra_ms_over_plain": {k: round(med[k] - med["plain"], 4) for k in ("viz", "levels")},
                      # per level: the slab written once and read at most once per patch, the map written once, the index
                      "level_extra_bytes": [batch * t * D * 4 + required_bytes(batch, P0, D, out_bytes) for t in tokens]}), flush=True)
    assert same, "forward_dense(blocks=...) and the viz_mode route disagree"


def required_bytes(B, P0, D, out_bytes):
    """What the gather has to move: the map once, one fp32 row per patch at most, the index."""
    return B * P0 * D * (out_bytes + 4) + 4 * B * P0


def run(tag, batch, steps, rounds, fmt, dtype, only_dense=False):
    import torch
    m = _create(tag)
    tdtype = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, *SIZE, generator=g).cuda()
    if tag == "dpcknn":
        m.density_noise = {blk: torch.rand(batch, P, generator=g).cuda() for blk, _, P in m._stage_shapes()}
    dense = lambda: m.forward_dense(x, output_fmt=fmt, dtype=tdtype, fill=0.0)
    if only_dense:
        m.use_graph = False                                    # plain launches: every kernel shows under its own name in the trace
        for _ in range(steps + 2):
            dense()
        torch.cuda.synchronize()
        m.check_status()
        return
    la, fa, ia = torch_dense(m, x, fmt, tdtype, 0.0)
    lb, db = dense()
    bits = torch.int16 if tdtype == torch.bfloat16 else torch.int32
    same = bool(torch.equal(la, lb) and torch.equal(ia, db["index"]) and torch.equal(fa.view(bits), db["features"].view(bits)))
    sides = {"plain": lambda: m(x), "torch": lambda: torch_dense(m, x, fmt, tdtype, 0.0), "dense": dense}
    for fn in sides.values():
        for _ in range(2):
            fn()
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(round(_event_ms(fn, steps), 4))
    m.check_status()
    med = {k: statistics.median(v) for k, v in ms.items()}
    P0, D = m.patch_embed.num_patches, m.embed_dim
    print(json.dumps({"leg": "forward", "model": MODELS[tag], "B": batch, "size": list(SIZE), "fmt": fmt, "dtype": dtype, "steps": steps, "bitwise_equal": same,
                      "n_last": int(m._last_tokens[-1]), "ms_per_batch": ms, "median_ms_per_batch": med,
                      "extra_ms_over_plain": {k: round(med[k] - med["plain"], 4) for k in ("torch", "dense")},
                      "gather_required_bytes": required_bytes(batch, P0, D, 2 if dtype == "bf16" else 4),
                      "gather_distinct_bytes": batch * P0 * D * (2 if dtype == "bf16" else 4) + 4 * batch * int(m._last_tokens[-1]) * D}), flush=True)
    assert same, "forward_dense and the torch restatement disagree"


def kernels_levels(a):
    """rocprofv3 --kernel-trace --stats over a child that runs forward_dense(blocks=...) and then the L single-level gathers: one JSON line per
    model with the batched gather against the sum of the single-level ones, and the level taps and the index."""
    L = len(a.levels)
    for tag in a.models:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   "--child", "--models", tag, "--batch", str(a.batch), "--steps", str(a.steps), "--fmt", a.fmt, "--dtype", a.dtype, "--size",
                   str(SIZE[0]), str(SIZE[1]), "--levels", *[str(b) for b in a.levels]] + (["--no-norm"] if a.no_norm else [])
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
            rows = []
            for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
                rows += list(csv.DictReader(open(path)))
        out = {"leg": "level_kernels", "model": MODELS[tag], "B": a.batch, "blocks": a.levels, "norm": not a.no_norm, "fmt": a.fmt, "dtype": a.dtype}
        names = (("dense_gather_levels", "gather_levels"), ("dense_index_levels", "index_levels"), ("dense_gather", "gather_single"),
                 ("final_tokens_kernel", "level_tap"), ("cls_tap_kernel", "level_tap"))
        for row in rows:
            key = next((k for pat, k in names if pat in row["Name"]), None)
            if key is None or (key == "level_tap" and ("cls_tap" in row["Name"]) != a.no_norm):
                continue
            calls = int(row["Calls"])
            total_ns = float(row["TotalDurationNs"]) if row.get("TotalDurationNs") else float(row["AverageNs"]) * calls
            ent = out.setdefault(key, {"calls": 0, "total_us": 0.0})
            ent["calls"] += calls
            ent["total_us"] = round(ent["total_us"] + total_ns / 1e3, 3)
            for col in ("MinNs", "MaxNs"):
                if row.get(col):
                    ent[col[:3].lower() + "_us"] = round(float(row[col]) / 1e3, 3)
        for ent in (v for v in out.values() if isinstance(v, dict)):
            ent["average_us"] = round(ent["total_us"] / max(1, ent["calls"]), 3)
        need = L * required_bytes(a.batch, (SIZE[0] // 16) * (SIZE[1] // 16), 384, 2 if a.dtype == "bf16" else 4)
        if "gather_levels" in out and "gather_single" in out:
            one, many = out["gather_levels"]["average_us"], out["gather_single"]["average_us"] * L
            out["gather_required_bytes"] = need
            out["levels_us_vs_sum_of_singles_us"] = [one, round(many, 3)]
            out["gather_levels_TB_per_s"] = round(need / (one * 1e-6) / 1e12, 3)
            out["gather_singles_TB_per_s"] = round(need / (many * 1e-6) / 1e12, 3)
            out["of_hbm_copy_rate"] = round(need / (one * 1e-6) / 1e12 / HBM_COPY_TBS, 3)
        print(json.dumps(out), flush=True)


def kernels(a):
    """rocprofv3 --kernel-trace --stats over a child that only runs forward_dense: one JSON line per model with the two kernels' average
    duration and the gather's required bytes per second."""
    for tag in a.models:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   "--child", "--models", tag, "--batch", str(a.batch), "--steps", str(a.steps), "--fmt", a.fmt, "--dtype", a.dtype, "--size",
                   str(SIZE[0]), str(SIZE[1])]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
            rows = []
            for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
                rows += list(csv.DictReader(open(path)))
        out = {"leg": "kernels", "model": MODELS[tag], "B": a.batch, "fmt": a.fmt, "dtype": a.dtype}
        need = required_bytes(a.batch, (SIZE[0] // 16) * (SIZE[1] // 16), 384, 2 if a.dtype == "bf16" else 4)
        for row in rows:
            for key in ("dense_gather", "dense_index"):
                if key in row["Name"]:
                    calls = int(row["Calls"])
                    avg_ns = float(row["AverageNs"]) if row.get("AverageNs") else float(row["TotalDurationNs"]) / calls
                    out[key] = {"calls": calls, "average_us": round(avg_ns / 1e3, 3)}
        if "dense_gather" in out:
            tbs = need / (out["dense_gather"]["average_us"] * 1e-6) / 1e12
            out["gather_required_bytes"] = need
            out["gather_TB_per_s"] = round(tbs, 3)
            out["of_hbm_copy_rate"] = round(tbs / HBM_COPY_TBS, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--fmt", default="NCHW", choices=["NCHW", "NHWC"])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--size", type=int, nargs=2, default=list(SIZE), metavar=("H", "W"), help="input height and width, multiples of 16")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--levels", type=int, nargs="*", default=None, help="the levels mode: the blocks (default 2 5 8 11)")
    ap.add_argument("--no-norm", action="store_true", help="levels mode: the rows as they stand, not their final norm")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    SIZE = tuple(a.size)
    if a.levels is not None:
        a.levels = a.levels or [2, 5, 8, 11]
        if a.models == list(MODELS):
            a.models = ["deit", "topk", "tome", "dpcknn"]
    if a.kernels and not a.child:
        kernels_levels(a) if a.levels is not None else kernels(a)
    elif a.levels is not None:
        for tag in a.models:
            run_levels(tag, a.batch, a.steps, a.rounds, a.fmt, a.dtype, a.levels, not a.no_norm, child=a.child)
    else:
        import torch
        assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
        for tag in a.models:
            run(tag, a.batch, a.steps, a.rounds, a.fmt, a.dtype, only_dense=a.child)
