#!/usr/bin/env python3
"""Headline benchmark: images/s of the DeiT-S Top-K (keep_rate 0.7, reduction_loc 3,6,9) forward pass on MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus N --steps K --warmup W        (self-launching: the parent starts the N ranks below as child processes)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" = one pass of the hot path (model.forward through the native executor) over one synthetic batch of
256 images already resident in HBM (BASELINE.json configs[1]).  Data-parallel inference shards images over
ranks with no data-path collective: every rank runs its own batch of 256 -> weak scaling.
Rank 0 prints ONE JSON line.  A plain run does only what that line's headline needs: set up, warm up, time the K steps,
write --dump-outputs, print.  --full adds the extra legs, all outside the timed region:
  the forward_async == model(x) check, the same forward one at a time and as plain launches
  finetune      fwd + bwd + AdamW through the HIP training path (every rank: the legs contain the gradient collectives)
and at N=1 on rank 0:
  roofline      per-launch HIP-event timing of the same forward, kernel by kernel, on the launch stream
  other_configs, per_config, drift_vs_fp32_path, drift_trained, bf16x3_mode
  cpu_baseline  the oracle (fp32 torch-CPU restatement of the reference) timed on this box's host cores
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

BATCH = 256
MODEL = "topk_small_patch16_224"
KEEP_RATE, REDUCTION_LOC = [0.7], [3, 6, 9]
PEAK_BF16_TFLOPS = 2500.0     # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md chip table)
def _in_kernel_clock_ghz(kernel="gemm_bf16_pc", default=2.0):
    """The shader clock the kernel runs at INSIDE the headline forward, measured in the kernel (s_memtime / s_memrealtime,
    tools/lab/clock_probe.py -> profiles/r06_clock.json): 2.0 GHz for gemm_bf16_pc, 2.1 GHz for mlp_fused_kernel on the box of round 6."""
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "r06_clock.json")))["in_model_mhz"][kernel] / 1e3
    except (OSError, KeyError, ValueError):
        return default


# gemm_bf16_pc's K-loop ceiling from the L2 -> LDS feed (see roofline_from): 85.3 FLOP per fed byte x 33 B/clk/CU x 256 CUs x the clock the
# kernel is MEASURED to run at in the model (round 5 assumed 1.45 GHz from single-kernel lab stamps: 1045; measured in round 6: ~2.0 GHz)
FEED_CEILING_TFLOPS = round(85.3 * 33.0 * 256 * _in_kernel_clock_ghz() / 1e3, 0)
PEAK_HBM_GBPS = 8000.0
# Forwards in flight during the timed steps: 2 = every step is enqueued with model.forward_async (two side streams, each with its own
# workspace and captured graph): step k + 1 starts while step k's last launches drain, the device fills one forward's tails (partial last
# rounds of the persistent kernels, the short launches of the last stage) with the other's.  Every step is a complete forward of its own
# batch and all K steps finish inside the timed bracket; `ms_per_step` is wall time / K (throughput), the line also carries the
# one-forward-at-a-time figure (`ms_per_step_one_in_flight`).  TR_BENCH_IN_FLIGHT=1 times the old way.
IN_FLIGHT = max(1, int(os.environ.get("TR_BENCH_IN_FLIGHT", "2")))


def build_model(name=MODEL, keep_rate=KEEP_RATE, loc=REDUCTION_LOC, device="cuda", img_size=224, qkv_gain=4.0):
    import tokenreduction_amd as tra
    torch.manual_seed(0)
    args = types.SimpleNamespace(keep_rate=list(keep_rate), reduction_loc=list(loc), dyvit_distill=False, k_neighbors=5,
                                 equal_weight=False, cluster_iters=3, sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False,
                                 min_radius=None)
    m = tra.create_model(name, pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0,
                         drop_block_rate=None, img_size=img_size, args=args)
    m.pipeline_depth = max(2, IN_FLIGHT)        # side streams of model.forward_async
    with torch.no_grad():                       # "peaky" attention so the Top-K sees a realistic score spread
        for blk in m.blocks:
            blk.attn.qkv.weight.mul_(qkv_gain)
    return m.to(device).eval()


def quick_images_per_s(model, x, iters=10, reps=3, in_flight=None):
    """Informational legs (dense baseline, other families): best of `reps` timed runs of `iters` forwards -- a one-off stall
    (allocator growth, first-touch of a fresh workspace) must not halve a number that is only measured once.  in_flight (default: the
    headline's IN_FLIGHT): 2 = the forwards go through model.forward_async, two at a time on two streams; 1 = model(x) on one stream."""
    k = IN_FLIGHT if in_flight is None else in_flight
    go = (lambda: model.forward_async(x)) if (k > 1 and not getattr(model, "dynamic_width", False)) else (lambda: model(x))
    for _ in range(4):
        go()
    best = 0.0
    for _ in range(reps):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(iters):
            go()
        torch.cuda.synchronize()
        best = max(best, x.shape[0] * iters / (time.perf_counter() - t1))
    return best


def model_flops_per_image(tokens_per_block, D=384, P=196, classes=1000, n0=197):
    """patch-embed + sum_blocks[8 D^2 N_attn + 4 N_attn^2 D + 16 D^2 N_mlp] + head."""
    f = 2.0 * P * 768 * D + 2.0 * D * classes
    n_attn = n0
    for n_mlp in tokens_per_block:
        f += 8.0 * D * D * n_attn + 4.0 * n_attn * n_attn * D + 16.0 * D * D * n_mlp
        n_attn = n_mlp
    return f


def profile_forward(model, x, reps=5):
    """Per-launch-group HIP-event timing of the EXECUTOR (tr_profile_begin / tr_profile_end: an event on the launch stream after
    every launch the library enqueues).  Returns {label: dict(ms, flops, bytes, launches)} with ms = the MEDIAN over `reps`
    forwards of the group's summed durations (one disturbed forward must not skew a table measured once)."""
    import ctypes as C
    from tokenreduction_amd import _lib
    lib = _lib.load()
    graph, model.use_graph = model.use_graph, False          # plain launches: events cannot be recorded inside a graph replay
    try:
        model(x)
        torch.cuda.synchronize()
        per_rep, cap = [], 4096
        labels = C.create_string_buffer(cap * 48)
        ms, fl, by = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
        for _ in range(reps):
            _lib.check(lib.tr_profile_begin(torch.cuda.current_stream().cuda_stream), "tr_profile_begin")
            model(x)
            n = lib.tr_profile_end(cap, labels, ms, fl, by)
            assert 0 < n <= cap, n
            rep = {}
            for i in range(n):
                name = labels.raw[i * 48:(i + 1) * 48].split(b"\0", 1)[0].decode()
                a = rep.setdefault(name, dict(ms=0.0, flops=0.0, bytes=0.0, launches=0))
                a["ms"] += ms[i]; a["flops"] += fl[i]; a["bytes"] += by[i]; a["launches"] += 1
            per_rep.append(rep)
    finally:
        model.use_graph = graph
    agg = {}
    for k in per_rep[0]:
        agg[k] = dict(per_rep[0][k], ms=sorted(r[k]["ms"] for r in per_rep)[reps // 2])
    return agg


def roofline_leg(model, x, reps=5):
    """Kernel table + roofline of the dominant kernel from profile_forward()."""
    roof, table, total_ms = roofline_from(profile_forward(model, x, reps), full=True)
    return roof, table, total_ms


def roofline_from(agg, full=False):
    total_ms = sum(a["ms"] for a in agg.values())
    table = {}
    for k, a in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
        t = a["ms"] * 1e-3
        tf, gb = a["flops"] / t / 1e12, a["bytes"] / t / 1e9
        table[k] = dict(share=round(a["ms"] / total_ms, 4), launches_per_fwd=a["launches"], avg_us=round(1e3 * a["ms"] / a["launches"], 2),
                        tflops=round(tf, 2), gbps=round(gb, 1), mfma_frac=round(tf / PEAK_BF16_TFLOPS, 4),
                        hbm_frac=round(gb / PEAK_HBM_GBPS, 4))
    dom = max(agg, key=lambda k: agg[k]["ms"])
    a = agg[dom]
    if a["flops"] > 0:
        ach = a["flops"] / (a["ms"] * 1e-3) / 1e12
        roof = dict(bound="mfma", kernel=dom, achieved=round(ach, 2), peak=PEAK_BF16_TFLOPS, unit="TFLOP/s",
                    frac=round(ach / PEAK_BF16_TFLOPS, 4), traffic=None,
                    flops_per_launch=a["flops"] / a["launches"], avg_launch_us=round(1e3 * a["ms"] / a["launches"], 2))
    else:
        ach = a["bytes"] / (a["ms"] * 1e-3) / 1e9
        roof = dict(bound="hbm", kernel=dom, achieved=round(ach, 1), peak=PEAK_HBM_GBPS, unit="GB/s",
                    frac=round(ach / PEAK_HBM_GBPS, 4), traffic=None,
                    bytes_per_launch=a["bytes"] / a["launches"], avg_launch_us=round(1e3 * a["ms"] / a["launches"], 2))
    if dom.startswith("gemm_bf16_pc"):
        # what bounds this kernel before the matrix pipes do (profiles/r01_gemm_lab.md): the K-loop of a 256 x 128 tile
        # feeds 48 KiB through the CU's L2 -> LDS path (~33 B/clk, measured with the DMA-only ablation) per 4.19 MFLOP = 85 FLOP per
        # fed byte; at the in-kernel clock measured inside this forward (profiles/r06_clock.json) that is the ceiling below
        roof["secondary_bound"] = dict(name="L2->LDS feed of the 256x128x64 tile at the measured in-kernel clock", ceiling=FEED_CEILING_TFLOPS,
                                       unit="TFLOP/s", frac=round(ach / FEED_CEILING_TFLOPS, 4),
                                       basis=f"85.3 FLOP per fed byte x 33 B/clk/CU x 256 CUs x {_in_kernel_clock_ghz():.2f} GHz (s_memtime / s_memrealtime "
                                             "inside the kernel, profiles/r06_clock.json)")
    if dom.startswith("mlp_fused_kernel") or dom.startswith("gemm_bf16_pc"):
        ghz = _in_kernel_clock_ghz("mlp_fused_kernel" if dom.startswith("mlp") else "gemm_bf16_pc")
        roof["in_kernel_clock_ghz"] = ghz
        roof["frac_of_peak_at_that_clock"] = round(ach / (PEAK_BF16_TFLOPS * ghz / 2.4), 4)
    roof["share_of_step"] = round(a["ms"] / total_ms, 4)
    roof["traffic_source"] = "not collected for this config (PMC passes cover the headline config)"
    if not full:
        return dict(roof, profiled_ms_per_step=round(total_ms, 3))
    return roof, table, total_ms


def kernel_source_hash():
    """sha256 over the kernel sources the shipped .so was built from: a PMC summary is only trusted for the sources it was
    collected on (tools/prof_summary.py stores the same hash)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "tokenreduction_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "tokenreduction_amd", "csrc", "*.h"))):
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def cpu_baseline_leg(model, budget_s=25.0):
    """The oracle (port of the reference's eval forward, fp32, torch CPU) on a bounded sample of the same workload: SURVEY 8d's
    protocol -- torch.set_num_threads(host cores available), 10 warm-up + 30 timed passes, median -- on a batch sized so that the
    whole leg stays within ~budget_s seconds (the batch is stated in `sample`)."""
    import oracle
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    params = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    cfg = oracle.VitConfig(family="topk", embed_dim=384, depth=12, num_heads=6, num_classes=1000,
                           keep_rate=list(KEEP_RATE), reduction_loc=list(REDUCTION_LOC))
    x = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    # torch's intra-op pool degrades badly when oversubscribed (256 threads: 45 s per pass on the GPU box): nproc is the
    # protocol's thread count, capped at the count that a 2-image probe shows is not slower than half of it
    cores = avail
    while cores > 8:
        torch.set_num_threads(cores)
        oracle.vit_forward(params, x[:2], cfg)
        t0 = time.perf_counter(); oracle.vit_forward(params, x[:2], cfg); t_full = time.perf_counter() - t0
        torch.set_num_threads(cores // 2)
        oracle.vit_forward(params, x[:2], cfg)
        t0 = time.perf_counter(); oracle.vit_forward(params, x[:2], cfg); t_half = time.perf_counter() - t0
        if t_full <= t_half:
            break
        cores //= 2
    torch.set_num_threads(cores)
    t0 = time.perf_counter(); oracle.vit_forward(params, x[:4], cfg); per_img = (time.perf_counter() - t0) / 4
    bs = max(1, min(32, int(budget_s / 40.0 / max(per_img, 1e-4))))        # 10 + 30 passes within the budget
    xs = x[:bs]
    for _ in range(10):
        oracle.vit_forward(params, xs, cfg)
    times = []
    for _ in range(30):
        t0 = time.perf_counter()
        oracle.vit_forward(params, xs, cfg)
        times.append(time.perf_counter() - t0)
    med = sorted(times)[len(times) // 2]
    return dict(value=round(bs / med, 1), unit="images/s", cores=cores, kind="port",
                sample=f"median of 30 timed forward passes (after 10 warm-up) of batch {bs} of the same model/config, fp32 torch-CPU "
                       f"oracle, {cores} of {avail} host threads, {sum(times):.1f} s timed")


def oracle_forward(family, params, x, cfg, grad=False):
    """The oracle's forward of `family` (the CPU restatement of the reference, test infrastructure: used here as the cpu_baseline only).
    grad=True: the undecorated function under autograd (the public ones run under torch.no_grad())."""
    import oracle
    fn = {"topk": oracle.vit_forward, "tome": oracle.tome_forward, "ats": oracle.ats_forward, "dpcknn": oracle.dpcknn_forward,
          "sinkhorn": oracle.sinkhorn_forward, "kmedoids": oracle.kmedoids_forward}[family]
    f = fn.__wrapped__ if grad else fn
    if family == "dpcknn":       # the density tie-break noise (dpcknn.py:71-72) is an input of the oracle: one torch.rand draw per stage
        noise, prev = {}, cfg.num_patches
        for blk, cnt in sorted(oracle.dpcknn_cluster_counts(cfg).items()):
            noise[blk] = torch.rand(x.shape[0], prev, generator=torch.Generator().manual_seed(blk))
            prev = cnt
        return f(params, x, cfg, noise)
    return f(params, x, cfg)


def cpu_config_leg(model, family, keep_rate, loc, img_size, train, budget_s=10.0):
    """cpu_baseline of one more BASELINE config: the oracle on a bounded sample (a few images, `budget_s` seconds of CPU work) of the same
    model / config on this box's host cores; train=True: forward + cross-entropy + backward by torch.autograd over the oracle (the
    reference's training step without the optimizer, engine.py:60-76)."""
    import oracle
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = min(avail, 16)                      # what the headline leg's probe settles on (torch's pool collapses when oversubscribed)
    torch.set_num_threads(cores)
    params = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    cfg = oracle.VitConfig(family=family, img_size=img_size, embed_dim=model.embed_dim, depth=model.depth, num_heads=model.num_heads,
                           num_classes=1000, keep_rate=list(keep_rate), reduction_loc=list(loc))
    x = torch.randn(2, 3, img_size, img_size, generator=torch.Generator().manual_seed(1))
    y = torch.tensor([1, 2])

    def once():
        if not train:
            return oracle_forward(family, params, x, cfg)
        leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        with torch.enable_grad():
            loss = torch.nn.functional.cross_entropy(oracle_forward(family, leaves, x, cfg, grad=True), y)
            loss.backward()
        return loss
    once()
    times, t_start = [], time.perf_counter()
    while len(times) < 3 or (time.perf_counter() - t_start < budget_s and len(times) < 30):
        t0 = time.perf_counter()
        once()
        times.append(time.perf_counter() - t0)
    med = sorted(times)[len(times) // 2]
    return dict(value=round(2 / med, 2), unit="images/s", cores=cores, kind="port",
                sample=f"median of {len(times)} passes of batch 2 ({'forward + cross-entropy + backward (torch.autograd)' if train else 'eval forward'}), "
                       f"fp32 torch-CPU oracle, {cores} of {avail} host threads, {sum(times):.1f} s timed")


def train_roofline_leg(name, keep_rate, loc, batch, device, reps=3):
    """Kernel table + roofline of the dominant kernel of one TRAINING step (forward with tape + backward; the optimizer's torch kernels are
    not in the table) from the library's launch profiler."""
    import ctypes as C
    from tokenreduction_amd import _lib
    lib = _lib.load()
    model = build_model(name, keep_rate, loc, device).train()
    x = torch.randn(batch, 3, 224, 224, generator=torch.Generator().manual_seed(200)).to(device)
    y = torch.randint(0, 1000, (batch,), generator=torch.Generator().manual_seed(300)).to(device)

    def step():
        model.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(model(x), y).backward()
    step()
    torch.cuda.synchronize()
    cap = 8192
    labels = C.create_string_buffer(cap * 48)
    ms, fl, by = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    per_rep = []
    for _ in range(reps):
        _lib.check(lib.tr_profile_begin(torch.cuda.current_stream().cuda_stream), "tr_profile_begin")
        step()
        n = lib.tr_profile_end(cap, labels, ms, fl, by)
        assert 0 < n <= cap, n
        rep = {}
        for i in range(n):
            nm = labels.raw[i * 48:(i + 1) * 48].split(b"\0", 1)[0].decode()
            a = rep.setdefault(nm, dict(ms=0.0, flops=0.0, bytes=0.0, launches=0))
            a["ms"] += ms[i]; a["flops"] += fl[i]; a["bytes"] += by[i]; a["launches"] += 1
        per_rep.append(rep)
    agg = {}
    for k in per_rep[0]:       # median over the reps that have the label (a label missing from a later rep must not lose the leg)
        vals = sorted(r[k]["ms"] for r in per_rep if k in r)
        agg[k] = dict(per_rep[0][k], ms=vals[len(vals) // 2])
    return roofline_from(agg), model


def finetune_leg(name, keep_rate, loc, batch, device, dist, steps=8, warmup=3, img_size=224):
    """fwd + loss + bwd + AdamW step through the HIP training path (engine.py:50-91 without the data loader): images/s over all
    ranks.  Under torch.distributed the gradients are averaged by tokenreduction_amd.dp.FlatGradReducer (RCCL reduce-scatter +
    all-gather per bucket, overlapped with the backward)."""
    steps = int(os.environ.get("TR_BENCH_FINETUNE_STEPS", steps))           # test rigs shorten the legs
    warmup = min(warmup, steps)
    model = build_model(name, keep_rate, loc, device, img_size).train()
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1
    x = torch.randn(batch, 3, img_size, img_size, generator=torch.Generator().manual_seed(200 + rank)).to(device)
    y = torch.randint(0, 1000, (batch,), generator=torch.Generator().manual_seed(300 + rank)).to(device)
    from tokenreduction_amd.optim import FusedAdamW              # one launch per step, bit-identical to torch.optim.AdamW(fused=True)
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.05, model=model)
    if dist is not None:
        from tokenreduction_amd.dp import FlatGradReducer
        red = FlatGradReducer().attach(model)
        red.broadcast_parameters(model)
    else:
        red = None
    last = [None]

    def step():
        loss = torch.nn.functional.cross_entropy(model(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        last[0] = loss

    el = timed_steps(step, steps, warmup, dist, torch.cuda.synchronize, device)
    assert torch.isfinite(last[0]).item()
    dp = None
    if red is not None:
        # ONE more step, outside the timed region, with events around every bucket: which part of the gradient mean the backward hides
        # (range_ms vs collective_ms per bucket, exposed_ms at the end) -- DESIGN section 5's 0.2 ms / bucket model is checked against this
        red.record_timing = True
        step()
        dp = red.timing()
        red.record_timing = False
        if dp is not None:
            try:
                dp["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception as e:          # gloo rigs
                dp["rccl_version"] = f"n/a ({type(e).__name__})"
            dp["nccl_env"] = {k: v for k, v in os.environ.items() if k.startswith(("NCCL_", "RCCL_", "HSA_ENABLE_IPC"))}
    return {"dp": dp, "images_per_s": round(world * batch * steps / el, 1), "ms_per_step": round(1e3 * el / steps, 3), "batch_per_gpu": batch,
            "n_gpus": world, "steps": steps, "warmup": warmup, "optimizer": "tokenreduction_amd.optim.FusedAdamW (one launch; bit-identical to torch AdamW(fused=True))", "loss_last": round(last[0].item(), 4),
            "tokens_per_block": model._last_tokens}


def timed_steps(step, steps, warmup, dist, sync, device):
    """W untimed + K timed steps bracketed by barrier + device sync on both sides; returns MAX-over-ranks seconds."""
    for _ in range(warmup):
        step()
    if dist is not None:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    el = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([el], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = t.item()
        dist.barrier()
    return el


def pmc_traffic(kernel_label, workload="headline"):
    """HBM bytes per launch of `kernel_label` from the committed PMC summary of `workload` (tools/prof_r04.sh + tools/prof_summary.py:
    profiles/<tag>_<workload>_pmc_traffic.json; FETCH_SIZE / WRITE_SIZE in separate rocprofv3 --pmc passes, gfx950 corrections) --
    NOT measured in this run, and only used when the summary was collected on the kernel sources this library was built from
    (source hash), else None with the reason."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"*_{workload}_pmc_traffic.json")))
    if not files and workload == "headline":
        files = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", "r0*_pmc_traffic.json")) if "_final_" in f or "_a_" in f)
    if not files:
        return None
    tbl = json.load(open(files[-1]))
    if tbl.get("_kernel_source_hash") != kernel_source_hash():
        return dict(hbm_bytes_per_launch=None, source=os.path.basename(files[-1]),
                    note="stale: collected on other kernel sources than the ones built here; re-run tools/prof_r04.sh")
    m = re.match(r"(\w+)<EPI_(\w+)>", kernel_label)
    epi = {"BF16": 0, "GELU_BF16": 1, "RESID_F32": 2, "F32": 3, "PATCH_F32": 4, "GELU_KEEP": 16, "DGELU": 17}
    key = f"{m.group(1)}<{epi[m.group(2)]}>" if m and m.group(2) in epi else kernel_label
    v = tbl.get(key)
    if v is None:       # labels of the launch profiler carry no template arguments: first table key that starts with the label
        v = next((t for k, t in tbl.items() if not k.startswith("_") and k.split("<")[0] == key.split("<")[0]), None)
    return None if v is None else dict(hbm_bytes_per_launch=v["hbm_bytes_per_launch"], source=os.path.basename(files[-1]),
                                       collected="offline (committed profile), not in this run")


def attach_traffic(roof, workload):
    """`traffic` of a roofline record: HBM bytes per launch of its kernel from the committed PMC summary of `workload` (or null + why)."""
    t = pmc_traffic(roof["kernel"], workload)
    roof["traffic"] = None if t is None else t.get("hbm_bytes_per_launch")
    roof["traffic_unit"] = "B/launch"
    roof["traffic_source"] = ("no committed PMC summary for this workload" if t is None else
                              t.get("source") + " (" + t.get("collected", "") + ")" + ("" if t.get("note") is None else ": " + t["note"]))
    return roof


def fenced(fn, *args, **kw):
    """An informational leg must never cost the JSON line: its exception becomes its value."""
    try:
        return fn(*args, **kw)
    except Exception as e:      # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"[:300]}


def headline_record(a, world, headline, eager_ms, note=None):
    """The contract's JSON record of the headline measurement (BASELINE.json configs[1])."""
    el, tokens = headline["el"], headline["tokens"]
    ips = world * BATCH * a.steps / el
    gflop = model_flops_per_image(tokens) / 1e9
    rec = {
        "metric": "images/sec DeiT-S Top-K keep_rate=0.7 forward (aggregate over n_gpus; per-GPU = value/n_gpus)",
        "value": round(ips, 1), "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(1e3 * el / a.steps, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"{MODEL} keep_rate=0.7 reduction_loc=3,6,9 batch={BATCH}/GPU 224x224 eval forward "
                               f"(BASELINE.json configs[1])", "global_batch": BATCH * world,
                   "tokens_per_block": tokens, "gflop_per_image": round(gflop, 3), "parallelism": f"dp{world}"},
        "launch_mode": ("hipGraph replay of the executor's launch sequence; " +
                        (f"{IN_FLIGHT} forwards in flight (model.forward_async: step k + 1 is enqueued on a second stream with its own workspace "
                         "while step k drains; every step is a complete forward of its batch, all K finish inside the timed bracket)"
                         if IN_FLIGHT > 1 else "one forward at a time")),
        "forwards_in_flight": IN_FLIGHT,
        "ms_per_step_one_in_flight": None if headline.get("one_ms") is None else round(headline["one_ms"], 3),
        "images_per_s_one_in_flight": None if headline.get("one_ms") is None else round(world * BATCH / headline["one_ms"] * 1e3, 1),
        "ms_per_step_plain_launches": None if eager_ms is None else round(eager_ms, 3),
        "model_tflops": round(ips * gflop / 1e3, 1),
        "model_mfma_frac": round(ips * gflop / 1e3 / (PEAK_BF16_TFLOPS * world), 4),
    }
    if headline.get("dp"):
        rec["dp"] = headline["dp"]
    if note:
        rec["note"] = note
    return rec


def self_launch(nproc, argv):
    """Parent of an N-rank run started as plain `python bench.py --gpus N`: one child (torch.distributed.run, which forks one rank per GPU)
    on a free local port; stdout is passed through line by line (rank 0's JSON line is the last line), the child's return code is ours.
    The parent makes no HIP call: `import torch` alone does not initialise the device."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes fails without it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)
    for line in proc.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
    return proc.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run the extra legs (one-at-a-time and plain-launch timings, forward_async check, fine-tune, "
                         "roofline, other configs, drift, cpu_baseline); a plain run only sets up, warms up, times the steps and prints")
    ap.add_argument("--no-extra", action="store_true", help="skip the extra legs even with --full (a run without --full has none)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the RCCL process group even at world size 1 (exercises the N>1 code path on one GPU)")
    ap.add_argument("--selftest-gloo", action="store_true",
                    help="CPU-only check of the multi-process harness (gloo, no model): each rank's step sleeps 10 ms x (rank+1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the logits of the last timed step as DIR/logits.npy (float32; rank r > 0: "
                         "DIR/logits_rank<r>.npy); the inputs are seeded, so two builds can be compared output for output")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    extra = a.full and not a.no_extra

    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        # `python bench.py --gpus N` without a launcher: this process becomes the PARENT -- it never touches the device -- and starts the N
        # ranks as fresh children through torch.distributed.run (a child process, never an exec: a process that has initialised the GPU must
        # not be replaced), relays rank 0's JSON line and the launcher's exit code.  train.py:405-407 / utils.py:216-238 expect the same
        # env-variable rendezvous.
        sys.exit(self_launch(a.gpus, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}: run `python bench.py --gpus {a.gpus}` (self-launching) or torch.distributed.run"
    dist = None
    if world > 1 or a.force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if a.selftest_gloo:
        if os.environ.get("TR_BENCH_SELFTEST_FAIL_RANK") == str(rank):      # test hook: a rank that dies must fail the whole run
            sys.exit(7)
        if dist is not None:
            dist.init_process_group("gloo")
        el = timed_steps(lambda: time.sleep(0.01 * (rank + 1)), a.steps, a.warmup, dist, lambda: None, torch.device("cpu"))
        if rank == 0:
            print(json.dumps({"metric": "selftest", "value": round(world * BATCH * a.steps / el, 1), "unit": "images/s",
                              "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                              "ms_per_step": round(1e3 * el / a.steps, 3), "scaling": "weak"}), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return
    # TR_BENCH_SHARE_GPU=1 (test rigs with ONE GPU): all ranks use cuda:0 and the collectives go through gloo (RCCL refuses two ranks
    # on one device) -- exercises the N > 1 code path end to end; the numbers it prints mean nothing.
    share = os.environ.get("TR_BENCH_SHARE_GPU") == "1"
    if dist is not None:
        torch.cuda.set_device(0 if share else local_rank)
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", local_rank if (world > 1 and not share) else 0)

    # data-parallel inference: every rank owns its own shard of images (one batch of 256), weights replicated, no collective
    # on the data path
    model = build_model(device=dev)
    x = torch.randn(BATCH, 3, 224, 224, generator=torch.Generator().manual_seed(100 + rank)).to(dev)
    out = [None]
    pend = []

    def step():
        out[0] = model(x)

    def step_in_flight():                    # one step = one forward of the batch, enqueued beside the previous one (see IN_FLIGHT)
        pend.append(model.forward_async(x))
        if len(pend) > 4:
            pend.pop(0)

    if IN_FLIGHT > 1:
        # part of setting the model up (like packing its weights), not of the W warm-up steps: every side stream's workspace exists and its
        # graph is captured before the first step, whatever --warmup says
        for _ in range(2 * max(2, IN_FLIGHT)):
            model.forward_async(x).result()
        torch.cuda.synchronize()
    el = timed_steps(step_in_flight if IN_FLIGHT > 1 else step, a.steps, a.warmup, dist, torch.cuda.synchronize, dev)
    if pend:
        out[0] = pend[-1].result()
        if extra:
            ref = model(x)                   # the same batch, one forward at a time: the pipelined steps computed the same bits
            assert torch.equal(out[0], ref), "forward_async and model(x) disagree"
    assert torch.isfinite(out[0]).all()
    model.check_status()        # what only the device knows (the fused Mlp's stream-K hand-over record) fails the run here, not silently
    if a.dump_outputs:          # what a caller of the timed path received from its last step: the logits [BATCH, 1000], 1 MB per rank
        import numpy as np
        os.makedirs(a.dump_outputs, exist_ok=True)
        np.save(os.path.join(a.dump_outputs, "logits.npy" if rank == 0 else f"logits_rank{rank}.npy"),
                out[0].detach().float().cpu().numpy())
    one_ms = 1e3 * timed_steps(step, a.steps, 2, dist, torch.cuda.synchronize, dev) / a.steps if IN_FLIGHT > 1 and extra else None
    eager_ms = None
    if rank == 0 and extra:                   # the same forward as plain launches (model.use_graph = False): what the graph replay saves
        model.use_graph = False
        eager_ms = 1e3 * timed_steps(step, a.steps, 2, None, torch.cuda.synchronize, dev) / a.steps
        model.use_graph = True

    # fine-tune legs (all ranks take part: they contain the gradient collectives).  Extra key, outside the headline's timed region.
    # They must never cost the headline line: every leg is fenced (an exception becomes an "error" entry), and at N > 1 a watchdog
    # prints the headline without them and ends the process if a collective hangs (the legs have only ever run at N = 1 on RCCL).
    finetune = None
    headline = {"el": el, "tokens": list(model._last_tokens), "one_ms": one_ms}
    if dist is not None:
        # what the process group itself reports (not the command line): rank count, backend, and the device every rank ran on
        me = torch.tensor([rank, torch.cuda.current_device()], device=dev, dtype=torch.int32)
        seen = [torch.zeros_like(me) for _ in range(dist.get_world_size())]
        dist.all_gather(seen, me)
        headline["dp"] = {"world": dist.get_world_size(), "backend": dist.get_backend(),
                          "cuda_device_by_rank": {str(int(v[0])): int(v[1]) for v in seen}}
    if extra:
        import threading
        done = threading.Event()

        def watchdog():
            if done.wait(float(os.environ.get("TR_BENCH_FINETUNE_TIMEOUT", "420"))):
                return
            # the headline line is flushed first (the forward was measured), then the process ends NON-ZERO: a hung collective is a
            # failure of the run and must reach the driver as one (round-2 verdict: it used to exit 0)
            if rank == 0:
                print(json.dumps(headline_record(a, world, headline, None, "fine-tune legs timed out (collective hang?)")), flush=True)
            os._exit(3)
        if world > 1:
            threading.Thread(target=watchdog, daemon=True).start()
        finetune = {}
        for label, args_ in (("topk_small kr0.7 B=256/GPU (configs[1] model, fwd+bwd+AdamW)", (MODEL, KEEP_RATE, REDUCTION_LOC, BATCH, dev, dist)),
                             # BASELINE.json configs[3]: DeiT-B ATS / DPC-KNN keep_rate 0.5, DP fine-tune at 128 images per GPU (1024 on 8 GPUs)
                             ("ats_base kr0.5 B=128/GPU (configs[3], fwd+bwd+AdamW)", ("ats_base_patch16_224", [0.5], [3, 6, 9], 128, dev, dist, 6, 2)),
                             ("dpcknn_base kr0.5 B=128/GPU (configs[3], fwd+bwd+AdamW)", ("dpcknn_base_patch16_224", [0.5], [3, 6, 9], 128, dev, dist, 6, 2))):
            try:
                finetune[label] = finetune_leg(*args_)
            except Exception as e:          # noqa: BLE001 -- reported in the line, the headline stands
                finetune[label] = {"error": f"{type(e).__name__}: {e}"[:300]}
                if world > 1:
                    break                   # the other ranks are inside a collective: no further legs
        done.set()
    if rank == 0:
        ips = world * BATCH * a.steps / el
        tokens = model._last_tokens
        gflop = model_flops_per_image(tokens) / 1e9
        rec = headline_record(a, world, headline, eager_ms)
        if finetune is not None:
            rec["finetune"] = finetune
        if world == 1 and extra:
            for label, name, kr, loc, bsz in (("deit_small dense B=256 (fwd+bwd+AdamW)", "deit_small_patch16_224_local", [1.0], [], 256),
                                              ("evit_small kr0.7 B=256 (fwd+bwd+AdamW)", "evit_small_patch16_224", [0.7], [3, 6, 9], 256),
                                              ("tome_small r16 B=256 (fwd+bwd+AdamW)", "tome_small_patch16_224",
                                               [196 - 16 * (i + 1) for i in range(12)], list(range(12)), 256)):
                rec["finetune"][label] = finetune_leg(name, kr, loc, bsz, dev, None, steps=5, warmup=2)
            roof, table, step_ms = roofline_leg(model, x)
            # `traffic`: HBM bytes per launch of the dominant kernel as a plain number (or null), from the PMC passes committed with the
            # profile of these very kernel sources (source hash); where it came from / why it is null goes to `traffic_source`
            attach_traffic(roof, "headline")
            rec["roofline"] = roof
            rec["kernels"] = table
            rec["profiled_ms_per_step"] = round(step_ms, 3)      # same executor, plain launches with an event after each
            # no-reduction DeiT-S through the same kernels: the baseline the north_star's speed-up is quoted against
            dense = build_model("deit_small_patch16_224_local", [1.0], [], dev)
            d_ips = quick_images_per_s(dense, x)
            rec["dense_deit_s_images_per_s"] = round(d_ips, 1)
            rec["speedup_vs_dense"] = round(ips / d_ips, 3)
            # the other single-GPU BASELINE configs, same batch, same kernels (informational; `value` stays configs[1] Top-K)
            others = {}
            for label, name, kr, loc in (("evit_small kr0.7 (configs[1])", "evit_small_patch16_224", [0.7], [3, 6, 9]),
                                         ("tome_small r16 every block (configs[2])", "tome_small_patch16_224",
                                          [196 - 16 * (i + 1) for i in range(12)], list(range(12))),
                                         ("topk_small kr0.5 (north_star speed-up target)", MODEL, [0.5], [3, 6, 9]),
                                         ("dyvit_small kr0.7 (eval path)", "dyvit_small_patch16_224", [0.7], [3, 6, 9]),
                                         ("sit_small kr0.7", "sit_small_patch16_224", [0.7], [3, 6, 9]),
                                         ("ats_small kr0.7 (static K padding)", "ats_small_patch16_224", [0.7], [3, 6, 9]),
                                         ("dpcknn_small kr0.7", "dpcknn_small_patch16_224", [0.7], [3, 6, 9]),
                                         ("sinkhorn_small kr0.7", "sinkhorn_small_patch16_224", [0.7], [3, 6, 9]),
                                         ("kmedoids_small kr0.7", "kmedoids_small_patch16_224", [0.7], [3, 6, 9]),
                                         ("patchmerger_small kr0.7", "patchmerger_small_patch16_224", [0.7], [3, 6, 9])):
                m2 = build_model(name, kr, loc, dev)
                o_ips = quick_images_per_s(m2, x)
                others[label] = {"images_per_s": round(o_ips, 1), "speedup_vs_dense": round(o_ips / d_ips, 3),
                                 "tokens_per_block": m2._last_tokens}
                if kr == [0.5]:
                    # north_star's target line: what the FLOP count allows (the ">= 4 x" target would need 4 x fewer FLOPs than dense: not
                    # at this schedule), and the drift of this very schedule against the fp32 executor (random-init weights: drift_trained
                    # has the trained-weight numbers under "keep_rate_0.5")
                    others[label]["flop_ceiling_vs_dense"] = round(model_flops_per_image([197] * 12) / model_flops_per_image(m2._last_tokens), 3)
                    m2.precision = "fp32"
                    l32 = m2(x[:64]).float()
                    dr = {}
                    for prec in ("bf16", "bf16x3"):
                        m2.precision = prec
                        lb = m2(x[:64]).float()
                        dr[prec] = {"logit_rel_l2": float(f"{((lb - l32).norm() / l32.norm()).item():.3e}"),
                                    "logit_max_abs": float(f"{(lb - l32).abs().max().item():.3e}"),
                                    "top1_agreement": round((lb.argmax(1) == l32.argmax(1)).float().mean().item(), 4)}
                    m2.precision = "bf16"
                    others[label]["drift_vs_fp32_path"] = dr
                del m2
            # forward throughput of the DeiT-B configurations BASELINE names (configs[3] families at 224^2, configs[4] at 384^2);
            # their DP fine-tuning / 8-GPU sweeps are not measured here
            for label, name, kr, img, bsz in (("ats_base kr0.5 224^2 B=128 (configs[3] family, forward)", "ats_base_patch16_224", [0.5], 224, 128),
                                              ("dpcknn_base kr0.5 224^2 B=128 (configs[3] family, forward)", "dpcknn_base_patch16_224", [0.5], 224, 128),
                                              ("sinkhorn_base kr0.25 384^2 B=64 (configs[4] family)", "sinkhorn_base_patch16_224", [0.25], 384, 64),
                                              ("kmedoids_base kr0.25 384^2 B=64 (configs[4] family)", "kmedoids_base_patch16_224", [0.25], 384, 64)):
                m2 = build_model(name, kr, [3, 6, 9], dev, img_size=img)
                xb = torch.randn(bsz, 3, img, img, generator=torch.Generator().manual_seed(7)).to(dev)
                o_ips = quick_images_per_s(m2, xb)
                others[label] = {"images_per_s": round(o_ips, 1), "tokens_per_block": m2._last_tokens}
                if name.startswith("ats_"):
                    # the reference's dynamic width (ats.py:77-78: every sampling block shrinks to the batch maximum of unique ids): opt-in,
                    # plain launches with one read-back per sampling block instead of a hipGraph replay
                    m2.dynamic_width = True
                    d_ips = quick_images_per_s(m2, xb)
                    others[label]["dynamic_width"] = {"images_per_s": round(d_ips, 1), "tokens_per_block": m2._last_tokens,
                                                      "note": "model.dynamic_width = True: rows = batch max of unique sampled ids, as the "
                                                              "reference; random-init weights -- a trained model's cdf is peakier (fewer unique ids)"}
                del m2, xb
            rec["other_configs"] = others
            # drift of the bf16 product path against the SAME executor in the reference's fp32 arithmetic (validation kernels):
            # synthetic weights and inputs, so these are numerics indicators, not accuracy claims.  The dense model shows the
            # arithmetic drift alone; with Top-K every flipped boundary token changes the token set of all later blocks.
            def drift(m, xs):
                out = {"images": int(xs.shape[0])}
                m.precision = "fp32"
                lf = m(xs).float()
                for prec in ("bf16", "bf16x3"):
                    m.precision = prec
                    lb = m(xs).float()
                    out[prec] = {"logit_rel_l2": float(f"{((lb - lf).norm() / lf.norm()).item():.3e}"),
                                 "logit_max_abs": float(f"{(lb - lf).abs().max().item():.3e}"),
                                 "top1_agreement": round((lb.argmax(1) == lf.argmax(1)).float().mean().item(), 4)}
                m.precision = "bf16"
                return out
            rec["drift_vs_fp32_path"] = {"dense_deit_s": drift(dense, x[:64]), "topk_kr0.7": drift(model, x[:64]),
                                         "note": "random-init weights (qkv x4): near-flat, ill-conditioned logits"}
            # the same with the plain initialisation (trunc_normal(0.02), no qkv gain): near-uniform attention, i.e. what random
            # weights give without the conditioning stress -- SURVEY 8d's well-conditioned counterpart of the "peaky" variant
            plain_dense = build_model("deit_small_patch16_224_local", [1.0], [], dev, qkv_gain=1.0)
            plain_topk = build_model(qkv_gain=1.0, device=dev)
            rec["drift_vs_fp32_path"]["plain_init"] = {"dense_deit_s": drift(plain_dense, x[:64]), "topk_kr0.7": drift(plain_topk, x[:64])}
            del plain_dense, plain_topk
            # precision="bf16x3": the fp32 executor with Linears + attention as split-bf16 (hi/lo) products on the matrix cores -- the
            # mode that meets north_star's 1e-3-abs logit tolerance against the reference's golden vectors (tests/test_hip_split.py)
            model.precision = "bf16x3"
            x3_ips = quick_images_per_s(model, x, iters=3, reps=2)
            model.precision = "bf16"
            rec["bf16x3_mode"] = {"images_per_s": round(x3_ips, 1), "ms_per_step": round(BATCH / x3_ips * 1e3, 3),
                                  "vs_bf16_product_path": round(x3_ips / ips, 3),
                                  "label": "images/s of the split-bf16 executor: logits <= 1e-3 abs on every image whose token decisions equal the "
                                           "reference's (all golden cases: tests/test_hip_split.py); how many images of a trained model flip a "
                                           "boundary token and then miss 1e-3: drift_trained.bf16x3.images_over_1e-3*.  The bf16 `value` is not within 1e-3.",
                                  "note": "same config as `value`; 3 MFMAs per product, fp32 activations, fp32 twins for every non-GEMM op"}
            rec["cpu_baseline"] = cpu_baseline_leg(model)
            # SURVEY 8d asks the same three numbers (images/s, fraction of the dominant kernel's roofline, CPU baseline) for every BASELINE
            # config, not only the headline: configs[2] ToMe r16 (eval), configs[3] DeiT-B ATS / DPC-KNN kr 0.5 (the per-GPU shape of the DP
            # fine-tune: a training step at 128 images), configs[4] DeiT-B Sinkhorn / K-Medoids kr 0.25 at 384^2 (eval)
            per = {}
            tome_kr = [196 - 16 * (i + 1) for i in range(12)]

            def eval_config(name, fam, kr, loc, img, bsz, workload):
                m2 = build_model(name, kr, loc, dev, img_size=img)
                xb = torch.randn(bsz, 3, img, img, generator=torch.Generator().manual_seed(7)).to(dev)
                entry = {"images_per_s": round(quick_images_per_s(m2, xb), 1), "tokens_per_block": m2._last_tokens,
                         "roofline": attach_traffic(roofline_from(profile_forward(m2, xb, 3)), workload),
                         "cpu_baseline": fenced(cpu_config_leg, m2, fam, kr, loc, img, train=False)}
                if img == 384:       # configs[4]: "DP inference throughput sweep" -- the per-GPU batch sweep (8 GPUs: x 8, no collective)
                    sweep = {}
                    for b2 in (32, 64, 128, 256):
                        xs = torch.randn(b2, 3, img, img, generator=torch.Generator().manual_seed(8)).to(dev)
                        sweep[str(b2)] = round(quick_images_per_s(m2, xs, iters=5, reps=2), 1)
                        del xs
                    entry["images_per_s_by_batch"] = sweep
                return entry

            def train_config(name, fam, kr, workload):
                roof, m3 = train_roofline_leg(name, kr, [3, 6, 9], 128, dev)
                ft = rec["finetune"].get(next(k for k in rec["finetune"] if k.startswith(name.split("_patch")[0])), {})
                return {"images_per_s": ft.get("images_per_s"), "ms_per_step": ft.get("ms_per_step"), "roofline": attach_traffic(roof, workload),
                        "cpu_baseline": fenced(cpu_config_leg, m3, fam, kr, [3, 6, 9], 224, train=True)}

            for label, name, fam, kr, loc, img, bsz, wl in (
                    ("configs[2] tome_small r16 eval B=256", "tome_small_patch16_224", "tome", tome_kr, list(range(12)), 224, 256, "tome"),
                    ("configs[4] sinkhorn_base kr0.25 384^2 eval B=64", "sinkhorn_base_patch16_224", "sinkhorn", [0.25], [3, 6, 9], 384, 64, "sinkb384"),
                    ("configs[4] kmedoids_base kr0.25 384^2 eval B=64", "kmedoids_base_patch16_224", "kmedoids", [0.25], [3, 6, 9], 384, 64, "kmedb384")):
                per[label] = fenced(eval_config, name, fam, kr, loc, img, bsz, wl)
            for label, name, fam, kr, wl in (("configs[3] ats_base kr0.5 train step B=128", "ats_base_patch16_224", "ats", [0.5], "atsb_train"),
                                             ("configs[3] dpcknn_base kr0.5 train step B=128", "dpcknn_base_patch16_224", "dpcknn", [0.5], "dpcknnb_train")):
                per[label] = fenced(train_config, name, fam, kr, wl)
            # drift of the product path on TRAINED weights (tools/drift_trained.py): 600 AdamW steps of the HIP training path on a
            # separable synthetic task, then >= 10 k held-out images under the fp32, bf16 and bf16x3 executors
            import importlib.util
            spec = importlib.util.spec_from_file_location("drift_trained", os.path.join(ROOT, "tools", "drift_trained.py"))
            dt = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(dt)
            rec["drift_trained"] = fenced(dt.run, dev)
            rec["per_config"] = per
        try:        # RCCL writes its banner through C stdio: flush it first so the JSON line is the last thing on stdout
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        print(json.dumps(rec), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
