"""The cases of the forward executor's launch trace (tests/golden/executor_trace.json): what each case builds and runs, shared by the
generator (tests/golden/gen_executor_trace.py) and the test (tests/test_executor_trace_gpu.py).

run_case(name) -> (launches, digest): the (label, flops, bytes) of every launch of ONE plain-launch forward (hipGraph replay off), and a
sha256 over the bytes of everything that forward wrote for its caller -- logits, kept / complement ids, soft assignments, Features,
tokens per block, and for a training forward the whole activation tape.  Every output buffer is zero-filled before the recorded
forward, so the bytes the executor does not write are defined.  Every random input (density noise, Gumbel noise, DropPath draws,
dropout masks, the first medoids, the augmentation table) comes from a fixed seed."""
import ctypes as C
import hashlib

import numpy as np
import torch

from tests._launches import record
from tests._params import GOLDEN_CASES, make_images

MICRO = ["deit_micro", "topk_micro", "evit_micro", "evit_micro_explicit", "tome_micro", "ats_micro", "dyvit_micro", "sit_micro",
         "dpcknn_micro", "dpcknn_micro_equal", "kmedoids_micro", "kmedoids_micro_equal", "sinkhorn_micro", "patchmerger_micro",
         "heuristic_micro_l2", "sit_tiny"]
WIDE = ["topk_micro", "tome_micro", "ats_micro", "sit_micro", "sinkhorn_micro", "patchmerger_micro", "dyvit_micro", "kmedoids_micro"]
TRAIN = ["deit_micro", "topk_micro", "evit_micro", "tome_micro", "ats_micro", "dyvit_micro", "sit_micro", "dpcknn_micro", "kmedoids_micro",
         "sinkhorn_micro", "patchmerger_micro", "heuristic_micro_l2", "topk_micro_droppath", "topk_micro_dropout", "evit_micro_dropout",
         "dyvit_micro_train", "dyvit_tiny_train", "sinkhorn_micro_384"]
# DeiT-S width (the only one that reaches the fused Mlp): (set_mlp_fused, set_mlp_ln, set_mlp_resid_ln, set_cls_tail, forward_async) --
# the full product of the four switches, and one forward in flight beside others (forward_async) under the default switches
SMALL = ["deit_small", "topk_small_kr07"]
SWITCHES = [(fused, ln, resid, tail, 0) for fused in (-1, 0, 1) for ln in (0, 1, 2) for resid in (0, 1) for tail in (0, 1)] + [(-1, 1, 0, 1, 1)]


def _cases():
    c = {}
    for n in MICRO:
        c[f"eval/{n}/bf16"] = dict(base=n)
    for prec in ("fp32", "bf16x3"):
        for n in WIDE:
            c[f"eval/{n}/{prec}"] = dict(base=n, precision=prec)
    for n in ("topk_micro", "evit_micro", "dpcknn_micro", "sit_micro"):
        c[f"eval/{n}/viz"] = dict(base=n, viz=True)
    c["eval/deit_micro/headless"] = dict(base="deit_micro", headless=True)
    c["eval/deit_micro/headless_fp32"] = dict(base="deit_micro", headless=True, precision="fp32")
    c["eval/topk_micro/u8_nchw"] = dict(base="topk_micro", pixels="nchw")
    c["eval/topk_micro/u8_nhwc"] = dict(base="topk_micro", pixels="nhwc")
    c["eval/ats_micro/dynamic_width"] = dict(base="ats_micro", dynamic_width=True)
    c["eval/topk_micro_384/bf16"] = dict(base="topk_micro_384")
    for n in SMALL:
        for fused, ln, resid, tail, conc in SWITCHES:
            c[f"eval/{n}/fused{fused}_ln{ln}_resid{resid}_tail{tail}" + ("_async" if conc else "")] = dict(
                base=n, switches=(fused, ln, resid, tail), concurrent=bool(conc))
    for n in TRAIN:
        c[f"train/{n}"] = dict(base=n, train=True)
    c["train/topk_micro/headless"] = dict(base="topk_micro", train=True, headless=True)
    c["train/topk_micro/u8"] = dict(base="topk_micro", train=True, pixels="nchw")
    c["train/topk_micro/aug"] = dict(base="topk_micro", train=True, pixels="nhwc", aug=True, batch=4)
    return c


CASES = _cases()
# eval bf16 micro cases: their hashes must reproduce at the commit the fixture is recorded from
MUST_HASH = [f"eval/{n}/bf16" for n in MICRO]


def device_header():
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "compute_units": p.multi_processor_count}


def _digest(parts):
    h = hashlib.sha256()
    for t in parts:
        if t is None:
            continue
        if torch.is_tensor(t):
            t = t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()
        h.update(np.ascontiguousarray(t).tobytes())
    return h.hexdigest()


def _seeded_inputs(model, case, spec, B):
    """Every random input of the forward from a fixed seed (set once: the attributes are re-read by every forward)."""
    g = torch.Generator().manual_seed(case["xseed"] + 1234)
    fam = case["family"]
    if fam == "dpcknn":
        model.density_noise = {blk: torch.rand(B, P, generator=g) for blk, _, P in model._stage_shapes()}
    if spec.get("train"):
        if fam == "dyvit":
            P = model.patch_embed.num_patches
            model.gumbel_noise = {j: -torch.empty(B, P, 2).exponential_(generator=g).log() for j in range(len(model.pruning_loc))}
        if case.get("drop_path"):
            model.drop_path_draws = torch.rand(2 * model.depth, B, generator=g)
        if case.get("drop_rate"):
            from tokenreduction_amd import _lib
            n = int(_lib.load().tr_vit_dropout_mask_bytes(C.byref(model._pack(need_transposed=True)["cfg"]), B))
            model.dropout_draws = [(torch.rand(n, generator=g) >= case["drop_rate"]).to(torch.uint8)]


def _input(case, spec, B):
    S = case.get("img_size", 224)
    if not spec.get("pixels"):
        return make_images(B, S, case["xseed"]).cuda()
    u8 = torch.randint(0, 256, (B, 3, S, S), generator=torch.Generator().manual_seed(case["xseed"]), dtype=torch.uint8).cuda()
    if spec["pixels"] == "nhwc":
        u8 = u8.contiguous(memory_format=torch.channels_last)
    if not spec.get("aug"):
        return u8
    from tests.test_device_augment import make_table
    from tokenreduction_amd import augment
    F = np.float32
    # erased + pasted, blended, untouched, erased + blended: boxes off the 8- and 16-pixel grids, one touching the right and bottom edge
    rows = [dict(kind=2, yl=37, yh=S - 50, xl=21, xh=S - 3, erased=1, ey=30, eh=61, ex=45, ew=83, noise_off=0),
            dict(kind=1, lam=F(0.3), oml=F(1.0 - 0.3)), {},
            dict(kind=1, lam=F(0.75), oml=F(1) - F(0.75), erased=1, ey=S - 70, eh=70, ex=S - 99, ew=99, noise_off=3 * 61 * 83)]
    noise = torch.randn(3 * (61 * 83 + 70 * 99), generator=torch.Generator().manual_seed(S))
    return augment.AugmentedBatch(u8, make_table(rows[:B]), noise.cuda())


_SMALL_MODELS = {}


def _set_switches(ops, fused, ln, resid, tail):
    return (ops.set_mlp_fused(fused), ops.set_mlp_ln(ln), int(ops.set_mlp_resid_ln(bool(resid))), int(ops.set_cls_tail(bool(tail))))


def run_case(name):
    from tests.test_hip_model import build_model
    from tokenreduction_amd import ops
    spec = CASES[name]
    case = dict(GOLDEN_CASES[spec["base"]])
    B = case["batch"] = spec.get("batch", case["batch"])
    if "switches" in spec:                     # the DeiT-S models are built once; a new set of switches starts from fresh workspaces
        if spec["base"] not in _SMALL_MODELS:
            _SMALL_MODELS[spec["base"]] = build_model(case)[0]
        model = _SMALL_MODELS[spec["base"]]
        model._ws = {}
    else:
        model, _, _ = build_model(case)
    model.viz_mode = bool(spec.get("viz"))
    model.use_graph = False
    model.precision = spec.get("precision", "bf16")
    model.dynamic_width = bool(spec.get("dynamic_width"))
    if spec.get("headless"):
        model.reset_classifier(0)
    if spec.get("pixels"):
        model.set_pixel_input()
    if spec.get("train"):
        model.train()
    _seeded_inputs(model, case, spec, B)
    x = _input(case, spec, B)
    out = []

    def forward():
        np.random.seed(case["xseed"])          # K-Medoids equal_weight draws its first medoids from numpy's global generator
        out[:] = [model.forward_async(x).result() if spec.get("concurrent") else model(x)]

    before = _set_switches(ops, *spec["switches"]) if "switches" in spec else None
    try:
        forward()                              # warm-up: allocates the workspace, the outputs and the tape
        torch.cuda.synchronize()
        if spec.get("train"):
            bufs = [model._train_state().tape]
        else:
            ws = model._last_ws
            bufs = [ws["kept"], ws["compl"], ws.get("soft"), ws.get("feat")]
        for b in bufs:
            if b is not None:
                b.zero_()
        torch.cuda.synchronize()
        launches = record(forward)
        torch.cuda.synchronize()
        if not spec.get("train"):
            model.check_status()
    finally:
        if before is not None:
            _set_switches(ops, *before)
    res = out[0]
    flat = []
    for r in (res if isinstance(res, (tuple, list)) else [res]):          # logits; DyViT training: + features, decisions, stage predictions
        flat += list(r) if isinstance(r, (tuple, list)) else [r]
    flat = [t for t in flat if torch.is_tensor(t)]                        # (viz_mode's dict is read from the buffers below)
    tokens = np.asarray(model._last_tokens, dtype=np.int32)
    return launches, _digest(flat + [tokens] + bufs)
