"""What the operand declaration (models.Op rows; DESIGN.md, "The operand declaration") puts into the executor's structs, as digests -- to
compare two commits (profiles/operand_table_lab.md).

    python tools/operand_trace.py [--dump]
        No GPU.  One sha256 per configuration over: (a) the stage operands a recording stand-in for models._Packer receives from
        _pack_stages -- per struct field the packer method, shape, dtype and sha of the values, and the struct's scalar members;
        (b) TrainState.grads_struct under four requires_grad patterns -- per trunk / block / stage field the parameter and byte offset in
        the flat buffer it points at (or the LayerScale scratch, or NULL), the discarded names (sorted: the backward only zeroes them) and
        the LayerScale unfold items with addresses made relative; (c) the transposed stage operands: field, shape, sha; (d)
        _grad_slot_numel of every parameter, TrainState.offsets and block_slices.  --dump prints the records themselves.
    python tools/operand_trace.py --gpu
        On the device, fixed seeds: per micro case of tests/_params.GRAD_CASES one eval forward and one training forward + backward +
        FusedAdamW step (the DPC-KNN noise and DyViT's Gumbel draws through the tests' hooks, dropout and DropPath off); the sha256
        (first 16 hex digits) of the eval logits, the train logits, TrainState.flat and all parameters after the step.
    python tools/operand_trace.py --host-time
        No GPU.  Host time of TrainState.grads_struct (built per backward call) for two DeiT-S models: 5 repeats of 50 calls.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import tokenreduction_amd as tra
from tokenreduction_amd import _lib, finetune
from tokenreduction_amd.training import TrainState


def _ptr_fields(struct):
    return [n for n, t in struct._fields_ if t is C.c_void_p]


TRUNK, BLOCK, STAGE = (_ptr_fields(s) for s in (_lib.TrVitWeights, _lib.TrBlockWeights, _lib.TrStageWeights))
SCALARS = [n for n, t in _lib.TrStageWeights._fields_ if t is not C.c_void_p]


def sha(t):
    t = t.detach().contiguous()
    return hashlib.sha256(t.view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b"").hexdigest()[:16]


def configs():
    """(label, factory, constructor kwargs, args overrides)"""
    out = [(n, n, {}, {}) for n in tra.list_models() if "_tiny_patch16_224" in n]
    out += [(f"{f}_tiny+equal_weight", f"{f}_tiny_patch16_224", {}, dict(equal_weight=True)) for f in ("dpcknn", "kmedoids")]
    out += [(f"{f}+init_values", f, dict(init_values=1e-5), {}) for f in ("sit_tiny_patch16_224", "deit_tiny_patch16_224_local_viz")]
    out += [(f"topk_tiny+{k}={v!r}", "topk_tiny_patch16_224", {k: v}, {})
            for k, v in (("no_embed_class", True), ("num_classes", 0), ("global_pool", "avg"), ("num_classes", 10))]
    return out


def make(factory, kw, over):
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False, dyvit_distill=False, k_neighbors=5, equal_weight=False,
                                 cluster_iters=3, sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None)
    args.__dict__.update(over)
    torch.manual_seed(0)
    kw = dict(dict(num_classes=100), **kw)
    return tra.create_model(factory, pretrained=False, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None, img_size=224, args=args, **kw)


class RecordingPacker:
    """Stands in for models._Packer: hands out one fake address per call and remembers what the call was given."""
    want_t = True
    dev = torch.device("cpu")

    def __init__(self):
        self.calls = {}

    def _rec(self, method, t):
        addr = 4096 * (len(self.calls) + 1)
        self.calls[addr] = (method, list(t.shape), str(t.dtype), sha(t.float()))
        return addr

    def w16(self, t, transposed=False):
        a = self._rec("w16", t)
        return (a, None) if transposed else a

    def f32(self, t):
        return self._rec("f32", t)


def stage_operands(model):
    """(a) and (c): {"blk.field": call record} + scalar members, and the transposed copies {"blk.field": (shape, sha)}."""
    W, pk = _lib.TrVitWeights(), RecordingPacker()
    model._pack_stages(W, pk)
    ops = {}
    for loc in range(model.depth):
        st = W.stage[loc]
        for f in STAGE:
            if getattr(st, f):
                ops[f"{loc}.{f}"] = pk.calls[getattr(st, f)]
        sc = {f: getattr(st, f) for f in SCALARS if getattr(st, f)}
        if sc:
            ops[f"{loc}.scalars"] = sc
    tr = {f"{loc}.{f}": t for (loc, f), t in model._stage_t.items()}
    return ops, {k: (list(t.shape), sha(t)) for k, t in sorted(tr.items())}


def _attn_only(model):
    if hasattr(model.head, "weight"):
        finetune.freeze_attn_only(model)
    else:       # headless: freeze_attn_only's rule without the classifier
        for n, p in model.named_parameters():
            p.requires_grad = ".attn." in n or n == "pos_embed"


def _only(prefix):
    def f(model):
        for n, p in model.named_parameters():
            p.requires_grad = n.startswith(prefix)
    return f


PATTERNS = [("all", _only(""), False), ("attn_only", _attn_only, False), ("head", _only("head."), False), ("frozen+dx", _only("\0"), True)]


def gradients(model, st):
    """(b): what every gradient pointer points at, per requires_grad pattern."""
    flat0, nflat = st.flat.data_ptr(), 4 * st.flat.numel()
    starts = sorted((o, n) for n, o in st.offsets.items())
    params = {p.data_ptr(): n for n, p in model.named_parameters()}
    ls0 = st.ls["scratch"].data_ptr() if st.ls else None

    def where(a):
        if not a:
            return None
        if flat0 <= a < flat0 + nflat:
            off = (a - flat0) // 4
            o, n = [s for s in starts if s[0] <= off][-1]
            return [n, 4 * (off - o)]
        if a in params:
            return ["param", params[a]]
        return ["ls", a - ls0]

    out = {}
    for label, mask, want_dx in PATTERNS:
        mask(model)
        G, discarded = st.grads_struct(model, want_dx)
        rec = {f: where(getattr(G, f)) for f in TRUNK}
        for i in range(model.depth):
            rec.update({f"blocks.{i}.{f}": where(getattr(G.blocks[i], f)) for f in BLOCK})
            rec.update({f"stage.{i}.{f}": where(getattr(G.stage[i], f)) for f in STAGE})
        rec = {k: v for k, v in rec.items() if v is not None}
        items = [[blk] + [where(a) for a in it[:8]] + list(it[8:]) for blk, it in st.ls["items"]] if st.ls else None
        out[label] = dict(fields=rec, discarded=sorted(discarded), ls_items=items)
    _only("")(model)
    return out


def trace(label, factory, kw, over):
    model = make(factory, kw, over)
    ops, tr = stage_operands(model)
    st = TrainState(model)
    rec = dict(stage_operands=ops, transposed=tr, grads=gradients(model, st),
               slots={n: int(model._grad_slot_numel(n, p)) for n, p in model.named_parameters()},
               offsets=st.offsets, view_off=st.view_off, block_slices=[list(s) for s in st.block_slices])
    text = json.dumps(rec, sort_keys=True, default=float)
    return hashlib.sha256(text.encode()).hexdigest(), rec


def gpu_cases():
    from tests._params import GOLDEN_CASES, GRAD_CASES
    return [n for n in GRAD_CASES if GOLDEN_CASES[n]["embed_dim"] <= 192]


def gpu_trace(name):
    from tests._params import GOLDEN_CASES, grad_labels, make_images
    from tests.test_hip_model import build_model
    from tokenreduction_amd.optim import FusedAdamW
    case = dict(GOLDEN_CASES[name], drop_rate=0.0, drop_path=0.0)
    model, _, _ = build_model(case)
    model.viz_mode = False
    B, g = case["batch"], torch.Generator().manual_seed(case["xseed"] + 1234)
    if case["family"] == "dpcknn":
        model.density_noise = {blk: torch.rand(B, P, generator=g) for blk, _, P in model._stage_shapes()}
    if case["family"] == "dyvit":
        P = model.patch_embed.num_patches
        model.gumbel_noise = {j: -torch.empty(B, P, 2).exponential_(generator=g).log() for j in range(len(model.pruning_loc))}
    x = make_images(B, case.get("img_size", 224), case["xseed"]).cuda()
    np.random.seed(case["xseed"])          # K-Medoids equal_weight draws its first medoids from numpy's global generator
    ev = model(x)
    model.train()
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.05, model=model)
    out = model(x)
    logits = out[0] if isinstance(out, tuple) else out
    torch.nn.functional.cross_entropy(logits, grad_labels(case).cuda()).backward()
    flat = sha(model._train_state().flat)
    opt.step()
    torch.cuda.synchronize()
    return dict(eval=sha(ev), train=sha(logits), flat=flat, params=sha(torch.cat([p.detach().reshape(-1) for p in model.parameters()])))


def host_time():
    import time
    for factory in ("sit_small_patch16_224", "dyvit_small_patch16_224"):
        model = make(factory, {}, {})
        st = TrainState(model)
        st.grads_struct(model)
        reps = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(50):
                st.grads_struct(model)
            reps.append((time.perf_counter() - t0) / 50 * 1e3)
        print(f"{factory}: grads_struct ms per call, 5 repeats of 50: {' '.join(f'{r:.3f}' for r in reps)}  median {sorted(reps)[2]:.3f} max {max(reps):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--dump", action="store_true")
    ap.add_argument("--host-time", action="store_true")
    a = ap.parse_args()
    if a.host_time:
        return host_time()
    if a.gpu:
        assert torch.cuda.is_available(), "needs a GPU"
        for name in gpu_cases():
            print(name, json.dumps(gpu_trace(name)), flush=True)
        return
    for cfg in configs():
        digest, rec = trace(*cfg)
        print(f"{cfg[0]:48s} {digest}", flush=True)
        if a.dump:
            print(json.dumps(rec, sort_keys=True, default=float, indent=1))


if __name__ == "__main__":
    main()
