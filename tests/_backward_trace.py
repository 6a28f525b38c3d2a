"""The cases of the backward executor's launch trace (tests/golden/backward_trace.json): what each case builds and runs, shared by the
generator (tests/golden/gen_backward_trace.py) and the test (tests/test_backward_trace_gpu.py).

run_case(name) -> (launches, digest): the (label, flops, bytes) of every launch of ONE backward (csrc/tr_train.hip: one tr_vit_backward call,
or one per block range under a stub gradient reducer), and a sha256 over the flat gradient buffer, followed by the input gradient where the
case asks for one.  The forward runs unrecorded, with every random input seeded as tests/_executor_trace.py seeds it.  Before the recorded
backward the backward workspace is filled with 0xFF bytes -- NaN as fp32 and as bf16, so a lost memset shows in the bits -- and, for a
fresh (overwriting) backward, the flat gradient buffer with a fixed finite pattern, so the slices the executor does not write are defined."""
import hashlib

import numpy as np
import torch

from tests._executor_trace import TRAIN, _seeded_inputs, device_header  # noqa: F401  (device_header: for the generator and the test)
from tests._launches import record
from tests._params import GOLDEN_CASES, make_images

FULL = TRAIN + ["dpcknn_micro_equal", "sit_tiny", "topk_micro_384", "kmedoids_micro_384", "ats_micro_384", "dyvit_micro_train_384"]
SMALL = ["topk_small_kr07", "dyvit_small_train"]          # DeiT-S width, batch 2: the four-layer weight-gradient group plans differently
RANGES = ["topk_micro", "evit_micro", "tome_micro", "ats_micro", "kmedoids_micro", "sit_micro", "sinkhorn_micro", "patchmerger_micro",
          "dpcknn_micro", "dyvit_micro_train", "topk_micro_droppath", "topk_micro_dropout"]
FROZEN_ON = ["topk_micro", "ats_micro", "kmedoids_micro", "sit_micro", "dyvit_micro_train"]
FROZEN = ["attn_only", "trunk_below_2", "head_only", "head_norm", "proj1_only"]
PLAN3 = [(3, 3), (2, 1), (0, 0)]          # the block ranges of the stub reducer (every micro case has four blocks)
PLAN1 = [(3, 3), (2, 2), (1, 1), (0, 0)]


def _cases():
    c = {}
    for n in FULL:
        c[f"full/{n}"] = dict(base=n)
    for n in SMALL:
        c[f"full/{n}"] = dict(base=n, batch=2)
    for n in RANGES:
        c[f"ranges/{n}"] = dict(base=n, plan=PLAN3)
    for n in ("topk_micro", "ats_micro"):
        c[f"ranges1/{n}"] = dict(base=n, plan=PLAN1)
    for n in ("topk_micro", "dpcknn_micro", "sit_micro", "dyvit_micro_train", "topk_micro_dropout"):
        c[f"dx/{n}"] = dict(base=n, dx=True)
    c["dx_ranges/topk_micro"] = dict(base="topk_micro", dx=True, plan=PLAN3)
    for n in ("topk_micro", "dyvit_micro_train", "sit_micro"):
        c[f"acc/{n}"] = dict(base=n, acc=True)
    for form in FROZEN:
        for n in FROZEN_ON:
            c[f"{form}/{n}"] = dict(base=n, frozen=form)
    c["attn_only_dx/topk_micro"] = dict(base="topk_micro", frozen="attn_only", dx=True)
    c["trunk_below_2_ranges/topk_micro"] = dict(base="topk_micro", frozen="trunk_below_2", plan=PLAN3)
    c["headless/topk_micro"] = dict(base="topk_micro", headless=True)
    for n in ("topk_micro", "tome_micro", "ats_micro"):          # (the last two: the weighted pool)
        c[f"avg/{n}"] = dict(base=n, pool=True)
    c["avg_headless/topk_micro"] = dict(base="topk_micro", pool=True, headless=True)
    c["avg_head_norm/topk_micro"] = dict(base="topk_micro", pool=True, frozen="head_norm")
    return c


CASES = _cases()
# the plain micro cases: their hashes must reproduce at the commit the fixture is recorded from, under the poisoned workspace
MUST_HASH = [f"full/{n}" for n in FULL if n.endswith("_micro")]
# cases recorded with a zero-filled workspace: at the recorded commit their backward reads workspace it never wrote (the generator's
# finiteness check under the 0xFF fill fails); at most two, none of MUST_HASH
ZERO_WS = []


def single_call(name):
    """The single-call case a block-range case must agree with bit for bit, or None."""
    kind, base = name.split("/", 1)
    return {"ranges": f"full/{base}", "ranges1": f"full/{base}", "dx_ranges": f"dx/{base}"}.get(kind)


class _BlockRanges:
    """What training._VitTrainFn.backward asks of a gradient reducer, without a process group: one tr_vit_backward call per range of
    `plan`, nothing reduced."""
    sync = True

    def __init__(self, plan):
        self._plan = plan

    def plan(self, block_slices, depth):
        return [(hi, lo, 0, 0) for hi, lo in self._plan]

    def reduce_slice(self, flat, start, stop):
        pass

    def finish(self, flat):
        pass


def _freeze(model, form):
    if form == "attn_only":          # the reference's list (train.py:372-392), as tests/test_frozen_gpu.py sets it
        from tokenreduction_amd import finetune
        finetune.freeze_attn_only(model)
        return
    keep = {"trunk_below_2": ("head.", "blocks.2.", "blocks.3."), "head_only": ("head.",), "head_norm": ("head.", "norm."),
            "proj1_only": ("head.", "blocks.1.attn.proj.")}[form]          # proj1_only: the stop block skips what only feeds below it
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith(keep)


def _outputs(out):
    """The differentiable outputs of a training forward: logits / features; DyViT: + the distillation features and every stage prediction."""
    flat = []
    for r in (out if isinstance(out, (tuple, list)) else [out]):
        flat += list(r) if isinstance(r, (tuple, list)) else [r]
    return [t for t in flat if torch.is_tensor(t) and t.requires_grad]


def run(name, poison=True):
    """(launches, digest, model) of the case; poison False: the workspace is zero-filled instead (ZERO_WS)."""
    from tests.test_hip_model import build_model
    spec = CASES[name]
    case = dict(GOLDEN_CASES[spec["base"]])
    B = case["batch"] = spec.get("batch", case["batch"])
    model, _, _ = build_model(case)
    model.viz_mode = False
    model.use_graph = False
    if spec.get("pool"):
        model.global_pool = "avg"
    if spec.get("headless"):
        model.reset_classifier(0)
    model.train()
    if spec.get("frozen"):
        _freeze(model, spec["frozen"])
    _seeded_inputs(model, case, dict(train=True), B)
    x = make_images(B, case.get("img_size", 224), case["xseed"]).cuda()
    if spec.get("dx"):
        x.requires_grad_(True)
    if spec.get("plan"):
        model._grad_reducer = _BlockRanges(spec["plan"])
    gen = torch.Generator().manual_seed(case["xseed"] + 4321)

    def forward():
        np.random.seed(case["xseed"])          # K-Medoids equal_weight draws its first medoids from numpy's global generator
        outs = _outputs(model(x))
        return outs, [torch.randn(o.shape, generator=gen).cuda() for o in outs]          # fixed, non-zero: DyViT's dpred and dfeat are there

    try:
        if spec.get("acc"):                    # the first micro-step leaves every parameter a gradient: the recorded backward accumulates
            torch.autograd.backward(*forward())
        outs, grads = forward()
        torch.cuda.synchronize()
        st = model._train_state()
        st.bws.fill_(0xFF if poison else 0)
        if not spec.get("acc"):
            assert all(p.grad is None for p in model.parameters())
            st.flat.copy_((torch.arange(st.flat.numel(), device=st.flat.device) % 251).float() * 0.25 - 31.0)
        torch.cuda.synchronize()
        launches = record(lambda: torch.autograd.backward(outs, grads))
        torch.cuda.synchronize()
    finally:
        model._grad_reducer = None
    h = hashlib.sha256()
    for t in [st.flat] + ([x.grad] if spec.get("dx") else []):
        h.update(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    return launches, h.hexdigest(), model


def run_case(name):
    launches, digest, _ = run(name, poison=name not in ZERO_WS)
    return launches, digest


def nonfinite_trainable(model):
    """The trainable parameters whose slice of the flat gradient buffer is not finite (the generator's check under the 0xFF fill: none)."""
    st = model._train_state()
    return [n for n, p in st.order if p.requires_grad and not bool(torch.isfinite(st.views[n]).all())]
