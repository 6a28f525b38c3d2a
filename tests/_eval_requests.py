"""How every public eval entry of a model answers a request it cannot serve, as plain JSON: shared by tests/golden/gen_eval_requests.py
(which records it) and tests/test_eval_requests.py (which compares against the record).

The input is a CPU tensor, so every call ends in an exception and no GPU is needed: per (model state, call) the exception's type and its
full message -- which pins the text of every refusal and, where several apply, which one wins."""
from __future__ import annotations

import types

import torch

import tokenreduction_amd as tra

MODEL = "topk_small_patch16_224"

# (label, call on (model, x)): every public entry that takes an eval request
CALLS = [
    ("forward_taps", lambda m, x: m.forward_taps(x, cls_blocks=(3, 6, 9, 11))),
    ("forward_taps(block 99)", lambda m, x: m.forward_taps(x, cls_blocks=(3, 99))),
    ("forward_decisions", lambda m, x: m.forward_decisions(x)),
    ("forward_decisions(taps)", lambda m, x: m.forward_decisions(x, cls_blocks=(3,), final_tokens=True)),
    ("forward_dense", lambda m, x: m.forward_dense(x)),
    ("forward_dense(blocks=(99,))", lambda m, x: m.forward_dense(x, blocks=(99,))),
    ("forward_dense(output_fmt='CHWN')", lambda m, x: m.forward_dense(x, output_fmt="CHWN")),
    ("forward_dense(dtype=float16)", lambda m, x: m.forward_dense(x, dtype=torch.float16)),
    ("forward_dense(blocks=(3, -9))", lambda m, x: m.forward_dense(x, blocks=(3, -9))),
    ("forward_dense(blocks=())", lambda m, x: m.forward_dense(x, blocks=())),
    ("forward_dense(blocks=(3, 11))", lambda m, x: m.forward_dense(x, blocks=(3, 11), norm=False)),
    ("get_intermediate_layers(n=99)", lambda m, x: m.get_intermediate_layers(x, n=99)),
    ("get_intermediate_layers(n=2)", lambda m, x: m.get_intermediate_layers(x, n=2)),
    ("forward_async", lambda m, x: m.forward_async(x).result()),
    ("forward_async(cls_blocks)", lambda m, x: m.forward_async(x, cls_blocks=(3, 6)).result()),
    ("forward_async(cls_blocks, block 99)", lambda m, x: m.forward_async(x, cls_blocks=(3, 99)).result()),
    ("forward_async(final_tokens)", lambda m, x: m.forward_async(x, final_tokens=True).result()),
    ("forward_async(decisions)", lambda m, x: m.forward_async(x, decisions=True).result()),
    ("forward_async(decisions, cls_blocks)", lambda m, x: m.forward_async(x, cls_blocks=(3,), decisions=True).result()),
    ("forward_async(dense={})", lambda m, x: m.forward_async(x, dense={}).result()),
    ("forward_async(dense={}, decisions)", lambda m, x: m.forward_async(x, dense={}, decisions=True).result()),
    ("forward_async(dense={}, cls_blocks)", lambda m, x: m.forward_async(x, dense={}, cls_blocks=(3,)).result()),
    ("forward_async(dense=blocks (99,))", lambda m, x: m.forward_async(x, dense=dict(blocks=(99,))).result()),
    ("forward_async(dense=output_fmt 'CHWN')", lambda m, x: m.forward_async(x, dense=dict(output_fmt="CHWN")).result()),
]

# (label, train mode, viz_mode, dynamic_width); the last one has every refusal apply at once
STATES = [("eval", False, False, False), ("train", True, False, False), ("viz_mode", False, True, False),
          ("dynamic_width", False, False, True), ("train+viz_mode+dynamic_width", True, True, True)]


def make_model():
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False)
    torch.manual_seed(0)
    return tra.create_model(MODEL, pretrained=False, num_classes=10, img_size=224, args=args)


def outcome(model, state, call):
    """[exception type, message] of `call` on a CPU image with the model in `state`; ["returned", type name] if it raises nothing."""
    _, train, viz, dyn = state
    model.train(train)
    model.viz_mode, model.dynamic_width = viz, dyn
    try:
        out = call(model, torch.zeros(1, 3, 224, 224))
    except Exception as e:             # noqa: BLE001 -- the record is the exception, whatever it is
        return [type(e).__name__, str(e)]
    finally:
        model.eval()
        model.viz_mode, model.dynamic_width = False, False
    return ["returned", type(out).__name__]


def matrix(model=None):
    """{state label: {call label: outcome}}"""
    model = model or make_model()
    return {state[0]: {label: outcome(model, state, call) for label, call in CALLS} for state in STATES}
