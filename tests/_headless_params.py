"""Golden cases of headless models (num_classes = 0: head = nn.Identity(), deit_viz.py:142,182): the twelve families' micro cases of
tests/_params.py (D = 128, 224 x 224, same weight / image seeds and schedules) at batch 2.  The reference's output is then
pre_logits(norm(x)[:, 0]), the final-normed CLS row [B, D]; the fixtures (tests/golden/<name>.npz, written by
tests/golden/gen_golden_headless.py) hold it under "logits" like every other fixture."""
from tests._params import GOLDEN_CASES

_MICRO = {"deit": "deit_micro", "topk": "topk_micro", "evit": "evit_micro", "tome": "tome_micro", "dyvit": "dyvit_micro", "sit": "sit_micro",
          "dpcknn": "dpcknn_micro", "ats": "ats_micro", "sinkhorn": "sinkhorn_micro", "kmedoids": "kmedoids_micro",
          "patchmerger": "patchmerger_micro", "heuristic": "heuristic_micro_l2"}

HEADLESS_CASES = {}
for _fam, _src in _MICRO.items():
    _c = dict(GOLDEN_CASES[_src])
    _c.update(num_classes=0, batch=2)
    HEADLESS_CASES[f"headless_{_fam}_micro"] = _c


def drop_head(params: dict) -> dict:
    """tests/_params.make_params at num_classes = 0 still names head.weight [0, D] / head.bias [0]; a headless model has no such keys."""
    return {k: v for k, v in params.items() if not k.startswith("head.")}
