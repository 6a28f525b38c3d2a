"""The request of an eval forward -- what it returns beside the logits -- as one hashable record, and the wording and order of the refusals
of the model's eval entries (models.VisionTransformer._eval_request builds the record and raises the refusals)."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch


class DenseOutput(NamedTuple):
    """How a dense feature map is written: "NCHW" / "NHWC", torch.float32 / torch.bfloat16, the value of a patch no row stands for."""
    fmt: str
    dtype: torch.dtype
    fill: float


class Levels(NamedTuple):
    """The blocks whose streams a multi-level dense request puts on the grid (ascending), through the model's final norm or as they stand."""
    blocks: tuple
    norm: bool


class EvalRequest(NamedTuple):
    """What an eval forward returns beside the logits: hashable, so it is part of the captured graph's key.  Built by
    VisionTransformer._eval_request, which validates; the default is the plain forward."""
    cls_blocks: Optional[tuple] = None         # output taps: the blocks whose CLS row is tapped, ascending; None: no output taps
    final_tokens: bool = False                 # output taps: the final norm of every row after the last block
    decisions: bool = False                    # the stages' decisions in record form
    dense: Optional[DenseOutput] = None        # a dense feature map ...
    levels: Optional[Levels] = None            # ... of these blocks; None: of the last block's final-normed rows

    @property
    def taps(self):
        """(blocks, final_tokens) as the executor serves them, or None.  The single dense map is made of the final_tokens tap's rows."""
        if self.dense is not None and self.levels is None:
            return (), True
        return None if self.cls_blocks is None else (self.cls_blocks, self.final_tokens)

    @property
    def wants_decisions(self):
        """A dense map's rows -- the final_tokens tap's or the level taps' -- are placed by the stages' record-form decisions."""
        return self.decisions or self.dense is not None

    def graph_key(self):
        """The request's part of a graph key: (taps[, ("dense", fmt, dtype, fill[, blocks, norm])][, True: with decisions])."""
        dense = () if self.dense is None else (("dense",) + self.dense + (self.levels or ()),)
        return (self.taps,) + dense + ((True,) if self.wants_decisions else ())


# The refusals of an eval request: per feature {check: message}, in the order in which the checks win ("args": the request's own arguments
# are validated there).  Output taps look at their blocks before the input, and the synchronous forward_taps runs under dynamic_width.
REFUSE_CPU = "input is on {device}: tokenreduction_amd has no CPU path (HIP kernels only)"
_DYNAMIC_WIDTH = ("{what} cannot run under dynamic_width (the token counts of a stage are then data dependent and the executor synchronises "
                  "mid-forward): switch dynamic_width off or use viz_mode")
_TAPS_DYNAMIC_WIDTH = "{what} with output taps cannot run under dynamic_width (the executor synchronises mid-forward): use forward_taps"


def _refusals(name, executor, same, viz_has, then):
    return {"train": f"{name} are an eval feature: call model.eval() first (the training executor {executor})",
            "viz_mode": f"{name} and viz_mode are two ways to the same {same}: switch viz_mode off ({viz_has})", **then}


_ROWS = ("has no taps", "rows", "viz_data['Features'] already holds every row of every recorded block")
_INPUT_FIRST = {"dynamic_width": _DYNAMIC_WIDTH, "cpu": REFUSE_CPU, "args": None}
REFUSALS = {
    "taps": _refusals("output taps", *_ROWS, {"args": None, "cpu": REFUSE_CPU, "dynamic_width": _TAPS_DYNAMIC_WIDTH}),
    "decisions": _refusals("decision taps", "records no decisions", "records", "viz_data already holds Kept_Tokens / Assignment_Maps on the host",
                           _INPUT_FIRST),
    "dense": _refusals("dense feature maps", *_ROWS, _INPUT_FIRST)}

# forward_dense_train, the dense map of a TRAINING forward: the same kind of table, checked in this order by models.forward_dense_train
# ("args": _dense_arguments).  "dyvit" and "precision" raise NotImplementedError, the others RuntimeError.
DENSE_TRAIN_REFUSALS = {
    "eval": "{what} is the dense feature map of a training forward, with a gradient: call model.train() first (in eval mode forward_dense "
            "returns the same map, without a gradient)",
    "viz_mode": "{what} and viz_mode do not go together: viz_mode records an eval forward on the host; switch viz_mode off",
    "cpu": REFUSE_CPU,
    "dynamic_width": _DYNAMIC_WIDTH,
    "args": None,
    "precision": "{what}: the training path is bf16 (fp32 accumulate); set model.precision = 'bf16'",
    "dyvit": "{what} is not built for DyViT: its training forward keeps every token in the stream under a differentiable policy, so there "
             "is no reduced stream to put back on the grid, and it has a feature output of its own (dyvit_distillation)"}
