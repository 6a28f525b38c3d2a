"""The fixed summation order of the partial-sum reduces (csrc/tr_backward.hip reduce_block), restated in fp32 on the CPU, and the cases of
the LayerNorm parameter reduce that hold both block layouts to it bit for bit.  No GPU needed: tests/test_reduce_ref.py checks the model
itself; tests/test_hip_train_glue_ops.py holds the kernels to it."""
import functools

import torch

from tests import _param_grad_ref as R

FLAT, TALL = 4, 16                              # partial-lanes of the 64 x 4 and the 16 x 16 block layout


def kernel_order_sum(part, prefill, lanes=FLAT):
    """sum_s part[s] in the kernels' order: lane y of `lanes` adds partials y, y + lanes, ... (whole groups of four elements: 4 * lanes
    partials at a time as (v0 + v1) + (v2 + v3), then one by one; the ragged last group: one by one), the lanes are combined in lane order,
    the destination is added last."""
    S, count = part.shape
    lanes_full, lanes_tail = [], []
    for y in range(lanes):
        a = torch.zeros_like(part[0])
        s = y
        while s + 3 * lanes < S:
            a = a + ((part[s] + part[s + lanes]) + (part[s + 2 * lanes] + part[s + 3 * lanes]))
            s += 4 * lanes
        while s < S:
            a = a + part[s]
            s += lanes
        lanes_full.append(a)
        t = torch.zeros_like(part[0])
        for s in range(y, S, lanes):
            t = t + part[s]
        lanes_tail.append(t)
    full, tail = lanes_full[0], lanes_tail[0]
    for y in range(1, lanes):
        full, tail = full + lanes_full[y], tail + lanes_tail[y]
    a = torch.where(torch.arange(count) < count // 4 * 4, full, tail)
    return a if prefill is None else a + prefill


def layout_lanes(S, count):
    """The layout a pair reduce (a Linear's dW / db, a LayerNorm's d_gamma / d_beta) must take: tall iff S >= 64 and every count <= 4096"""
    return TALL if S >= 64 and count <= 4096 else FLAT


# ---- the LayerNorm parameter reduce: S = grid = min(512, ceil(M / 4)) partials of D elements.  S: 63 the last flat one, 64 / 65 / 80 / 128 /
# 512 tall with 1, 1 + 1, 1 + 16, 2 and 8 unrolled groups per lane; M = 2052: the grid capped at 512 (a workgroup walks more than 4 rows).
# D: one chunk; exactly one tall block; one chunk into the second tall block; DeiT-S.
LN_REDUCE_M = tuple(4 * S for S in (63, 64, 65, 80, 128, 512)) + (2052,)
LN_REDUCE_D = (4, 64, 68, 384)
LN_REDUCE_SHAPES = [(M, D) for M in LN_REDUCE_M for D in LN_REDUCE_D]


def ln_grid(M):
    return min(512, (M + 3) // 4)


@functools.lru_cache(maxsize=None)
def ln_partials_model(M, D, eps=1e-6):
    """(d_gamma partials, d_beta partials), each [grid, D] fp32, of R.ln_case(M, D) as ln_bwd_kernel lays them out: wave w of workgroup b
    walks rows 4 b + w, + 4 grid, ... and the four waves are added in wave order.  fp32 on the CPU: the same values as the device's up to
    rounding, not its bits -- what the CPU can say about the inputs of the GPU test.  Shared: read-only."""
    c = R.ln_case(M, D)
    x, dy = c["x"], c["dy"].float()
    xc = x - x.mean(-1, keepdim=True)
    xhat = xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + torch.tensor(eps))
    grid = ln_grid(M)
    out = []
    for rows in (dy * xhat, dy):
        waves = []
        for w in range(4):
            a = torch.zeros(grid, D)
            for r0 in range(0, M, 4 * grid):
                sel = rows[r0 + w:min(M, r0 + 4 * grid):4]
                a[:sel.shape[0]] = a[:sel.shape[0]] + sel
            waves.append(a)
        out.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    return tuple(out)
