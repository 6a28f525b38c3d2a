"""Float64 CPU references, input builders and the case tables of the edge-shape tests of the LayerNorm backward and the parameter-gradient
kernels (csrc/tr_backward.hip: ln_bwd_kernel, wgrad_kernel, colsum_kernel and the partial reduces; csrc/tr_wgrad_pc.hip: wgrad_pc_kernel).

Every reference is the CLOSED FORM the kernel's header comment states, evaluated in float64 on the operands exactly as the kernel reads
them (fp32, or bf16-rounded where the C ABI takes bf16; eps as the float the C ABI receives) -- no autograd here.
tests/test_param_grad_ref.py proves each closed form against torch.autograd in float64 at every shape of the tables (CPU suite);
tests/test_hip_param_grad_edges.py compares the kernels with them (GPU suite), in the forms the backward executor (csrc/tr_train.hip)
calls them: shared and short workspaces, strided operands, in-place and accumulating LayerNorm backward, both row scatters.

LayerNorm inputs (ln_case): every row of x has its own scale 10^U(-1, 1) and its own shift, so a row normalised with another row's
statistics shows; when M > 3, row 3 is the constant 0.5 -- every fp32 partial sum of it is exact, xhat = 0, rstd = eps^-1/2, and its
gradient is about 10^3 x the others (what `rstd` without eps, or a per-tensor bound, would hide).
Parameter-gradient inputs (operand): small integers in [-2, 2] keep every sum exact in fp32 (|sum| <= 4 M < 2^24 at every shape below),
so the result does not depend on the number of token ranges and is compared with torch.equal.  The operands are SLICES of larger
buffers filled with 7: rows before and after the operand, the columns left and right of it where it is strided, and with yskip the
skipped CLS rows -- anything read from outside the operand changes an integer.  Gaussian operands of the same layout serve the
tolerance checks.

`python -m tests._param_grad_ref` prints, per LayerNorm case, what a plain float32 evaluation of the same formulas costs against float64:
the worst row of g relative to that row's largest magnitude, d_gamma and d_beta relative to their largest magnitudes, next to the bound
the GPU test applies (LN_BOUNDS).  tests/test_param_grad_ref.py pins that cost below half of each bound.
"""
import functools

import torch

F64 = torch.float64
FILL = 7.0                                      # what surrounds every parameter-gradient operand

# ---------------------------------------------------------------------------------------------------------------- bounds
# the ones tests/test_hip_backward.py applies; g is held PER ROW (relative to that row's largest reference magnitude), not per tensor
LN_BOUNDS = {"g": 1e-4, "dgamma": 2e-4, "dbeta": 2e-4}
LN_DBETA_ABS = 1e-5
DW_BOUND, DW_ABS = 2e-4, 1e-6                   # Gaussian dW: 2e-4 max|ref| + 1e-6
DB_BOUND, DB_ABS = 1e-4, 1e-5                   # Gaussian db and column sums: 1e-4 max|ref| + 1e-5

# ---------------------------------------------------------------------------------------------------------------- LayerNorm case tables
# ln_bwd_kernel<NCH, ADD, PARAMS>: one wave per row, grid min(512, ceil(M / 4)), NCH = ceil(D / 256).
# D: 4 = one lane; 64, 192, 256 = NCH 1 (16, 48, 64 lanes); 260 = NCH 2 with ONE lane in the second chunk; 384, 512 = NCH 2; 516 = NCH 3
# with one lane in the third; 768 = NCH 3; 1020, 1024 = NCH 4 (the last lane without / with a chunk)
LN_D = (4, 64, 192, 256, 260, 384, 512, 516, 768, 1020, 1024)
# M: 1, 2, 3 = waves without a row store zero partials; 5 = two workgroups; 252 / 253 = grid 63 / 64, the switch between the 64 x 4 and the
# tall reduce; 257 = 65 partials, the tall reduce's unrolled loop plus tail; 2048 / 2049 = one row per wave / the first second pass;
# 4100 = uneven passes
LN_M = (1, 2, 3, 5, 252, 253, 257, 2048, 2049, 4100)
LN_EPS = (1e-6, 1e-5)                           # the ViT norms / the predictors' nn.LayerNorm default
# every D at M in {5, 253}, every M at D in {192, 1020}
LN_SHAPES = sorted({(M, D) for M in (5, 253) for D in LN_D} | {(M, D) for M in LN_M for D in (192, 1020)})
# the executor's forms (in place, no bf16 copy, accumulate, frozen, strided): two workgroups with a one-lane second chunk; the reduce
# switch; a second grid pass
LN_FORM_SHAPES = [(5, 260), (253, 192), (2049, 384)]
# the final norm on CLS rows: (B, D), written at stride Nl * D
LN_FINAL_CASES = [(1, 260), (3, 192), (130, 384)]
LN_FINAL_NL = 5
# scatter (B, K, n_out, D): everything kept; the shape tests/test_hip_backward.py holds; M = 37 x 69 = 2553 > 2048 rows: the image / row
# decode in a second grid pass
LN_SCATTER_CASES = [(1, 1, 2, 64), (3, 20, 50, 384), (37, 68, 197, 192)]

# ---------------------------------------------------------------------------------------------------------------- parameter-gradient tables
# One row: (M, N, K, ly, lx, yskip, fits).  ly / lx: None = contiguous rows, (left, ld) = a column slice starting at column `left` of a
# buffer `ld` wide.  yskip: None or (B, P): dY is [B, P + 1, N] and M = B P.  fits: the workspaces the case runs at -- None = what the
# library recommends, "x4" = four times that (the executor's shared buffer), an int = room for that many partials (forces S <= fit).
# General kernel (wgrad_kernel: 128 x 128 tiles, 64-row slabs):
WGRAD_CASES = [
    (1, 8, 8, None, None, None, (None,)),                        # one row; column clamp N - 8 = 0
    (63, 8, 16, None, None, None, (None, 1)),                    # one row short of a slab
    (64, 16, 8, None, None, None, (None, 1)),                    # exactly one slab
    (65, 8, 8, None, None, None, (None, 1)),                     # a second range of one row
    (63, 192, 192, None, None, None, (None,)),                   # 192-multiples but M < 64: stays on this kernel
    (129, 72, 264, (8, 128), (0, 272), None, (None, 2)),         # the predictor's strided form; K over three tiles with an 8-wide tail
    (453, 136, 120, None, None, None, (1, 3, None, "x4")),       # second N tile 8 columns wide (bias tail); 8 slabs, 5 rows in the last;
                                                                 # fit = 3: ranges of 3, 3, 2 slabs
    (3969, 64, 56, None, None, None, (None,)),                   # S = 63: the 64 x 4 reduce for dW (3584 elements) and db
    (4033, 64, 56, None, None, None, (None,)),                   # S = 64: the tall reduce, no tail
    (4097, 64, 56, None, None, None, (None,)),                   # S = 65: the tall reduce with its tail
    (15, 128, 24, None, None, (3, 5), (None, 2)),                # yskip, fewer rows than a slab
    (280, 136, 72, None, None, (4, 70), (None, 2)),              # yskip not aligned to the slab
]
# 192-tile kernel (wgrad_pc_kernel: M >= 64, N and K multiples of 192):
WGRAD_PC_CASES = [
    (64, 192, 192, None, None, None, (None,)),                   # one unit, one slab
    (65, 192, 384, None, None, None, (None, 1)),                 # second slab holds one row
    (1000, 192, 192, None, None, None, (1, 2, 5, None, "x4")),   # planner picks 16 ranges: the bias partials sit behind S_max partials
    (1000, 576, 192, (0, 640), (192, 384), None, (1, None)),     # the same with the strides tests/test_hip_backward.py uses
    (180, 192, 768, None, None, (5, 36), (1,)),                  # yskip: loader row stepping under a forced re-plan
]
# Groups (tr_linear_bwd_group), layers (M, N, K).  The split counts are what plan_group yields today: reasons, not assertions.
GROUP_CASES = [
    [(64, 192, 192), (64, 192, 192)],                            # smallest direct store: every layer one range
    [(65, 192, 192), (64, 384, 192)],                            # S = (2, 1): one layer split, so no direct store
    [(130, 192, 192), (64, 192, 384), (191, 384, 192), (64, 192, 192)],       # four layers, ragged last slabs, every reduce segment
    [(1000, 192, 192), (70, 576, 192)],                          # S = 16: the reduce's unrolled loop without a tail
    [(1090, 192, 192), (64, 192, 192)],                          # S >= 17: the unrolled loop plus tail
]
GROUP_DIRECT = {0}                                               # indices of GROUP_CASES stored in place when overwriting
GROUP_FALLBACK = 2                                               # the group that also runs with a workspace of its largest single layer
# Column sums (M, N, ldy, yskip):
COLSUM_CASES = [
    (1, 2, None, None), (31, 6, None, None),                     # N below one float4: the reduce's ragged branch
    (33, 514, None, None),                                       # second column block with a single thread pair; two ranges
    (35, 8, None, None),                                         # the 4-row loop's remainder of 3
    (8193, 8, None, None),                                       # the 256-range cap, 33 rows per range
    (100, 1000, None, (10, 10)),                                 # yskip
    (100, 1000, (0, 1008), (10, 10)),                            # yskip and a row stride
]
GELU_SIZES = (8, 8 * 257)                                        # one chunk; one chunk past a full workgroup


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def eps32(eps):
    """eps as the kernel receives it: the C ABI takes a float"""
    return float(torch.tensor(eps, dtype=torch.float32).double())


# ---------------------------------------------------------------------------------------------------------------- LayerNorm backward
@functools.lru_cache(maxsize=None)
def ln_case(M, D, seed=0):
    """dy bf16 [M, D], x fp32 [M, D] (per-row scale and shift; row 3 constant), gamma = 1 + 0.3 N(0, 1), g_in ~ N(0, 1).  Shared: read-only."""
    g = _gen(5000 + 7 * M + D + seed)
    scale = 10.0 ** (torch.rand(M, 1, generator=g) * 2.0 - 1.0)
    shift = torch.randn(M, 1, generator=g)
    x = torch.randn(M, D, generator=g) * scale + shift
    if M > 3:
        x[3] = 0.5
    return dict(dy=torch.randn(M, D, generator=g).bfloat16(), x=x, gamma=1.0 + 0.3 * torch.randn(D, generator=g),
                g_in=torch.randn(M, D, generator=g))


def ln_rows(dy, x, gamma, eps, g_in, dtype=F64):
    """The closed form above ln_bwd_kernel, row by row, in `dtype`: (g_in + dx [M, D], d_gamma [D], d_beta [D]).
    xhat = (x - mean) rstd; dyg = dy gamma; dx = rstd (dyg - mean(dyg) - xhat mean(dyg xhat)); d_gamma = sum dy xhat; d_beta = sum dy."""
    dy, x, gamma = dy.to(dtype), x.to(dtype), gamma.to(dtype)
    e = torch.tensor(eps, dtype=torch.float32).to(dtype)
    xc = x - x.mean(-1, keepdim=True)
    rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + e)
    xhat = xc * rstd
    dyg = dy * gamma
    dx = rstd * (dyg - dyg.mean(-1, keepdim=True) - xhat * (dyg * xhat).mean(-1, keepdim=True))
    rows = dx if g_in is None else g_in.to(dtype) + dx
    return rows, (dy * xhat).sum(0), dy.sum(0)


def scatter_rows(idx, n_out, fused=False):
    """Destination row in [B * n_out] of every input row [B, n_in]: row 0 -> 0, row r -> 1 + idx[b, r - 1]; the fused row -> -1."""
    B, K = idx.shape
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < n_out - 1, "idx outside [0, n_out - 1)"
    dst = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + idx.long()], dim=1) + torch.arange(B)[:, None] * n_out
    if fused:
        dst = torch.cat([dst, torch.full((B, 1), -1)], dim=1)
    return dst.reshape(-1)


def ln_bwd_ref(dy, x, gamma, eps, g_in, idx=None, n_out=None, fused=False, add=False):
    """float64: (g, d_gamma, d_beta) -- plain: g [M, D]; with idx int32 [B, K]: g [B * n_out, D], the rows scattered (dropped rows zero) and,
    when fused, a fourth result g_fused [B, D].  add: repeated ids are summed (otherwise they must be distinct per image)."""
    rows, dgamma, dbeta = ln_rows(dy, x, gamma, eps, g_in)
    if idx is None:
        return rows, dgamma, dbeta
    B, K = idx.shape
    D = rows.shape[1]
    dst = scatter_rows(idx, n_out, fused)
    keep = dst >= 0
    if not add:
        assert dst[keep].unique().numel() == int(keep.sum()), "repeated ids need add=True"
    g = torch.zeros(B * n_out, D, dtype=F64).index_add_(0, dst[keep], rows[keep])
    if fused:
        return g, dgamma, dbeta, rows[~keep]
    return g, dgamma, dbeta


@functools.lru_cache(maxsize=None)
def scatter_idx(B, K, n_out, kind="distinct", seed=0):
    """int32 [B, K] ids in [0, n_out - 1).  distinct: a random subset per image, image 0 holding 0 and n_out - 2.  pairs: ids 2j and 2j + 1
    equal.  empty: as distinct, but the LAST image's ids are all 0 (K-Medoids' empty clusters all name token 0)."""
    g = _gen(6000 + B + K + seed)
    P = n_out - 1
    assert 1 <= K <= P
    idx = torch.stack([torch.randperm(P, generator=g)[:K] for _ in range(B)])
    row = [i for i in idx[0].tolist() if i not in (0, P - 1)]
    first = ([0, P - 1] if P > 1 else [0])[:K]
    idx[0] = torch.tensor((first + row)[:K])[torch.randperm(K, generator=g)]
    if kind == "pairs":
        idx[:, 1::2] = idx[:, 0:K - K % 2:2]
    elif kind == "empty":
        idx[-1] = 0
    else:
        assert kind == "distinct"
    idx = idx.to(torch.int32)
    assert int(idx.min()) >= 0 and int(idx.max()) < P
    return idx


# ---------------------------------------------------------------------------------------------------------------- parameter gradients
def operand(rows, cols, layout=None, kind="int", seed=0, skip=None):
    """One bf16 operand [rows, cols] inside a FILL-filled buffer: 4 rows before, 3 after, and with layout = (left, ld) the columns
    [left, left + cols) of `ld`.  skip = (B, P): rows = B (P + 1), every (P + 1)-th row from the first keeps FILL (the CLS rows yskip steps
    over).  -> (buf [rows + 7, ld], view [rows, cols] of it)."""
    left, ld = layout if layout is not None else (0, cols)
    assert left + cols <= ld and left % 8 == 0 and ld % 2 == 0
    g = _gen(7000 + seed)
    val = torch.randint(-2, 3, (rows, cols), generator=g).float() if kind == "int" else torch.randn(rows, cols, generator=g)
    if skip is not None:
        B, P = skip
        assert rows == B * (P + 1)
        val.view(B, P + 1, cols)[:, 0] = FILL
    buf = torch.full((rows + 7, ld), FILL, dtype=torch.bfloat16)
    view = buf[4:4 + rows, left:left + cols]
    view.copy_(val)
    return buf, view


def drop_skipped(dy, yskip):
    """The rows a yskip launch reads: [B (P + 1), N] -> [B P, N]"""
    if not yskip:
        return dy
    N = dy.shape[-1]
    return dy.reshape(-1, yskip + 1, N)[:, 1:].reshape(-1, N)


def wgrad_ref(dy, x, yskip=0):
    """float64 (dW [N, K], db [N]) from the bf16 operands"""
    y = drop_skipped(dy, yskip).to(F64)
    assert y.shape[0] == x.shape[0]
    return y.t() @ x.to(F64), y.sum(0)


def colsum_ref(dy, yskip=0):
    return drop_skipped(dy, yskip).to(F64).sum(0)


@functools.lru_cache(maxsize=None)
def wgrad_case(M, N, K, ly=None, lx=None, skip=None, kind="int", seed=0):
    """-> dict(ybuf, dy, xbuf, x, yskip, dw, db): the operand views as the launch takes them and the float64 results.  Shared: read-only."""
    yrows = M if skip is None else skip[0] * (skip[1] + 1)
    assert skip is None or skip[0] * skip[1] == M
    ybuf, dy = operand(yrows, N, ly, kind, seed=3 * (M + N + K) + seed, skip=skip)
    xbuf, x = operand(M, K, lx, kind, seed=3 * (M + N + K) + 1 + seed)
    yskip = 0 if skip is None else skip[1]
    dw, db = wgrad_ref(dy, x, yskip)
    return dict(ybuf=ybuf, dy=dy, xbuf=xbuf, x=x, yskip=yskip, dw=dw, db=db)


@functools.lru_cache(maxsize=None)
def colsum_case(M, N, ly=None, skip=None, kind="int", seed=0):
    yrows = M if skip is None else skip[0] * (skip[1] + 1)
    assert skip is None or skip[0] * skip[1] == M
    ybuf, dy = operand(yrows, N, ly, kind, seed=5 * (M + N) + seed, skip=skip)
    yskip = 0 if skip is None else skip[1]
    return dict(ybuf=ybuf, dy=dy, yskip=yskip, db=colsum_ref(dy, yskip))


# ---------------------------------------------------------------------------------------------------------------- float32 cost
def row_rel(got, want):
    """worst row of |got - want| relative to that row's largest |want| (float64)"""
    want = want.to(F64)
    err = (got.to(F64) - want).abs().amax(-1)
    return float((err / want.abs().amax(-1).clamp_min(1e-300)).max())


def max_rel(got, want):
    want = want.to(F64)
    return float((got.to(F64) - want).abs().max() / want.abs().max().clamp_min(1e-300))


def ln_f32_cost(M, D, eps):
    """What plain float32 evaluation of the closed form costs against float64: {"g": per row, "dgamma", "dbeta"}"""
    c = ln_case(M, D)
    g, dg, db = ln_rows(c["dy"], c["x"], c["gamma"], eps, c["g_in"])
    g32, dg32, db32 = ln_rows(c["dy"], c["x"], c["gamma"], eps, c["g_in"], dtype=torch.float32)
    return {"g": row_rel(g32, g), "dgamma": max_rel(dg32, dg), "dbeta": max_rel(db32, db)}


def ln_all_shapes():
    """every (M, D) a LayerNorm test of tests/test_hip_param_grad_edges.py runs"""
    scat = {(B * (K + 1 + f), D) for B, K, _, D in LN_SCATTER_CASES for f in (0, 1)}
    return sorted(set(LN_SHAPES) | set(LN_FORM_SHAPES) | set(LN_FINAL_CASES) | scat)


if __name__ == "__main__":
    worst = {k: (0.0, None) for k in LN_BOUNDS}
    for M, D in ln_all_shapes():
        for eps in LN_EPS:
            cost = ln_f32_cost(M, D, eps)
            print(f"layernorm_bwd {M, D} eps={eps:g}: " + "; ".join(
                f"{k} fp32-vs-fp64 {v:.2e} (bound {LN_BOUNDS[k]:.1e}{'' if v <= 0.5 * LN_BOUNDS[k] else ' MORE THAN HALF'})" for k, v in cost.items()))
            for k, v in cost.items():
                if v > worst[k][0]:
                    worst[k] = (v, (M, D, eps))
    print("worst: " + "; ".join(f"{k} {v:.2e} at {at}" for k, (v, at) in worst.items()))
