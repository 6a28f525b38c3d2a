"""Float64 CPU references, input builders and the case tables of the edge-shape tests of the forward LayerNorm kernels
(csrc/tr_norm.hip: layernorm_kernel, layernorm_half_kernel, gather_layernorm_kernel; csrc/tr_rowops.h: ln_row_store).

The forward LayerNorm is the anchor of the suite's bit-identity chain: tr_lnlin, both fused-Mlp LN forms, tr_final_tokens_f32 and the
_to / two-residual / fp32-output forms are held only as bit-identical to ops.layernorm / ops.layernorm_f32.  tests/test_ln_fwd_ref.py proves
the reference here against torch.nn.functional.layer_norm in float64 and pins what plain float32 costs (CPU suite);
tests/test_hip_layernorm_fwd_edges.py compares the kernels with it (GPU suite).

Reference: ln_ref is the closed form y = (x - mean) / sqrt(var + eps) gamma + beta in float64, fed the operands exactly as the kernel reads
them: fp32 x, gamma and beta, eps as the float the C ABI receives, and where residuals are pending the fp32 sum (x + d1) + d2 evaluated in
fp32 in that order (one or two IEEE additions: the exact expectation of what the kernel stores), then widened.  ln_f32 is the same two-pass
algorithm in float32 with torch's own summation order.

Inputs (ln_case): row r of a case belongs to family FAMILIES[(r + offset) % 7]; the tiny-M cases run once per offset, so every family sits
in every row position of a workgroup:
  gauss    N(0.5, 3^2), what tests/test_hip_ops.py uses           offset   N(100, 1): the mean is large against the spread
  onehot   a single 5.0 in a row of zeros                         outlier  N(0, 1) with one channel at 300 and one at -120 (trained ViT streams)
  tiny     N(0, 1e-4^2): eps dominates the variance               huge     N(0, 1e4^2)
  const    0, 1, -4, 0.5 or 1024 in every channel: 0 and +- powers of two, so every fp32 partial sum and the mean are exact at every D of the
           table in any summation order, x - mean is 0 and the result is EXACTLY beta
Excluded on purpose: constants that are no power of two, and rows whose |mean| / std is in the thousands -- plain fp32 two-pass evaluation of
those is off by 1e-2 .. 5e-1 of the row's largest output, and a bound that lets the reference's own fp32 form pass would hold nothing.
(With a pending residual added, a constant row is mean c, std 0.3: the residual forms run at M <= 9, where the constants are 0, 1 and -4.)

Bounds.  `python -m tests._ln_fwd_ref` prints, over every table case, family, stream form and eps in {1e-6, 1e-5}, the worst row of ln_f32
against ln_ref relative to that row's largest |reference|: LN_F32_WORST = 1.4e-5 (printed: 1.34e-05, family offset, row 5 of
M = 9, D = 8, eps 1e-6; every other family stays below 6e-7).  LN_FWD_BOUND = 4 x that, applied per row to every fp32 output: the margin covers another addition order, rsqrtf against 1 / sqrtf (one fp32 ulp each) and fma contraction.
bf16 outputs get no new number: bit-equal to the round-to-nearest-even of the fp32-output form, and within 1.01 bf16 ulp + 1e-4 of the
float64 reference (the bound of tests/test_hip_ops.py).  Stream writes and gathered rows are torch.equal.  EViT's fused row (the weighted
sum over the dropped tokens) is measured the same way: fuse_f32 accumulates token after token in fp32, fuse_ref in float64;
FUSE_F32_WORST = 9.9e-7 of the row's largest magnitude (printed: 9.85e-07, 288 dropped tokens, D = 260, no residual), FUSE_BOUND = 4 x that.
"""
import functools

import torch

import oracle

F64 = torch.float64

# ---------------------------------------------------------------------------------------------------------------- bounds
LN_F32_WORST = 1.4e-5                           # printed by `python -m tests._ln_fwd_ref`; tests/test_ln_fwd_ref.py holds ln_f32 below it
LN_FWD_BOUND = 4 * LN_F32_WORST
FUSE_F32_WORST = 9.9e-7
FUSE_BOUND = 4 * FUSE_F32_WORST
BF16_ULPS, BF16_ABS = 1.01, 1e-4                # tests/test_hip_ops.py::test_layernorm

# ---------------------------------------------------------------------------------------------------------------- case tables
# layernorm_kernel<F32, NCH, OUT32>: one wave per row, four rows per workgroup, NCH = ceil(D / 256), every load clamps its chunk index to
# D / 4 - 1.  D: 4, 8, 12 = rows narrower than one wave (1, 2, 3 lanes); 128, 192 = NCH 1; 252 / 256 / 260 = the last lane of NCH 1 without /
# with a chunk / NCH 2 with ONE lane in the second chunk; 508 / 512 / 516, 764 / 768 / 772 and 1020 / 1024 the same for NCH 2 / 3, 3 / 4 and
# the end of NCH 4; 384 = layernorm_half_kernel on the bf16 path (half a wave per row, eight rows per workgroup) and NCH 2 on the fp32 path
LN_D = (4, 8, 12, 128, 192, 252, 256, 260, 384, 508, 512, 516, 764, 768, 772, 1020, 1024)
LN_NCH_ENDS = {1: (4, 256), 2: (260, 512), 3: (516, 768), 4: (772, 1024)}        # the narrowest and the widest row of every NCH
LN_HALF_D = 384
LN_M_WAVE = (1, 3, 4, 5, 9)                     # one row; one short of / equal to / one past a workgroup's four rows; a third workgroup of one
LN_M_HALF = (1, 7, 8, 9, 17)                    # the same around the half kernel's eight rows
LN_M_ALL = 35                                   # every family with every constant (7 x 5 rows), offset 0 only
LN_EPS = (1e-6, 1e-5)                           # cfg->ln_eps / the DyViT predictor norms of csrc/tr_vit.hip
FAMILIES = ("gauss", "offset", "onehot", "outlier", "tiny", "huge", "const")
CONSTS = (0.0, 1.0, -4.0, 0.5, 1024.0)
OFFSETS = tuple(range(len(FAMILIES)))


def ln_tiny_m(D):
    return LN_M_HALF if D == LN_HALF_D else LN_M_WAVE


# (M, D, offsets): the tiny-M cases at every offset, the all-families case at offset 0
LN_SHAPES = [(M, D, OFFSETS) for D in LN_D for M in ln_tiny_m(D)] + [(LN_M_ALL, D, (0,)) for D in LN_D]
# the executor's forms (pending residuals, no stream write, out of place, strided CLS rows, the fp32 residual): one ragged D per NCH, the
# half kernel and one lane; one row, two workgroups with a tail of one, three with a tail of one (two at D = 384)
LN_FORM_D = (4, 252, 260, 384, 764, 1020)
LN_FORM_M = (1, 5, 9)
LN_FORM_OFFSETS = (0, 4)                        # M = 5: gauss .. tiny, then tiny huge const gauss offset
LN_FORM_SHAPES = [(M, D) for D in LN_FORM_D for M in LN_FORM_M]
LN_CLS_N = (2, 69)                              # tokens per image of the strided CLS-row final norm (ldx = ldd = N D)
STREAMS = ("x", "d1", "d12", "df")              # the stream a form normalises: x, x + d1, (x + d1) + d2 (bf16 residuals), x + df (fp32)

# gather_layernorm_kernel<F32, NCH>: four gathered rows per workgroup, plus one workgroup per image for EViT's fused row, whose four waves
# take every fourth dropped token, 64 per trip of the i0 loop, four rows per step of the inner loop (cnt = a wave's tokens in the trip).
# (B, N, K): K + 1 gathered rows = 2, 4, 5, 8, 9 around the four-row blocks (one row is no gather: the library asks K >= 1); dropped tokens
# c = N - 1 - K:  1 .. 5 = waves with one token or none, wave 0 with two;  11, 14 = cnt 3 3 3 2 and 4 4 3 3 (the tail of the four-row step);
# 255 / 256 / 257 / 259 = 63 or 64 per wave / 64 each / wave 0 makes a second trip of one / three waves do;  288 = the 384^2 image at keep
# rate 0.5 (576 patches, second trip of eight);  513 = wave 0 makes a third trip
GATHER_CASES = [(2, 3, 1), (2, 6, 3), (1, 8, 4), (2, 12, 7), (2, 14, 8), (2, 14, 2), (1, 19, 4), (2, 257, 1), (1, 260, 3), (2, 262, 4),
                (1, 267, 7), (2, 577, 288), (1, 519, 5)]
GATHER_PLAIN_CASES = [c for c in GATHER_CASES if c[1] <= 19 or c[1] == 577]       # without the fused row the dropped tokens are never read
GATHER_D = (4, 260, 384, 1024)                  # one lane; NCH 2 with one lane in the second chunk; DeiT-S; the widest row
GATHER_ALL_ROWS = [(2, 9, 252), (2, 9, 260), (1, 6, 764), (2, 5, 1020)]           # idx = NULL: (B, N, D), one per NCH, families as rows
GATHER_KEPT_ALL = [(2, 6, 4), (1, 5, 384), (2, 9, 260)]                           # K = N - 1, an empty complement: (B, N, D)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def eps32(eps):
    """eps as the kernel receives it: the C ABI takes a float"""
    return float(torch.tensor(eps, dtype=torch.float32).double())


# ---------------------------------------------------------------------------------------------------------------- inputs
def family_of(r, offset):
    return FAMILIES[(r + offset) % len(FAMILIES)]


def family_rows(M, D, offset, g):
    """fp32 [M, D]: row r of family (r + offset) % 7 (see the module docstring)"""
    x = torch.empty(M, D)
    for r in range(M):
        z = torch.randn(D, generator=g)
        f = family_of(r, offset)
        if f == "gauss":
            x[r] = z * 3.0 + 0.5
        elif f == "offset":
            x[r] = z + 100.0
        elif f == "onehot":
            x[r] = 0.0
            x[r, (7 * r + 3) % D] = 5.0
        elif f == "outlier":
            x[r] = z
            x[r, D // 3], x[r, (2 * D) // 3] = 300.0, -120.0
        elif f == "tiny":
            x[r] = z * 1e-4
        elif f == "huge":
            x[r] = z * 1e4
        else:
            x[r] = CONSTS[((r + offset) // len(FAMILIES)) % len(CONSTS)]
    return x


@functools.lru_cache(maxsize=None)
def ln_params(D):
    """gamma = 1 + 0.1 N(0, 1), beta = 0.1 N(0, 1), fp32 [D]"""
    g = _gen(9000 + D)
    return 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


@functools.lru_cache(maxsize=None)
def ln_case(M, D, offset=0):
    """x fp32 [M, D] by families; d1, d2 independent bf16 N(0, 0.3^2); df fp32 N(0, 0.3^2); gamma, beta; fam: the family of every row.
    Shared: read-only."""
    g = _gen(8000 + 31 * M + D + 977 * offset)
    x = family_rows(M, D, offset, g)
    d1, d2 = (torch.randn(M, D, generator=g) * 0.3).bfloat16(), (torch.randn(M, D, generator=g) * 0.3).bfloat16()
    df = torch.randn(M, D, generator=g) * 0.3
    gamma, beta = ln_params(D)
    return dict(x=x, d1=d1, d2=d2, df=df, gamma=gamma, beta=beta, fam=[family_of(r, offset) for r in range(M)])


def stream_sum(x, d1=None, d2=None):
    """(x + d1) + d2 in fp32, in that order: what the kernel normalises and, where it writes the stream, stores -- exactly"""
    s = x
    if d1 is not None:
        s = s + d1.float()
    if d2 is not None:
        s = s + d2.float()
    return s


def stream_of(c, kind):
    return {"x": lambda: c["x"], "d1": lambda: stream_sum(c["x"], c["d1"]), "d12": lambda: stream_sum(c["x"], c["d1"], c["d2"]),
            "df": lambda: stream_sum(c["x"], c["df"])}[kind]()


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_ref(x, gamma, beta, eps):
    """float64 closed form over the last dim.  mean = sum / D (a division: exact for the constant rows)."""
    x, D = x.to(F64), x.shape[-1]
    xc = x - x.sum(-1, keepdim=True) / D
    var = (xc * xc).sum(-1, keepdim=True) / D
    return xc / torch.sqrt(var + eps32(eps)) * gamma.to(F64) + beta.to(F64)


def ln_f32(x, gamma, beta, eps):
    """the same two passes in float32, sums in torch's order"""
    assert x.dtype == torch.float32 and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    D = x.shape[-1]
    xc = x - x.sum(-1, keepdim=True) / D
    var = (xc * xc).sum(-1, keepdim=True) / D
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return xc * rstd * gamma + beta


def row_rel_all(got, want):
    """per row: |got - want| relative to that row's largest |want| (float64)"""
    want = want.to(F64)
    err = (got.to(F64) - want).abs().amax(-1)
    return err / want.abs().amax(-1).clamp_min(1e-300)


def ln_cases():
    """every (M, D, offset, stream kind) a LayerNorm test runs"""
    for M, D, offsets in LN_SHAPES:
        for o in offsets:
            yield M, D, o, "x"
    for M, D in LN_FORM_SHAPES:
        for o in LN_FORM_OFFSETS:
            for kind in STREAMS:
                yield M, D, o, kind
    for B, N, D in GATHER_ALL_ROWS:
        yield B * N, D, 0, "x"


def ln_f32_cost(M, D, offset, kind, eps):
    """per row: what ln_f32 costs against ln_ref on that case"""
    c = ln_case(M, D, offset)
    s = stream_of(c, kind)
    return row_rel_all(ln_f32(s, c["gamma"], c["beta"], eps), ln_ref(s, c["gamma"], c["beta"], eps))


# ---------------------------------------------------------------------------------------------------------------- gather (+ EViT's fused row)
@functools.lru_cache(maxsize=None)
def gather_case(B, N, K, D):
    """x fp32 [B, N, D] ~ N(0.5, 3^2); d bf16 / df fp32 residuals; idx int64 [B, K] = oracle.cls_topk_select of random ranking scores;
    compl [B, P - K]; scores fp32 [B, P], the fused row's weights: U(0, 1), the weight of every fifth dropped token from the second on 0, and one dominant weight
    (40) on the LAST dropped token of image 0 and the first of the others -- a dropped or doubled token moves the row far beyond its
    bound.  Shared: read-only."""
    g = _gen(10000 + 13 * N + 7 * K + D + B)
    P = N - 1
    x = torch.randn(B, N, D, generator=g) * 3.0 + 0.5
    d = (torch.randn(B, N, D, generator=g) * 0.3).bfloat16()
    df = torch.randn(B, N, D, generator=g) * 0.3
    idx = oracle.cls_topk_select(torch.rand(B, P, generator=g), K)
    compl = oracle.complement_idx(idx, P)
    scores = torch.rand(B, P, generator=g)
    for b in range(B):
        cb = compl[b]
        scores[b, cb[1::5]] = 0.0
        if cb.numel():
            scores[b, cb[-1 if b == 0 else 0]] = 40.0
    gamma, beta = ln_params(D)
    return dict(x=x, d=d, df=df, idx=idx, compl=compl, scores=scores, gamma=gamma, beta=beta)


def gather_source(c, delta):
    """the fp32 rows the kernel gathers from: x, x + d (bf16) or x + df (fp32)"""
    return c["x"] if delta is None else stream_sum(c["x"], c["d" if delta == "bf16" else "df"])


def gather_ref(src, idx, scores=None):
    """float64: (rows [B, K + 1 (+ 1), D], the fused row apart [B, D] | None) by oracle.gather_compact / oracle.evit_fuse"""
    if scores is None:
        return oracle.gather_compact(src.to(F64), idx), None
    rows, _ = oracle.evit_fuse(src.to(F64), idx, scores.to(F64))
    return rows, rows[:, -1]


def fuse_f32(src, compl, scores):
    """EViT's fused row in float32, token after token in the complement's order: [B, D]"""
    B, _, D = src.shape
    out = torch.zeros(B, D)
    for b in range(B):
        for t in compl[b].tolist():
            out[b] = out[b] + src[b, 1 + t] * scores[b, t]
    return out


def fuse_f32_cost(B, N, K, D, delta):
    c = gather_case(B, N, K, D)
    src = gather_source(c, delta)
    return row_rel_all(fuse_f32(src, c["compl"], c["scores"]), gather_ref(src, c["idx"], c["scores"])[1])


def _measure():
    worst, per_family = (0.0, None), {f: 0.0 for f in FAMILIES}
    for M, D, o, kind in ln_cases():
        fam = ln_case(M, D, o)["fam"]
        for eps in LN_EPS:
            rel = ln_f32_cost(M, D, o, kind, eps)
            for r in range(M):
                per_family[fam[r]] = max(per_family[fam[r]], float(rel[r]))
            r = int(rel.argmax())
            if float(rel[r]) > worst[0]:
                worst = (float(rel[r]), f"row {r} of M = {M}, D = {D}, offset {o}, stream {kind}, eps {eps:g}, family {fam[r]}")
    print("LayerNorm, ln_f32 against ln_ref, worst row relative to its largest |reference|, per family:")
    for f, v in per_family.items():
        print(f"  {f:8s} {v:.2e}")
    print(f"worst: {worst[0]:.2e} at {worst[1]}  (LN_F32_WORST {LN_F32_WORST:.1e}, LN_FWD_BOUND {LN_FWD_BOUND:.1e})")
    fworst = (0.0, None)
    for B, N, K in GATHER_CASES:
        for D in GATHER_D:
            for delta in (None, "bf16", "f32"):
                rel = fuse_f32_cost(B, N, K, D, delta)
                if float(rel.max()) > fworst[0]:
                    fworst = (float(rel.max()), f"image {int(rel.argmax())} of B, N, K = {B, N, K} ({N - 1 - K} dropped), D = {D}, delta {delta}")
    print(f"EViT fused row, fuse_f32 against float64: worst {fworst[0]:.2e} at {fworst[1]}  (FUSE_F32_WORST {FUSE_F32_WORST:.1e}, "
          f"FUSE_BOUND {FUSE_BOUND:.1e})")


if __name__ == "__main__":
    _measure()
