"""Float64 CPU references, input builders and the case tables of the edge-shape tests of the soft-assignment backward kernels
(csrc/tr_soft_bwd.hip: tr_soft_dweights, tr_soft_dsrc, tr_token_softmax_bwd, tr_sinkhorn_bwd, tr_add_into_bf16).

Every reference is the CLOSED FORM the kernel file's header states, evaluated in float64 on the fp32 operands exactly as the kernel reads
them -- no autograd here.  tests/test_soft_bwd_ref.py proves each closed form against float64 torch.autograd over the oracle's restatement
(torch.softmax over the tokens, oracle.sinkhorn_transport, torch.einsum) at every shape of the tables (CPU suite);
tests/test_hip_soft_bwd_edges.py compares the kernels with them (GPU suite).

Layouts as the kernels': token-major matrices [B, N, ld] with row 0 of an image (CLS) unused and columns K..ld padding; g = d out
[B, K+1, D] with row 0 the CLS row.  The builders fill everything a kernel must NOT read -- row 0 of g, src, wt, logits, scores and dplan,
columns K..ld of the token-major matrices -- with NaN: one stray read and the output shows it.  The references slice those regions away
before any arithmetic, and tests/test_soft_bwd_ref.py asserts that no NaN reaches a reference output.

`python -m tests._soft_bwd_ref` prints the measured numbers the GPU bounds rest on: per Sinkhorn case the distance between float32 and
float64 autograd through oracle.sinkhorn_transport (per element relative to the image's rms gradient, per token row and per centre column
relative L2), and the factor F derived from them; per product / softmax case what torch's float32 evaluation costs against the derived
bound.  The table it printed when the cases were fixed is SINKHORN_F32_MEASURED below; tests/test_soft_bwd_ref.py re-measures it.
"""
import math

import numpy as np
import torch

F64 = torch.float64
U32 = 2.0 ** -24                 # unit roundoff of fp32 (round to nearest)
BF16 = 2.0 ** -8                 # unit roundoff of bf16 (8 significant bits, round to nearest even)
NAN = float("nan")


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u) for fp32: the relative error bound of n chained fp32 roundings."""
    return n * U32 / (1.0 - n * U32)


def pad8(k):
    return (k + 7) // 8 * 8


def pad64(k):
    return (k + 63) // 64 * 64


# ---------------------------------------------------------------------------------------------------------------- case tables
# tr_soft_dweights / tr_soft_dsrc (B, N, K, D, ldl): bgemm_f32_kernel has 64 x 64 output tiles and a contraction step of 16.  dW is
# [P, K] with contraction D, dsrc is [P, D] with contraction K.  P = N - 1 in {1, 63, 64, 65, 130}, K in {1, 15, 16, 17, 63, 64, 65},
# D in {8, 24, 64, 100, 192} (shorter than one step, multiples of 16 and not, two column tiles for dsrc); ldl = K, pad8(K), pad8(K) + 8
SOFT_CASES = [
    (1, 2, 1, 8, 1), (2, 64, 15, 24, 16), (1, 65, 16, 64, 16), (3, 66, 17, 100, 32), (2, 131, 63, 192, 64), (1, 65, 64, 8, 64),
    (2, 66, 65, 24, 80), (1, 131, 65, 100, 72), (1, 2, 64, 192, 72), (2, 64, 1, 64, 8), (1, 131, 17, 64, 17), (3, 64, 63, 8, 63),
    (1, 66, 15, 192, 24), (2, 65, 16, 100, 16)]
# tr_token_softmax_bwd (B, N, K, ldl, ldo, real): 32 columns per workgroup (K in {1, 31, 32, 33, 70}), 8 token groups (P in {1, 7, 8, 9,
# 23}: groups empty, exactly full, ragged); ldl != ldo, ldo = K, pad8(K), pad64(K); real = the weights are a softmax over the tokens of
# scale * logits, else an arbitrary positive matrix (the kernel's formula does not assume that a column sums to one)
SOFTMAX_CASES = [
    (1, 2, 1, 8, 1, True), (2, 8, 31, 32, 31, False), (1, 9, 32, 40, 32, True), (3, 10, 33, 33, 40, False), (2, 24, 70, 72, 128, True),
    (1, 24, 33, 48, 64, False), (2, 9, 1, 1, 8, True), (1, 2, 70, 80, 72, False)]
SOFTMAX_SCALE = 0.7
# tr_sinkhorn_bwd (B, N, K, iters, eps, ldl, ldo, Z in LDS): 16 waves over k, 1024 threads over p, LDS stride PP = P | 1 (both parities
# of P), iters 1 and 8 (SB_MAXIT), K > P, the two shapes either side of the 160 KB switch and the two with P = 1025 > 1024 threads.
# K = 1 or P = 1 are degenerate: the plan is constant and the gradient mathematically zero
SINKHORN_CASES = [
    (2, 2, 1, 1, 1.0, 8, 1, True), (1, 2, 3, 2, 1.0, 3, 8, True), (3, 30, 1, 3, 1.0, 8, 64, True), (2, 30, 7, 5, 1.0, 8, 7, True),
    (1, 30, 7, 8, 0.1, 16, 64, True), (3, 17, 16, 1, 1.0, 16, 24, True), (2, 66, 17, 8, 0.5, 24, 64, True), (2, 20, 33, 3, 1.0, 40, 33, True),
    (2, 289, 128, 3, 1.0, 128, 128, True), (2, 290, 129, 3, 1.0, 136, 192, False), (1, 1026, 3, 1, 1.0, 8, 64, True),
    (2, 1026, 40, 2, 0.7, 40, 64, False)]
SB_MAXIT, SB_LDS_LIMIT = 8, 160 * 1024
# refusals of tr_sinkhorn_bwd (N, K, iters, eps, ldo): TR_ERR_SHAPE before anything is launched
SINKHORN_REFUSED = [(30, 7, 0, 1.0, 8), (30, 7, SB_MAXIT + 1, 1.0, 8), (30, 7, 3, 0.0, 8), (30, 7, 3, 1.0, 6)]
# tr_add_into_bf16: the vector body takes four elements per thread, 1024 per workgroup; n % 4 != 0 leaves the scalar tail
ADD_CASES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 1027, 4099]


def sinkhorn_lds_bytes(N, K, iters, zlds):
    """sinkhorn_bwd_lds of csrc/tr_soft_bwd.hip, restated."""
    P = N - 1
    PP = P | 1
    return ((K * PP if zlds else 0) + 2 * (iters + 1) * (K + P) + K + P) * 4


def sinkhorn_degenerate(N, K):
    return K == 1 or N == 2


for _B, _N, _K, _it, _eps, _ldl, _ldo, _zlds in SINKHORN_CASES:
    # which side of the LDS switch a case is on is part of the table: a change to the formula fails here instead of moving a case
    assert (sinkhorn_lds_bytes(_N, _K, _it, True) <= SB_LDS_LIMIT) == _zlds, (_N, _K, _it)
    assert sinkhorn_lds_bytes(_N, _K, _it, _zlds) <= SB_LDS_LIMIT and 1 <= _it <= SB_MAXIT and _ldl >= _K and _ldo >= _K
assert sinkhorn_lds_bytes(289, 128, 3, True) == 40736 * 4 and sinkhorn_lds_bytes(290, 129, 3, True) > SB_LDS_LIMIT
assert {(c[1] - 1) % 2 for c in SINKHORN_CASES} == {0, 1}

# float32 against float64 autograd through oracle.sinkhorn_transport, as `python -m tests._soft_bwd_ref` printed it for the table above
# (N, K, iters, eps) -> (max |fp32 - fp64| / rms(fp64 over the image), worst token row, worst centre column (relative L2)).
# The GPU test allows F x the image's rms per element on top of the bf16 rounding, F = 8 x the worst first entry: the kernel sums in
# another order than torch's float32 and uses its own expf.
SINKHORN_F32_MEASURED = {
    (30, 7, 5, 1.0): (1.50e-06, 9.41e-07, 7.11e-07),
    (30, 7, 8, 0.1): (1.06e-05, 1.21e-05, 2.03e-06),
    (17, 16, 1, 1.0): (1.60e-06, 4.51e-07, 5.07e-07),
    (66, 17, 8, 0.5): (7.12e-06, 1.50e-06, 1.24e-06),
    (20, 33, 3, 1.0): (2.74e-06, 4.99e-07, 5.79e-07),
    (289, 128, 3, 1.0): (6.75e-06, 1.00e-06, 9.40e-07),
    (290, 129, 3, 1.0): (5.49e-06, 9.94e-07, 9.92e-07),
    (1026, 3, 1, 1.0): (2.43e-06, 1.27e-05, 4.08e-07),
    (1026, 40, 2, 0.7): (1.77e-05, 1.74e-06, 1.31e-06),
}
SINKHORN_F = 8 * max(v[0] for v in SINKHORN_F32_MEASURED.values())          # 8 x 1.77e-5 = 1.42e-4
# the worst row (1.27e-5) and column (2.03e-6) stay below the 1.5e-5 by which the largest relative error of a bf16 rounding,
# 2^-8 / (1 + 2^-8), is short of 2^-8: the row / column bound 2^-8 is the bf16 rounding with slack, not an fp32 allowance


# ---------------------------------------------------------------------------------------------------------------- builders
def _rng(seed):
    return np.random.default_rng(seed)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _token_major(rng, B, N, K, ld, scale=1.0, positive=False):
    """[B, N, ld] fp32: values on the patch rows of columns < K, NaN on row 0 and in columns K..ld."""
    v = rng.standard_normal((B, N - 1, K)) * scale
    t = torch.full((B, N, ld), NAN)
    t[:, 1:, :K] = _f32(1.2 + np.abs(v) if positive else v)               # positive: every entry, so every column sum, above 1.2
    return t


def _rows(rng, B, R, D, scale=1.0):
    """[B, R, D] fp32 with row 0 of every image NaN."""
    t = _f32(rng.standard_normal((B, R, D)) * scale)
    t[:, 0] = NAN
    return t


def soft_case(B, N, K, D, ldl, seed=0):
    """g = d out [B, K+1, D], src [B, N, D], wt [B, N, ldl] (a softmax over the tokens)."""
    rng = _rng(100 + seed)
    wt = torch.full((B, N, ldl), NAN)
    wt[:, 1:, :K] = torch.softmax(_f32(rng.standard_normal((B, N - 1, K))).double(), dim=1).float()
    return dict(g=_rows(rng, B, K + 1, D, 0.1), src=_rows(rng, B, N, D), wt=wt, K=K)


def softmax_case(B, N, K, ldl, ldo, real, seed=0):
    rng = _rng(200 + seed)
    logits = _token_major(rng, B, N, K, ldl)
    if real:
        wt = torch.full((B, N, ldl), NAN)
        wt[:, 1:, :K] = torch.softmax(logits[:, 1:, :K].double() * SOFTMAX_SCALE, dim=1).float()
    else:
        wt = _token_major(rng, B, N, K, ldl, scale=0.7, positive=True)
    return dict(wt=wt, dwt=_token_major(rng, B, N, K, ldl, scale=0.5), logits=logits, scale=SOFTMAX_SCALE, K=K)


def sinkhorn_case(B, N, K, iters, eps, ldl, seed=0):
    rng = _rng(300 + seed)
    return dict(scores=_token_major(rng, B, N, K, ldl, scale=0.3), dplan=_token_major(rng, B, N, K, ldl), K=K, eps=eps, iters=iters)


def add_case(n, seed=0):
    rng = _rng(400 + seed)
    return dict(a=_f32(rng.standard_normal(n)), y=_f32(rng.standard_normal(n)).bfloat16())


# ---------------------------------------------------------------------------------------------------------------- closed forms
def soft_dweights_ref(g, src, K):
    """dW[b, p, k] = <g[b, 1+k], src[b, 1+p]> -> (dW [B, P, K], sum_d |g| |src| of the same shape)."""
    g, s = g[:, 1:K + 1].to(F64), src[:, 1:].to(F64)
    return torch.einsum("bkd,bpd->bpk", g, s), torch.einsum("bkd,bpd->bpk", g.abs(), s.abs())


def soft_dsrc_ref(g, wt, K):
    """dsrc[b, 1+p] = sum_k W[b, 1+p, k] g[b, 1+k] -> (dsrc [B, P, D], sum_k |W| |g|)."""
    g, w = g[:, 1:K + 1].to(F64), wt[:, 1:, :K].to(F64)
    return torch.einsum("bpk,bkd->bpd", w, g), torch.einsum("bpk,bkd->bpd", w.abs(), g.abs())


def token_softmax_bwd_ref(wt, dwt, logits, scale, K):
    """c[k] = sum_p W dW;  ds = scale W (dW - c);  d scale = sum W (dW - c) logits.
    -> (ds [B, P, K], dscale, S = sum_p |W dW| [B, 1, K], sum of |W| (|dW| + S) |logits|: the absolute terms of d scale)."""
    w, dw = wt[:, 1:, :K].to(F64), dwt[:, 1:, :K].to(F64)
    c = (w * dw).sum(1, keepdim=True)
    S = (w * dw).abs().sum(1, keepdim=True)
    v = w * (dw - c)
    if logits is None:
        return scale * v, None, S, None
    lg = logits[:, 1:, :K].to(F64)
    return scale * v, (v * lg).sum(), S, (w.abs() * (dw.abs() + S) * lg.abs()).sum()


def token_softmax_floor(wt, dwt, scale, K, S, extra=0.0):
    """The fp32 part of the ds bound (tests/test_hip_soft_bwd_edges.py states the derivation): |scale| |W| (gamma_3 (|dW| + S) +
    gamma_(P+8) S + extra)."""
    w, dw = wt[:, 1:, :K].to(F64).abs(), dwt[:, 1:, :K].to(F64).abs()
    P = w.shape[1]
    return abs(scale) * w * (gamma(3) * (dw + S) + gamma(P + 8) * S + extra)


def sinkhorn_bwd_ref(scores, dplan, K, eps, iters):
    """The unrolled log-domain iterations backwards (header of csrc/tr_soft_bwd.hip), Z0 = scores / eps as [B, K, P]:
      forward   u_t = norm - LSE_p(Z0 + v_(t-1)),  v_t = norm - LSE_k(Z0 + u_t),  plan = exp(Z0 + u_T + v_T - norm),  norm = -log(K + P)
      backward  dZ = dZf = dplan * plan;  du = rowsum(dZf), dv = colsum(dZf);  for t = T..1:
                  A_t = softmax_k(Z0 + u_t) (= exp(Z0 + u_t + v_t - norm)):      dZ -= dv A_t;  du -= sum_p dv A_t
                  B_t = softmax_p(Z0 + v_(t-1)) (= exp(Z0 + u_t + v_(t-1) - norm)):  dZ -= du B_t;  dv = -sum_k du B_t;  du = 0
                dscores = dZ / eps.
    A_t and B_t are evaluated as the softmaxes they are, so a single row or column gives exactly 1 and the degenerate cases exactly 0.
    -> ds [B, P, K]"""
    z = scores[:, 1:, :K].to(F64).transpose(1, 2) / eps
    gp = dplan[:, 1:, :K].to(F64).transpose(1, 2)
    B, Kk, P = z.shape
    norm = -math.log(Kk + P)
    u, v = [torch.zeros(B, Kk, dtype=F64)], [torch.zeros(B, P, dtype=F64)]
    for _ in range(iters):
        u.append(norm - torch.logsumexp(z + v[-1][:, None, :], dim=2))
        v.append(norm - torch.logsumexp(z + u[-1][:, :, None], dim=1))
    dzf = gp * (z + u[-1][:, :, None] + v[-1][:, None, :] - norm).exp()
    dz, du, dv = dzf.clone(), dzf.sum(2), dzf.sum(1)
    for t in range(iters, 0, -1):
        m = torch.softmax(z + u[t][:, :, None], dim=1) * dv[:, None, :]
        dz = dz - m
        du = du - m.sum(2)
        m = torch.softmax(z + v[t - 1][:, None, :], dim=2) * du[:, :, None]
        dz = dz - m
        dv = -m.sum(1)
        du = torch.zeros_like(du)
    return (dz / eps).transpose(1, 2).contiguous()


def add_into_bf16_ref(a, y):
    """bf16(a + float(y)): one fp32 sum, one rounding to nearest even."""
    return (a + y.float()).bfloat16()


# ---------------------------------------------------------------------------------------------------------------- autograd restatements
def softmax_autograd(wt, dwt, logits, scale, K, real, dtype=F64):
    """ds and d scale by autograd.  real: W = softmax over the tokens of scale * logits.  Otherwise through y = W (z - sum_p W z),
    z = scale * logits, with W held constant: the map whose (symmetric) Jacobian diag(W) - W W^T the kernel's formula applies."""
    lg = logits[:, 1:, :K].to(dtype).clone().requires_grad_(True)
    sc = torch.tensor(scale, dtype=dtype, requires_grad=True)
    dw = dwt[:, 1:, :K].to(dtype)
    if real:
        y = torch.softmax(lg * sc, dim=1)
    else:
        w = wt[:, 1:, :K].to(dtype)
        z = lg * sc
        y = w * (z - (w * z).sum(1, keepdim=True))
    gl, gs = torch.autograd.grad((y * dw).sum(), (lg, sc))
    return gl, gs


def sinkhorn_autograd(scores, dplan, K, eps, iters, dtype=F64):
    import oracle
    s = scores[:, 1:, :K].to(dtype).clone().requires_grad_(True)
    plan = oracle.sinkhorn_transport(s.transpose(1, 2), eps, iters).transpose(1, 2)
    gs, = torch.autograd.grad((plan * dplan[:, 1:, :K].to(dtype)).sum(), s)
    return gs


def image_rms(t):
    """rms over each image of [B, P, K] -> [B, 1, 1]"""
    return t.to(F64).pow(2).mean(dim=(1, 2), keepdim=True).sqrt()


def row_col_rel(got, want):
    """worst relative L2 over the token rows and over the centre columns of [B, P, K]"""
    d, w = got.to(F64) - want.to(F64), want.to(F64)
    row = (d.norm(dim=2) / w.norm(dim=2).clamp_min(1e-300)).max()
    col = (d.norm(dim=1) / w.norm(dim=1).clamp_min(1e-300)).max()
    return float(row), float(col)


def sinkhorn_f32_measure():
    """{(N, K, iters, eps): (max |fp32 - fp64| / image rms, worst row rel L2, worst column rel L2)} over the non-degenerate cases"""
    out = {}
    for B, N, K, iters, eps, ldl, ldo, _ in SINKHORN_CASES:
        if sinkhorn_degenerate(N, K):
            continue
        c = sinkhorn_case(B, N, K, iters, eps, ldl)
        want = sinkhorn_autograd(**c)
        got = sinkhorn_autograd(**c, dtype=torch.float32)
        out[(N, K, iters, eps)] = (float(((got.double() - want).abs() / image_rms(want)).max()),) + row_col_rel(got, want)
    return out


def _report():
    for B, N, K, D, ldl in SOFT_CASES:
        c = soft_case(B, N, K, D, ldl)
        for name, (want, mag), L, got in (("dW", soft_dweights_ref(c["g"], c["src"], K), D,
                                           torch.einsum("bkd,bpd->bpk", c["g"][:, 1:], c["src"][:, 1:])),
                                          ("dsrc", soft_dsrc_ref(c["g"], c["wt"], K), K,
                                           torch.einsum("bpk,bkd->bpd", c["wt"][:, 1:, :K], c["g"][:, 1:]))):
            r = float(((got.double() - want).abs() / (gamma(L) * mag)).max())
            print(f"soft {B, N, K, D, ldl} {name}: torch fp32 uses {r:.3f} of the bound gamma_{L} sum |a||b|")
    for B, N, K, ldl, ldo, real in SOFTMAX_CASES:
        c = softmax_case(B, N, K, ldl, ldo, real)
        want, dsc, S, mag = token_softmax_bwd_ref(**c)
        got, gsc = softmax_autograd(**c, real=real, dtype=torch.float32)
        floor = token_softmax_floor(c["wt"], c["dwt"], c["scale"], K, S)
        r = float(((got.double() - want).abs() / floor.clamp_min(1e-300)).max()) if want.numel() else 0.0
        print(f"softmax {B, N, K, ldl, ldo, real}: torch fp32 ds uses {r:.3f} of the fp32 floor; d scale err {abs(float(gsc) - float(dsc)):.2e} "
              f"(sum of absolute terms {float(mag):.2e})")
    m = sinkhorn_f32_measure()
    print("SINKHORN_F32_MEASURED = {")
    for k, v in m.items():
        print(f"    {k}: ({v[0]:.2e}, {v[1]:.2e}, {v[2]:.2e}),")
    print("}")
    print(f"F = 8 x {max(v[0] for v in m.values()):.2e} = {8 * max(v[0] for v in m.values()):.2e}; worst row {max(v[1] for v in m.values()):.2e}, "
          f"worst column {max(v[2] for v in m.values()):.2e} (bound 2^-8 = {BF16:.2e})")


if __name__ == "__main__":
    _report()
