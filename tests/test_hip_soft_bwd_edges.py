"""GPU parity of the soft-assignment backward kernels at their edge shapes (csrc/tr_soft_bwd.hip: tr_soft_dweights, tr_soft_dsrc,
tr_token_softmax_bwd, tr_sinkhorn_bwd, tr_add_into_bf16): the whole gradient path of SiT, PatchMerger and Sinkhorn before a reducing stage.

tests/test_hip_backward.py holds these kernels at model shapes under one whole-tensor norm.  The shapes here (tests/_soft_bwd_ref.py, with
the reason for each next to its table) are the smallest that reach every tile edge, loop tail and kernel switch.  The checker is the
float64 closed form of _soft_bwd_ref.py -- proven against float64 autograd on the CPU by tests/test_soft_bwd_ref.py -- fed the same fp32
operands as the kernel, and EVERY element is held to a bound of its own.

Partial-write contract.  Every output is handed over filled with a sentinel (a NaN whose payload no arithmetic produces) between guard
words.  The kernels write the patch rows of columns < K, ds also a zero CLS row for those columns; everything else -- the CLS rows of dW
and dsrc, columns K..ld on every row, the guards -- must hold the sentinel afterwards, and no written element may be NaN: the inputs carry
NaN wherever a kernel must not read (row 0 of g, src, wt, logits, scores, dplan; columns K..ld).

Bounds (u = 2^-24, gamma_n = n u / (1 - n u)):
  dW, dsrc   fp32 products of contraction length L (D for dW, K for dsrc), fma-accumulated in some order:
             |got - want| <= gamma_L sum_l |a_l| |b_l|, the right-hand side in float64 from the same operands.
  ds of the softmax (bf16).  The kernel forms c^ = sum_p W dW in fp32 (P products, at most ceil(P/8) + 7 additions on any path:
             |c^ - c| <= gamma_(P+8) S, S = sum_p |W dW|), then x^ = scale W (dW - c^) with three more roundings:
             |x^ - want| <= |scale| |W| (gamma_3 |dW - c| + (1 + gamma_3) gamma_(P+8) S) <= floor := |scale| |W| (gamma_3 (|dW| + S) + gamma_(P+8) S)
             up to second order, and stores got = bf16(x^), |got - x^| <= 2^-8 |x^|.  So
             |got - want| <= 2^-8 |want| + (1 + 2^-8) floor.
  d scale    sum over all (b, p, k) of W (dW - c^) logits: each term within gamma_(P+11) |W| (|dW| + S) |logits| of its exact value, then
             at most ceil(P/8) + 3 + 6 additions in the workgroup, one per partial and one for the accumulated start value:
             |got - want| <= gamma_L (sum |W| (|dW| + S) |logits| + |start|), L = P + 11 + ceil(P/8) + 10 + B ceil(K/32).
  ds of Sinkhorn (bf16): per element 2^-8 |want| + F rms(want over the image), F = 8 x the worst float32-against-float64 autograd ratio
             over the table (R.SINKHORN_F32_MEASURED, 1.42e-4); per token row and per centre column relative L2 <= 2^-8.  Degenerate cases
             (K = 1 or P = 1) are mathematically zero: the 2 iters + 1 terms of an element cancel, each term is at most max |dplan| / eps
             in magnitude and carries the rounding of its expf argument (|argument| <= 16: about 1e-6 relative), so what is left is of
             the order of (2 iters + 1) 1e-6 max |dplan| / eps; asserted |ds| <= 1e-4 max |dplan| / eps.
  add_into_bf16   bit-equal to (a + y.float()).bfloat16().
The stage chains compose the kernels as tr_vit_backward does (forward weights from the forward kernel, dW feeding the softmax / Sinkhorn
backward) and are compared end to end with float64 autograd from the logits under the same bounds, widened only by what the forward
weights' fp32 error adds (stated at `_softmax_chain` and `test_chain_sinkhorn`).
"""
import functools
import math

import pytest
import torch

from tests import _soft_bwd_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
GUARD = 256
SENT32, SENT16 = 0x7FA5A5A5, 0x7FA5          # signalling-NaN payloads: not zero, not the default quiet NaN (0x7fc00000 / 0x7fc0)
TR_ERR_SHAPE, TR_ERR_ALIGN = -1, -2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


class _Out:
    """An output tensor of `shape` filled with the sentinel, between GUARD sentinel words on either side."""

    def __init__(self, shape, dtype):
        self.idt, self.sent = (torch.int32, SENT32) if dtype == torch.float32 else (torch.int16, SENT16)
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 2 * GUARD,), self.sent, dtype=self.idt, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(dtype).view(*shape)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[GUARD + self.n:] == self.sent).all())

    def untouched(self, region):
        """region: a slice of self.t -> every element still the sentinel"""
        return bool((region.contiguous().view(self.idt) == self.sent).all())


def _cuda(c, *names):
    return [None if c[n] is None else c[n].cuda() for n in names]


def _assert_elementwise(got, want, bound, what):
    """every element: |got - want| <= bound (float64, CPU); prints the worst use of the bound"""
    got, want = got.detach().to(F64).cpu(), want.to(F64)
    assert got.shape == want.shape, what
    assert not bool(got.isnan().any()), f"{what}: NaN in the written region (a read of a forbidden row / column, or an element left unwritten)"
    if got.numel() == 0:
        return
    err = (got - want).abs()
    use = err / bound.clamp_min(1e-300)
    i = int(use.argmax())
    print(f"{what}: worst |got - want| / bound = {float(use.max()):.3f} (err {float(err.reshape(-1)[i]):.3e}, bound {float(bound.reshape(-1)[i]):.3e})")
    assert bool((err <= bound).all()), (f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond their bound, worst at flat index {i}: "
                                       f"err {float(err.reshape(-1)[i]):.3e} > {float(bound.reshape(-1)[i]):.3e}")


# one case and one float64 reference per table row, shared by the parametrizations that use it; nothing below writes to them
@functools.lru_cache(maxsize=None)
def _soft(B, N, K, D, ldl):
    c = R.soft_case(B, N, K, D, ldl)
    return c, R.soft_dweights_ref(c["g"], c["src"], K), R.soft_dsrc_ref(c["g"], c["wt"], K)


@functools.lru_cache(maxsize=None)
def _softmax(B, N, K, ldl, ldo, real):
    c = R.softmax_case(B, N, K, ldl, ldo, real)
    return c, R.token_softmax_bwd_ref(**c)


@pytest.mark.parametrize("B,N,K,D,ldl", R.SOFT_CASES)
def test_soft_dweights_dsrc(ops, B, N, K, D, ldl):
    """bgemm_f32_kernel at the edges of its 64 x 64 tiles and of its contraction step of 16, NT (dW) and NN (dsrc), every row stride."""
    c, (dw_ref, dw_mag), (dsrc_ref, dsrc_mag) = _soft(B, N, K, D, ldl)
    g, wt, src = _cuda(c, "g", "wt", "src")
    dwt, dsrc = _Out((B, N, ldl), torch.float32), _Out((B, N, D), torch.float32)
    r_dwt, r_dsrc = ops.soft_merge_bwd(g, wt, src, dwt=dwt.t, dsrc=dsrc.t)
    assert r_dwt is dwt.t and r_dsrc is dsrc.t
    assert dwt.guards_intact() and dsrc.guards_intact(), "written outside the output"
    assert dwt.untouched(dwt.t[:, 0]) and dsrc.untouched(dsrc.t[:, 0]), "the CLS row of dW / dsrc was written"
    assert dwt.untouched(dwt.t[:, :, K:]), "columns K..ldl of dW were written"
    _assert_elementwise(dwt.t[:, 1:, :K], dw_ref, R.gamma(D) * dw_mag, "dW")
    _assert_elementwise(dsrc.t[:, 1:], dsrc_ref, R.gamma(K) * dsrc_mag, "dsrc")
    # the wrapper's own outputs: zero wherever the kernels do not write, the same values where they do
    f_dwt, f_dsrc = ops.soft_merge_bwd(g, wt, src)
    assert torch.equal(f_dwt[:, 1:, :K], dwt.t[:, 1:, :K]) and torch.equal(f_dsrc[:, 1:], dsrc.t[:, 1:])
    assert float(f_dwt[:, 0].abs().max()) == 0.0 and float(f_dsrc[:, 0].abs().max()) == 0.0
    assert K == ldl or float(f_dwt[:, :, K:].abs().max()) == 0.0


def _check_ds_contract(ds, K):
    assert ds.guards_intact(), "ds: written outside the output"
    assert ds.untouched(ds.t[:, :, K:]), "ds: columns K..ldo were written"
    assert bool((ds.t[:, 0, :K].contiguous().view(torch.int16) == 0).all()), "ds: the CLS row is not exactly zero for k < K"


def _dscale_len(B, P, K):
    return P + 11 + (P + 7) // 8 + 10 + B * ((K + 31) // 32)


@pytest.mark.parametrize("mode", ["no_dscale", "dscale", "accumulate"])
@pytest.mark.parametrize("B,N,K,ldl,ldo,real", R.SOFTMAX_CASES)
def test_token_softmax_bwd(ops, B, N, K, ldl, ldo, real, mode):
    """32-column workgroups and 8 token groups empty / full / ragged, ldl != ldo, weights normalised and not; d scale absent, written,
    accumulated onto a non-zero start value."""
    c, (ds_ref, dscale_ref, S, mag) = _softmax(B, N, K, ldl, ldo, real)
    wt, dwt, logits = _cuda(c, "wt", "dwt", "logits")
    ds = _Out((B, N, ldo), torch.bfloat16)
    start = -3.25
    if mode == "no_dscale":
        r_ds, dscale = ops.token_softmax_bwd(wt, dwt, None, c["scale"], K, ds=ds.t)
        assert dscale is None
    else:
        acc = mode == "accumulate"
        dsc0 = torch.full((1,), start if acc else float("nan"), device="cuda")
        r_ds, dscale = ops.token_softmax_bwd(wt, dwt, logits, c["scale"], K, ds=ds.t, dscale=dsc0, accumulate=acc)
        assert dscale is dsc0
        want = float(dscale_ref) + (start if acc else 0.0)
        bound = R.gamma(_dscale_len(B, N - 1, K)) * (float(mag) + (abs(start) if acc else 0.0))
        err = abs(float(dscale.double()) - want)
        print(f"d scale: err {err:.3e}, bound {bound:.3e} (value {want:.6f})")
        assert err <= bound, f"d scale: {float(dscale)} against {want}: err {err:.3e} > {bound:.3e}"
    assert r_ds is ds.t
    _check_ds_contract(ds, K)
    floor = R.token_softmax_floor(c["wt"], c["dwt"], c["scale"], K, S)
    _assert_elementwise(ds.t[:, 1:, :K].float(), ds_ref, R.BF16 * ds_ref.abs() + (1 + R.BF16) * floor, "ds")
    if mode == "dscale":
        f_ds, f_dscale = ops.token_softmax_bwd(wt, dwt, logits, c["scale"], K, want_dscale=True)          # the wrapper's own outputs
        assert f_ds.shape == (B, N, R.pad64(K)) and torch.equal(f_ds[:, 1:, :K], ds.t[:, 1:, :K]) and torch.equal(f_dscale, dscale)
        assert float(f_ds[:, 0].float().abs().max()) == 0.0 and float(f_ds[:, :, K:].float().abs().max()) == 0.0


@pytest.mark.parametrize("B,N,K,iters,eps,ldl,ldo,zlds", R.SINKHORN_CASES)
def test_sinkhorn_bwd(ops, B, N, K, iters, eps, ldl, ldo, zlds):
    """16 waves over k, 1024 threads over p (P = 1025 takes a second trip), both parities of the LDS stride, iters 1 and 8, K > P, the
    last shape with Z in LDS and the first without."""
    c = R.sinkhorn_case(B, N, K, iters, eps, ldl)
    want = R.sinkhorn_bwd_ref(**c)
    scores, dplan = _cuda(c, "scores", "dplan")
    ds = _Out((B, N, ldo), torch.bfloat16)
    assert ops.sinkhorn_bwd(scores, dplan, K, eps, iters, ds=ds.t) is ds.t
    _check_ds_contract(ds, K)
    got = ds.t[:, 1:, :K].float()
    if R.sinkhorn_degenerate(N, K):
        assert float(want.abs().max()) == 0.0
        bound = 1e-4 * float(c["dplan"][:, 1:, :K].abs().max()) / eps
        _assert_elementwise(got, want, torch.full_like(want, bound), "ds (degenerate)")
        return
    _assert_elementwise(got, want, R.BF16 * want.abs() + R.SINKHORN_F * R.image_rms(want), "ds")
    row, col = R.row_col_rel(got.cpu(), want)
    print(f"ds: worst token row {row:.3e}, worst centre column {col:.3e} (relative L2, bound {R.BF16:.3e})")
    assert row <= R.BF16 and col <= R.BF16, f"ds: worst token row {row:.3e}, worst centre column {col:.3e} > 2^-8"


def test_sinkhorn_bwd_default_output(ops):
    """without a given ds the wrapper allocates a zeroed [B, N, pad64(K)]"""
    B, N, K, iters, eps, ldl = 2, 30, 7, 5, 1.0, 8
    c = R.sinkhorn_case(B, N, K, iters, eps, ldl)
    scores, dplan = _cuda(c, "scores", "dplan")
    ds = _Out((B, N, 7), torch.bfloat16)
    ops.sinkhorn_bwd(scores, dplan, K, eps, iters, ds=ds.t)
    fresh = ops.sinkhorn_bwd(scores, dplan, K, eps, iters)
    assert fresh.shape == (B, N, 64) and torch.equal(fresh[:, 1:, :K], ds.t[:, 1:, :K])
    assert float(fresh[:, 0].float().abs().max()) == 0.0 and float(fresh[:, :, K:].float().abs().max()) == 0.0
    wide = ops.sinkhorn_bwd(scores, dplan, K, eps, iters, ldo=16)
    assert wide.shape == (B, N, 16) and torch.equal(wide[:, :, :K], fresh[:, :, :K])


@pytest.mark.parametrize("N,K,iters,eps,ldo", R.SINKHORN_REFUSED)
def test_sinkhorn_bwd_refusals(ops, N, K, iters, eps, ldo):
    """iters outside 1..8, eps = 0, ldo < K: TR_ERR_SHAPE, and nothing is launched (the output keeps its sentinel)"""
    from tokenreduction_amd import _lib
    B, ldl = 1, 8
    c = R.sinkhorn_case(B, N, K, max(1, min(iters, R.SB_MAXIT)), 1.0, ldl)
    scores, dplan = _cuda(c, "scores", "dplan")
    ds = _Out((B, N, 8), torch.bfloat16)
    rc = _lib.load().tr_sinkhorn_bwd(scores.data_ptr(), dplan.data_ptr(), ldl, float(eps), iters, ds.t.data_ptr(), ldo, B, N, K,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == TR_ERR_SHAPE
    assert ds.untouched(ds.t) and ds.guards_intact()
    with pytest.raises(RuntimeError, match=r"tr_sinkhorn_bwd failed \(code -1\)"):
        ops.sinkhorn_bwd(scores, dplan, K, eps, iters, ldo=ldo)


def _add_buffers(n):
    c = R.add_case(n)
    a = torch.zeros(n + 8, device="cuda")
    a[:n] = c["a"].cuda()
    y = _Out((n + 4,), torch.bfloat16)                     # y proper is y.t[:n]; y.t[n:] are four more guard words directly behind it
    y.t[:n] = c["y"].cuda()
    return c, a, y


@pytest.mark.parametrize("n", R.ADD_CASES)
def test_add_into_bf16(ops, n):
    """whole vectors of four, the scalar tail (n % 4 != 0), one element, nothing, a second workgroup (n > 1024)"""
    from tokenreduction_amd import _lib
    c, a, y = _add_buffers(n)
    rc = _lib.load().tr_add_into_bf16(a.data_ptr(), y.t.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert y.guards_intact() and y.untouched(y.t[n:]), "written past the end of y"
    want = R.add_into_bf16_ref(**c)
    assert torch.equal(y.t[:n].cpu().view(torch.int16), want.view(torch.int16)), "not bit-equal to (a + y.float()).bfloat16()"
    if n:
        y2 = c["y"].cuda()
        assert ops.add_into_bf16(c["a"].cuda(), y2) is y2 and torch.equal(y2.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("a_off,y_off", [(4, 0), (0, 2)])
def test_add_into_bf16_refuses_misaligned(ops, a_off, y_off):
    """`a` 4 bytes off a 16-byte boundary, `y` 2 bytes off an 8-byte boundary: TR_ERR_ALIGN, y unchanged"""
    from tokenreduction_amd import _lib
    n = 64
    c, a, y = _add_buffers(n)
    before = y.buf.clone()
    assert a.data_ptr() % 16 == 0 and y.t.data_ptr() % 8 == 0
    rc = _lib.load().tr_add_into_bf16(a.data_ptr() + a_off, y.t.data_ptr() + y_off, n - 2, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == TR_ERR_ALIGN
    assert torch.equal(y.buf, before)


# ---------------------------------------------------------------------------------------------------------------- stage chains
def _chain_inputs(seed, B, N, K, D, ldl, logit_scale):
    """zero-padded as the training forward's buffers are (the forward kernels own these layouts); g row 0 is the CLS gradient, unused here"""
    gen = torch.Generator().manual_seed(seed)
    logits = torch.zeros(B, N, ldl)
    logits[:, 1:, :K] = torch.randn(B, N - 1, K, generator=gen) * logit_scale
    x, src = torch.randn(B, N, D, generator=gen), torch.randn(B, N, D, generator=gen)
    g = torch.randn(B, K + 1, D, generator=gen) * 0.1
    g[:, 0] = float("nan")
    return logits, x, src, g


def _softmax_chain(ops, B, N, K, D, ldl, own_rows):
    """softmax over tokens -> merge (tr_softassign_merge_fast, which leaves the weights in the logits' copy), then tr_soft_dweights /
    tr_soft_dsrc -> tr_token_softmax_bwd onto zeroed outputs, as tr_vit_backward composes them; against float64 autograd from the logits.

    What the forward's fp32 weights add to the bounds: W^ = W (1 + d), |d| <= cW := gamma_(P+16) + 8 u max |scale logits| (the exponent's
    argument: product, max subtraction, base change; expf, a sum of P terms in 8 groups, one division), and dW^ = dW + e,
    |e| <= E := gamma_D sum |g| |src|.  To first order x = scale W (dW - c) moves by at most
    |scale| |W| (cW (|dW| + 2 S) + E + sum_p |W| E), which enters the floor; 1 % is added for the second order."""
    scale = R.SOFTMAX_SCALE
    logits, x, src, g = _chain_inputs(77 + K, B, N, K, D, ldl, 1.0)
    if own_rows:
        src = x                                                # SiT sums the stream's own rows; PatchMerger their LayerNorm image
    P = N - 1
    lg = logits[:, 1:, :K].to(F64).clone().requires_grad_(True)
    sc = torch.tensor(scale, dtype=F64, requires_grad=True)
    s64 = src[:, 1:].to(F64).clone().requires_grad_(True)
    w64 = torch.softmax(lg * sc, dim=1)
    out = torch.einsum("bpk,bpd->bkd", w64, s64)
    g_lg, g_sc, g_src = torch.autograd.grad((out * g[:, 1:].to(F64)).sum(), (lg, sc, s64))
    w64 = w64.detach()

    wbuf = logits.cuda().clone()
    x_out, _ = ops.softassign_merge_fast(wbuf, scale, x.cuda(), K, apply_softmax=True, src=src.cuda())
    dwt, dsrc = ops.soft_merge_bwd(g.cuda(), wbuf, src.cuda())
    ds, dscale = ops.token_softmax_bwd(wbuf, dwt, logits.cuda(), scale, K, want_dscale=True)
    assert float(ds[:, 0].float().abs().max()) == 0.0 and float(ds[:, :, K:].float().abs().max()) == 0.0 and float(dsrc[:, 0].abs().max()) == 0.0

    cW = R.gamma(P + 16) + 8 * R.U32 * float((lg.detach() * scale).abs().max())
    dw_ref, dw_mag = R.soft_dweights_ref(g, src, K)
    _assert_elementwise(dwt[:, 1:, :K], dw_ref, R.gamma(D) * dw_mag, "chain dW")
    wfull = torch.zeros(B, N, K, dtype=F64)
    wfull[:, 1:] = w64
    dsrc_ref, dsrc_mag = R.soft_dsrc_ref(g, wfull, K)
    _assert_elementwise(dsrc[:, 1:], g_src, (R.gamma(K) + 1.01 * cW) * dsrc_mag, "chain dsrc")
    assert float((dsrc_ref - g_src).abs().max()) <= 1e-10 * float(g_src.abs().max())
    dwfull = torch.zeros(B, N, K, dtype=F64)
    dwfull[:, 1:] = dw_ref
    ref_ds, ref_dscale, S, mag = R.token_softmax_bwd_ref(wfull, dwfull, logits, scale, K)
    assert float((ref_ds - g_lg).abs().max()) <= 1e-10 * float(g_lg.abs().max())
    E = R.gamma(D) * dw_mag
    extra = 1.01 * (cW * (dw_ref.abs() + 2 * S) + E + (w64 * E).sum(1, keepdim=True))
    floor = R.token_softmax_floor(wfull, dwfull, scale, K, S, extra=extra)
    _assert_elementwise(ds[:, 1:, :K].float(), g_lg, R.BF16 * g_lg.abs() + (1 + R.BF16) * floor, "chain ds")
    bound = R.gamma(_dscale_len(B, P, K)) * float(mag) + float((w64 * extra * lg.detach().abs()).sum())
    err = abs(float(dscale.double()) - float(g_sc))
    print(f"chain d scale: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_chain_sit(ops):
    """SiT: the merged rows are the stream's own; K = 33 is one column past a softmax workgroup, P = 65 one row past a tile"""
    _softmax_chain(ops, 2, 66, 33, 100, 40, own_rows=True)


def test_chain_patchmerger(ops):
    """PatchMerger: the merged rows are another tensor (the LayerNorm image); P = 9 leaves the token groups ragged, D = 24 a ragged step"""
    _softmax_chain(ops, 3, 10, 17, 24, 24, own_rows=False)


def test_chain_sinkhorn(ops):
    """plan (tr_sinkhorn) -> merge, then tr_soft_dweights / tr_soft_dsrc -> tr_sinkhorn_bwd, against float64 autograd from the scores.
    ds: the Sinkhorn bound as it stands (the backward never reads the plan; dW's own fp32 error, bounded by gamma_D sum |g| |src| and
    checked here, is part of what F's factor of 8 allows).  dsrc reads the forward's plan W^ = W (1 + d): the plan's exponent
    Z + u_T + v_T - norm collects 2 iters log-sum-exps, each within gamma_(max(P, K) + 16) + 8 u A of its exact value (A = the largest
    |Z| + |u| + |v|; log-sum-exp is 1-Lipschitz, so the errors add), and the final sum: |d| <= cW := (2 iters + 1) (gamma_(max(P,K)+16) + 8 u A)."""
    import oracle
    B, N, K, D, ldl, iters, eps = 2, 66, 17, 100, 24, 8, 0.5
    scores, x, src, g = _chain_inputs(91, B, N, K, D, ldl, 0.3)
    P = N - 1
    s64 = scores[:, 1:, :K].to(F64).clone().requires_grad_(True)
    r64 = src[:, 1:].to(F64).clone().requires_grad_(True)
    plan = oracle.sinkhorn_transport(s64.transpose(1, 2), eps, iters).transpose(1, 2)                 # [B, P, K]
    out = torch.einsum("bpk,bpd->bkd", plan, r64)
    g_s, g_src = torch.autograd.grad((out * g[:, 1:].to(F64)).sum(), (s64, r64))
    plan = plan.detach()

    wt, _ = ops.sinkhorn(scores.cuda(), K, eps, iters)
    x_out = ops.weighted_merge(wt, x.cuda(), src.cuda(), K)
    dwt, dsrc = ops.soft_merge_bwd(g.cuda(), wt, src.cuda())
    ds = ops.sinkhorn_bwd(scores.cuda(), dwt, K, eps, iters)
    assert float(ds[:, 0].float().abs().max()) == 0.0 and float(ds[:, :, K:].float().abs().max()) == 0.0 and float(dsrc[:, 0].abs().max()) == 0.0

    dw_ref, dw_mag = R.soft_dweights_ref(g, src, K)
    _assert_elementwise(dwt[:, 1:, :K], dw_ref, R.gamma(D) * dw_mag, "chain dW")
    A = float(s64.detach().abs().max()) / eps + 2 * (math.log(K + P) + float(s64.detach().abs().max()) / eps + math.log(max(K, P)))
    cW = (2 * iters + 1) * (R.gamma(max(P, K) + 16) + 8 * R.U32 * A)
    wfull = torch.zeros(B, N, K, dtype=F64)
    wfull[:, 1:] = plan
    _, dsrc_mag = R.soft_dsrc_ref(g, wfull, K)
    _assert_elementwise(dsrc[:, 1:], g_src, (R.gamma(K) + 1.01 * cW) * dsrc_mag, "chain dsrc")
    got = ds[:, 1:, :K].float()
    _assert_elementwise(got, g_s, R.BF16 * g_s.abs() + R.SINKHORN_F * R.image_rms(g_s), "chain ds")
    row, col = R.row_col_rel(got.cpu(), g_s)
    print(f"chain ds: worst token row {row:.3e}, worst centre column {col:.3e}")
    assert row <= R.BF16 and col <= R.BF16
    assert x_out.shape == (B, K + 1, D)
