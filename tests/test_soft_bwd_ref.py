"""The closed-form float64 references of tests/_soft_bwd_ref.py against torch.autograd in float64, at every shape of the case tables (no
GPU): the forward of each op is the oracle's restatement -- torch.einsum for the merge, torch.softmax over the tokens, oracle.
sinkhorn_transport --, the loss is <output, upstream gradient>, and the closed form must equal the autograd gradient to 1e-10 of the
image's rms gradient.  This proves the references and the input builders before the GPU tests (tests/test_hip_soft_bwd_edges.py) compare
the kernels with them.  The builders' NaN fill (everything a kernel must not read) must never reach a reference output."""
import pytest
import torch

from tests import _soft_bwd_ref as R

F64 = torch.float64
TOL = 1e-10


def _close(got, want, what):
    """per element, against TOL x the rms of the image's gradient ([B, rows, cols])"""
    assert got.shape == want.shape and not bool(got.isnan().any()) and not bool(want.isnan().any()), what
    if want.numel() == 0:
        return
    err = (got - want).abs() / R.image_rms(want).clamp_min(1e-300)
    assert float(err.max()) <= TOL, f"{what}: closed form differs from autograd by {float(err.max()):.3e} of the image's rms"


def _nan_filled(t, K):
    return bool(t[:, 0].isnan().all()) and bool(t[:, :, K:].isnan().all()) and not bool(t[:, 1:, :K].isnan().any())


@pytest.mark.parametrize("B,N,K,D,ldl", R.SOFT_CASES)
def test_soft_merge_bwd_ref(B, N, K, D, ldl):
    c = R.soft_case(B, N, K, D, ldl)
    assert _nan_filled(c["wt"], K) and bool(c["g"][:, 0].isnan().all()) and bool(c["src"][:, 0].isnan().all())
    dw, dw_mag = R.soft_dweights_ref(c["g"], c["src"], K)
    dsrc, dsrc_mag = R.soft_dsrc_ref(c["g"], c["wt"], K)
    w = c["wt"][:, 1:, :K].to(F64).clone().requires_grad_(True)
    s = c["src"][:, 1:].to(F64).clone().requires_grad_(True)
    out = torch.einsum("bpk,bpd->bkd", w, s)                                   # sit.py:39, patchmerger.py:38, sinkhorn.py:83
    gw, gs = torch.autograd.grad((out * c["g"][:, 1:].to(F64)).sum(), (w, s))
    assert dw.shape == (B, N - 1, K) and dsrc.shape == (B, N - 1, D)
    _close(dw, gw, "dW"), _close(dsrc, gs, "dsrc")
    assert bool((dw.abs() <= dw_mag).all()) and bool((dsrc.abs() <= dsrc_mag).all()) and not bool(dw_mag.isnan().any() | dsrc_mag.isnan().any())


@pytest.mark.parametrize("B,N,K,ldl,ldo,real", R.SOFTMAX_CASES)
def test_token_softmax_bwd_ref(B, N, K, ldl, ldo, real):
    c = R.softmax_case(B, N, K, ldl, ldo, real)
    assert ldl != ldo and all(_nan_filled(c[n], K) for n in ("wt", "dwt", "logits"))
    wt = c["wt"].to(F64)
    if real:
        # the closed form on the float64 softmax itself (the builder's weights are these, rounded to fp32 for the kernel)
        wt[:, 1:, :K] = torch.softmax(c["logits"][:, 1:, :K].to(F64) * c["scale"], dim=1)
        assert float((wt[:, 1:, :K] - c["wt"][:, 1:, :K].to(F64)).abs().max()) <= 2.0 ** -24
        assert float((wt[:, 1:, :K].sum(1) - 1).abs().max()) <= 1e-12
    else:
        assert float((wt[:, 1:, :K].sum(1) - 1).abs().min()) > 0.05, "the arbitrary weights must not be normalised"
    ds, dscale, S, mag = R.token_softmax_bwd_ref(wt, c["dwt"], c["logits"], c["scale"], K)
    gl, gs = R.softmax_autograd(wt, c["dwt"], c["logits"], c["scale"], K, real)
    _close(ds, gl, "ds")
    assert abs(float(dscale) - float(gs)) <= TOL * float(mag), f"d scale: {float(dscale)} against {float(gs)}"
    assert not bool(S.isnan().any()) and float(mag) == float(mag)
    floor = R.token_softmax_floor(c["wt"], c["dwt"], c["scale"], K, S)
    assert floor.shape == ds.shape and not bool(floor.isnan().any()) and float(floor.min()) >= 0.0
    ds2, dscale2, _, mag2 = R.token_softmax_bwd_ref(wt, c["dwt"], None, c["scale"], K)
    assert torch.equal(ds2, ds) and dscale2 is None and mag2 is None


@pytest.mark.parametrize("B,N,K,iters,eps,ldl,ldo,zlds", R.SINKHORN_CASES)
def test_sinkhorn_bwd_ref(B, N, K, iters, eps, ldl, ldo, zlds):
    c = R.sinkhorn_case(B, N, K, iters, eps, ldl)
    assert _nan_filled(c["scores"], K) and _nan_filled(c["dplan"], K)
    ds = R.sinkhorn_bwd_ref(**c)
    gs = R.sinkhorn_autograd(**c)
    assert ds.shape == (B, N - 1, K)
    if R.sinkhorn_degenerate(N, K):
        # one centre or one token: the plan is the constant 1 (K = 1) or 1 / K (P = 1) whatever the scores
        assert float(ds.abs().max()) == 0.0 and float(gs.abs().max()) == 0.0
    else:
        assert float(gs.abs().min()) > 0.0
        _close(ds, gs, "ds")


def test_sinkhorn_table():
    """what the issue of the 160 KB switch and of the 1024-thread column loop needs from the table, and the measured F"""
    cases = {(c[1], c[2], c[3], c[4]): c for c in R.SINKHORN_CASES}
    assert len(cases) == len(R.SINKHORN_CASES) == 12
    assert cases[(289, 128, 3, 1.0)][7] and not cases[(290, 129, 3, 1.0)][7]
    assert cases[(1026, 3, 1, 1.0)][7] and not cases[(1026, 40, 2, 0.7)][7]
    assert {c[3] for c in R.SINKHORN_CASES} >= {1, R.SB_MAXIT}
    assert set(R.SINKHORN_F32_MEASURED) == {k for k in cases if not R.sinkhorn_degenerate(k[0], k[1])}
    assert any(c[0] > 1 for c in R.SINKHORN_CASES)
    for N, K, iters, eps, ldo in R.SINKHORN_REFUSED:
        assert iters < 1 or iters > R.SB_MAXIT or eps <= 0 or ldo < K


def test_sinkhorn_f32_measurement_holds():
    """torch's own float32 evaluation stays within the recorded table's factor: F = 8 x the worst recorded ratio covers a float32
    evaluation in another summation order (this build's torch included)"""
    m = R.sinkhorn_f32_measure()
    assert set(m) == set(R.SINKHORN_F32_MEASURED)
    assert max(v[0] for v in m.values()) <= R.SINKHORN_F / 2
    assert max(max(v[1], v[2]) for v in m.values()) <= 2.0 ** -8 / (1 + 2.0 ** -8) * 2.0 ** -8       # the slack of the row / column bound: 1.5e-5


@pytest.mark.parametrize("n", R.ADD_CASES)
def test_add_into_bf16_ref(n):
    c = R.add_case(n)
    want = R.add_into_bf16_ref(**c)
    assert want.dtype == torch.bfloat16 and want.shape == (n,) and not bool(want.isnan().any())
    # the fp32 sum is exact in float64, so rounding the float64 sum twice (to fp32, then to bf16) is the same computation
    assert torch.equal(want, (c["a"].double() + c["y"].double()).float().bfloat16())


def test_tables_cover_every_listed_value():
    P = {c[1] - 1 for c in R.SOFT_CASES}
    assert P == {1, 63, 64, 65, 130} and {c[2] for c in R.SOFT_CASES} == {1, 15, 16, 17, 63, 64, 65}
    assert {c[3] for c in R.SOFT_CASES} == {8, 24, 64, 100, 192}
    kinds = {("K" if ldl == K else "pad8" if ldl == R.pad8(K) else "pad8+8" if ldl == R.pad8(K) + 8 else "?") for _, _, K, _, ldl in R.SOFT_CASES}
    assert kinds == {"K", "pad8", "pad8+8"}
    assert {c[2] for c in R.SOFTMAX_CASES} == {1, 31, 32, 33, 70} and {c[1] - 1 for c in R.SOFTMAX_CASES} == {1, 7, 8, 9, 23}
    for _, _, K, ldl, ldo, _ in R.SOFTMAX_CASES:
        assert ldl != ldo and ldl >= K and ldo in (K, R.pad8(K), R.pad64(K))
    assert {("K" if ldo == K else "pad8" if ldo == R.pad8(K) else "pad64") for _, _, K, _, ldo, _ in R.SOFTMAX_CASES} >= {"K", "pad8", "pad64"}
    assert sum(c[5] for c in R.SOFTMAX_CASES) * 2 == len(R.SOFTMAX_CASES)
    for table in (R.SOFT_CASES, R.SOFTMAX_CASES, R.SINKHORN_CASES):
        assert all(1 <= c[0] <= 3 for c in table) and any(c[0] > 1 for c in table)
    assert R.ADD_CASES == [0, 1, 3, 4, 5, 1023, 1024, 1025, 1027, 4099]
