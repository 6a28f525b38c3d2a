"""GPU parity of the family, head and embedding backward kernels at their edge shapes (csrc/tr_backward.hip: tr_head_bwd, tr_embed_bwd,
tr_evit_fuse_bwd, tr_tome_merge_bwd, tr_cluster_merge_bwd, tr_ats_scatter; csrc/tr_soft_bwd.hip: tr_rownorm_bwd), through the C ABI.

tests/test_hip_backward.py holds each of these kernels at one shape that avoids every tail, clamp and second loop pass.  The shapes here
(tests/_family_bwd_ref.py, with the reason for each next to its table) are the smallest that reach them.  The checker is the float64
closed form of _family_bwd_ref.py -- proven against float64 autograd on the CPU by tests/test_family_bwd_ref.py -- fed the same fp32 /
bf16-rounded operands as the kernel.

Bounds: the ones the single-shape tests of tests/test_hip_backward.py already apply, relative to the output's largest magnitude --
1e-5 (EViT g_out, ToMe g: one fp32 product), 1e-4 (dscore, dpos, dcls), 2e-4 (cluster g and d sw, dW), 1e-3 of |d sw| for d sb, 1e-5
absolute for the head's db, atol 1e-6 / rtol 1e-4 per element for rownorm.  `python -m tests._family_bwd_ref` shows what plain float32
evaluation costs at every shape here: at most 6.2e-6 (dscore at (1, 197, 195, 192)) against the 1e-4 bound, 1.3e-6 (d sw at
(1, 642, 640, 64)) against 2e-4, below 1e-6 everywhere else -- no bound had to be re-derived for a longer reduction.  Every bf16 copy is
held to 2^-8 of the reference's largest magnitude AND must be bit-equal to round-to-nearest-even of the fp32 output written next to it
(the kernels pack the very value they store).  tr_ats_scatter copies: exact.
"""
import functools

import pytest
import torch

from tests import _family_bwd_ref as R

pytestmark = pytest.mark.gpu

BF16 = 2.0 ** -8
GUARD = 256


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _cuda(case, *names):
    return [None if case[n] is None else case[n].cuda() for n in names]


def _err(got, want):
    """(max |got - want|, max |want|), float64 on the CPU"""
    want = want.double()
    return float((got.double().cpu() - want).abs().max()), float(want.abs().max())


def _assert_rel(got, want, bound, what):
    err, scale = _err(got, want)
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, relative {err / max(scale, 1e-300):.3e} (bound {bound:.1e})")
    assert err <= bound * scale, f"{what}: max err {err:.3e} > {bound:.1e} x {scale:.3e}"


def _assert_bf16_copy(gb, g32, want, what):
    _assert_rel(gb.float(), want, BF16, what)
    assert torch.equal(gb.view(torch.int16), g32.bfloat16().view(torch.int16)), f"{what}: not the round-to-nearest-even of the fp32 output"


def _prior(seed, shape, scale):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


# one case and one float64 reference per table row, shared by the parametrizations that use it; nothing below writes to them
@functools.lru_cache(maxsize=None)
def _head(B, C, D):
    c = R.head_case(B, C, D)
    return c, R.head_bwd_ref(**c)


@functools.lru_cache(maxsize=None)
def _embed(B, N, D):
    c = R.embed_case(B, N, D)
    return c, R.embed_bwd_ref(**c)


@functools.lru_cache(maxsize=None)
def _cluster(B, N, K, D, sb, weighted):
    c = R.cluster_case(B, N, K, D, sb, weighted=weighted)
    return c, R.cluster_merge_bwd_ref(c["g_in"], c["x0"], c["x1"], c["wtok"], c["assign"], c["sw"])


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,C,D", R.HEAD_CASES)
def test_head_bwd(ops, B, C, D, accumulate):
    """Row clamp (B % 4 != 0), column clamp (D = 200), every pattern of the five-deep class loop and its tail; (5, 24, 200) also takes
    tr_wgrad_bf16 through K = 200, a K that is a multiple of 8 but not of its 128-column tile."""
    c, (dxn_ref, dw_ref, db_ref) = _head(B, C, D)
    dl, w, xn = _cuda(c, "dlogits", "w", "xn")
    dxn, dw, db = ops.head_bwd(dl, w, xn)
    assert dxn.shape == (B, D) and dw.shape == (C, D) and db.shape == (C,)
    _assert_rel(dxn.float(), dxn_ref, BF16, "dxn")
    _assert_rel(dw, dw_ref, 2e-4, "dW")
    err = _err(db, db_ref)[0]
    assert err <= 1e-5, f"db: max err {err:.3e}"
    if accumulate:
        dw0, db0 = _prior(11, (C, D), _err(dw, dw_ref)[1]), _prior(12, (C,), float(db_ref.abs().max()))
        dxn2, dw2, db2 = ops.head_bwd(dl, w, xn, accumulate=True, dw=dw0.clone(), db=db0.clone())
        assert torch.equal(dxn2, dxn)
        for want in (dw0 + dw, dw0.double().cpu() + dw_ref):
            _assert_rel(dw2, want.cpu(), 2e-4, "dW (accumulate)")
        for want in (db0 + db, db0.double().cpu() + db_ref):
            assert _err(db2, want.cpu())[0] <= 1e-5, "db (accumulate)"


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,N,D", R.EMBED_CASES)
def test_embed_bwd(ops, B, N, D, accumulate):
    """Ragged last block (t >= nch and the clamped load index), empty batch lanes (B < 4, B % 4 != 0), accumulate on and off."""
    c, (dpos_ref, dcls_ref) = _embed(B, N, D)
    g, = _cuda(c, "g")
    # the destinations sit between guard words (a workgroup spans 64 chunks = 256 floats: what a missing tail test could overrun)
    pbuf, cbuf = torch.full((N * D + 2 * GUARD,), 7.25, device="cuda"), torch.full((D + 2 * GUARD,), 7.25, device="cuda")
    dpos, dcls = ops.embed_bwd(g, dpos=pbuf[GUARD:GUARD + N * D].view(N, D), dcls=cbuf[GUARD:GUARD + D])
    for buf, n in ((pbuf, N * D), (cbuf, D)):
        assert bool((buf[:GUARD] == 7.25).all()) and bool((buf[GUARD + n:] == 7.25).all()), "written outside the destination"
    scale = float(dpos_ref.abs().max())
    _assert_rel(dpos, dpos_ref, 1e-4, "dpos")
    assert _err(dcls, dcls_ref)[0] <= 1e-4 * scale, "dcls"
    assert torch.equal(dcls, dpos[0]), "d cls_token is the batch sum of row 0: the same sum d pos_embed[0] holds"
    fresh_pos, fresh_cls = ops.embed_bwd(g)                       # destinations of the wrapper's own
    assert torch.equal(fresh_pos, dpos) and torch.equal(fresh_cls, dcls)
    if accumulate:
        p0, c0 = _prior(13, (N, D), scale), _prior(14, (D,), scale)
        pbuf[GUARD:GUARD + N * D] = p0.reshape(-1)
        cbuf[GUARD:GUARD + D] = c0
        dpos2, dcls2 = ops.embed_bwd(g, accumulate=True, dpos=pbuf[GUARD:GUARD + N * D].view(N, D), dcls=cbuf[GUARD:GUARD + D])
        for buf, n in ((pbuf, N * D), (cbuf, D)):
            assert bool((buf[:GUARD] == 7.25).all()) and bool((buf[GUARD + n:] == 7.25).all()), "written outside the destination"
        for want in (p0 + fresh_pos, p0.double().cpu() + dpos_ref):
            _assert_rel(dpos2, want.cpu(), 1e-4, "dpos (accumulate)")
        for want in (c0 + fresh_cls, c0.double().cpu() + dcls_ref):
            assert _err(dcls2, want.cpu())[0] <= 1e-4 * float((p0.double().cpu() + dpos_ref).abs().max()), "dcls (accumulate)"


@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("B,N,K,D", R.EVIT_CASES)
def test_evit_fuse_bwd(ops, B, N, K, D, with_delta):
    """Every chunk count, fewer chunks than lanes (D = 64, 192), fewer complement tokens than waves, delta given and NULL; rows outside the
    complement (row 0 included) keep what they held."""
    c = R.evit_case(B, N, K, D, with_delta=with_delta)
    g_ref, ds_ref, touched = R.evit_fuse_bwd_ref(**c)
    x, delta, compl, scores, g_fused = _cuda(c, "x", "delta", "compl", "scores", "g_fused")
    g_out = torch.full((B, N, D), 7.25, device="cuda")
    gb_out = torch.full((B, N, D), -3.5, dtype=torch.bfloat16, device="cuda")
    dscore = ops.evit_fuse_bwd(x, delta, compl, scores, g_fused, g_out, gb_out)
    g_out, gb_out, dscore = g_out.cpu(), gb_out.cpu(), dscore.cpu()
    assert bool((g_out[~touched] == 7.25).all()) and bool((gb_out[~touched] == -3.5).all()), "a row outside 1 + compl was written"
    assert bool((dscore[~touched] == 0).all()), "dscore outside 1 + compl is not zero"
    _assert_rel(g_out[touched], g_ref[touched], 1e-5, "g_out")
    _assert_rel(dscore, ds_ref, 1e-4, "dscore")
    _assert_bf16_copy(gb_out[touched], g_out[touched], g_ref[touched], "gb_out")


@pytest.mark.parametrize("with_size", [True, False])
@pytest.mark.parametrize("B,N,r,D", R.TOME_CASES)
def test_tome_merge_bwd(ops, B, N, r, D, with_size):
    """Even and odd N, the largest r (only CLS unmerged), index loops past one 256-thread pass, shared destinations, size_in NULL."""
    c = R.tome_case(B, N, r, D, with_size=with_size)
    want = R.tome_merge_bwd_ref(**c)
    gm, size_in, size_out, unm, src, dst = _cuda(c, "g_merged", "size_in", "size_out", "unm", "src", "dst")
    g, gb = ops.tome_merge_bwd(gm, size_in, size_out, unm, src, dst, N)
    assert g.shape == (B, N, D)
    _assert_rel(g, want, 1e-5, "g")
    _assert_bf16_copy(gb.cpu(), g.cpu(), want, "gb")


@pytest.mark.parametrize("mode", ["unweighted", "weighted", "weighted_accumulate"])
@pytest.mark.parametrize("B,N,K,D,sb", R.CLUSTER_CASES)
def test_cluster_merge_bwd(ops, B, N, K, D, sb, mode):
    """K = 1, K = P, K past one 256-thread pass and K = 640, P > 640 (assignments walked in global memory), fewer workgroups per image
    (B x 8 > 2048), every chunk count; token weights of the order of the 1e-6 in W_c (score bias -13)."""
    weighted = mode != "unweighted"
    c, (g_ref, dsw_ref, dsb_ref) = _cluster(B, N, K, D, sb, weighted)
    g_in, x0, x1, wtok, assign, sw = _cuda(c, "g_in", "x0", "x1", "wtok", "assign", "sw")
    g, gb, dsw, dsb = ops.cluster_merge_bwd(g_in, x0, x1, wtok, assign, sw)
    _assert_rel(g, g_ref, 2e-4, "g")
    _assert_bf16_copy(gb.cpu(), g.cpu(), g_ref, "gb")
    if not weighted:
        assert dsw is None and dsb is None
        return
    s_sw = float(dsw_ref.abs().max())
    _assert_rel(dsw, dsw_ref, 2e-4, "dsw")
    err = _err(dsb, dsb_ref)[0]
    print(f"dsb: err {err:.3e} on |dsw| {s_sw:.3e}")
    assert err <= 1e-3 * s_sw, f"dsb: err {err:.3e} > 1e-3 x {s_sw:.3e}"
    if mode == "weighted_accumulate":
        w0, b0 = _prior(15, (D,), s_sw), _prior(16, (1,), s_sw)
        g2, gb2, dsw2, dsb2 = ops.cluster_merge_bwd(g_in, x0, x1, wtok, assign, sw, accumulate=True, dsw=w0.clone(), dsb=b0.clone())
        assert torch.equal(g2, g) and torch.equal(gb2, gb)
        for want in (w0 + dsw, w0.double().cpu() + dsw_ref):
            _assert_rel(dsw2, want.cpu(), 2e-4, "dsw (accumulate)")
        for want in (b0 + dsb, b0.double().cpu() + dsb_ref):
            assert _err(dsb2, want.cpu())[0] <= 1e-3 * s_sw, "dsb (accumulate)"


@pytest.mark.parametrize("B,N,Ks,D,kind", R.ATS_CASES)
def test_ats_scatter(ops, B, N, Ks, D, kind):
    """Ks = 1, Ks = N without padding, every row after CLS padded, a ragged last block (B Ks % 4 != 0), at every chunk count."""
    c = R.ats_case(B, N, Ks, D, kind)
    g_ref, d_ref = R.ats_scatter_ref(**c)
    g, dao, ids = _cuda(c, "g", "dao_s", "ids")
    gf, df = ops.ats_scatter(g, dao, ids, N)
    assert gf.dtype == torch.float32 and df.dtype == torch.bfloat16 and gf.shape == df.shape == (B, N, D)
    assert torch.equal(gf.double().cpu(), g_ref) and torch.equal(df.double().cpu(), d_ref)


@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("M,D", R.ROWNORM_CASES)
def test_rownorm_bwd(ops, M, D, with_db):
    """D < 64 (lanes without an element), D no multiple of 64, one row (three idle waves), the bf16 addend given and NULL."""
    c = R.rownorm_case(M, D, with_db=with_db)
    x, da, db = _cuda(c, "x", "da", "db")
    dx = ops.rownorm_bwd(x, da, db)
    torch.testing.assert_close(dx.cpu().double(), R.rownorm_bwd_ref(**c), atol=1e-6, rtol=1e-4)
