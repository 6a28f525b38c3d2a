"""GPU, op level: tr_token_pool and tr_token_pool_bwd (csrc/tr_pool.hip) against tests/_pool_ref.py's fp64 arithmetic.

tr_token_pool, per output element:  |err| <= (N + 4) * 2^-24 * (sum_n w_n |v_n| / sum_n w_n)  -- N - 2 additions of the sum, the two additions
behind v = (x + d1) + d2, the product and the division, each rounding relative to a partial result that sum_n w_n |v_n| bounds.  That counts
the roundings behind v relative to |v|, so the inputs keep those two additions from cancelling: image 0 and image 2 are large-mean rows
(100 + N(0,1) and -50 + N(0,1) with residuals of 0.25 N(0,1): a bf16 or otherwise short accumulator misses the bound by orders of magnitude),
image 1 is zero-mean on a grid (x in steps of 2^-6, the residuals in steps of 2^-4, all within +-8) where the additions behind v are exact and
the sum over the rows cancels.  Row 0 of x and entry 0 of the weights (the CLS token's) hold NaN: they are not part of the pool.
Shapes: one patch token (N = 2), odd counts, row groups partly filled (50) and evenly filled (65: two rows in each of the 32), 197 / 198, 577,
1025; every
width of the factories and 64; B = 1 and 3 (at these sizes the launch takes its 16-column slabs; B = 40 at D = 384 / 768 takes the 32- and
64-column ones, test_slab_widths_give_the_same_bits).
tr_token_pool_bwd: row 0 exactly 0, every other element within 3 * 2^-24 relative of the fp64 value (three roundings: the reciprocal and two
products; the weights are integers, so their sum is exact), every element of a NaN-prefilled g overwritten."""
import ctypes

import pytest
import torch

from tests import _pool_ref

pytestmark = pytest.mark.gpu

NS = [2, 3, 50, 65, 197, 198, 577, 1025]
DS = [64, 192, 384, 768]
MODES = [("none", None, 0), ("bf16", torch.bfloat16, 1), ("bf16", torch.bfloat16, 2), ("fp32", torch.float32, 1), ("fp32", torch.float32, 2)]
WEIGHTS = ["null", "ones", "sizes", "mask", "zero_image"]
U = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def ops():
    from tokenreduction_amd import ops
    return ops


def _inputs(N, D, seed, B=3):
    """x fp32 [B, N, D] and two residuals (fp32 values that bf16 holds exactly), as the module docstring describes them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, D, generator=g)
    d = [0.25 * torch.randn(B, N, D, generator=g) for _ in range(2)]
    d = [t.bfloat16().float() for t in d]
    for b in range(B):
        if b % 3 == 1:          # zero-mean, on a grid: exact additions behind v
            x[b] = (x[b] * 2.0).clamp(-8, 8).mul(64).round().div(64)
            for t in d:
                t[b] = (t[b] * 8.0).clamp(-8, 8).mul(16).round().div(16)
        else:
            x[b] += 100.0 if b % 3 == 0 else -50.0
    x[:, 0] = float("nan")
    return x, d


def _weight(kind, B, N, seed):
    g = torch.Generator().manual_seed(seed + 7)
    if kind == "null":
        return None
    if kind == "ones":
        w = torch.ones(B, N)
    elif kind == "mask":        # 0/1 with an all-zero tail (ATS padding)
        w = (torch.rand(B, N, generator=g) < 0.7).float()
        w[:, N - (N - 1) // 3:] = 0
        if N > 2:
            w[:, 1] = 1
    else:                       # integer sizes 1..7 (ToMe); zero_image: image B-2 (or 0) has no weight at all
        w = torch.randint(1, 8, (B, N), generator=g).float()
        if kind == "zero_image":
            w[max(B - 2, 0)] = 0
    w[:, 0] = float("nan")
    return w


def _dev(t, dtype=None):
    return None if t is None else t.to(dtype or t.dtype).cuda().contiguous()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", NS)
def test_token_pool_matches_fp64_within_the_derived_bound(ops, N, D):
    x, d = _inputs(N, D, 1000 * N + D)
    xd = _dev(x)
    worst = 0.0
    for label, dtype, nd in MODES:
        dd = [_dev(t, dtype) for t in d[:nd]] + [None] * (2 - nd)
        v = _pool_ref.stream(x, *[t for t in d[:nd]])
        for kind in WEIGHTS:
            w = _weight(kind, 3, N, N + D)
            want, bound = _pool_ref.pool(v, w), _pool_ref.pool_bound(v, w)
            got3 = ops.token_pool(xd, dd[0], dd[1], weight=_dev(w))
            got1 = ops.token_pool(xd[:1].contiguous(), None if dd[0] is None else dd[0][:1].contiguous(),
                                  None if dd[1] is None else dd[1][:1].contiguous(), weight=None if w is None else _dev(w[:1]))
            for got, ref, bnd in ((got3.cpu().double(), want, bound), (got1.cpu().double(), want[:1], bound[:1])):
                assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (label, nd, kind)
                err = (got - ref).abs()
                assert bool((err <= bnd).all()), (label, nd, kind, float((err - bnd).max()), float(err.max()))
                live = bnd > 0
                if bool(live.any()):
                    worst = max(worst, float((err[live] / bnd[live]).max()))
            if kind == "zero_image":
                assert bool((got3[1] == 0).all()) and not bool(got3[1].signbit().any())           # exact (positive) zeros, not NaN
            if kind == "mask" and N == 2:
                assert bool(((got3 == 0) | (_dev(w)[:, 1:2] > 0)).all())
    print(f"\n[N={N} D={D}] worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("N,D", [(2, 64), (65, 192), (197, 384), (198, 768), (1025, 384)])
def test_token_pool_bit_properties(ops, N, D):
    x, d = _inputs(N, D, 5 * N + D)
    xd, d1, d2 = _dev(x), _dev(d[0], torch.bfloat16), _dev(d[1], torch.bfloat16)
    for kind in ("null", "sizes", "mask"):
        w = _dev(_weight(kind, 3, N, N))
        a = ops.token_pool(xd, d1, d2, weight=w)
        b = ops.token_pool(xd, d1, d2, weight=w)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), kind                          # two launches, the same bits
        for i in range(3):                                                                         # an image pools to the same bits alone
            one = ops.token_pool(xd[i:i + 1].contiguous(), d1[i:i + 1].contiguous(), d2[i:i + 1].contiguous(),
                                 weight=None if w is None else w[i:i + 1].contiguous())
            assert torch.equal(one[0].view(torch.int32), a[i].view(torch.int32)), (kind, i)
    ones = torch.ones(3, N, device="cuda")
    for dd in ((None, None), (d1, None), (d1, d2), (_dev(d[0]), _dev(d[1]))):
        assert torch.equal(ops.token_pool(xd, *dd, weight=ones).view(torch.int32), ops.token_pool(xd, *dd).view(torch.int32))


@pytest.mark.parametrize("D", [384, 768])
def test_slab_widths_give_the_same_bits(ops, D):
    """B = 40: B * D / 64 reaches 256 workgroups of 64 columns at D = 768 and stays below at D = 384 (32 columns); a single image takes 16.
    The row groups and their order are the same in all three, so every image pools to the bits it has alone."""
    N = 70
    x, d = _inputs(N, D, D, B=40)
    xd, d1 = _dev(x), _dev(d[0], torch.bfloat16)
    w = _dev(_weight("sizes", 40, N, 3))
    all40 = ops.token_pool(xd, d1, weight=w)
    want, bound = _pool_ref.pool(_pool_ref.stream(x, d[0]), w.cpu()), _pool_ref.pool_bound(_pool_ref.stream(x, d[0]), w.cpu())
    assert bool(((all40.cpu().double() - want).abs() <= bound).all())
    for i in (0, 1, 17, 39):
        one = ops.token_pool(xd[i:i + 1].contiguous(), d1[i:i + 1].contiguous(), weight=w[i:i + 1].contiguous())
        assert torch.equal(one[0].view(torch.int32), all40[i].view(torch.int32)), i
    eight = ops.token_pool(xd[:8].contiguous(), d1[:8].contiguous(), weight=w[:8].contiguous())
    assert torch.equal(eight.view(torch.int32), all40[:8].view(torch.int32))


def test_bad_shapes_return_tr_err_shape_without_launching(ops):
    from tokenreduction_amd import _lib
    from tests import _launches
    lib = _lib.load()
    x = torch.zeros(2, 5, 64, device="cuda")
    out = torch.full((2, 64), 3.0, device="cuda")
    g = torch.full((2, 5, 64), 3.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def calls():
        for B, N, D in ((2, 1, 64), (2, 5, 32), (2, 5, 96), (0, 5, 64)):
            assert lib.tr_token_pool(x.data_ptr(), None, None, 0, None, out.data_ptr(), B, N, D, st) == -1
            assert lib.tr_token_pool_bwd(out.data_ptr(), None, g.data_ptr(), B, N, D, st) == -1
    assert _launches.labels(calls) == []
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((g == 3.0).all())
    with pytest.raises(RuntimeError, match="tr_token_pool"):
        ops.token_pool(torch.zeros(1, 1, 64, device="cuda"))
    with pytest.raises(ValueError, match="weight"):
        ops.token_pool(x, weight=torch.ones(2, 4, device="cuda"))


@pytest.mark.parametrize("N,D,B", [(2, 64, 1), (3, 192, 3), (65, 384, 3), (197, 384, 3), (198, 768, 1), (577, 64, 3), (1025, 384, 1)])
def test_token_pool_bwd(ops, N, D, B):
    g_ = torch.Generator().manual_seed(N * D + B)
    gp = torch.randn(B, D, generator=g_)
    for kind in WEIGHTS:
        w = _weight(kind, B, N, N + B)
        want = _pool_ref.pool_bwd(gp, N, None if w is None else w.nan_to_num(0.0))
        buf = torch.full((B, N, D), float("nan"), device="cuda")
        got = ops.token_pool_bwd(_dev(gp), N, weight=_dev(w), out=buf)
        assert got.data_ptr() == buf.data_ptr()
        got = got.cpu()
        assert bool(torch.isfinite(got).all()), kind                                               # every element of the NaN prefill overwritten
        assert bool((got[:, 0] == 0).all())
        err = (got.double() - want).abs()
        assert bool((err <= 3 * U * want.abs()).all()), (kind, float((err / want.abs().clamp_min(1e-300)).max() / U))
        if kind == "zero_image":
            assert bool((got[max(B - 2, 0)] == 0).all())
        again = ops.token_pool_bwd(_dev(gp), N, weight=_dev(w))
        assert torch.equal(again.cpu().view(torch.int32), got.view(torch.int32))


def test_token_pool_library_op_and_its_autograd(ops):
    import tokenreduction_amd.torch_ops  # noqa: F401
    OPS = torch.ops.tokenreduction_amd
    x, _ = _inputs(50, 192, 9)
    x[:, 0] = 1.0
    w = _weight("sizes", 3, 50, 1).nan_to_num(1.0)
    xd = x.cuda().requires_grad_(True)
    out = OPS.token_pool(xd, w.cuda())
    assert torch.equal(out.detach().view(torch.int32), ops.token_pool(x.cuda(), weight=w.cuda()).view(torch.int32))
    G = torch.randn(3, 192, generator=torch.Generator().manual_seed(2)).cuda()
    out.backward(G)
    assert torch.equal(xd.grad.view(torch.int32), ops.token_pool_bwd(G, 50, weight=w.cuda()).view(torch.int32))
    xr = x.double().requires_grad_(True)
    (_pool_ref.pool(xr, w) * G.cpu().double()).sum().backward()
    assert bool(((xd.grad.cpu().double() - xr.grad).abs() <= 3 * U * xr.grad.abs()).all())
    out = OPS.token_pool(xd.detach(), None)
    assert torch.equal(out.view(torch.int32), ops.token_pool(x.cuda()).view(torch.int32))
