"""GPU tests of the training executor's glue kernels (csrc/tr_backward.hip, csrc/tr_norm.hip) at the op boundary: dropout / DropPath
scaling, casts, fixed-order partial sums, the out-of-place and fp32-output LayerNorms, copies, and the fused weight repack.  These
kernels have no arithmetic freedom, so every check is exact (torch.equal on values or bits) unless it says otherwise."""
import numpy as np
import pytest
import torch

from tests import _param_grad_ref as R
from tests import _reduce_ref as RR
from tests._reduce_ref import kernel_order_sum as _kernel_order_sum      # the reduces' fixed order, fp32 on the CPU

pytestmark = pytest.mark.gpu

SENTINEL = 7.25


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _keep_bytes(n, g):
    """Keep mask with bytes other than 0 / 1: any non-zero byte keeps."""
    vals = torch.tensor([0, 0x80, 0x01, 0xff, 0], dtype=torch.uint8)
    return vals[torch.randint(0, 5, (n,), generator=g)]


# ------------------------------------------------------------------------------------------------------------------- dropout / DropPath
@pytest.mark.parametrize("n", [8, 16, 2048, 2056, 2040, 50432 * 384])
def test_dropout_bf16(ops, n):
    """dst = keep ? bf16(src * mul) : 0 with ONE rounding, out of place and in place (the executor's form); elements behind n untouched."""
    g = _gen(n % 1000)
    src = torch.randn(n + 8, generator=g).bfloat16()
    keep = _keep_bytes(n + 8, g)
    mul = 1.0 / (1.0 - 0.15)
    want = torch.where(keep[:n] != 0, (src[:n].float() * torch.tensor(mul)).bfloat16(), torch.zeros((), dtype=torch.bfloat16))
    dst = torch.full((n + 8,), SENTINEL).bfloat16().cuda()
    ops.dropout(src.cuda(), keep.cuda(), mul, dst=dst, n=n)
    assert torch.equal(_bits(dst[:n].cpu()), _bits(want)), "out of place"
    assert torch.equal(dst[n:].cpu(), torch.full((8,), SENTINEL).bfloat16()), "elements behind n were written"
    inplace = src.clone().cuda()
    ops.dropout(inplace, keep.cuda(), mul, dst=inplace, n=n)
    assert torch.equal(_bits(inplace[:n].cpu()), _bits(want)), "in place"
    assert torch.equal(_bits(inplace[n:].cpu()), _bits(src[n:])), "in place: elements behind n were written"


@pytest.mark.parametrize("n", [4, 8, 1024, 1028, 1020, 3 * 197 * 384])
def test_dropout_f32(ops, n):
    g = _gen(n % 1000 + 1)
    src = torch.randn(n + 4, generator=g)
    keep = _keep_bytes(n + 4, g)
    mul = 1.0 / (1.0 - 0.3)
    want = torch.where(keep[:n] != 0, src[:n] * torch.tensor(mul), torch.zeros(()))
    dst = torch.full((n + 4,), SENTINEL).cuda()
    ops.dropout(src.cuda(), keep.cuda(), mul, dst=dst, n=n)
    assert torch.equal(_bits(dst[:n].cpu()), _bits(want)) and torch.equal(dst[n:].cpu(), torch.full((4,), SENTINEL))
    inplace = src.clone().cuda()
    ops.dropout(inplace, keep.cuda(), mul, dst=inplace, n=n)
    assert torch.equal(_bits(inplace[:n].cpu()), _bits(want)) and torch.equal(inplace[n:].cpu(), src[n:])


def test_dropout_refuses_ragged_counts_and_misaligned_pointers(ops):
    src = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    src32 = torch.zeros(64, device="cuda")
    keep = torch.ones(80, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="code -1"):
        ops.dropout(src, keep, 1.0, n=12)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.dropout(src32, keep, 1.0, n=6)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.dropout(src[4:36], keep, 1.0, dst=src[4:36], n=32)         # data 8 bytes off
    with pytest.raises(RuntimeError, match="code -2"):
        ops.dropout(src[:32], keep[4:36], 1.0, n=32)                     # mask 4 bytes off (needs 8)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.dropout(src32[:32], keep[2:34], 1.0, n=32)                   # fp32: mask 2 bytes off (needs 4)


@pytest.mark.parametrize("B,rows,D", [(1, 1, 8), (3, 197, 384), (5, 50, 192), (2, 577, 768), (256, 1, 8)])
def test_rowscale(ops, B, rows, D):
    g = _gen(B + rows + D)
    src = torch.randn(B, rows, D, generator=g).bfloat16()
    scale = torch.where(torch.rand(B, generator=g) < 0.3, torch.zeros(B), torch.full((B,), 1.0 / 0.9))
    scale[0] = 0.0
    want = (src.float() * scale[:, None, None]).bfloat16()
    got = ops.rowscale(src.cuda(), scale.cuda()).cpu()
    assert torch.equal(_bits(got), _bits(want))
    assert float(got[0].float().abs().max()) == 0.0
    inplace = src.clone().cuda()
    ops.rowscale(inplace, scale.cuda(), dst=inplace)
    assert torch.equal(_bits(inplace.cpu()), _bits(want))
    if D == 8:
        with pytest.raises(RuntimeError, match="code -1"):
            ops.rowscale(torch.zeros(B, rows, 12, dtype=torch.bfloat16, device="cuda"), scale.cuda())


# ------------------------------------------------------------------------------------------------------------------- casts, partial sums
def test_f32_to_bf16_rounds_to_nearest_even(ops):
    g = _gen(3)
    x = torch.randn(4096 + 4, generator=g) * torch.pow(torch.tensor(10.0), torch.randint(-6, 7, (4100,), generator=g).float())
    # values exactly on a tie between two bf16 neighbours (odd and even below), infinities, NaN, signed zero, a value that rounds to inf
    ties = torch.from_numpy(np.array([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x7f800000, 0xff800000, 0x7fc00000, 0x80000000, 0x7f7fffff,
                                      0x3f807fff, 0x3f808001, 0x40490fdb], dtype=np.uint32).view(np.float32).copy())
    x[:ties.numel()] = ties
    got = ops.f32_to_bf16(x.cuda()).cpu()
    want = x.bfloat16()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])
    with pytest.raises(RuntimeError, match="code -1"):
        ops.f32_to_bf16(torch.zeros(6, device="cuda"))


@pytest.mark.parametrize("count", [1, 2, 255, 1027, 4096])
@pytest.mark.parametrize("S", [1, 2, 37])
def test_reduce_partials(ops, S, count):
    """dst (+)= sum_s part[s], equal to the sequential fp32 sum over s with torch.equal: on values whose every partial sum is exact in fp32
    (multiples of 2^-10 below 32: any order gives the same bits, a dropped, doubled or misplaced partial does not), and on random fp32 data
    for S <= 2 (where no order is left).  At S = 37 on random data the kernel's own fixed order -- four interleaved lanes, csrc/tr_backward.hip
    partial_reduce_kernel -- is restated on the CPU and held bit for bit, and the sequential sum to fp32 accuracy."""
    g = _gen(S * 7 + count)
    exact = torch.randint(-32 * 1024, 32 * 1024, (S, count), generator=g).float() / 1024.0
    rand = torch.randn(S, count, generator=g)
    pre_exact = torch.randint(-1024, 1024, (count,), generator=g).float() / 1024.0
    pre_rand = torch.randn(count, generator=g)

    def seq(part, prefill):
        a = torch.zeros(count)
        for s in range(S):
            a = a + part[s]
        return a if prefill is None else a + prefill                       # the destination is added last

    for part, prefill in ((exact, pre_exact), (rand, pre_rand)):
        for acc in (False, True):
            dst = prefill.clone().cuda()
            got = ops.reduce_partials(part.cuda(), dst=dst, accumulate=acc).cpu()
            pf = prefill if acc else None
            if part is exact or S <= 2:
                assert torch.equal(got, seq(part, pf)), f"accumulate={acc}: differs from the sequential fp32 sum"
            else:
                assert torch.equal(got, _kernel_order_sum(part, pf)), f"accumulate={acc}: differs from the kernel's documented order"
                want = part.double().sum(0) + (0 if pf is None else pf.double())
                assert float((got.double() - want).abs().max()) <= 38 * 2.0 ** -24 * float(part.abs().sum(0).max() + 4)


WS_SENT = -12345.5          # fills the workspace of the test below: a partial the first kernel did not write shows


@pytest.mark.parametrize("M,D", RR.LN_REDUCE_SHAPES)
def test_layernorm_param_reduce_order(ops, M, D):
    """The pair reduce behind tr_layernorm_bwd in BOTH block layouts, bit for bit on Gaussian data: outside a deferred context the
    [grid][D] partials of d_gamma and d_beta stay in the caller's workspace; their sum is restated on the CPU in the order of the layout the
    call site must take (16 x 16 iff grid >= 64 and D <= 4096, 64 x 4 below) and compared with torch.equal, overwriting and accumulating
    (the prior is added last).  Where the layouts differ on these very partials (tests/test_reduce_ref.py: they do at every S >= 64 on
    the fp32 restatement of these inputs) the other layout's order fails this test."""
    c = R.ln_case(M, D)
    S = RR.ln_grid(M)
    lanes = RR.layout_lanes(S, D)
    g = _gen(M + D)
    for acc in (False, True):
        prior_g, prior_b = torch.randn(D, generator=g), torch.randn(D, generator=g)
        ws = torch.full((2 * S * D,), WS_SENT, device="cuda")
        _, _, dgamma, dbeta = ops.layernorm_bwd(c["dy"].cuda(), c["x"].cuda(), c["gamma"].cuda(), 1e-6, g_in=c["g_in"].cuda(), accumulate=acc,
                                                dgamma=prior_g.clone().cuda(), dbeta=prior_b.clone().cuda(), ws=ws)
        part = ws.cpu()
        assert not bool((part == WS_SENT).any()), "a partial was not written"
        pg, pb = part[:S * D].view(S, D), part[S * D:].view(S, D)
        want_g = _kernel_order_sum(pg, prior_g if acc else None, lanes)
        want_b = _kernel_order_sum(pb, prior_b if acc else None, lanes)
        other = RR.TALL if lanes == RR.FLAT else RR.FLAT
        differ = int((want_g != _kernel_order_sum(pg, prior_g if acc else None, other)).sum() +
                     (want_b != _kernel_order_sum(pb, prior_b if acc else None, other)).sum())
        print(f"M={M} D={D} S={S} lanes={lanes} accumulate={acc}: {differ} of {2 * D} sums would differ in the other layout")
        if S >= 64 and D >= 64:      # a third of the sums and more on the CPU restatement; D = 4 has eight sums in all: held there only
            assert differ >= 1, "the two layouts agree on these partials: the case cannot tell them apart"
        assert torch.equal(dgamma.cpu(), want_g), f"accumulate={acc}: d_gamma differs from the {lanes}-lane order"
        assert torch.equal(dbeta.cpu(), want_b), f"accumulate={acc}: d_beta differs from the {lanes}-lane order"


# ------------------------------------------------------------------------------------------------------------------- LayerNorm variants
def _ln_inputs(M, D, seed):
    g = _gen(seed)
    x = torch.randn(M, D, generator=g) * 2.0 + 0.5
    x[0] = 300.0 + 0.01 * torch.randn(D, generator=g)                      # |mean| >> std
    if M > 2:
        x[2] = -4.0                                                        # a constant row
    gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    d1 = torch.randn(M, D, generator=g).bfloat16()
    d2 = torch.randn(M, D, generator=g).bfloat16()
    return x, gamma, beta, d1, d2


@pytest.mark.parametrize("M,D", [(50, 384), (7, 192), (130, 768), (5, 1024), (33, 128)])
def test_layernorm_to_is_bitwise_the_in_place_form(ops, M, D):
    x, gamma, beta, d1, _ = _ln_inputs(M, D, M + D)
    for delta in (None, d1):
        xin = x.clone().cuda()
        y_ref = ops.layernorm(xin, gamma.cuda(), beta.cuda(), 1e-5, delta=None if delta is None else delta.cuda())
        # out of place, every operand a column slice of a wider tensor (ldx, ldxo, ldd != D)
        wide_x = torch.full((M, D + 8), SENTINEL).cuda()
        wide_x[:, 4:4 + D] = x.cuda()
        wide_o = torch.full((M, D + 12), SENTINEL).cuda()
        wide_d = torch.full((M, D + 4), SENTINEL).bfloat16().cuda()
        if delta is not None:
            wide_d[:, 4:] = delta.cuda()
        before = wide_x.clone()
        y = ops.layernorm_to(wide_x[:, 4:4 + D], wide_o[:, :D], gamma.cuda(), beta.cuda(), 1e-5, delta=None if delta is None else wide_d[:, 4:])
        assert torch.equal(_bits(y), _bits(y_ref)), "y differs from tr_layernorm_bf16"
        assert torch.equal(_bits(wide_o[:, :D]), _bits(xin)), "x_out differs from the in-place sum"
        assert torch.equal(_bits(wide_x), _bits(before)), "the input was written"
        assert torch.equal(wide_o[:, D:].cpu(), torch.full((M, 12), SENTINEL)), "x_out written beyond its D columns"


@pytest.mark.parametrize("M,D", [(50, 384), (7, 192), (130, 768), (33, 128)])
def test_layernorm_bf16_f32(ops, M, D):
    """bf16(y) bit-identical to tr_layernorm_bf16 / _to / tr_layernorm2_bf16 for 0 / 1 / 2 pending residuals, x_out in place, out of place
    and NULL; y itself against float64 LayerNorm of the fp32 sum the kernel normalises.  Tolerance of y: fp32 statistics of D <= 768
    values -- the mean and the variance each carry ~sqrt(D) * 2^-24 relative error of sum |x| resp. sum (x - mean)^2, so
    |y - ref| <= 1e-5 * |gamma| * (|x - mean| / std) + (on rows with |mean| >> std, where x - mean loses |mean| / std * 2^-24) the same
    factor more: 2e-5 * max|ref| + 2^-23 * |mean| / std * |gamma| per row."""
    x, gamma, beta, d1, d2 = _ln_inputs(M, D, M + D + 1)
    gc, bc = gamma.cuda(), beta.cuda()
    eps = 1e-6
    for nres in (0, 1, 2):
        da = d1.cuda() if nres >= 1 else None
        db = d2.cuda() if nres == 2 else None
        xs = x.clone().cuda()
        if nres == 0:
            y16 = ops.layernorm(xs, gc, bc, eps)
        elif nres == 1:
            y16 = ops.layernorm(xs, gc, bc, eps, delta=da)
        else:
            y16 = ops.layernorm2(xs, gc, bc, eps, da, db)
        if nres <= 1:
            xo = torch.empty(M, D, device="cuda")
            assert torch.equal(_bits(ops.layernorm_to(x.clone().cuda(), xo, gc, bc, eps, delta=da)), _bits(y16))
        for mode in ("null", "inplace", "out"):
            xin = x.clone().cuda()
            x_out = None if mode == "null" else (xin if mode == "inplace" else torch.full((M, D), SENTINEL).cuda())
            y = ops.layernorm_bf16_f32(xin, gc, bc, eps, delta=da, delta2=db, x_out=x_out)
            assert torch.equal(_bits(y.bfloat16()), _bits(y16)), f"{nres} residuals, x_out {mode}: bf16(y) differs from the bf16 norm"
            if mode == "null" or (mode == "out"):
                assert torch.equal(_bits(xin), _bits(x.cuda())), f"{nres} residuals, x_out {mode}: the input was written"
            if mode != "null":
                assert torch.equal(_bits(x_out), _bits(xs)), f"{nres} residuals, x_out {mode}: the sum differs"
        v = xs.cpu().double()                                              # the fp32 sum the kernel normalised
        mean, var = v.mean(-1, keepdim=True), v.var(-1, unbiased=False, keepdim=True)
        ref = (v - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
        tol = 2e-5 * ref.abs().amax(-1, keepdim=True) + 2.0 ** -23 * mean.abs() / torch.sqrt(var + eps) * gamma.abs().max().double()
        err = (y.cpu().double() - ref).abs()
        assert bool((err <= tol).all()), f"{nres} residuals: y off by {float((err - tol).max()):.3e} beyond the fp32-statistics tolerance"


# ------------------------------------------------------------------------------------------------------------------- copies
@pytest.mark.parametrize("n", [4, 1024, 1028, 3 * 197 * 384])
def test_residual_snapshot(ops, n):
    g = _gen(n % 997)
    x = torch.randn(n, generator=g)
    d32 = torch.randn(n, generator=g)
    d16 = d32.bfloat16()
    xc = x.cuda()
    assert torch.equal(ops.residual_snapshot(xc).cpu(), x)
    assert torch.equal(ops.residual_snapshot(xc, d16.cuda()).cpu(), x + d16.float())
    assert torch.equal(ops.residual_snapshot(xc, d32.cuda()).cpu(), x + d32)
    assert torch.equal(xc.cpu(), x)


@pytest.mark.parametrize("B,N", [(1, 1), (3, 197), (2, 577), (5, 256), (256, 3)])
def test_broadcast_rows(ops, B, N):
    src = torch.randn(N, generator=_gen(B + N))
    assert torch.equal(ops.broadcast_rows(src.cuda(), B).cpu(), src.expand(B, N))


# ------------------------------------------------------------------------------------------------------------------- fused weight repack
def _guarded(shape, dtype, off_elems):
    """A destination view `off_elems` elements into a sentinel-filled device buffer with guard space behind it."""
    n = shape[0] * shape[1]
    buf = torch.full((n + off_elems + 64,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[off_elems:off_elems + n].view(shape)


def test_cast_pack(ops):
    """Several items in one launch: rows, cols from {1, 63, 64, 65, 384, 1000, 1536} mixed, dst / dst_t NULL per item, cols % 4 != 0 and
    rows % 4 != 0 (the scalar straight / transposed stores), and sources / destinations that start 4 / 2 bytes into their buffers (the
    alignment tests of the vector paths); bytes around every destination untouched."""
    g = _gen(11)
    # (rows, cols, want dst, want dst_t, src offset in floats, dst offset in bf16 elements, dst_t offset)
    specs = [(384, 1536, True, True, 0, 0, 0), (1536, 384, True, True, 0, 0, 0), (1000, 384, True, True, 0, 0, 0), (64, 64, True, True, 0, 0, 0),
             (65, 63, True, True, 0, 0, 0), (63, 65, True, True, 0, 0, 0), (1, 384, True, True, 0, 0, 0), (384, 1, True, True, 0, 0, 0),
             (1, 1, True, True, 0, 0, 0), (64, 384, True, False, 0, 0, 0), (384, 64, False, True, 0, 0, 0),
             (384, 64, True, True, 1, 0, 0),           # src 4 bytes off: scalar loads
             (64, 384, True, True, 0, 1, 0),           # dst 2 bytes off: scalar straight stores
             (384, 384, True, True, 0, 0, 1),          # dst_t 2 bytes off: scalar transposed stores
             (1000, 1000, True, True, 0, 2, 2),        # dst / dst_t 4 bytes off (not 8-byte aligned)
             (65, 1000, True, True, 0, 0, 0), (1000, 65, True, True, 0, 0, 0), (130, 66, True, True, 0, 0, 0)]
    items, checks = [], []
    for rows, cols, wd, wt, so, do, to in specs:
        sbuf = torch.randn(rows * cols + so + 4, generator=g).cuda()
        src = sbuf[so:so + rows * cols].view(rows, cols)
        dbuf, dst = _guarded((rows, cols), torch.bfloat16, do) if wd else (None, None)
        tbuf, dst_t = _guarded((cols, rows), torch.bfloat16, to) if wt else (None, None)
        items.append((src, dst, dst_t))
        checks.append((src, dbuf, dst, do, tbuf, dst_t, to))
    ops.cast_pack(items)
    for i, (src, dbuf, dst, do, tbuf, dst_t, to) in enumerate(checks):
        n = src.numel()
        sent = torch.tensor(SENTINEL).bfloat16()
        if dst is not None:
            assert torch.equal(_bits(dst.cpu()), _bits(src.cpu().bfloat16())), f"item {i} {tuple(src.shape)}: dst"
            assert bool((dbuf[:do].cpu() == sent).all()) and bool((dbuf[do + n:].cpu() == sent).all()), f"item {i}: bytes around dst were written"
        if dst_t is not None:
            assert torch.equal(_bits(dst_t.cpu()), _bits(src.cpu().t().contiguous().bfloat16())), f"item {i} {tuple(src.shape)}: dst_t"
            assert bool((tbuf[:to].cpu() == sent).all()) and bool((tbuf[to + n:].cpu() == sent).all()), f"item {i}: bytes around dst_t were written"
