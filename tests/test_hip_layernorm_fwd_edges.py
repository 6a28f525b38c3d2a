"""GPU parity of the forward LayerNorm kernels at their shape and value edges, in every form the executors call them (csrc/tr_norm.hip:
layernorm_kernel, layernorm_half_kernel, gather_layernorm_kernel; csrc/tr_rowops.h: ln_row_store), through the C ABI by way of the ops
wrappers.

This is where the suite's bit-identity chain is anchored: tr_lnlin, both fused-Mlp LN forms, tr_final_tokens_f32 and the out-of-place /
two-residual / fp32-output forms are held elsewhere only as bit-identical to ops.layernorm / ops.layernorm_f32, which
tests/test_hip_ops.py holds at five shapes, one Gaussian and one eps.  The shapes here (tests/_ln_fwd_ref.py, with the reason for each
next to its table) reach every chunk count at both of its ends, rows narrower than a wave, every workgroup tail of both kernels, the fused
EViT row's second and third 64-token trip and every remainder of its four-row step; the values are seven families (Gaussian, large mean,
one-hot, outlier channels, tiny, huge, constant) rotated through every row position; eps is 1e-6 and 1e-5.  The checker is the float64
closed form of _ln_fwd_ref.py -- proven against torch.nn.functional.layer_norm on the CPU by tests/test_ln_fwd_ref.py -- fed the same
fp32 / bf16 operands as the kernel.  Every form is compared with that reference, not with another form.

Everything the library may write (y, x_out, the stream x) is a slice of a sentinel-filled buffer with GUARD elements on either side;
nothing outside may change, nor the gap columns between strided rows, nor the rows a strided launch steps over.  Every case runs twice
and must be bitwise equal.

Bounds (tests/_ln_fwd_ref.py; `python -m tests._ln_fwd_ref` prints the measurements): fp32 outputs within LN_FWD_BOUND = 5.6e-5 of THAT
ROW's largest reference magnitude, 4 x the worst row of plain float32 evaluation against float64 over all these inputs (1.34e-05: the
large-mean family at D = 8; every other family below 6e-7); bf16 outputs bit-equal to the round-to-nearest-even of the fp32-output form
and within 1.01 bf16 ulp + 1e-4 of the reference (the bound of tests/test_hip_ops.py); constant rows exactly bf16(beta); stream writes and
gathered rows torch.equal; EViT's fused row within FUSE_BOUND = 4.0e-6 of its largest magnitude (4 x 9.85e-07, float32 token-after-token
accumulation against float64 at 288 dropped tokens).

Everything kept (K = N - 1) with the fused row asked for: ops.gather_layernorm used to hand the library a NULL complement (an empty
tensor has no storage), the library laid K + 1 rows out in a buffer made for K + 2, and the caller read misplaced and unwritten rows.
Pinned: K + 2 rows, the fused row exactly zero, its y exactly bf16(beta) -- what the C executor, whose complement pointer is never NULL,
always did.
"""
import functools

import pytest
import torch

from tests import _ln_fwd_ref as R

pytestmark = pytest.mark.gpu

BF16_ULP = 2.0 ** -8
GUARD = 256
SENT = 7.25                 # around every output, in the gaps of strided rows and in the rows a strided launch steps over
BF = torch.bfloat16
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------------------ helpers
class Guarded:
    """rows x ld elements between two guards of a sentinel-filled buffer; `rows` [rows, cols] is what the library is handed (the first
    `cols` columns of every row: contiguous when ld == cols), `inner` what it holds at the start"""

    def __init__(self, rows, cols, dtype=F32, inner=None, ld=None, fill=SENT):
        self.r, self.c, self.ld, self.fill = int(rows), int(cols), int(cols if ld is None else ld), fill
        self.buf = torch.full((self.r * self.ld + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.full = self.buf[GUARD:GUARD + self.r * self.ld].view(self.r, self.ld)
        self.rows = self.full if self.ld == self.c else self.full[:, :self.c]
        if inner is not None:
            self.rows.copy_(inner.reshape(self.r, self.c))

    def check(self, what):
        n = self.r * self.ld
        assert bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + n:] == self.fill).all()), f"{what}: written outside"
        if self.ld != self.c:
            assert bool((self.full[:, self.c:] == self.fill).all()), f"{what}: a gap between two rows was written"
        return self

    def untouched(self):
        return bool((self.full == self.fill).all())

    def get(self):
        return self.rows.detach().cpu().clone()


def _assert_rows(got, want, bound, what):
    """every row within `bound` of that row's largest reference magnitude"""
    want = want.double().cpu().reshape(-1, want.shape[-1])
    got = got.double().cpu().reshape(-1, want.shape[-1])
    err, scale = (got - want).abs().amax(-1), want.abs().amax(-1)
    rel = err / scale.clamp_min(1e-300)
    w = int(rel.argmax())
    print(f"{what}: worst row {w}: err {float(err[w]):.3e}, row scale {float(scale[w]):.3e}, relative {float(rel[w]):.3e} (bound {bound:.1e})")
    assert bool((err <= bound * scale).all()), f"{what}: row {w} off by {float(rel[w]):.3e} of its largest magnitude (bound {bound:.1e})"


def _assert_bf16(got, want, what):
    """tests/test_hip_ops.py::assert_close_bf16(ulps=1.01, abs_floor=1e-4) against the float64 reference"""
    got, want = got.double().cpu().reshape(want.shape), want.double().cpu()
    tol = R.BF16_ULPS * BF16_ULP * want.abs() + R.BF16_ABS
    bad = (got - want).abs() > tol
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max abs err {float((got - want).abs().max()):.3e}"


def _bits(t):
    return t.view(torch.int16)


def _assert_rounding(yb, y32, what):
    assert torch.equal(_bits(yb.cpu()), _bits(y32.cpu().bfloat16().reshape(yb.shape))), f"{what}: not the round-to-nearest-even of the fp32-output form"


@functools.lru_cache(maxsize=None)
def _params(D):
    g, b = R.ln_params(D)
    return g.cuda(), b.cuda()


def _twice(run):
    """run() -> tuple of CPU tensors; twice, bitwise equal"""
    a, b = run(), run()
    assert len(a) == len(b) and all(torch.equal(_bits(p) if p.dtype == BF else p, _bits(q) if q.dtype == BF else q) for p, q in zip(a, b)), \
        "not bitwise reproducible"
    return a


def _const_rows(c):
    return [r for r, f in enumerate(c["fam"]) if f == "const"]


# ------------------------------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("M,D,offsets", R.LN_SHAPES, ids=[f"{M}x{D}" for M, D, _ in R.LN_SHAPES])
def test_layernorm_shapes(ops, M, D, offsets, eps):
    """tr_layernorm_bf16_f32, tr_layernorm_bf16 and tr_layernorm_f32 on the same rows at every chunk-count boundary, rows narrower than a wave
    and every workgroup tail of both kernels, every value family in every row position (the tiny-M cases once per offset), two eps."""
    g, b = _params(D)
    for o in offsets:
        c = R.ln_case(M, D, o)
        ref = R.ln_ref(c["x"], c["gamma"], c["beta"], eps)

        def run():
            X = Guarded(M, D, inner=c["x"])
            Y32, YB, YF = Guarded(M, D), Guarded(M, D, BF), Guarded(M, D)
            assert ops.layernorm_bf16_f32(X.rows, g, b, eps, y=Y32.rows).data_ptr() == Y32.rows.data_ptr()
            ops.layernorm(X.rows, g, b, eps, y=YB.rows)
            ops.layernorm_f32(X.rows, g, b, eps, y=YF.rows)
            for G, what in ((X, "x"), (Y32, "y (bf16 path, fp32 out)"), (YB, "y (bf16)"), (YF, "y (fp32 path)")):
                G.check(what)
            assert torch.equal(X.get(), c["x"]), "a LayerNorm without a pending residual wrote the stream"
            return Y32.get(), YB.get(), YF.get()
        y32, yb, yf = _twice(run)
        what = f"offset {o}"
        _assert_rows(y32, ref, R.LN_FWD_BOUND, f"{what}: tr_layernorm_bf16_f32")
        _assert_rows(yf, ref, R.LN_FWD_BOUND, f"{what}: tr_layernorm_f32")
        _assert_rounding(yb, y32, f"{what}: tr_layernorm_bf16")
        _assert_bf16(yb, ref, f"{what}: tr_layernorm_bf16")
        rows = _const_rows(c)
        if rows:
            beta = c["beta"].expand(len(rows), D)
            assert torch.equal(y32[rows], beta) and torch.equal(yf[rows], beta), f"{what}: a constant row is not exactly beta"
            assert torch.equal(_bits(yb[rows]), _bits(beta.bfloat16())), f"{what}: a constant row is not exactly bf16(beta)"


# ------------------------------------------------------------------------------------------------------------------------ 2. forms
def _check_pair(y32, yb, ref, what):
    """the fp32-output form against the reference, the bf16 form as its rounding and against the reference"""
    _assert_rows(y32, ref, R.LN_FWD_BOUND, f"{what} (fp32 out)")
    _assert_rounding(yb, y32, what)
    _assert_bf16(yb, ref, what)


FORMS = ["delta_in_place", "two_deltas", "no_stream_write", "to_with_delta", "to_copy", "cls_rows_2", "cls_rows_69", "f32_delta"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("M,D", R.LN_FORM_SHAPES)
def test_layernorm_forms(ops, M, D, eps, form):
    """The forms the executors call, each against the float64 reference of the stream it must normalise, the stream it stores torch.equal to
    the fp32 sum: a pending bf16 residual in place; two; no stream write; out of place into strided rows with and without a residual (then a
    copy; the source never written); the CLS rows of [M, N, D] at stride N D; the fp32 residual of the fp32 path.  Strides other than D
    reach ldxo, ldd and ldd2."""
    g, b = _params(D)
    for o in R.LN_FORM_OFFSETS:
        c = R.ln_case(M, D, o)
        x, d1, d2, df = c["x"], c["d1"].cuda(), c["d2"].cuda(), c["df"].cuda()

        def ref_of(kind):
            s = R.stream_of(c, kind)
            return s, R.ln_ref(s, c["gamma"], c["beta"], eps)
        what = f"{form}, offset {o}"
        if form == "delta_in_place":
            s, ref = ref_of("d1")

            def run():
                X, X2, YB, Y32 = Guarded(M, D, inner=x), Guarded(M, D, inner=x), Guarded(M, D, BF), Guarded(M, D)
                ops.layernorm(X.rows, g, b, eps, delta=d1, y=YB.rows)
                ops.layernorm_bf16_f32(X2.rows, g, b, eps, delta=d1, x_out=X2.rows, y=Y32.rows)
                for G in (X, X2, YB, Y32):
                    G.check(what)
                return X.get(), X2.get(), YB.get(), Y32.get()
            xs, xs2, yb, y32 = _twice(run)
            assert torch.equal(xs, s) and torch.equal(xs2, s), f"{what}: the stream is not x + d"
            _check_pair(y32, yb, ref, what)
        elif form == "two_deltas":
            s, ref = ref_of("d12")

            def run():
                X, YB = Guarded(M, D, inner=x), Guarded(M, D, BF)
                ops.layernorm2(X.rows, g, b, eps, d1, d2, y=YB.rows)
                # the fp32-output form out of place, every operand at a stride of its own
                X2, XO, Y32 = Guarded(M, D, inner=x, ld=D + 12), Guarded(M, D, ld=D + 4), Guarded(M, D)
                D1, D2 = Guarded(M, D, BF, inner=d1, ld=D + 4), Guarded(M, D, BF, inner=d2, ld=D + 8)
                ops.layernorm_bf16_f32(X2.rows, g, b, eps, delta=D1.rows, delta2=D2.rows, x_out=XO.rows, y=Y32.rows)
                for G in (X, YB, X2, XO, Y32, D1, D2):
                    G.check(what)
                assert torch.equal(X2.get(), x), f"{what}: the source of an out-of-place call was written"
                return X.get(), XO.get(), YB.get(), Y32.get()
            xs, xo, yb, y32 = _twice(run)
            assert torch.equal(xs, s) and torch.equal(xo, s), f"{what}: the stream is not (x + d1) + d2"
            _check_pair(y32, yb, ref, what)
        elif form == "no_stream_write":
            for kind, dd in (("d1", (d1, None)), ("d12", (d1, d2))):
                s, ref = ref_of(kind)

                def run():
                    X, YB, Y32 = Guarded(M, D, inner=x), Guarded(M, D, BF), Guarded(M, D)
                    ops.layernorm2(X.rows, g, b, eps, dd[0], dd[1], write_x=False, y=YB.rows)
                    ops.layernorm_bf16_f32(X.rows, g, b, eps, delta=dd[0], delta2=dd[1], x_out=None, y=Y32.rows)
                    for G in (X, YB, Y32):
                        G.check(what)
                    return X.get(), YB.get(), Y32.get()
                xs, yb, y32 = _twice(run)
                assert torch.equal(xs, x), f"{what}: the stream was written"
                _check_pair(y32, yb, ref, f"{what}, {kind}")
        elif form in ("to_with_delta", "to_copy"):
            s, ref = ref_of("d1" if form == "to_with_delta" else "x")

            def run():
                X, XO, YB = Guarded(M, D, inner=x, ld=D + 8), Guarded(M, D, ld=D + 4), Guarded(M, D, BF)
                D1 = Guarded(M, D, BF, inner=d1, ld=D + 4)
                ops.layernorm_to(X.rows, XO.rows, g, b, eps, delta=D1.rows if form == "to_with_delta" else None, y=YB.rows)
                XO2, Y32 = Guarded(M, D, ld=D + 4), Guarded(M, D)
                ops.layernorm_bf16_f32(X.rows, g, b, eps, delta=D1.rows if form == "to_with_delta" else None, x_out=XO2.rows, y=Y32.rows)
                for G in (X, XO, XO2, YB, Y32, D1):
                    G.check(what)
                assert torch.equal(X.get(), x), f"{what}: the source was written"
                return XO.get(), XO2.get(), YB.get(), Y32.get()
            xo, xo2, yb, y32 = _twice(run)
            assert torch.equal(xo, s) and torch.equal(xo2, s), f"{what}: x_out is not the sum (without a residual: a copy)"
            _check_pair(y32, yb, ref, what)
        elif form.startswith("cls_rows"):
            N = int(form.rsplit("_", 1)[1])
            assert N in R.LN_CLS_N
            for kind in ("x", "d1"):
                s, ref = ref_of(kind)

                def run():
                    # [M, N, D]: the CLS row of every image holds the case's row, every other row the sentinel
                    X, D1 = Guarded(M, D, inner=x, ld=N * D), Guarded(M, D, BF, inner=d1, ld=N * D)
                    YB, Y32 = Guarded(M, D, BF), Guarded(M, D)
                    dl = D1.full.view(M, N, D) if kind == "d1" else None
                    ops.layernorm_bf16_f32(X.rows, g, b, eps, delta=None if dl is None else D1.rows, x_out=None, y=Y32.rows)
                    ops.layernorm(X.full.view(M, N, D), g, b, eps, rows=M, ldx=N * D, delta=dl, ldd=N * D, y=YB.rows)
                    for G in (X, D1, YB, Y32):
                        G.check(what)             # the gap check: rows 1 .. N - 1 of every image keep the sentinel
                    return X.get(), YB.get(), Y32.get()
                xs, yb, y32 = _twice(run)
                assert torch.equal(xs, s), f"{what}, {kind}: the CLS rows of the stream are not the sum"
                _check_pair(y32, yb, ref, f"{what}, {kind}")
        else:
            assert form == "f32_delta"
            s, ref = ref_of("df")

            def run():
                X, YF = Guarded(M, D, inner=x), Guarded(M, D)
                X2, DF, YF2 = Guarded(M, D, inner=x, ld=D + 4), Guarded(M, D, inner=df, ld=D + 8), Guarded(M, D)
                ops.layernorm_f32(X.rows, g, b, eps, delta=df, y=YF.rows)
                ops.layernorm_f32(X2.rows, g, b, eps, delta=DF.rows, y=YF2.rows)
                for G in (X, YF, X2, DF, YF2):
                    G.check(what)
                return X.get(), X2.get(), YF.get(), YF2.get()
            xs, xs2, yf, yf2 = _twice(run)
            assert torch.equal(xs, s) and torch.equal(xs2, s), f"{what}: the stream is not x + d"
            _assert_rows(yf, ref, R.LN_FWD_BOUND, what)
            _assert_rows(yf2, ref, R.LN_FWD_BOUND, f"{what}, strided")


# ------------------------------------------------------------------------------------------------------------------------ 3. gather
@functools.lru_cache(maxsize=8)
def _gather_gpu(B, N, K, D):
    c = R.gather_case(B, N, K, D)
    return {k: (v.int() if k in ("idx", "compl") else v).cuda() for k, v in c.items()}


def _gather_run(ops, cg, B, N_out, D, f32, delta, fuse, idx=True):
    XO, Y = Guarded(B * N_out, D), Guarded(B * N_out, D, F32 if f32 else BF)
    dl = None if delta is None else cg["df" if f32 else "d"]
    ops.gather_layernorm(cg["x"], cg["idx"] if idx else None, cg["compl"] if fuse else None, cg["scores"] if fuse else None, cg["gamma"],
                         cg["beta"], 1e-6, delta=dl, x_out=XO.rows.view(B, N_out, D), y=Y.rows.view(B, N_out, D), f32=f32)
    XO.check("x_out"), Y.check("y")
    return XO.get().view(B, N_out, D), Y.get().view(B, N_out, D)


def _gather_params():
    out = []
    for fuse, cases in ((True, R.GATHER_CASES), (False, R.GATHER_PLAIN_CASES)):
        out += [pytest.param(B, N, K, fuse, id=f"{B}x{N}-keep{K}-{'fused' if fuse else 'plain'}") for B, N, K in cases]
    return out


@pytest.mark.parametrize("with_delta", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("D", R.GATHER_D)
@pytest.mark.parametrize("B,N,K,fuse", _gather_params())
def test_gather_layernorm_edges(ops, B, N, K, fuse, D, f32, with_delta):
    """tr_gather_layernorm_bf16 / _f32 with and without a pending residual: the gathered rows bit-exact at every tail of the four-row
    workgroups; EViT's fused row within FUSE_BOUND of the float64 weighted sum at every remainder of its four-row step, on both sides of
    the second 64-token trip, at 288 dropped tokens (the 384^2 image) and in a third trip -- weights with zeros and one dominant token;
    y against the LayerNorm of the rows the kernel stored."""
    c, cg = R.gather_case(B, N, K, D), _gather_gpu(B, N, K, D)
    delta = None if not with_delta else ("f32" if f32 else "bf16")
    src = R.gather_source(c, delta)
    want, want_fused = R.gather_ref(src, c["idx"], c["scores"] if fuse else None)
    N_out = K + 1 + int(fuse)
    got_x, got_y = _twice(lambda: _gather_run(ops, cg, B, N_out, D, f32, delta, fuse))
    assert torch.equal(got_x[:, :K + 1], want[:, :K + 1].float()), "a gathered row is not a copy of its source row"
    if fuse:
        _assert_rows(got_x[:, K + 1], want_fused, R.FUSE_BOUND, f"fused row ({N - 1 - K} dropped)")
    ref = R.ln_ref(got_x, c["gamma"], c["beta"], 1e-6)
    if f32:
        _assert_rows(got_y, ref, R.LN_FWD_BOUND, "y")
    else:
        _assert_bf16(got_y, ref, "y")
        if D != R.LN_HALF_D:        # ln_row_store is the tail of layernorm_kernel too (at D = 384 that entry point runs the half kernel)
            g, b = _params(D)
            y32 = ops.layernorm_bf16_f32(got_x.view(-1, D).cuda(), g, b, 1e-6)
            _assert_rows(y32, ref, R.LN_FWD_BOUND, "y (fp32-output form of the stored rows)")
            _assert_rounding(got_y.view(-1, D), y32, "y")


@pytest.mark.parametrize("with_delta", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("B,N,D", R.GATHER_ALL_ROWS)
def test_gather_kernel_without_ids_is_the_plain_layernorm(ops, B, N, D, f32, with_delta):
    """idx = NULL: the LayerNorm of all N rows of every image through the gather kernel, one case per chunk count, the value families as
    rows; with x_out the rows (plus the residual) are stored, torch.equal."""
    c = R.ln_case(B * N, D)
    g, b = _params(D)
    dl = None if not with_delta else (c["df"] if f32 else c["d1"])
    s = c["x"] if dl is None else R.stream_sum(c["x"], dl)
    ref = R.ln_ref(s, c["gamma"], c["beta"], 1e-6)
    cg = dict(x=c["x"].cuda().view(B, N, D), d=c["d1"].cuda().view(B, N, D), df=c["df"].cuda().view(B, N, D), gamma=g, beta=b)
    got_x, got_y = _twice(lambda: _gather_run(ops, cg, B, N, D, f32, dl, False, idx=False))
    assert torch.equal(got_x.view(-1, D), s), "x_out is not the stream"
    if f32:
        _assert_rows(got_y, ref, R.LN_FWD_BOUND, "y")
    else:
        _assert_bf16(got_y.view(-1, D), ref, "y")
        rows = _const_rows(c)
        if dl is None and rows:
            assert torch.equal(_bits(got_y.view(-1, D)[rows]), _bits(c["beta"].expand(len(rows), D).bfloat16())), "a constant row is not bf16(beta)"
    Y = Guarded(B * N, D, F32 if f32 else BF)
    x_out, y = ops.gather_layernorm(cg["x"], None, None, None, g, b, 1e-6, delta=None if dl is None else cg["df" if f32 else "d"],
                                    y=Y.rows.view(B, N, D), f32=f32)
    Y.check("y")
    assert x_out is None and torch.equal(Y.get().view(B, N, D), got_y), "without x_out the same y"


# ------------------------------------------------------------------------------------------------------------------------ 4. K = N - 1
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("B,N,D", R.GATHER_KEPT_ALL)
def test_gather_fused_with_nothing_dropped(ops, B, N, D, f32):
    """K = N - 1, compl of shape [B, 0], the fused row asked for: K + 2 rows per image, the gathered rows copies, the fused row exactly zero
    (an empty sum) and its y exactly beta (bf16(beta) on the bf16 path) -- see the module docstring for what the wrapper did before."""
    K = N - 1
    c, cg = R.gather_case(B, N, K, D), _gather_gpu(B, N, K, D)
    assert cg["compl"].shape == (B, 0)
    got_x, got_y = _twice(lambda: _gather_run(ops, cg, B, K + 2, D, f32, None, True))
    assert got_x.shape == (B, K + 2, D) and got_y.shape == (B, K + 2, D)
    assert torch.equal(got_x[:, :K + 1], R.gather_ref(c["x"], c["idx"])[0].float()), "a gathered row is not a copy of its source row"
    assert bool((got_x[:, K + 1] == 0).all()), "the fused row of an empty complement is not zero"
    beta = c["beta"].expand(B, D)
    assert torch.equal(got_y[:, K + 1], beta) if f32 else torch.equal(_bits(got_y[:, K + 1]), _bits(beta.bfloat16())), "y of the zero row is not beta"
    ref = R.ln_ref(got_x, c["gamma"], c["beta"], 1e-6)
    if f32:
        _assert_rows(got_y, ref, R.LN_FWD_BOUND, "y")
    else:
        _assert_bf16(got_y, ref, "y")


# ------------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_write_nothing(ops):
    """D % 4 != 0, D = 1028, ldxo < D, a second residual without the first, tr_layernorm2_bf16 without any: the library's error and
    message, nothing launched -- y, x_out and the stream keep what they held.  (A second residual on the fp32 path cannot be asked for:
    tr_layernorm_f32 has no such parameter.)"""
    M = 5
    held = []

    def bufs(D, ld=None):
        X, XO, YB, Y32 = Guarded(M, D, ld=ld), Guarded(M, D), Guarded(M, D, BF), Guarded(M, D)
        held.extend([X, XO, YB, Y32])
        return X, XO, YB, Y32
    for D, ld in ((6, 8), (1028, 1028)):
        g, b = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
        X, XO, YB, Y32 = bufs(D, ld)            # D = 6: rows of 6 at a stride of 8, so that only D is wrong
        with pytest.raises(RuntimeError, match=r"code -1\): tr_layernorm: need D % 4 == 0, D <= 1024"):
            ops.layernorm_bf16_f32(X.rows, g, b, 1e-6, y=Y32.rows)
        with pytest.raises(RuntimeError, match=r"code -1\): tr_layernorm: need D % 4 == 0, D <= 1024"):
            ops.layernorm_f32(X.rows, g, b, 1e-6, y=Y32.rows)
        if ld == D:
            with pytest.raises(RuntimeError, match=r"code -1\): tr_layernorm: need D % 4 == 0, D <= 1024"):
                ops.layernorm(X.rows, g, b, 1e-6, y=YB.rows)
    D = 260
    g, b = _params(D)
    d = R.ln_case(M, D)["d1"].cuda()
    X, XO, YB, Y32 = bufs(D)
    with pytest.raises(RuntimeError, match=r"code -1\): tr_layernorm: bad x_out stride 256"):
        ops.layernorm_to(X.rows, XO.rows, g, b, 1e-6, delta=d, y=YB.rows, ldxo=D - 4)
    with pytest.raises(RuntimeError, match=r"code -1\): tr_layernorm: bad x_out stride 256"):
        ops.layernorm_bf16_f32(X.rows, g, b, 1e-6, delta=d, x_out=XO.rows, y=Y32.rows, ldxo=D - 4)
    with pytest.raises(RuntimeError, match=r"code -1\): tr_layernorm: a second residual needs the first"):
        ops.layernorm_bf16_f32(X.rows, g, b, 1e-6, delta2=d, x_out=XO.rows, y=Y32.rows)
    with pytest.raises(RuntimeError, match=r"code -3\): tr_layernorm2_bf16: needs a pending residual"):
        ops.layernorm2(X.rows, g, b, 1e-6, None, d, y=YB.rows)
    with pytest.raises(RuntimeError, match=r"code -1\): tr_layernorm: bad delta stride 256"):
        ops.layernorm_to(X.rows, XO.rows, g, b, 1e-6, delta=d, y=YB.rows, ldd=D - 4)
    torch.cuda.synchronize()
    for G in held:
        G.check("refused call")
        assert G.untouched(), "a refused call wrote to its output or to the stream"
