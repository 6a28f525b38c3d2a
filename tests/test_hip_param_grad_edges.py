"""GPU parity of the LayerNorm backward and the parameter-gradient kernels in the forms the backward executor (csrc/tr_train.hip) calls
them (csrc/tr_backward.hip: ln_bwd_kernel, wgrad_kernel, colsum_kernel, the partial reduces, gelu; csrc/tr_wgrad_pc.hip: wgrad_pc_kernel),
through the C ABI by way of the ops wrappers.

tests/test_hip_backward.py holds these kernels at a handful of shapes, with exactly the workspace the library recommends, contiguous
operands, a separate LayerNorm output and both parameter gradients.  The executor shares one workspace over all ops (larger than most
need, smaller than some), hands over column slices, runs the LayerNorm backward in place, accumulating, without the bf16 copy and on
strided CLS rows.  The shapes here (tests/_param_grad_ref.py, with the reason for each next to its table) are the smallest that reach
every chunk count, reduce kernel, re-plan and tail.  The checker is the float64 closed form of _param_grad_ref.py -- proven against
float64 autograd on the CPU by tests/test_param_grad_ref.py -- fed the same fp32 / bf16 operands as the kernel.

Outputs AND workspaces are slices of sentinel-filled buffers with GUARD elements on either side: nothing outside [N, K], [N], [M, D] or
ws[:ws_floats] may change.  Every accumulate check starts from a distinct random prior and expects prior + result.  Every case runs
twice and must be bitwise equal (the atomic scatter-add excepted).

Bounds (all from tests/test_hip_backward.py; none is new): integer operands torch.equal; Gaussian dW 2e-4 max|ref| + 1e-6, db and column
sums 1e-4 max|ref| + 1e-5; LayerNorm g 1e-4 of THAT ROW's largest reference magnitude (per row, not per tensor: the constant row 3 is
10^3 x the others), d_gamma 2e-4 max|ref|, d_beta 2e-4 max|ref| + 1e-5; every bf16 copy within 2^-8 of the row's largest magnitude and
bit-equal to round-to-nearest-even of the fp32 g stored next to it.  `python -m tests._param_grad_ref` shows what plain float32
evaluation costs on these inputs: at most 2.9e-6 per row (at (253, 4)), 6.3e-7 for d_gamma, 7.4e-8 for d_beta -- no bound had to be
re-derived.
"""
import functools

import pytest
import torch

from tests import _param_grad_ref as R

pytestmark = pytest.mark.gpu

BF16 = 2.0 ** -8
GUARD = 256
SENT = 7.25                 # around and under every output
WS_SENT = -12345.5          # in and around every workspace: a partial that is read without having been written shows in the result


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from tokenreduction_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------------ helpers
class Guarded:
    """n elements between two guards of a sentinel-filled buffer"""

    def __init__(self, n, fill=SENT, dtype=torch.float32, inner=None):
        self.n, self.fill = int(n), fill
        self.buf = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.n]
        if inner is not None:
            self.view.copy_(inner.reshape(-1)) if torch.is_tensor(inner) else self.view.fill_(inner)

    def check(self, what):
        assert bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all()), f"{what}: written outside"

    def untouched(self):
        return bool((self.view == self.fill).all())


def _on_gpu(buf, view):
    """the same slice of a copy of `buf` on the GPU"""
    return buf.cuda().as_strided(view.shape, view.stride(), view.storage_offset())


def _prior(seed, shape, scale, integer=False):
    g = torch.Generator().manual_seed(seed)
    if integer:
        return torch.randint(-50, 51, shape, generator=g).float().cuda()
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _assert_max(got, want, rel, absolute, what):
    want = want.double().cpu()
    err, scale = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, relative {err / max(scale, 1e-300):.3e} (bound {rel:.1e} + {absolute:.0e})")
    assert err <= rel * scale + absolute, f"{what}: max err {err:.3e} > {rel:.1e} x {scale:.3e} + {absolute:.0e}"


def _assert_rows(got, want, bound, what):
    """every row within `bound` of that row's largest reference magnitude (a zero reference row must be zero)"""
    want = want.double().cpu()
    err, scale = (got.double().cpu() - want).abs().amax(-1), want.abs().amax(-1)
    rel = err / scale.clamp_min(1e-300)
    w = int(rel.argmax())
    print(f"{what}: worst row {w}: err {float(err[w]):.3e}, row scale {float(scale[w]):.3e}, relative {float(rel[w]):.3e} (bound {bound:.1e})")
    assert bool((err <= bound * scale).all()), f"{what}: row {w} off by {float(rel[w]):.3e} of its largest magnitude (bound {bound:.1e})"


def _assert_bf16_copy(gb, g32, want, what):
    _assert_rows(gb.float(), want, BF16, what)
    assert torch.equal(gb.view(torch.int16), g32.bfloat16().view(torch.int16)), f"{what}: not the round-to-nearest-even of the fp32 output"


def _assert_ln_params(dgamma, dbeta, ref, prior=(None, None), what=""):
    """d_gamma / d_beta against the float64 reference (+ the prior they were added to), bounds relative to the reference's magnitude"""
    for got, want, p, absolute, name in ((dgamma, ref[1], prior[0], 0.0, "d_gamma"), (dbeta, ref[2], prior[1], R.LN_DBETA_ABS, "d_beta")):
        total = want if p is None else p.double().cpu() + want
        err, scale = float((got.double().cpu() - total).abs().max()), float(want.abs().max())
        bound = R.LN_BOUNDS["dgamma" if name == "d_gamma" else "dbeta"]
        print(f"{name}{what}: max err {err:.3e}, scale {scale:.3e}, relative {err / max(scale, 1e-300):.3e} (bound {bound:.1e})")
        assert err <= bound * scale + absolute, f"{name}{what}: max err {err:.3e} > {bound:.1e} x {scale:.3e}"


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm backward
@functools.lru_cache(maxsize=None)
def _ln_ref(M, D, eps, with_g_in=True):
    c = R.ln_case(M, D)
    return R.ln_bwd_ref(c["dy"], c["x"], c["gamma"], eps, c["g_in"] if with_g_in else None)


@functools.lru_cache(maxsize=None)
def _ln_gpu(M, D):
    c = R.ln_case(M, D)
    return {k: v.cuda() for k, v in c.items()}


def _ln_run(ops, lib, M, D, eps, g_in, **kw):
    """the plain form in guarded buffers: (g, gb, dgamma, dbeta), guards checked"""
    c = _ln_gpu(M, D)
    G, DG, DB = Guarded(M * D), Guarded(D), Guarded(D)
    W = Guarded(lib.tr_layernorm_bwd_workspace_floats(M, D), WS_SENT)
    out = ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], eps, g_in=g_in, g_out=G.view.view(M, D), dgamma=DG.view, dbeta=DB.view, ws=W.view, **kw)
    for b, what in ((G, "g_out"), (DG, "d_gamma"), (DB, "d_beta"), (W, "workspace")):
        b.check(what)
    return out


@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("M,D", R.LN_SHAPES)
def test_layernorm_bwd_shapes(ops, lib, M, D, eps):
    """Every chunk count and ragged last chunk at two and 64 workgroups; every grid size, reduce kernel and pass count at NCH 1 and 4."""
    c, ref = _ln_gpu(M, D), _ln_ref(M, D, eps)
    g, gb, dgamma, dbeta = _ln_run(ops, lib, M, D, eps, c["g_in"])
    _assert_rows(g, ref[0], R.LN_BOUNDS["g"], "g")
    _assert_bf16_copy(gb.cpu(), g.cpu(), ref[0], "gb")
    _assert_ln_params(dgamma, dbeta, ref)
    again = _ln_run(ops, lib, M, D, eps, c["g_in"])
    assert all(torch.equal(a, b) for a, b in zip(again, (g, gb, dgamma, dbeta))), "not bitwise reproducible"


_LN_BASE = {}


def _ln_base(ops, lib, M, D, eps):
    if (M, D, eps) not in _LN_BASE:
        _LN_BASE[M, D, eps] = _ln_run(ops, lib, M, D, eps, _ln_gpu(M, D)["g_in"])
    return _LN_BASE[M, D, eps]


@pytest.mark.parametrize("form", ["separate", "no_g_in", "in_place", "no_gb", "accumulate", "no_params", "strided"])
@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("M,D", R.LN_FORM_SHAPES)
def test_layernorm_bwd_forms(ops, lib, M, D, eps, form):
    """The forms the executor calls: in place (g_in is g_out), no bf16 copy, accumulating parameter gradients, a frozen norm, row strides."""
    c, ref = _ln_gpu(M, D), _ln_ref(M, D, eps)
    g0, gb0, dg0, db0 = _ln_base(ops, lib, M, D, eps)
    if form == "separate":
        _assert_rows(g0, ref[0], R.LN_BOUNDS["g"], "g")
        _assert_bf16_copy(gb0.cpu(), g0.cpu(), ref[0], "gb")
        _assert_ln_params(dg0, db0, ref)
    elif form == "no_g_in":
        ref = _ln_ref(M, D, eps, False)
        g, gb, dgamma, dbeta = _ln_run(ops, lib, M, D, eps, None)
        _assert_rows(g, ref[0], R.LN_BOUNDS["g"], "g")
        _assert_bf16_copy(gb.cpu(), g.cpu(), ref[0], "gb")
        assert torch.equal(dgamma, dg0) and torch.equal(dbeta, db0), "the parameter gradients do not depend on g_in"
    elif form == "in_place":
        G, DG, DB = Guarded(M * D, inner=c["g_in"]), Guarded(D), Guarded(D)
        gv = G.view.view(M, D)
        g, gb, dgamma, dbeta = ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], eps, g_in=gv, g_out=gv, dgamma=DG.view, dbeta=DB.view)
        G.check("g (in place)")
        assert g.data_ptr() == gv.data_ptr()
        assert torch.equal(g, g0) and torch.equal(gb, gb0) and torch.equal(dgamma, dg0) and torch.equal(dbeta, db0), "in place differs from separate"
    elif form == "no_gb":
        g, gb, dgamma, dbeta = _ln_run(ops, lib, M, D, eps, c["g_in"], gb=False)
        assert gb is None and torch.equal(g, g0) and torch.equal(dgamma, dg0) and torch.equal(dbeta, db0)
    elif form == "accumulate":
        pg, pb = _prior(21, (D,), float(ref[1].abs().max())), _prior(22, (D,), float(ref[2].abs().max()))
        DG, DB, G = Guarded(D, inner=pg), Guarded(D, inner=pb), Guarded(M * D)
        W = Guarded(lib.tr_layernorm_bwd_workspace_floats(M, D), WS_SENT)
        g, gb, dgamma, dbeta = ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], eps, g_in=c["g_in"], g_out=G.view.view(M, D), accumulate=True,
                                                 dgamma=DG.view, dbeta=DB.view, ws=W.view)
        for b, what in ((G, "g_out"), (DG, "d_gamma"), (DB, "d_beta"), (W, "workspace")):
            b.check(what)
        assert torch.equal(g, g0) and torch.equal(gb, gb0)
        _assert_ln_params(dgamma, dbeta, ref, prior=(pg, pb), what=" (prior + result)")
    elif form == "no_params":
        g, gb, dgamma, dbeta = ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], eps, g_in=c["g_in"], params=False)
        assert dgamma is None and dbeta is None
        assert torch.equal(g, g0) and torch.equal(gb, gb0), "the frozen form changes the data gradient"
    else:
        xw = torch.full((M, D + 8), SENT, device="cuda")
        giw = torch.full((M, D + 4), SENT, device="cuda")
        gow = torch.full((M + 1, D + 12), SENT, device="cuda")
        xw[:, 4:4 + D], giw[:, :D] = c["x"], c["g_in"]
        DG, DB = Guarded(D), Guarded(D)
        g, gb, dgamma, dbeta = ops.layernorm_bwd(c["dy"], xw[:, 4:4 + D], c["gamma"], eps, g_in=giw[:, :D], g_out=gow[:M, 8:8 + D], dgamma=DG.view,
                                                 dbeta=DB.view)
        assert bool((gow[:, :8] == SENT).all()) and bool((gow[:, 8 + D:] == SENT).all()) and bool((gow[M] == SENT).all()), "a gap of g_out was written"
        assert torch.equal(gow[:M, 8:8 + D], g0) and torch.equal(gb, gb0) and torch.equal(dgamma, dg0) and torch.equal(dbeta, db0)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("B,D", R.LN_FINAL_CASES)
def test_layernorm_bwd_final_norm_on_cls_rows(ops, lib, B, D, eps, accumulate):
    """The final norm's backward: B CLS rows, no g_in, no bf16 copy, written at row stride Nl * D into the residual gradient [B, Nl, D];
    rows 1 .. Nl - 1 of every image keep what they held."""
    Nl = R.LN_FINAL_NL
    c, ref = _ln_gpu(B, D), _ln_ref(B, D, eps, False)
    pg, pb = _prior(23, (D,), float(ref[1].abs().max())), _prior(24, (D,), float(ref[2].abs().max()))
    runs = []
    for _ in range(2):
        G, DG, DB = Guarded(B * Nl * D), Guarded(D, inner=pg if accumulate else None), Guarded(D, inner=pb if accumulate else None)
        W = Guarded(lib.tr_layernorm_bwd_workspace_floats(B, D), WS_SENT)
        g, gb, dgamma, dbeta = ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], eps, g_out=G.view.view(B, Nl * D)[:, :D], gb=False,
                                                 accumulate=accumulate, dgamma=DG.view, dbeta=DB.view, ws=W.view)
        for b, what in ((G, "g_out"), (DG, "d_gamma"), (DB, "d_beta"), (W, "workspace")):
            b.check(what)
        assert gb is None
        full = G.view.view(B, Nl, D)
        assert bool((full[:, 1:] == SENT).all()), "a row other than the CLS row was written"
        runs.append((full[:, 0].clone(), dgamma.clone(), dbeta.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "not bitwise reproducible"
    _assert_rows(runs[0][0], ref[0], R.LN_BOUNDS["g"], "g")
    _assert_ln_params(runs[0][1], runs[0][2], ref, prior=(pg, pb) if accumulate else (None, None))


def _scatter_setup(B, K, n_out, D, fused, kind, eps):
    n_in = K + 1 + (1 if fused else 0)
    M = B * n_in
    c, idx = R.ln_case(M, D), R.scatter_idx(B, K, n_out, kind)
    ref = R.ln_bwd_ref(c["dy"], c["x"], c["gamma"], eps, c["g_in"], idx=idx, n_out=n_out, fused=fused, add=kind != "distinct")
    dst = R.scatter_rows(idx, n_out, fused)
    touched = torch.zeros(B * n_out, dtype=torch.bool)
    touched[dst[dst >= 0]] = True
    return M, _ln_gpu(M, D), idx.cuda(), ref, touched


def _scatter_run(ops, lib, c, idx, M, D, n_out, eps, **kw):
    B = idx.shape[0]
    G, DG, DB = Guarded(B * n_out * D, inner=0.0), Guarded(D), Guarded(D)
    W = Guarded(lib.tr_layernorm_bwd_workspace_floats(M, D), WS_SENT)
    out = ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], eps, g_in=c["g_in"], idx=idx, n_out=n_out, g_out=G.view.view(B * n_out, D),
                            dgamma=DG.view, dbeta=DB.view, ws=W.view, **kw)
    for b, what in ((G, "g_out"), (DG, "d_gamma"), (DB, "d_beta"), (W, "workspace")):
        b.check(what)
    return out


@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("B,K,n_out,D", R.LN_SCATTER_CASES)
def test_layernorm_bwd_scatter(ops, lib, B, K, n_out, D, fused, eps):
    """Backward of gather -> LayerNorm: row 0 -> 0, row r -> 1 + idx[b, r - 1] of ITS image (ids 0 and n_out - 2 included), EViT's fused row
    aside, dropped rows exactly zero; 2553 rows decode image and row in a second grid pass."""
    M, c, idx, ref, touched = _scatter_setup(B, K, n_out, D, fused, "distinct", eps)
    out = _scatter_run(ops, lib, c, idx, M, D, n_out, eps, fused=fused)
    g, gb = out[0].cpu(), out[1].cpu()
    assert g.shape == (B * n_out, D) and gb.shape == (B * n_out, D)
    assert bool((g[~touched] == 0).all()) and bool((gb[~touched].float() == 0).all()), "a dropped row is not zero"
    _assert_rows(g, ref[0], R.LN_BOUNDS["g"], "g")
    _assert_bf16_copy(gb, g, ref[0], "gb")
    _assert_ln_params(out[2], out[3], ref)
    if fused:
        _assert_rows(out[4], ref[3], R.LN_BOUNDS["g"], "g_fused")
    again = _scatter_run(ops, lib, c, idx, M, D, n_out, eps, fused=fused)
    assert all(torch.equal(a, b) for a, b in zip(again, out)), "not bitwise reproducible"


@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("kind", ["distinct", "pairs", "empty"])
@pytest.mark.parametrize("B,K,n_out,D", R.LN_SCATTER_CASES)
def test_layernorm_bwd_scatter_add(ops, lib, B, K, n_out, D, kind, eps):
    """tr_layernorm_bwd_scatter_add (the K-Medoids gather backward) against the float64 additive scatter: distinct ids give the plain
    scatter's bits; pairs of equal ids and an image whose ids are all 0 (empty clusters) are summed; no bf16 copy; dropped rows zero."""
    M, c, idx, ref, touched = _scatter_setup(B, K, n_out, D, False, kind, eps)
    g, gb, dgamma, dbeta = _scatter_run(ops, lib, c, idx, M, D, n_out, eps, add=True)
    assert gb is None
    assert bool((g.cpu()[~touched] == 0).all()), "a dropped row is not zero"
    _assert_rows(g, ref[0], R.LN_BOUNDS["g"], "g")
    _assert_ln_params(dgamma, dbeta, ref)
    plain = _scatter_run(ops, lib, c, R.scatter_idx(B, K, n_out, "distinct").cuda(), M, D, n_out, eps)
    assert torch.equal(dgamma, plain[2]) and torch.equal(dbeta, plain[3]), "the parameter gradients do not depend on the ids"
    if kind == "distinct":
        assert torch.equal(g, plain[0]), "distinct ids: one add onto zero per element is the plain scatter"


# ------------------------------------------------------------------------------------------------------------------------ parameter gradients
def _ws_floats(lib, M, N, K, fit, bias):
    rec = int(lib.tr_wgrad_workspace_floats(M, N, K))
    if fit is None:
        return rec
    if fit == "x4":
        return 4 * rec
    return fit * (N * K + (N if bias else 0))


def _pg_params():
    return [pytest.param(row, fit, id=f"{row[0]}x{row[1]}x{row[2]}{'-strided' if row[3] else ''}{'-yskip' if row[5] else ''}-ws_{fit or 'rec'}")
            for row in R.WGRAD_CASES + R.WGRAD_PC_CASES for fit in row[6]]


def _check_pg(got, want, kind, what, prior=None):
    """integers: exact; Gaussian: the bound of tests/test_hip_backward.py relative to the reference (not to prior + reference)"""
    dw = what.startswith("dW")
    if kind == "int":
        total = want.float() if prior is None else prior.cpu() + want.float()
        assert torch.equal(got.cpu(), total), f"{what}: {int((got.cpu() != total).sum())} of {total.numel()} integers wrong"
        return
    rel, absolute = (R.DW_BOUND, R.DW_ABS) if dw else (R.DB_BOUND, R.DB_ABS)
    total = want if prior is None else prior.double().cpu() + want
    err, scale = float((got.double().cpu() - total).abs().max()), float(want.abs().max())
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, relative {err / max(scale, 1e-300):.3e} (bound {rel:.1e} + {absolute:.0e})")
    assert err <= rel * scale + absolute, f"{what}: max err {err:.3e} > {rel:.1e} x {scale:.3e} + {absolute:.0e}"


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("row,fit", _pg_params())
def test_wgrad_and_linear_bwd_params(ops, lib, row, fit, kind):
    """tr_wgrad_bf16 and tr_linear_bwd_params at every slab, tile and reduce edge of both weight-gradient kernels, at the workspace the
    library recommends, at four times that (the executor's shared buffer: the bias partials of the 192-tile kernel then sit behind S_max
    weight partials, not behind S) and at room for `fit` partials (the S > fit clamp and the re-evened token ranges); dW of the fused call
    bit-equal to tr_wgrad_bf16's; accumulate onto a distinct prior; run twice."""
    M, N, K, ly, lx, skip, _ = row
    c = R.wgrad_case(M, N, K, ly, lx, skip, kind)
    dy, x, yskip = _on_gpu(c["ybuf"], c["dy"]), _on_gpu(c["xbuf"], c["x"]), c["yskip"]
    scale_w, scale_b = float(c["dw"].abs().max()), float(c["db"].abs().max())
    pw, pb = _prior(31, (N, K), scale_w, kind == "int"), _prior(32, (N,), scale_b, kind == "int")
    nw, nb = _ws_floats(lib, M, N, K, fit, False), _ws_floats(lib, M, N, K, fit, True)
    print(f"workspace floats: wgrad {nw}, linear_bwd_params {nb} (recommended {lib.tr_wgrad_workspace_floats(M, N, K)}, "
          f"{lib.tr_wgrad_workspace_floats(M, N, K) // (N * K + N)} partials)")

    def run_wgrad(prior=None):
        O, W = Guarded(N * K, inner=prior), Guarded(nw, WS_SENT)
        out = ops.wgrad(dy, x, out=O.view.view(N, K), accumulate=prior is not None, yskip=yskip, rows=M, ws=W.view)
        O.check("dW"), W.check("workspace")
        return out

    def run_both(prior=(None, None)):
        O, B, W = Guarded(N * K, inner=prior[0]), Guarded(N, inner=prior[1]), Guarded(nb, WS_SENT)
        out = ops.linear_bwd_params(dy, x, accumulate=prior[0] is not None, dw=O.view.view(N, K), db=B.view, yskip=yskip, ws=W.view)
        O.check("dW"), B.check("db"), W.check("workspace")
        return out
    dw = run_wgrad()
    _check_pg(dw, c["dw"], kind, "dW (wgrad)")
    dw2, db2 = run_both()
    assert torch.equal(dw2, dw), "dW of tr_linear_bwd_params differs from tr_wgrad_bf16's"
    _check_pg(db2, c["db"], kind, "db")
    assert torch.equal(run_wgrad(), dw), "wgrad: not bitwise reproducible"
    dw3, db3 = run_both()
    assert torch.equal(dw3, dw2) and torch.equal(db3, db2), "linear_bwd_params: not bitwise reproducible"
    _check_pg(run_wgrad(pw), c["dw"], kind, "dW (wgrad, prior + result)", prior=pw)
    dw4, db4 = run_both((pw, pb))
    _check_pg(dw4, c["dw"], kind, "dW (prior + result)", prior=pw)
    _check_pg(db4, c["db"], kind, "db (prior + result)", prior=pb)


def _group_layers(shapes, strided, kind):
    layers, refs = [], []
    for i, (M, N, K) in enumerate(shapes):
        ybuf, dy = R.operand(M, N, (8, N + 16) if strided else None, kind, seed=100 + 2 * i + M)
        xbuf, x = R.operand(M, K, (0, K + 8) if strided else None, kind, seed=101 + 2 * i + M)
        layers.append((_on_gpu(ybuf, dy), _on_gpu(xbuf, x)))
        refs.append(R.wgrad_ref(dy, x))
    return layers, refs


def _group_run(ops, layers, shapes, nws, priors=None):
    outs = [(Guarded(N * K, inner=None if priors is None else priors[i][0]), Guarded(N, inner=None if priors is None else priors[i][1]))
            for i, (M, N, K) in enumerate(shapes)]
    W = Guarded(nws, WS_SENT)
    got = ops.linear_bwd_group(layers, accumulate=priors is not None, outs=[(o.view.view(N, K), b.view) for (o, b), (M, N, K) in zip(outs, shapes)],
                               ws=W.view)
    for o, b in outs:
        o.check("dW"), b.check("db")
    W.check("workspace")
    return got, W.untouched()


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("gi", range(len(R.GROUP_CASES)))
def test_linear_bwd_group(ops, gi, strided, kind):
    """tr_linear_bwd_group: the direct store (no partial written: the workspace keeps its sentinel) exactly where every layer is one token
    range and the call overwrites; partials + partial_reduce8_kernel otherwise -- every segment, its unrolled loop with and without tail;
    operands contiguous and as column slices; accumulate onto distinct priors; run twice."""
    shapes = R.GROUP_CASES[gi]
    layers, refs = _group_layers(shapes, strided, kind)
    nws = ops.linear_bwd_group_workspace_floats(shapes)
    got, untouched = _group_run(ops, layers, shapes, nws)
    assert untouched == (gi in R.GROUP_DIRECT), "workspace written by a direct store, or kept by a launch that must reduce"
    for i, ((dw, db), (rw, rb)) in enumerate(zip(got, refs)):
        _check_pg(dw, rw, kind, f"dW layer {i}"), _check_pg(db, rb, kind, f"db layer {i}")
    again, _ = _group_run(ops, layers, shapes, nws)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(again, got)), "not bitwise reproducible"
    priors = [(_prior(40 + 2 * i, (N, K), float(refs[i][0].abs().max()), kind == "int"),
               _prior(41 + 2 * i, (N,), float(refs[i][1].abs().max()), kind == "int")) for i, (M, N, K) in enumerate(shapes)]
    acc, untouched = _group_run(ops, layers, shapes, nws, priors)
    assert not untouched, "an accumulating group goes through partials and the reduce"
    for i, ((dw, db), (rw, rb)) in enumerate(zip(acc, refs)):
        _check_pg(dw, rw, kind, f"dW layer {i} (prior + result)", prior=priors[i][0])
        _check_pg(db, rb, kind, f"db layer {i} (prior + result)", prior=priors[i][1])


@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_linear_bwd_group_falls_back_when_the_partials_do_not_fit(ops, lib, kind):
    """A workspace that holds the largest single layer but not the group's partials: separate tr_linear_bwd_params calls, same results."""
    shapes = R.GROUP_CASES[R.GROUP_FALLBACK]
    layers, refs = _group_layers(shapes, False, kind)
    single = max(int(lib.tr_wgrad_workspace_floats(M, N, K)) for M, N, K in shapes)
    assert single < ops.linear_bwd_group_workspace_floats(shapes), "the group's partials would fit: no fallback"
    got, untouched = _group_run(ops, layers, shapes, single)
    assert not untouched
    for i, ((dw, db), (rw, rb)) in enumerate(zip(got, refs)):
        _check_pg(dw, rw, kind, f"dW layer {i}"), _check_pg(db, rb, kind, f"db layer {i}")
        sw, sb = ops.linear_bwd_params(*layers[i])
        assert torch.equal(dw, sw) and torch.equal(db, sb), "the fallback is the separate call"


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("one_range", [True, False])
@pytest.mark.parametrize("M,N,ly,skip", R.COLSUM_CASES)
def test_colsum(ops, lib, M, N, ly, skip, one_range, kind):
    """tr_colsum_bf16: N below one float4 (the reduce's ragged branch), a second column block of one thread pair, the 4-row loop's remainder,
    the 256-range cap, yskip and a row stride; with room for one range and with the recommended workspace; accumulate; run twice."""
    c = R.colsum_case(M, N, ly, skip, kind)
    dy, yskip = _on_gpu(c["ybuf"], c["dy"]), c["yskip"]
    nws = N if one_range else int(lib.tr_colsum_workspace_floats(M, N))

    def run(prior=None):
        O, W = Guarded(N, inner=prior), Guarded(nws, WS_SENT)
        out = ops.colsum(dy, out=O.view, accumulate=prior is not None, yskip=yskip, rows=M, ws=W.view)
        O.check("db"), W.check("workspace")
        return out
    db = run()
    _check_pg(db, c["db"], kind, "db")
    assert torch.equal(run(), db), "not bitwise reproducible"
    p = _prior(51, (N,), float(c["db"].abs().max()), kind == "int")
    _check_pg(run(p), c["db"], kind, "db (prior + result)", prior=p)


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_workspace_below_one_partial_is_refused(ops, lib):
    """TR_ERR_SHAPE (-1), nothing launched, outputs at their sentinel.  The workspace handed over is large enough for the call: only the
    size told to the library is short."""
    M, N, K, D = 65, 16, 8, 64
    c = R.wgrad_case(M, N, K)
    dy, x = _on_gpu(c["ybuf"], c["dy"]), _on_gpu(c["xbuf"], c["x"])
    W = Guarded(4096, WS_SENT)
    O, B = Guarded(N * K), Guarded(N)
    with pytest.raises(RuntimeError, match=r"code -1"):
        ops.wgrad(dy, x, out=O.view.view(N, K), ws=W.view, ws_floats=N * K - 1)
    with pytest.raises(RuntimeError, match=r"code -1"):
        ops.linear_bwd_params(dy, x, dw=O.view.view(N, K), db=B.view, ws=W.view, ws_floats=N * K + N - 1)
    with pytest.raises(RuntimeError, match=r"code -1"):
        ops.colsum(dy, out=B.view, ws=W.view, ws_floats=N - 1)
    lc = _ln_gpu(5, D)
    G, DG, DB = Guarded(5 * D), Guarded(D), Guarded(D)
    with pytest.raises(RuntimeError, match=r"code -1"):
        ops.layernorm_bwd(lc["dy"], lc["x"], lc["gamma"], 1e-6, g_out=G.view.view(5, D), dgamma=DG.view, dbeta=DB.view, ws=W.view,
                          ws_floats=int(lib.tr_layernorm_bwd_workspace_floats(5, D)) - 1)
    shapes = R.GROUP_CASES[0]
    layers, _ = _group_layers(shapes, False, "int")
    big = Guarded(192 * 192 + 192, WS_SENT)
    outs = [(Guarded(N * K), Guarded(N)) for _, N, K in shapes]
    with pytest.raises(RuntimeError, match=r"code -1"):
        ops.linear_bwd_group(layers, outs=[(o.view.view(192, 192), b.view) for o, b in outs], ws=big.view, ws_floats=192 * 192 + 191)
    torch.cuda.synchronize()
    for b in [W, O, B, G, DG, DB, big] + [t for pair in outs for t in pair]:
        b.check("refused call")
        assert b.untouched(), "a refused call wrote to its output or workspace"


# ------------------------------------------------------------------------------------------------------------------------ gelu
@pytest.mark.parametrize("n", R.GELU_SIZES)
def test_gelu_and_gelu_bwd_at_one_chunk_and_past_a_workgroup(ops, n):
    """tr_gelu_bf16 / tr_gelu_bwd_bf16 at n = 8 (one chunk) and 8 x 257 (one chunk in a second workgroup), at the bounds
    tests/test_hip_backward.py applies at its one size; operands between guards."""
    g = torch.Generator().manual_seed(n)
    a = torch.randn(129, 64, generator=g).bfloat16().cuda()
    w = (torch.randn(16, 64, generator=g) * 0.2).bfloat16().cuda()
    bias = torch.randn(16, generator=g).cuda()
    # the op is elementwise: the first n pre-activations of a Linear against the first n outputs of its fused GELU epilogue
    P = Guarded(n, 3.0, torch.bfloat16, inner=ops.gemm(a, w, bias, ops.TR_EPI_BF16).reshape(-1)[:n])
    h, fused = ops.gelu(P.view), ops.gemm(a, w, bias, ops.TR_EPI_GELU_BF16).reshape(-1)[:n]
    P.check("pre")
    assert h.shape == (n,)
    assert torch.equal(h, fused) or float((h.float() - fused.float()).abs().max()) <= 2.0 ** -7 * 4
    xs = (torch.randn(n, generator=g) * 2.0).bfloat16()
    dh = torch.randn(n, generator=g).bfloat16()
    x64 = xs.double()
    want = dh.double() * (0.5 * (1.0 + torch.erf(x64 / 2.0 ** 0.5)) + x64 * torch.exp(-0.5 * x64 * x64) / (2.0 * torch.pi) ** 0.5)
    X, DH = Guarded(n, 3.0, torch.bfloat16, inner=xs.cuda()), Guarded(n, 3.0, torch.bfloat16, inner=dh.cuda())
    got = ops.gelu_bwd(X.view, DH.view)
    X.check("pre"), DH.check("dh")
    assert got.data_ptr() == DH.view.data_ptr()
    _assert_max(got.float(), want, BF16, 1e-6, "gelu_bwd")
