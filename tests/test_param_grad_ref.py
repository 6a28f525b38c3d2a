"""The closed-form float64 references of tests/_param_grad_ref.py against torch.autograd in float64, at every shape of the case tables
(no GPU): the closed form must equal the autograd gradient to 1e-10 of the gradient's largest magnitude, both row scatters included.
The integer builders must be exact in fp32 (so the GPU test may use torch.equal at any split count), and a plain float32 evaluation of the
LayerNorm closed form must cost less than half of each bound the GPU test (tests/test_hip_param_grad_edges.py) applies."""
import pytest
import torch

from tests import _param_grad_ref as R

F64 = torch.float64
TOL = 1e-10


def _close(got, want, what):
    err = float((got - want).abs().max())
    scale = float(want.abs().max())
    assert err <= TOL * scale + 1e-300, f"{what}: closed form differs from autograd by {err:.3e} (scale {scale:.3e})"


def _leaf(t):
    return t.to(F64).clone().requires_grad_(True)


def _ln_autograd(c, eps, rows_of, leaves, with_g_in=True):
    """loss = <LayerNorm(rows), dy> + <rows, g_in>: its gradient is what tr_layernorm_bwd hands on.  rows_of(): the LayerNorm input [M, D]
    built from `leaves` (the first two of which are gamma and beta)."""
    D = c["x"].shape[1]
    rows = rows_of()
    y = torch.nn.functional.layer_norm(rows, (D,), leaves[0], leaves[1], R.eps32(eps))
    loss = (y * c["dy"].to(F64)).sum()
    if with_g_in:
        loss = loss + (rows * c["g_in"].to(F64)).sum()
    return torch.autograd.grad(loss, leaves)


@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("M,D", sorted(set(R.LN_SHAPES) | set(R.LN_FORM_SHAPES) | set(R.LN_FINAL_CASES)))
def test_ln_bwd_ref(M, D, eps):
    c = R.ln_case(M, D)
    if M > 3:
        assert bool((c["x"][3] == 0.5).all()), "row 3 is the constant row"
    for with_g_in in (True, False):
        g, dgamma, dbeta = R.ln_bwd_ref(c["dy"], c["x"], c["gamma"], eps, c["g_in"] if with_g_in else None)
        x, gamma, beta = _leaf(c["x"]), _leaf(c["gamma"]), torch.zeros(D, dtype=F64, requires_grad=True)
        ag, ab, ax = _ln_autograd(c, eps, lambda: x, (gamma, beta, x), with_g_in)
        _close(g, ax, "g"), _close(dgamma, ag, "d_gamma"), _close(dbeta, ab, "d_beta")
        # row by row as well: the GPU test holds g per row, and the constant row is 10^3 x the others
        err = (g - ax).abs().amax(-1) / ax.abs().amax(-1).clamp_min(1e-300)
        assert float(err.max()) <= 1e-9, f"row {int(err.argmax())}: closed form differs from autograd by {float(err.max()):.3e} of the row"


@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("kind,fused", [("distinct", False), ("distinct", True), ("pairs", False), ("empty", False)])
@pytest.mark.parametrize("B,K,n_out,D", R.LN_SCATTER_CASES)
def test_ln_bwd_scatter_ref(B, K, n_out, D, kind, fused, eps):
    """gather -> LayerNorm: the gathered rows are full[b, 0], full[b, 1 + idx[b, :]] (+ the fused row, a tensor of its own); the gradient
    with respect to `full` is the scatter -- summed where ids repeat."""
    n_in = K + 1 + (1 if fused else 0)
    c = R.ln_case(B * n_in, D)
    idx = R.scatter_idx(B, K, n_out, kind)
    ids0 = set(R.scatter_idx(B, K, n_out, "distinct")[0].tolist())
    assert len(ids0) == K and 0 in ids0 and (n_out - 2 in ids0 or K < 2), "the ids include the first and the last patch row"
    if kind == "pairs" and K >= 2:
        assert bool((idx[:, 0] == idx[:, 1]).all())
    if kind == "empty":
        assert bool((idx[-1] == 0).all())
    out = R.ln_bwd_ref(c["dy"], c["x"], c["gamma"], eps, c["g_in"], idx=idx, n_out=n_out, fused=fused, add=kind != "distinct")
    # `full` and `extra` are zero leaves ADDED to the given rows: the gathered rows keep the builder's values even where ids repeat
    full = torch.zeros(B, n_out, D, dtype=F64, requires_grad=True)
    extra = torch.zeros(B, 1, D, dtype=F64, requires_grad=True)
    gamma, beta = _leaf(c["gamma"]), torch.zeros(D, dtype=F64, requires_grad=True)
    src = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + idx.long()], dim=1)

    def rows_of():
        parts = [torch.gather(full, 1, src[..., None].expand(-1, -1, D))] + ([extra] if fused else [])
        return torch.cat(parts, dim=1).reshape(B * n_in, D) + c["x"].to(F64)
    leaves = (gamma, beta, full) + ((extra,) if fused else ())
    grads = _ln_autograd(c, eps, rows_of, leaves)
    _close(out[0].view(B, n_out, D), grads[2], "g"), _close(out[1], grads[0], "d_gamma"), _close(out[2], grads[1], "d_beta")
    if fused:
        _close(out[3], grads[3][:, 0], "g_fused")
    touched = torch.zeros(B * n_out, dtype=torch.bool)
    dst = R.scatter_rows(idx, n_out, fused)
    touched[dst[dst >= 0]] = True
    assert float(out[0][~touched].abs().max() if bool((~touched).any()) else 0.0) == 0.0, "dropped rows are zero"


def _pg_rows():
    return [(r, "general") for r in R.WGRAD_CASES] + [(r, "pc") for r in R.WGRAD_PC_CASES]


@pytest.mark.parametrize("row,kernel", _pg_rows())
def test_wgrad_ref_and_exact_integers(row, kernel):
    M, N, K, ly, lx, skip, fits = row
    assert 4 * M < 2 ** 24
    assert (kernel == "pc") == (M >= 64 and N % 192 == 0 and K % 192 == 0), "the table a case sits in names the kernel that takes it"
    c = R.wgrad_case(M, N, K, ly, lx, skip)
    dy, x = c["dy"], c["x"]
    assert dy.shape[1] == N and x.shape == (M, K) and (ly is None or dy.stride(0) == ly[1]) and (lx is None or x.stride(0) == lx[1])
    y = R.drop_skipped(dy, c["yskip"])
    assert y.shape == (M, N) and float(y.float().abs().max()) <= 2 and float(x.float().abs().max()) <= 2, "the operand holds no fill value"
    if skip is not None:
        assert bool((dy.reshape(skip[0], skip[1] + 1, N)[:, 0] == R.FILL).all())
    assert torch.equal((y.float().t() @ x.float()).double(), c["dw"]) and torch.equal(y.float().sum(0).double(), c["db"])
    # the closed form is the gradient of <dy, x W^T + b>
    w, b = torch.zeros(N, K, dtype=F64, requires_grad=True), torch.zeros(N, dtype=F64, requires_grad=True)
    gw, gb = torch.autograd.grad(((x.to(F64) @ w.t() + b) * y.to(F64)).sum(), (w, b))
    assert torch.equal(gw, c["dw"]) and torch.equal(gb, c["db"])
    # everything around the operands is the fill value
    for buf, view in ((c["ybuf"], dy), (c["xbuf"], x)):
        mask = torch.ones_like(buf, dtype=torch.bool)
        left = (view.data_ptr() - buf.data_ptr()) // 2 % buf.shape[1]
        mask[4:4 + view.shape[0], left:left + view.shape[1]] = False
        assert bool((buf[mask] == R.FILL).all()) and int(mask.sum()) >= 7 * view.shape[1]
    g = R.wgrad_case(M, N, K, ly, lx, skip, kind="gauss")
    assert g["dy"].shape == dy.shape and g["dy"].stride() == dy.stride() and float(g["dw"].abs().max()) > 0


@pytest.mark.parametrize("M,N,ly,skip", R.COLSUM_CASES)
def test_colsum_ref_and_exact_integers(M, N, ly, skip):
    assert 4 * M < 2 ** 24
    c = R.colsum_case(M, N, ly, skip)
    y = R.drop_skipped(c["dy"], c["yskip"])
    assert y.shape == (M, N) and float(y.float().abs().max()) <= 2
    assert torch.equal(y.float().sum(0).double(), c["db"])


def test_group_tables():
    for layers in R.GROUP_CASES:
        assert 2 <= len(layers) <= 4 and all(M >= 64 and N % 192 == 0 and K % 192 == 0 and 4 * M < 2 ** 24 for M, N, K in layers)
    assert len(R.GROUP_CASES[R.GROUP_FALLBACK]) == 4


@pytest.mark.parametrize("eps", R.LN_EPS)
@pytest.mark.parametrize("M,D", R.ln_all_shapes())
def test_ln_float32_cost_stays_below_half_of_each_bound(M, D, eps):
    """The bounds of the GPU test were set for other shapes; at these, plain float32 must leave the kernels at least half of each."""
    cost = R.ln_f32_cost(M, D, eps)
    print(f"{M, D} eps={eps:g}: " + ", ".join(f"{k} {v:.2e}" for k, v in cost.items()))
    for k, v in cost.items():
        assert v <= 0.5 * R.LN_BOUNDS[k], f"{k}: float32 costs {v:.2e}, more than half of {R.LN_BOUNDS[k]:.1e}"
