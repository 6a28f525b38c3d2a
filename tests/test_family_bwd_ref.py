"""The closed-form float64 references of tests/_family_bwd_ref.py against torch.autograd in float64, at every shape of the case tables
(no GPU): the forward of each op is written as tests/test_hip_backward.py writes it, the loss is <output, upstream gradient>, and the
closed form must equal the autograd gradient to 1e-10 of the gradient's largest magnitude.  This proves the references and the input
builders before the GPU tests (tests/test_hip_family_bwd_edges.py) compare the kernels with them."""
import pytest
import torch

from tests import _family_bwd_ref as R

F64 = torch.float64
TOL = 1e-10


def _close(got, want, what):
    err = float((got - want).abs().max())
    scale = float(want.abs().max())
    assert err <= TOL * scale + 1e-300, f"{what}: closed form differs from autograd by {err:.3e} (scale {scale:.3e})"


def _leaf(t):
    return t.to(F64).clone().requires_grad_(True)


@pytest.mark.parametrize("B,C,D", R.HEAD_CASES)
def test_head_bwd_ref(B, C, D):
    c = R.head_case(B, C, D)
    dxn, dw, db = R.head_bwd_ref(**c)
    xn, w, b = _leaf(c["xn"]), _leaf(c["w"]), torch.zeros(C, dtype=F64, requires_grad=True)
    logits = xn @ w.t() + b
    gx, = torch.autograd.grad((logits * c["dlogits"].to(F64)).sum(), xn, retain_graph=True)
    gw, gb = torch.autograd.grad((logits * c["dlogits"].bfloat16().to(F64)).sum(), (w, b))      # the parameter gradients see dlogits in bf16
    _close(dxn, gx, "dxn"), _close(dw, gw, "dW"), _close(db, gb, "db")


@pytest.mark.parametrize("B,N,D", R.EMBED_CASES)
def test_embed_bwd_ref(B, N, D):
    c = R.embed_case(B, N, D)
    dpos, dcls = R.embed_bwd_ref(**c)
    g0 = torch.Generator().manual_seed(1)
    patches = torch.randn(B, N - 1, D, generator=g0, dtype=F64)
    pos, cls = torch.randn(N, D, generator=g0, dtype=F64, requires_grad=True), torch.randn(D, generator=g0, dtype=F64, requires_grad=True)
    x = torch.cat([cls.expand(B, 1, D), patches], dim=1) + pos[None]                              # topk.py:183-186
    gp, gc = torch.autograd.grad((x * c["g"].to(F64)).sum(), (pos, cls))
    _close(dpos, gp, "dpos"), _close(dcls, gc, "dcls")


@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("B,N,K,D", R.EVIT_CASES)
def test_evit_fuse_bwd_ref(B, N, K, D, with_delta):
    c = R.evit_case(B, N, K, D, with_delta=with_delta)
    g_out, dscore, touched = R.evit_fuse_bwd_ref(**c)
    xm = _leaf(c["x"].to(F64) + (c["delta"].to(F64) if with_delta else 0.0))
    sc = _leaf(c["scores"])
    ci = c["compl"].long()
    rows = torch.gather(xm[:, 1:], 1, ci[..., None].expand(-1, -1, D))
    extra = (rows * torch.gather(sc, 1, ci)[..., None]).sum(1)
    gx, gs = torch.autograd.grad((extra * c["g_fused"].to(F64)).sum(), (xm, sc))
    _close(g_out, gx, "g_out"), _close(dscore[:, 1:], gs, "dscore")
    assert not bool(touched[:, 0].any()) and int(touched.sum()) == B * (N - 1 - K)
    assert float(g_out[~touched].abs().max()) == 0.0 and float(dscore[~touched].abs().max()) == 0.0


@pytest.mark.parametrize("with_size", [True, False])
@pytest.mark.parametrize("B,N,r,D", R.TOME_CASES)
def test_tome_merge_bwd_ref(B, N, r, D, with_size):
    c = R.tome_case(B, N, r, D, with_size=with_size)
    if r >= 2:
        assert bool((c["dst"][:, 0] == c["dst"][:, 1]).all()), "two sources must share a destination"
    want = R.tome_merge_bwd_ref(**c)
    x = torch.randn(B, N, D, generator=torch.Generator().manual_seed(2), dtype=F64, requires_grad=True)
    x_out, size_out = R.tome_forward(x, c["size_in"], c["unm"], c["src"], c["dst"])
    assert torch.equal(size_out.float(), c["size_out"]) and x_out.shape == (B, N - r, D)
    gx, = torch.autograd.grad((x_out * c["g_merged"].to(F64)).sum(), x)
    _close(want, gx, "g")


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("B,N,K,D,sb", R.CLUSTER_CASES)
def test_cluster_merge_bwd_ref(B, N, K, D, sb, weighted):
    c = R.cluster_case(B, N, K, D, sb, weighted=weighted)
    x0 = _leaf(c["x0"])
    sw, sbl = (_leaf(c["sw"]), _leaf(c["sb"])) if weighted else (None, None)
    x1, w = R.cluster_forward(x0, c["assign"], K, sw, sbl)
    # the closed form on the float64 forward's own x1 and weights (the builder's are these, rounded to fp32 for the kernel)
    assert float((x1.detach() - c["x1"].to(F64)).abs().max()) <= 2.0 ** -23 * float(x1.detach().abs().max())
    g, dsw, dsb = R.cluster_merge_bwd_ref(c["g_in"], c["x0"], x1.detach(), w.detach() if weighted else None, c["assign"], c["sw"])
    grads = torch.autograd.grad((x1 * c["g_in"].to(F64)).sum(), (x0, sw, sbl) if weighted else (x0,))
    _close(g, grads[0], "g")
    if weighted:
        # d sw and d sb are sums of dlog_i = (w_i / W_c) <g_c, x_i - x_c>, and x_i - x_c cancels: within a cluster sum_i w_i (x_i - x_c) =
        # 1e-6 x_c, and a cluster of ONE token has x_i - x_c = x_i 1e-6 / W_c, six digits below its operands -- float64 keeps ten of them, in
        # the closed form and in autograd alike.  So both are compared on the scale of one term BEFORE that cancellation,
        # (w_i / W_c) |g_c| |x_i| (times max |x_i| for d sw), as the kernel test does for d sb; never below the gradient's own magnitude
        a = c["assign"].long()
        xi = c["x0"].to(F64)[:, 1:]
        W = torch.zeros(B, K, dtype=F64).scatter_add_(1, a, w.detach()) + 1e-6
        term = w.detach() / torch.gather(W, 1, a) * torch.gather(c["g_in"].to(F64)[:, 1:].norm(dim=-1), 1, a) * xi.norm(dim=-1)
        s_sw = max(float((term * xi.abs().amax(-1)).max()), float(grads[1].abs().max()))
        s_sb = max(float(term.max()), float(grads[2].abs().max()))
        assert float((dsw - grads[1]).abs().max()) <= TOL * s_sw, f"dsw: {float((dsw - grads[1]).abs().max()):.3e} (scale {s_sw:.3e})"
        assert float((dsb - grads[2]).abs().max()) <= TOL * s_sb, f"dsb: {float((dsb - grads[2]).abs().max()):.3e} (scale {s_sb:.3e})"
    else:
        assert dsw is None and dsb is None


@pytest.mark.parametrize("B,N,Ks,D,kind", R.ATS_CASES)
def test_ats_scatter_ref(B, N, Ks, D, kind):
    c = R.ats_case(B, N, Ks, D, kind)
    ids = c["ids"].long()
    valid = ids != 0
    valid[:, 0] = True
    assert int(valid.sum()) == {"full": B * Ks, "cls": B}.get(kind, int(valid.sum()))
    gf, df = R.ats_scatter_ref(**c)
    for want, up in ((gf, c["g"]), (df, c["dao_s"])):
        full = torch.randn(B, N, D, generator=torch.Generator().manual_seed(3), dtype=F64, requires_grad=True)
        sampled = torch.gather(full, 1, ids[..., None].expand(-1, -1, D))                        # ats.py:86,157; padded rows are never read
        gx, = torch.autograd.grad((sampled * up.to(F64) * valid[..., None]).sum(), full)
        assert torch.equal(want, gx)


@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("M,D", R.ROWNORM_CASES)
def test_rownorm_bwd_ref(M, D, with_db):
    c = R.rownorm_case(M, D, with_db=with_db)
    x = _leaf(c["x"])
    up = c["da"].to(F64) + (c["db"].to(F64) if with_db else 0.0)
    gx, = torch.autograd.grad((torch.nn.functional.normalize(x, p=2, dim=-1) * up).sum(), x)
    _close(R.rownorm_bwd_ref(**c), gx, "dx")


def test_tables_cover_every_width():
    """all five widths (NCH 1, 1, 2, 3, 4) appear in the tables of the ops that dispatch on the chunk count"""
    for table, col in ((R.EVIT_CASES, 3), (R.TOME_CASES, 3), (R.ATS_CASES, 3)):
        assert {c[col] for c in table} == set(R.D_ALL)
