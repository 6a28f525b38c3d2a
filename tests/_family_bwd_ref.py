"""Float64 CPU references, input builders and the case tables of the edge-shape tests of the family, head and embedding backward
kernels (csrc/tr_backward.hip: tr_head_bwd, tr_embed_bwd, tr_evit_fuse_bwd, tr_tome_merge_bwd, tr_cluster_merge_bwd, tr_ats_scatter;
csrc/tr_soft_bwd.hip: tr_rownorm_bwd).

Every reference is the CLOSED FORM the kernel's header comment states, evaluated in float64 on the operands exactly as the kernel reads
them (fp32, or bf16-rounded where the C ABI takes bf16) -- no autograd here.  tests/test_family_bwd_ref.py proves each closed form
against torch.autograd in float64 at every shape of the tables (CPU suite); tests/test_hip_family_bwd_edges.py compares the kernels with
them (GPU suite).  The builders turn (shape, seed) into a VALID case -- sorted complements, ToMe index sets with CLS unmerged, cluster
assignments in which every cluster owns a token, ATS id rows with unique valid ids -- and assert every index range on the CPU, so no
out-of-range index can reach a launch.

`python -m tests._family_bwd_ref` prints, per case and output, the distance between a float32 restatement of the op (torch's float32
arithmetic: the same formulas, torch's summation order) and the float64 reference, next to the bound the GPU test applies: what plain
float32 evaluation costs at each shape, measured without a kernel.
"""
import torch

F64 = torch.float64
D_ALL = (64, 192, 384, 768, 1024)               # NCH 1, 1, 2, 3, 4; 64 and 192 leave lanes >= 16 / >= 48 without a 16-byte chunk

# ---------------------------------------------------------------------------------------------------------------- case tables
# tr_head_bwd (B, C, D): B % 4 != 0 runs the row clamp; C = 8 never enters the five-deep class loop, C = 40 enters it for part 0 only,
# C = 48 for every part once, 1000 / 1008 are the ImageNet pattern and one step more; D = 200 is no multiple of 64 (column clamp)
HEAD_CASES = [(1, 8, 64), (5, 40, 192), (3, 48, 128), (7, 1000, 384), (2, 1008, 768), (6, 16, 1024), (5, 24, 200)]
# tr_embed_bwd (B, N, D): N * D / 4 = 32, 80 and 9456 chunks leave a ragged last block of 64 ((1, 2, 64) is half a block in all); 4800,
# 110784 and 768 fit exactly; B < 4 leaves batch lanes empty, B % 4 != 0 a ragged last batch pass
EMBED_CASES = [(1, 2, 64), (3, 5, 64), (5, 197, 192), (6, 50, 384), (2, 577, 768), (7, 3, 1024)]
# tr_evit_fuse_bwd (B, N, K, D): N - 1 - K complement tokens: 1, 4, 34, 1, 476
EVIT_CASES = [(1, 3, 1, 64), (1, 3, 1, 1024), (2, 7, 2, 192), (2, 7, 2, 384), (3, 60, 25, 384), (3, 60, 25, 768), (1, 197, 195, 64),
              (1, 197, 195, 192), (2, 577, 100, 768), (2, 577, 100, 1024)]
# tr_tome_merge_bwd (B, N, r, D): even and odd N, the largest legal r (only CLS unmerged), N whose halves exceed one 256-thread pass
TOME_CASES = [(1, 3, 1, 64), (2, 4, 1, 192), (2, 50, 24, 384), (2, 51, 25, 768), (1, 577, 288, 1024), (1, 578, 16, 64)]
# tr_cluster_merge_bwd (B, N, K, D, score bias): K = 1 and K = P, K past one 256-thread pass, K = 640 (all of sW), P > 640 (assignments
# walked in global memory), B x 8 > 2048 (fewer workgroups per image).  The score bias sets the scale of the token weights
# w = exp(x . sw + sb): at -13 they are of the order of the 1e-6 in W_c = sum w + 1e-6, so that term decides the result
CLUSTER_CASES = [(1, 2, 1, 64, 0.02), (2, 9, 8, 192, -13.0), (2, 99, 1, 128, 0.02), (1, 300, 257, 384, 0.02), (1, 642, 640, 64, -13.0),
                 (1, 700, 300, 128, 0.02), (260, 9, 4, 64, 0.02), (2, 99, 49, 1024, -13.0)]
# tr_ats_scatter (B, N, Ks, D, kind): "full" = no padding (Ks = N), "cls" = every row after CLS padded, "mixed" = a padded tail per image
ATS_CASES = [(1, 2, 1, 64, "mixed"), (1, 2, 1, 1024, "mixed"), (3, 50, 50, 192, "full"), (3, 50, 50, 768, "full"), (2, 50, 12, 64, "cls"),
             (2, 50, 12, 384, "cls"), (3, 41, 7, 192, "mixed"), (3, 41, 7, 768, "mixed"), (3, 41, 7, 1024, "mixed")]
# tr_rownorm_bwd (M, D): D < 64 leaves lanes without an element, 100 and 1000 are no multiples of 64
ROWNORM_CASES = [(1, 4), (5, 48), (6, 100), (77, 384), (3, 1000)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _in_range(idx, lo, hi, what):
    assert idx.dtype == torch.int32 and int(idx.min()) >= lo and int(idx.max()) < hi, f"{what}: index outside [{lo}, {hi})"


# ---------------------------------------------------------------------------------------------------------------- head
def head_case(B, C, D, seed=0):
    g = _gen(1000 + seed)
    return dict(dlogits=_randn(g, B, C, scale=0.01), w=_randn(g, C, D, scale=0.02).bfloat16(), xn=_randn(g, B, D).bfloat16())


def head_bwd_ref(dlogits, w, xn):
    """dxn = dlogits W (fp32 dlogits); dW = dl16^T xn and db = column sums of dl16, dl16 = dlogits rounded to bf16 (the GEMM operand)."""
    dl, dl16 = dlogits.to(F64), dlogits.bfloat16().to(F64)
    return dl @ w.to(F64), dl16.t() @ xn.to(F64), dl16.sum(0)


# ---------------------------------------------------------------------------------------------------------------- embedding
def embed_case(B, N, D, seed=0):
    return dict(g=_randn(_gen(2000 + seed), B, N, D))


def embed_bwd_ref(g):
    """d pos_embed[n] = sum_b g[b, n]; d cls_token = sum_b g[b, 0]."""
    g = g.to(F64)
    return g.sum(0), g[:, 0].sum(0)


# ---------------------------------------------------------------------------------------------------------------- EViT fused token
def evit_case(B, N, K, D, seed=0, with_delta=True):
    g = _gen(3000 + seed)
    P = N - 1
    assert 1 <= K < P
    compl = torch.stack([torch.randperm(P, generator=g)[K:].sort().values for _ in range(B)]).to(torch.int32)
    _in_range(compl, 0, P, "compl")
    assert compl.shape == (B, P - K) and bool((compl[:, 1:] > compl[:, :-1]).all()), "compl: not strictly ascending"
    return dict(x=_randn(g, B, N, D), delta=_randn(g, B, N, D).bfloat16() if with_delta else None, compl=compl,
                scores=torch.rand(B, P, generator=g), g_fused=_randn(g, B, D))


def evit_fuse_bwd_ref(x, delta, compl, scores, g_fused):
    """g_out[b, 1 + c_j] = s[b, c_j] g_fused[b];  dscore[b, 1 + c_j] = <x[b, 1 + c_j] + delta[b, 1 + c_j], g_fused[b]>.
    -> (g_out [B,N,D], dscore [B,N], touched [B,N] bool); rows outside 1 + compl are zero in both and False in `touched`."""
    B, N, D = x.shape
    xm = x.to(F64) + (delta.to(F64) if delta is not None else 0.0)
    gf, c = g_fused.to(F64), compl.long()
    g_out, dscore, touched = torch.zeros(B, N, D, dtype=F64), torch.zeros(B, N, dtype=F64), torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        g_out[b, 1 + c[b]] = scores[b, c[b]].to(F64)[:, None] * gf[b][None]
        dscore[b, 1 + c[b]] = xm[b, 1 + c[b]] @ gf[b]
        touched[b, 1 + c[b]] = True
    return g_out, dscore, touched


# ---------------------------------------------------------------------------------------------------------------- ToMe merge
def tome_case(B, N, r, D, seed=0, with_size=True):
    """unm: the na - r unmerged A-tokens (even positions), ascending, CLS (0) always among them; src: the r merged A-tokens; dst: their
    B-tokens (odd positions), of which two sources share one whenever r >= 2.  size_out is the forward's (sizes carry no gradient)."""
    g = _gen(4000 + seed)
    na, nb = (N + 1) // 2, N // 2
    assert N >= 3 and 1 <= r <= (N - 1) // 2
    unm, src, dst = [], [], []
    for _ in range(B):
        perm = torch.randperm(na - 1, generator=g) + 1
        src.append(perm[:r])
        unm.append(torch.cat([torch.zeros(1, dtype=torch.long), perm[r:]]).sort().values)
        d = torch.randint(0, nb, (r,), generator=g)
        if r >= 2:
            d[1] = d[0]
        dst.append(d)
    unm, src, dst = (torch.stack(t).to(torch.int32) for t in (unm, src, dst))
    _in_range(unm, 0, na, "unm"), _in_range(src, 1, na, "src"), _in_range(dst, 0, nb, "dst")
    for b in range(B):
        both = torch.cat([unm[b], src[b]]).sort().values
        assert torch.equal(both, torch.arange(na, dtype=torch.int32)), "unm and src must partition the A-tokens"
        assert int(unm[b, 0]) == 0
    size_in = (torch.rand(B, N, generator=g) * 3 + 1).floor() if with_size else None
    size_out = tome_forward(torch.zeros(B, N, 1, dtype=F64), size_in, unm, src, dst)[1].float()
    return dict(g_merged=_randn(g, B, N - r, D), size_in=size_in, size_out=size_out, unm=unm, src=src, dst=dst, N=N)


def tome_forward(x, size_in, unm, src, dst):
    """merge_wavg as the existing kernel test writes it -> (x_out [B, N - r, D], size_out [B, N - r]), float64, differentiable in x."""
    B, N = x.shape[:2]
    size = torch.ones(B, N, dtype=F64) if size_in is None else size_in.to(F64)
    xs = x * size[..., None]
    a_x, b_x, a_s, b_s = xs[:, 0::2], xs[:, 1::2], size[:, 0::2], size[:, 1::2]
    outs, sizes = [], []
    for b in range(B):
        u, s, d = unm[b].long(), src[b].long(), dst[b].long()
        outs.append(torch.cat([a_x[b, u], b_x[b].index_add(0, d, a_x[b, s])]))
        sizes.append(torch.cat([a_s[b, u], b_s[b].index_add(0, d, a_s[b, s])]))
    size_out = torch.stack(sizes)
    return torch.stack(outs) / size_out[..., None], size_out


def tome_out_row(unm, src, dst, N):
    """o(i) [B,N]: unmerged A-token -> its rank in unm; B-token 2t + 1 -> nu + t; merged A-token -> the slot of its destination."""
    B, nu = unm.shape
    o = torch.full((B, N), -1, dtype=torch.long)
    for b in range(B):
        o[b, 2 * unm[b].long()] = torch.arange(nu)
        o[b, 1::2] = nu + torch.arange(N // 2)
        o[b, 2 * src[b].long()] = nu + dst[b].long()
    assert int(o.min()) >= 0 and int(o.max()) < N - src.shape[1]
    return o


def tome_merge_bwd_ref(g_merged, size_in, size_out, unm, src, dst, N):
    """g_in[b, i] = size_in[b, i] / size_out[b, o(i)] * g_merged[b, o(i)]   (size_in = 1 when None)."""
    B = g_merged.shape[0]
    o = tome_out_row(unm, src, dst, N)
    s_in = torch.ones(B, N, dtype=F64) if size_in is None else size_in.to(F64)
    w = s_in / torch.gather(size_out.to(F64), 1, o)
    return w[..., None] * torch.gather(g_merged.to(F64), 1, o[..., None].expand(-1, -1, g_merged.shape[2]))


# ---------------------------------------------------------------------------------------------------------------- DPC-KNN CTM merge
def cluster_forward(x0, assign, K, sw=None, sb=None):
    """CTM merge as the existing kernel test writes it, float64, differentiable -> (x1 [B,K+1,D], token weights [B,P])."""
    xs = x0[:, 1:]
    B, P = xs.shape[:2]
    w = (xs @ sw + sb).exp() if sw is not None else torch.ones(B, P, dtype=F64)
    onehot = torch.nn.functional.one_hot(assign.long(), K).to(F64)
    W = torch.einsum("bpk,bp->bk", onehot, w) + 1e-6
    merged = torch.einsum("bpk,bp,bpd->bkd", onehot, w, xs) / W[..., None]
    return torch.cat([x0[:, :1], merged], dim=1), w


def cluster_case(B, N, K, D, sb=0.02, seed=0, weighted=True):
    """Every cluster owns at least one token.  x1 and the token weights are the float64 forward's, rounded to fp32 as the kernel reads them."""
    g = _gen(5000 + seed)
    P = N - 1
    assert 1 <= K <= P and K <= 640
    assign = torch.stack([torch.cat([torch.arange(K), torch.randint(0, K, (P - K,), generator=g)])[torch.randperm(P, generator=g)]
                          for _ in range(B)]).to(torch.int32)
    _in_range(assign, 0, K, "assign")
    for b in range(min(B, 4)):
        assert torch.bincount(assign[b].long(), minlength=K).min() >= 1, "empty cluster"
    x0 = _randn(g, B, N, D)
    sw = _randn(g, D, scale=0.5 / D ** 0.5) if weighted else None
    sbt = torch.tensor([sb], dtype=torch.float32) if weighted else None
    with torch.no_grad():
        x1, w = cluster_forward(x0.to(F64), assign, K, None if sw is None else sw.to(F64), None if sbt is None else sbt.to(F64))
    return dict(g_in=_randn(g, B, K + 1, D), x0=x0, x1=x1.float().contiguous(), wtok=w.float().contiguous() if weighted else None,
                assign=assign, sw=sw, sb=sbt)


def cluster_merge_bwd_ref(g_in, x0, x1, wtok, assign, sw):
    """W_c = sum_{i in c} w_i + 1e-6;  dlog_i = w_i <g_c, x_i - x_c> / W_c;  d x_i = (w_i / W_c) g_c + dlog_i sw;  d sw = sum_i dlog_i x_i;
    d sb = sum_i dlog_i;  the CLS row passes through.  Unweighted (sw None): w_i = 1, dlog_i = 0.  -> (g [B,N,D], dsw [D]|None, dsb [1]|None)"""
    B, N, D = x0.shape
    K, P, a = g_in.shape[1] - 1, N - 1, assign.long()
    w = wtok.to(F64) if sw is not None else torch.ones(B, P, dtype=F64)
    W = torch.zeros(B, K, dtype=F64).scatter_add_(1, a, w) + 1e-6
    ai = a[..., None].expand(-1, -1, D)
    gc, xc, xi = torch.gather(g_in.to(F64)[:, 1:], 1, ai), torch.gather(x1.to(F64)[:, 1:], 1, ai), x0.to(F64)[:, 1:]
    sc = w / torch.gather(W, 1, a)
    g = torch.empty(B, N, D, dtype=F64)
    g[:, 0] = g_in.to(F64)[:, 0]
    if sw is None:
        g[:, 1:] = sc[..., None] * gc
        return g, None, None
    dlog = sc * (gc * (xi - xc)).sum(-1)
    g[:, 1:] = sc[..., None] * gc + dlog[..., None] * sw.to(F64)
    return g, torch.einsum("bp,bpd->d", dlog, xi), dlog.sum().reshape(1)


# ---------------------------------------------------------------------------------------------------------------- ATS row scatter
def ats_case(B, N, Ks, D, kind="mixed", seed=0):
    """ids[b, 0] = 0 (CLS); valid ids are unique within an image and in [1, N); padded entries are 0 and follow the valid ones."""
    g = _gen(6000 + seed)
    assert 1 <= Ks <= N
    ids = torch.zeros(B, Ks, dtype=torch.int32)
    for b in range(B):
        nv = {"full": Ks - 1, "cls": 0, "mixed": (Ks - 1) * (b + 1) // (B + 1)}[kind]
        assert nv <= N - 1
        ids[b, 1:1 + nv] = (torch.randperm(N - 1, generator=g)[:nv] + 1).sort().values.to(torch.int32)
        valid = ids[b, 1:1 + nv]
        assert valid.unique().numel() == nv and (nv == 0 or (int(valid.min()) >= 1 and int(valid.max()) < N))
    _in_range(ids, 0, N, "ids")
    return dict(g=_randn(g, B, Ks, D), dao_s=_randn(g, B, Ks, D).bfloat16(), ids=ids, N=N)


def ats_scatter_ref(g, dao_s, ids, N):
    """full[b, ids[b, t]] = sampled[b, t] for t == 0 or ids[b, t] != 0; every other row of `full` is zero.  Exact copies."""
    B, Ks, D = g.shape
    gf, df = torch.zeros(B, N, D, dtype=F64), torch.zeros(B, N, D, dtype=F64)
    for b in range(B):
        for t in range(Ks):
            if t == 0 or int(ids[b, t]) != 0:
                gf[b, int(ids[b, t])] = g[b, t].to(F64)
                df[b, int(ids[b, t])] = dao_s[b, t].to(F64)
    return gf, df


# ---------------------------------------------------------------------------------------------------------------- L2 row normalize
def rownorm_case(M, D, seed=0, with_db=True):
    g = _gen(7000 + seed)
    return dict(x=_randn(g, M, D, scale=3.0), da=_randn(g, M, D), db=_randn(g, M, D).bfloat16() if with_db else None)


def rownorm_bwd_ref(x, da, db):
    """xh = x / max(|x|, 1e-12);  g = da + db;  dx = (g - xh <xh, g>) / max(|x|, 1e-12)."""
    x, g = x.to(F64), da.to(F64) + (db.to(F64) if db is not None else 0.0)
    nrm = x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    xh = x / nrm
    return (g - xh * (xh * g).sum(-1, keepdim=True)) / nrm


# ---------------------------------------------------------------------------------------------------------------- float32 restatements
def max_rel(got, want):
    """max |got - want| relative to max |want| (the measure of the fp32 outputs in the GPU tests)."""
    want = want.to(F64)
    return float((got.to(F64) - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _f32_report():
    """The ops in torch float32 against the float64 references, per case (module docstring)."""
    rows = []
    for B, C, D in HEAD_CASES:
        c = head_case(B, C, D)
        dx, dw, db = head_bwd_ref(**c)
        dl16 = c["dlogits"].bfloat16().float()
        rows.append((f"head {B, C, D}", {"dxn(fp32, before the bf16 rounding)": (max_rel(c["dlogits"] @ c["w"].float(), dx), 2.0 ** -8),
                                         "dW": (max_rel(dl16.t() @ c["xn"].float(), dw), 2e-4),
                                         "db(abs)": (float((dl16.sum(0).double() - db).abs().max()), 1e-5)}))
    for B, N, D in EMBED_CASES:
        c = embed_case(B, N, D)
        dpos, dcls = embed_bwd_ref(**c)
        rows.append((f"embed {B, N, D}", {"dpos": (max_rel(c["g"].sum(0), dpos), 1e-4),
                                          "dcls": (float((c["g"][:, 0].sum(0).double() - dcls).abs().max() / dpos.abs().max()), 1e-4)}))
    for B, N, K, D in EVIT_CASES:
        for wd in (True, False):
            c = evit_case(B, N, K, D, with_delta=wd)
            g_out, dscore, _ = evit_fuse_bwd_ref(**c)
            xm = c["x"] + (c["delta"].float() if wd else 0.0)
            ci = c["compl"].long()
            ds = torch.zeros(B, N)
            go = torch.zeros(B, N, D)
            for b in range(B):
                ds[b, 1 + ci[b]] = xm[b, 1 + ci[b]] @ c["g_fused"][b]
                go[b, 1 + ci[b]] = c["scores"][b, ci[b]][:, None] * c["g_fused"][b][None]
            rows.append((f"evit {B, N, K, D} delta={wd}", {"g_out": (max_rel(go, g_out), 1e-5), "dscore": (max_rel(ds, dscore), 1e-4)}))
    for B, N, r, D in TOME_CASES:
        for ws in (True, False):
            c = tome_case(B, N, r, D, with_size=ws)
            want = tome_merge_bwd_ref(**c)
            o = tome_out_row(c["unm"], c["src"], c["dst"], N)
            w = (c["size_in"] if ws else torch.ones(B, N)) / torch.gather(c["size_out"], 1, o)
            got = w[..., None] * torch.gather(c["g_merged"], 1, o[..., None].expand(-1, -1, D))
            rows.append((f"tome {B, N, r, D} size={ws}", {"g": (max_rel(got, want), 1e-5)}))
    for B, N, K, D, sb in CLUSTER_CASES:
        c = cluster_case(B, N, K, D, sb)
        g, dsw, dsb = cluster_merge_bwd_ref(c["g_in"], c["x0"], c["x1"], c["wtok"], c["assign"], c["sw"])
        a = c["assign"].long()
        W = torch.zeros(B, K).scatter_add_(1, a, c["wtok"]) + 1e-6
        ai = a[..., None].expand(-1, -1, D)
        gc, xc, xi = torch.gather(c["g_in"][:, 1:], 1, ai), torch.gather(c["x1"][:, 1:], 1, ai), c["x0"][:, 1:]
        sc = c["wtok"] / torch.gather(W, 1, a)
        dlog = sc * (gc * (xi - xc)).sum(-1)
        g32 = torch.cat([c["g_in"][:, :1], sc[..., None] * gc + dlog[..., None] * c["sw"]], dim=1)
        dsw32, dsb32 = torch.einsum("bp,bpd->d", dlog, xi), dlog.sum().reshape(1)
        rows.append((f"cluster {B, N, K, D} sb={sb}", {"g": (max_rel(g32, g), 2e-4), "dsw": (max_rel(dsw32, dsw), 2e-4),
                                                        "dsb(rel |dsw|)": (float((dsb32.double() - dsb).abs().max() / dsw.abs().max()), 1e-3)}))
    for M, D in ROWNORM_CASES:
        for wdb in (True, False):
            c = rownorm_case(M, D, with_db=wdb)
            want = rownorm_bwd_ref(**c)
            g = c["da"] + (c["db"].float() if wdb else 0.0)
            nrm = c["x"].norm(dim=-1, keepdim=True).clamp_min(1e-12)
            xh = c["x"] / nrm
            got = (g - xh * (xh * g).sum(-1, keepdim=True)) / nrm
            excess = ((got.double() - want).abs() - 1e-4 * want.abs()).max()
            rows.append((f"rownorm {M, D} db={wdb}", {"dx(abs beyond rtol 1e-4)": (float(excess), 1e-6)}))
    return rows


if __name__ == "__main__":
    for name, outs in _f32_report():
        print(name + ": " + "; ".join(f"{k} fp32-vs-fp64 {v:.2e} (bound {bnd:.1e}{'' if v <= bnd else ' EXCEEDED'})" for k, (v, bnd) in outs.items()))
