"""Stage-wise references for the clustering kernels (csrc/tr_cluster.hip) and the CPU measurement their distance bounds come from.

Only the distance matrix and one expf in the DPC-KNN density are floating-point work; everything after them is comparison logic.  The
staged entry points leave every intermediate in the caller's workspace, so tests/test_hip_cluster_stages.py holds
  * the distance matrix against float64, element by element, within the bound below, and
  * every decision kernel EXACTLY against the replays of this file, which are fed the float32 arrays read back from the device.

Workspace layout (tr_cluster.hip, tr_kmedoids / tr_kmedoids_equal / tr_dpcknn_cluster: `float* dist = ws; nrm = dist + B*P*P; ...`), P = N - 1:
  kmedoids   dist [B,P,P] | nrm [B,P]            | t [B,P]       | wrow [B,N]
  dpcknn     dist [B,P,P] | rowmax [B,P] (= nrm) | density [B,P] | score_rows [B,N]

Distances are compared squared and unscaled, q = (dist * sqrt_d)^2 (sqrt_d = 1 for K-Medoids, float32(sqrt(D)) for DPC-KNN), against
q64 = sum_d (x_i - x_j)^2 in float64, with n_i = |x_i|^2 and u = 2^-24:
  direct (P <= 25)       |q - q64| <= (D + 3) u q64; the diagonal is exactly 0.
  fp32 Gram              |q - q64| <= c (n_i + n_j), c = min(4 GRAM32[D], (D + 4) u).  GRAM32[D] is the worst |q32 - q64| / (n_i + n_j)
                         of torch's float32 matmul form (norms, Gram product, clamp, sqrt, division, all float32) over the tests' own
                         inputs; the kernel gets 4 x because its summation order differs (16-deep fma chains); (D + 4) u is the worst case.
  split-bf16 Gram        c = 2 (SPLIT_EMU[D] + GRAM32[D]).  SPLIT_EMU[D] is the worst element of a float64 emulation that splits every
                         operand into hi = bf16(v), lo = bf16(v - hi) and sums hi.hi + hi.lo + lo.hi (lo.lo dropped), over the inputs of the
                         split cases.
The clamp at 1e-30 and the Gram-form diagonal (rounding residue, not 0) fall under the same bound.  `python -m tests._cluster_ref` prints
GRAM32 and SPLIT_EMU per D over the inputs of DIST_CASES and TRAJ_CASES; the committed values are those figures as printed.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
F64 = torch.float64

# tile shapes of the three distance kernels (tr_cluster.hip: CT; GT, GTN) and the length up to which the direct form serves
CT, GT, GTN, DIRECT_MAX_P = 64, 256, 128, 25

# ---------------------------------------------------------------------------------------------------------------- the tests' shapes
# (kind, P, D, B): the distance cases of tests/test_hip_cluster_stages.py, shared with the measurement below.
_GRAM_P, _SPLIT_P = (26, 63, 64, 65, 129, 196, 257), (26, 127, 128, 129, 196)
_SPLIT_LARGE = ((255, 32), (256, 64), (257, 32), (260, 64), (384, 32), (385, 64), (513, 32), (576, 64), (1021, 32), (1024, 64))
DIST_CASES = ([("direct", P, D, 2) for P in (2, 16, 25) for D in (16, 64)]
              + [("gram", P, D, 2) for P in _GRAM_P for D in (16, 48, 384)] + [("gram", 196, 768, 2)]
              + [("gram", P, 32, 2) for P in (1023, 1024)]
              + [("split", P, D, 2) for P in _SPLIT_P for D in (128, 384)] + [("split", 196, 768, 2)]
              + [("split", P, D, 2) for P, D in _SPLIT_LARGE] + [("split", 576, 32, 3)])
# (P, K, D, iters, seed) of the float64-trajectory tests: B = 2; seeds from `python -m tests._cluster_ref scan` (see trajectory())
TRAJ_CASES = [(48, 6, 64, 3, 7), (70, 9, 64, 3, 2)]
TRAJ_FACTOR = 8.0

# worst |q32 - q64| / (n_i + n_j) per D, and the split emulation's, over the inputs above: `python -m tests._cluster_ref` (CPU)
GRAM32 = {16: 3.534e-07, 32: 4.704e-07, 48: 4.046e-07, 64: 5.333e-07, 128: 4.843e-07, 384: 9.123e-07, 768: 6.435e-07}
SPLIT_EMU = {32: 1.342e-05, 64: 8.716e-06, 128: 5.767e-06, 384: 4.392e-06, 768: 3.747e-06}


def kernel_for(P, D, fast):
    """launch_dist's dispatch."""
    if P <= DIRECT_MAX_P:
        return "direct"
    return "split" if fast and D % 32 == 0 else "gram"


def case_input(P, D, B, seed=0):
    """Unit Gaussians fp32 [B, P + 1, D]; row 0 (the CLS slot, which no clustering kernel may read) is NaN."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * P + 31 * D + B)
    x = torch.randn(B, P + 1, D, generator=g)
    x[:, 0] = float("nan")
    return x


def case_weights(P, B, H=3, seed=0):
    """colsum partials fp32 [B,H,4,N], uniform in [0,1) like a softmax's column sums are positive."""
    g = torch.Generator().manual_seed(500009 * seed + 13 * P + B)
    return torch.rand(B, H, 4, P + 1, generator=g)


# ---------------------------------------------------------------------------------------------------------------- workspace views
def workspace_views(ws, B, N, family):
    """Named views of the staged entry points' workspace (layout in the module docstring)."""
    P = N - 1
    o1 = B * P * P
    v = {"dist": ws[:o1].view(B, P, P)}
    names = {"kmedoids": ("nrm", "t", "wrow"), "dpcknn": ("rowmax", "density", "score_rows")}[family]
    v[names[0]] = ws[o1:o1 + B * P].view(B, P)
    v[names[1]] = ws[o1 + B * P:o1 + 2 * B * P].view(B, P)
    v[names[2]] = ws[o1 + 2 * B * P:o1 + 2 * B * P + B * N].view(B, N)
    return v


# ---------------------------------------------------------------------------------------------------------------- float64 distances
def sqdist64(x):
    """x [B,P,D] (any float dtype) -> sum_d (x_i - x_j)^2 in float64 [B,P,P], the direct form, in row chunks."""
    x = x.to(F64)
    B, P, D = x.shape
    out = torch.empty(B, P, P, dtype=F64)
    step = max(1, (1 << 24) // max(1, P * D))
    for i0 in range(0, P, step):
        d = x[:, i0:i0 + step, None, :] - x[:, None, :, :]
        out[:, i0:i0 + step] = (d * d).sum(-1)
    return out


def sqnorm64(x):
    x = x.to(F64)
    return (x * x).sum(-1)


def sqrt_d32(D):
    """DPC-KNN's divisor as the kernel holds it: (float)sqrt((double)D)."""
    return float(np.float32(math.sqrt(D)))


def unscale(dist, sqrt_d):
    """float32 dist -> q = (dist * sqrt_d)^2 in float64"""
    return (dist.to(F64) * sqrt_d) ** 2


def gram32_dist(x, sqrt_d):
    """torch's float32 matmul form of cdist(x, x) / sqrt_d: float32 norms, Gram product, clamp at 1e-30, sqrt, division."""
    x = x.float()
    n = (x * x).sum(-1)
    d2 = (n[:, :, None] + n[:, None, :] - 2.0 * (x @ x.transpose(1, 2))).clamp_min(1e-30)
    return d2.sqrt() / torch.tensor(sqrt_d, dtype=torch.float32)


def _bf16(v):
    return v.float().bfloat16().to(F64)


def split_emulation(x, drop=None):
    """q of the split-operand Gram product in float64: hi = bf16(v), lo = bf16(v - hi); x.y ~ hi.hi' + hi.lo' + lo.hi' (lo.lo' dropped);
    exact norms.  drop = "hl" | "lh" removes one cross term (the sensitivity test)."""
    x = x.float()
    hi = _bf16(x)
    lo = _bf16(x - hi.float())                       # x - hi is exact in float32
    g = hi @ hi.transpose(1, 2)
    if drop != "hl":
        g = g + hi @ lo.transpose(1, 2)
    if drop != "lh":
        g = g + lo @ hi.transpose(1, 2)
    n = sqnorm64(x)
    return n[:, :, None] + n[:, None, :] - 2.0 * g


def dist_coeff(kind, D):
    """c of |q - q64| <= c (n_i + n_j) for the two Gram kernels (module docstring)."""
    if kind == "gram":
        return min(4.0 * GRAM32[D], (D + 4) * U)
    if kind == "split":
        return 2.0 * (SPLIT_EMU[D] + GRAM32[D])
    raise ValueError(kind)


def skipped_mask(P):
    """[P,P] bool: element (r, c) lies in a tile dist_mfma_kernel does not compute (`if (j0 + GTN <= i0) return;`): its value is the
    mirror store of (c, r)."""
    r = torch.arange(P)
    i0, j0 = (r // GT) * GT, (r // GTN) * GTN
    return j0[None, :] + GTN <= i0[:, None]


def check_dist(dist, x, sqrt_d, kind, q64=None):
    """dist float32 [B,P,P] as a kernel of `kind` left it for the patch rows x [B,P,D]: every element finite and within the bound of q64;
    the direct kernel's diagonal exactly 0; pairs mirrored by the split kernel bitwise symmetric, every other pair symmetric within the
    bound.  A failure names the worst element and its tile."""
    B, P, D = x.shape
    dist = dist.detach().cpu().float()
    assert bool(torch.isfinite(dist).all()), f"{kind} P={P} D={D}: {int((~torch.isfinite(dist)).sum())} elements of dist are not finite"
    q64 = sqdist64(x) if q64 is None else q64
    q = unscale(dist, sqrt_d)
    n = sqnorm64(x)
    if kind == "direct":
        bound = (D + 3) * U * q64
        diag = torch.diagonal(dist, dim1=1, dim2=2)
        assert bool((diag == 0).all()), f"direct P={P} D={D}: diagonal not exactly 0 (max {float(diag.abs().max()):.3e})"
        ti, tj = CT, CT
    else:
        bound = dist_coeff(kind, D) * (n[:, :, None] + n[:, None, :])
        ti, tj = (GT, GTN) if kind == "split" else (CT, CT)

    def worst(err, what):
        ratio = err / bound.clamp_min(1e-300)
        ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
        idx = int(ratio.argmax())
        b, i, j = idx // (P * P), idx // P % P, idx % P
        w = float(ratio.flatten()[idx])
        print(f"{kind} P={P} D={D} sqrt_d={sqrt_d:.4g} {what}: worst error / bound = {w:.3f} at image {b} element ({i}, {j})")
        assert w <= 1.0, (f"{kind} P={P} D={D} {what}: image {b} element ({i}, {j}) in tile ({i // ti}, {j // tj}): error {float(err.flatten()[idx]):.3e} "
                          f"> bound {float(bound.flatten()[idx]):.3e} (q = {float(q.flatten()[idx]):.6e})")

    worst((q - q64).abs(), "against float64")
    worst((q - q.transpose(1, 2)).abs(), "symmetry")
    if kind == "split":
        m = skipped_mask(P)
        bits = dist.view(torch.int32)
        bad = (bits != bits.transpose(1, 2)) & m[None]
        if bool(bad.any()):
            b, i, j = (int(t[0]) for t in torch.nonzero(bad, as_tuple=True))
            raise AssertionError(f"split P={P} D={D}: element ({i}, {j}) of image {b}, in the skipped tile ({i // GT}, {j // GTN}), is not the "
                                 f"bitwise mirror of ({j}, {i}); {int(bad.sum())} such elements")
    return q64


# ---------------------------------------------------------------------------------------------------------------- exact replays
def _np(a):
    """float32 arrays read back from the device (or float64 ones from the CPU tests: the replays work in the dtype they are given)"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    return a


def replay_wrow(part):
    """kmed_weight_kernel: float32 sum over h, then wave, from 0, in that order.  part [B,H,4,N] -> [B,N]"""
    part = _np(part)
    acc = np.zeros((part.shape[0], part.shape[3]), part.dtype)
    for h in range(part.shape[1]):
        for wv in range(4):
            acc = acc + part[:, h, wv]
    return acc


def replay_centers(scores, K):
    """tr_cls_topk on one row of positive scores: stable descending sort.  scores [P] -> int64 [K]"""
    return np.argsort(-_np(scores), kind="stable")[:K]


def replay_weighted_init(wrow, K):
    """The weighted branch's first medoids: top-K of the patch columns of wrow [N]."""
    return replay_centers(_np(wrow)[1:], K)


def replay_kmed_init_equal(dist, K, first):
    """kmed_init_equal_kernel on one image: s_max[i] = running max over the chosen medoids c of dist[i, c] (COLUMN form), chosen tokens
    pinned to 0; the next medoid is the arg-max, ties -> smallest index."""
    d = _np(dist)
    P = d.shape[0]
    chosen = np.zeros(P, bool)
    chosen[first] = True
    s_max = d[:, first].copy()
    s_max[first] = 0.0
    centers = [int(first)]
    for _ in range(1, K):
        nw = int(np.argmax(np.maximum(s_max, 0)))                      # first occurrence of the maximum
        centers.append(nw)
        s_max = np.where(chosen, s_max, np.maximum(s_max, d[:, nw]))
        chosen[nw] = True
        s_max[nw] = 0.0
    return np.asarray(centers, np.int64)


def _assign_rows(d, centers):
    """first minimum over ascending k of dist[c_k, p] (the ROW form the kernels read)"""
    return np.argmin(d[np.asarray(centers, np.int64), :], axis=0)


def replay_kmed_iterate(dist, t, centers0, iters):
    """kmed_iterate_kernel on one image -> (centers int64 [K], assign int64 [P]).  Medoid update: the smallest (t[p], p) over the members
    and the kernel's start value (P * 1e6, 0) -- so an empty cluster falls to index 0; after `iters` updates one more assignment pass."""
    d, t = _np(dist), _np(t)
    P = d.shape[0]
    c = np.asarray(centers0, np.int64).copy()
    order = np.argsort(t, kind="stable")                               # ascending (t, p)
    rank = np.empty(P, np.int64)
    rank[order] = np.arange(P)
    masked = t.dtype.type(P) * t.dtype.type(1000000.0)
    for _ in range(iters):
        a = _assign_rows(d, c)
        best = np.full(c.shape[0], P, np.int64)
        np.minimum.at(best, a, rank)
        cand = order[np.minimum(best, P - 1)]
        wins = (best < P) & ((t[cand] < masked) | ((t[cand] == masked) & (cand == 0)))
        c = np.where(wins, cand, 0)
    return c, _assign_rows(d, c)


def replay_parent_score(dist, density, rowmax):
    """parent_score_kernel on one image: the distance to the nearest token of higher density, else the maximum of the row maxima; one
    multiply by the token's own density, in the inputs' precision.  -> [P]"""
    d, dn, rm = _np(dist), _np(density), _np(rowmax)
    dmax = max(rm.max(), rm.dtype.type(0))
    mn = np.where(dn[None, :] > dn[:, None], d, dmax).min(axis=1)
    return mn * dn


def replay_assign(dist, centers):
    """assign_kernel on one image: nearest centre per token (first on ties), then centres to themselves."""
    centers = np.asarray(centers, np.int64)
    a = _assign_rows(_np(dist), centers)
    a[centers] = np.arange(centers.shape[0])
    return a


def density64(dist, noise, k):
    """exp(-mean(k smallest d^2)) + noise * 1e-6 in float64 from a float32 matrix [B,P,P] -> (density [B,P], exponent argument [B,P])"""
    d = dist.detach().cpu().to(F64)
    near = torch.topk(d, k=k, dim=-1, largest=False).values
    a = (near ** 2).mean(-1)
    return (-a).exp() + (0 if noise is None else noise.detach().cpu().to(F64) * 1e-6), a


def density_bound(k, a_max):
    """Relative.  The kernel squares and adds k float32 values and divides by k (k + 2 roundings of the exponent's argument a, which move
    exp(-a) by a times as much relatively), takes expf (2 u) and adds the noise (1 u)."""
    return ((k + 2) * a_max + 3) * U


def rowcost64(dist, w):
    """t_i = sum_j dist[i, j] * w_i in float64.  dist [B,P,P] float32, w [B,P] float32"""
    return dist.detach().cpu().to(F64).sum(-1) * w.detach().cpu().to(F64)


# ---------------------------------------------------------------------------------------------------------------- stage checkers
def _bits(a):
    a = np.ascontiguousarray(_np(a))
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def check_kmedoids(v, part, first, K, iters, centers, assign, what=""):
    """One tr_kmedoids (part [B,H,4,N]) or tr_kmedoids_equal (part None, first) call: v = the workspace views read back, centers [B,K] and
    assign [B,P] its outputs.  wrow bit for bit the fixed-order sum (or ones); t within P u of float64 on the device's matrix (P positive
    terms); outputs in range and EQUAL to the replays fed the device's dist, t and wrow.  -> the replayed medoids [B,K]"""
    B, P = v["t"].shape
    centers, assign = np.asarray(centers, np.int64), np.asarray(assign, np.int64)
    wrow = replay_wrow(part) if part is not None else np.ones((B, P + 1), np.float32)
    assert np.array_equal(_bits(v["wrow"]), _bits(wrow)), f"{what}: wrow is not the fixed-order sum"
    t64 = rowcost64(v["dist"], v["wrow"][:, 1:])
    terr = ((v["t"].to(F64) - t64).abs() / t64.clamp_min(1e-300)).max().item()
    assert terr <= P * U, f"{what}: row cost off by {terr:.3e} relative (bound {P * U:.3e})"
    assert centers.min() >= 0 and centers.max() < P and assign.min() >= 0 and assign.max() < K, f"{what}: outputs out of range"
    out = []
    for b in range(B):
        c0 = replay_weighted_init(v["wrow"][b], K) if part is not None else replay_kmed_init_equal(v["dist"][b], K, first)
        c, a = replay_kmed_iterate(v["dist"][b], v["t"][b], c0, iters)
        assert np.array_equal(centers[b], c), f"{what} image {b}: medoids differ from the replay at {np.nonzero(centers[b] != c)[0][:8]}"
        assert np.array_equal(assign[b], a), f"{what} image {b}: assignment differs from the replay at tokens {np.nonzero(assign[b] != a)[0][:8]}"
        out.append(c)
    return np.stack(out)


def check_dpcknn(v, noise, k, K, centers, idx, scores, what=""):
    """One tr_dpcknn_cluster call through the staged launches: v = the workspace views read back; centers [B,K], idx [B,P], scores [B,P] its
    outputs.  Density within its derived bound of float64 on the device's matrix; then bit for bit: row maxima, parent scores, the
    returned scores, centres and assignment."""
    dist = v["dist"]
    B, P, _ = dist.shape
    centers, idx = np.asarray(centers, np.int64), np.asarray(idx, np.int64)
    assert torch.equal(v["rowmax"], dist.max(-1).values), f"{what}: row maxima"
    want, a = density64(dist, noise, k)
    rel = ((v["density"].to(F64) - want).abs() / want).max().item()
    bound = density_bound(k, float(a.max()))
    assert rel <= bound, f"{what}: density off by {rel:.3e} relative (bound {bound:.3e})"
    assert np.array_equal(_bits(scores), _bits(v["score_rows"][:, 1:])), f"{what}: returned scores are not the score rows"
    assert bool((v["score_rows"][:, 0] == 0).all()), f"{what}: CLS slot of the score rows"
    assert centers.min() >= 0 and centers.max() < P and idx.min() >= 0 and idx.max() < K, f"{what}: outputs out of range"
    for b in range(B):
        sc = replay_parent_score(dist[b], v["density"][b], v["rowmax"][b])
        assert np.array_equal(_bits(sc), _bits(scores[b])), f"{what} image {b}: parent scores differ from the replay"
        assert np.array_equal(centers[b], replay_centers(scores[b], K)), f"{what} image {b}: centres are not the stable descending sort"
        want_idx = replay_assign(dist[b], centers[b])
        assert np.array_equal(idx[b], want_idx), f"{what} image {b}: assignment differs from the replay at tokens {np.nonzero(idx[b] != want_idx)[0][:8]}"


# ---------------------------------------------------------------------------------------------------------------- float64 trajectory
def _margin(best, second):
    return float("inf") if second <= 0 else (second - best) / second


def trajectory(x, K, iters, w=None, first=None):
    """The oracle's kmedoids_fit (w [P] float32: weighted branch) or kmedoids_init_equal + kmedoids_fit (first: equal weights) in float64
    on ONE image x [P,D], with the smallest relative margin (second - best) / second over every decision taken on distances:
    best against second-best medoid per non-medoid token in every assignment pass, the cost of the new medoid against the runner-up in
    every cluster of two or more members, and the farthest-point arg-max.  (The weighted branch's first medoids are a sort of the float32
    weights themselves, which the device holds bit for bit: no margin.)  -> (centers [K], assign [P], margin)"""
    d = sqdist64(x[None])[0].sqrt().numpy()
    P = d.shape[0]
    margin = float("inf")
    if w is None:
        wv = np.ones(P)
        chosen = np.zeros(P, bool)
        chosen[first] = True
        s_max = d[:, first].copy()
        s_max[first] = 0.0
        c = [int(first)]
        for _ in range(1, K):
            order = np.argsort(-s_max, kind="stable")
            margin = min(margin, (s_max[order[0]] - s_max[order[1]]) / s_max[order[0]])
            nw = int(order[0])
            c.append(nw)
            s_max = np.where(chosen, s_max, np.maximum(s_max, d[:, nw]))
            chosen[nw] = True
            s_max[nw] = 0.0
        c = np.asarray(c, np.int64)
    else:
        wv = np.asarray(w, np.float64)
        c = np.argsort(-wv, kind="stable")[:K].astype(np.int64)
    t = d.sum(1) * wv

    def assign(c):
        nonlocal margin
        rows = d[c, :]
        a = np.argmin(rows, axis=0)
        if len(c) > 1:
            part = np.partition(rows, 1, axis=0)
            m = (part[1] - part[0]) / part[1]
            m[c] = np.inf                                         # a medoid's own distance is 0 against a full distance
            margin = min(margin, float(m.min()))
        return a

    for _ in range(iters):
        a = assign(c)
        new = np.zeros_like(c)
        for k in range(len(c)):
            mem = np.nonzero(a == k)[0]
            if len(mem) == 0:
                continue
            order = mem[np.argsort(t[mem], kind="stable")]
            new[k] = order[0]
            if len(mem) > 1:
                margin = min(margin, _margin(t[order[0]], t[order[1]]))
        c = new
    return c, assign(c), margin


def trajectory_rel_bound(x, kind):
    """The path's relative distance bound on the patch rows x [B,P,D]: |q - q64| <= c (n_i + n_j) is c (n_i + n_j) / (2 q64) relative on the
    distance itself (worst off-diagonal pair), plus P u for the float32 row cost built from it."""
    B, P, D = x.shape
    q64, n = sqdist64(x), sqnorm64(x)
    rel = dist_coeff(kind, D) * (n[:, :, None] + n[:, None, :]) / (2.0 * q64)
    rel[:, torch.arange(P), torch.arange(P)] = 0.0
    return float(rel.max()) + P * U


def traj_inputs(P, D, seed, B=2):
    return case_input(P, D, B, seed), case_weights(P, B, seed=seed)


def traj_reference(P, K, D, iters, seed, weighted, first=0):
    """-> (centers [B,K], assign [B,P], smallest margin) of the float64 trajectory on traj_inputs."""
    x, part = traj_inputs(P, D, seed)
    w = replay_wrow(part)[:, 1:]
    res = [trajectory(x[b, 1:], K, iters, w[b] if weighted else None, None if weighted else first) for b in range(x.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), min(r[2] for r in res)


# ---------------------------------------------------------------------------------------------------------------- the measurement (CPU)
@functools.lru_cache(maxsize=None)
def _measure_case(P, D, B, seed=0):
    """-> (gram32 figure, split-emulation figure) of one input, both scalings for the first"""
    x = case_input(P, D, B, seed)[:, 1:]
    q64, n = sqdist64(x), sqnorm64(x)
    nn = n[:, :, None] + n[:, None, :]
    g = max(float(((unscale(gram32_dist(x, s), s) - q64).abs() / nn).max()) for s in (1.0, sqrt_d32(D)))
    e = float(((split_emulation(x) - q64).abs() / nn).max()) if D % 32 == 0 else 0.0
    return g, e


def measure(cases=None):
    """-> (GRAM32, SPLIT_EMU) per D over the Gram-form inputs of DIST_CASES and TRAJ_CASES (or `cases`: (kind, P, D, B, seed))"""
    if cases is None:
        cases = [(kind, P, D, B, 0) for kind, P, D, B in DIST_CASES if kind != "direct"]
        cases += [(kind, P, D, 2, seed) for P, _, D, _, seed in TRAJ_CASES for kind in ("gram", "split")]
    gram, split = {}, {}
    for kind, P, D, B, seed in cases:
        g, e = _measure_case(P, D, B, seed)
        gram[D] = max(gram.get(D, 0.0), g)
        if kind == "split":
            split[D] = max(split.get(D, 0.0), e)
    return gram, split


def _scan(n_seeds=40):
    for P, K, D, iters, _ in TRAJ_CASES:
        for seed in range(n_seeds):
            x = traj_inputs(P, D, seed)[0][:, 1:]
            need = TRAJ_FACTOR * max(trajectory_rel_bound(x, "gram"), trajectory_rel_bound(x, "split"))
            m = min(traj_reference(P, K, D, iters, seed, True)[2], *(traj_reference(P, K, D, iters, seed, False, f)[2] for f in (0, P - 1)))
            print(f"(P, K, D, iters) = ({P}, {K}, {D}, {iters}) seed {seed}: smallest margin {m:.3e}, needed {need:.3e} {'ok' if m >= need else ''}")


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1 and sys.argv[1] == "scan":
        _scan()
    else:
        gram, split = measure()
        print("GRAM32 =", {D: float(f"{v:.3e}") for D, v in sorted(gram.items())})
        print("SPLIT_EMU =", {D: float(f"{v:.3e}") for D, v in sorted(split.items())})
