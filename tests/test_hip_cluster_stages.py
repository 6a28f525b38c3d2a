"""GPU parity of the clustering kernels (csrc/tr_cluster.hip), stage by stage, through the caller-owned workspace of ops.dpcknn_cluster,
ops.kmedoids and ops.kmedoids_equal.

Only the distance matrix and the density's expf are floating-point work: they are held against float64 within the bounds of
tests/_cluster_ref.py (derived, or measured on the CPU from the reference alone).  Everything after them is comparison logic and is held
EXACTLY -- no tolerance, no share of cases left out -- against the replays of _cluster_ref.py, fed the device's own dist, t, wrow, density
and rowmax, for every image.  On inputs whose float64 trajectory is decided by a margin of 8 x the distance bound, the K-Medoids results
equal the float64 trajectory itself.

Every call gets a workspace of the required size plus 256 floats, filled with a NaN bit pattern: afterwards every element of dist is
finite (a hole in the mirror coverage of dist_mfma_kernel would leave the pattern there) and the 256 extra floats are bitwise untouched.
The CLS row of every input is NaN: no clustering kernel may read it.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _cluster_ref as R

pytestmark = pytest.mark.gpu

NAN_BITS, TAIL = 0x7FA5A5A5, 256
U = R.U


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


class _Ws:
    """The caller-owned workspace of one call: NaN pattern everywhere, TAIL extra floats."""

    def __init__(self, ops, B, N):
        self.B, self.N = B, N
        self.need = ops.cluster_workspace_floats(B, N)
        self.bits = torch.full((self.need + TAIL,), NAN_BITS, dtype=torch.int32, device="cuda")
        self.ws = self.bits.view(torch.float32)

    def read(self, family):
        """-> CPU views of the stage intermediates, after the checks common to every case"""
        torch.cuda.synchronize()
        assert bool((self.bits[self.need:] == NAN_BITS).all()), "the floats behind the workspace were written"
        v = R.workspace_views(self.ws.cpu(), self.B, self.N, family)
        bad = ~torch.isfinite(v["dist"])
        if bool(bad.any()):
            raise AssertionError(f"{int(bad.sum())} elements of dist are not finite, first at (image, row, column) = "
                                 f"{[int(t[0]) for t in torch.nonzero(bad, as_tuple=True)]}")
        return v


@functools.lru_cache(maxsize=4)
def _q64(P, D, B):
    return R.sqdist64(R.case_input(P, D, B)[:, 1:])


def _run_dist(ops, x, entry, fast):
    """One call of either entry point that leaves dist -> (views, sqrt_d)"""
    B, N, D = x.shape
    w = _Ws(ops, B, N)
    if entry == "kmedoids":
        ops.kmedoids_equal(x.cuda(), 0, 1, 0, fast_dist=fast, ws=w.ws)
        return w.read("kmedoids"), 1.0
    ops.dpcknn_cluster(x.cuda(), 1, None, k=1, fast_dist=2 * fast, ws=w.ws)
    return w.read("dpcknn"), R.sqrt_d32(D)


# ------------------------------------------------------------------------------------------------------------------ (a) distance matrices
@pytest.mark.parametrize("kind,P,D,B", R.DIST_CASES, ids=lambda v: str(v))
def test_distance_matrix(ops, kind, P, D, B):
    """dist of both entry points (sqrt_d = 1 and sqrt(D)) against float64, every element, within the kernel's bound; symmetry; for the
    split kernel the pairs stored as mirror images bitwise symmetric."""
    fast = int(kind == "split")
    assert R.kernel_for(P, D, fast) == kind
    x = R.case_input(P, D, B)
    q64 = _q64(P, D, B)
    for entry in ("kmedoids", "dpcknn"):
        v, sqrt_d = _run_dist(ops, x, entry, fast)
        R.check_dist(v["dist"], x[:, 1:], sqrt_d, kind, q64)
        if entry == "kmedoids":
            # sqnorm_kernel: at most 16 fma per lane and 6 additions across the wave on any path (D <= 1024)
            n64 = R.sqnorm64(x[:, 1:])
            err = ((v["nrm"].double() - n64).abs() / n64).max().item()
            assert err <= 22 * U, f"squared norms off by {err:.3e} relative"


@pytest.mark.parametrize("P", [26, 65])
def test_fast_path_falls_back_to_the_fp32_kernel(ops, P):
    """D % 32 != 0: the fast path must take dist_kernel<false>; bit-identical to fast_dist = 0 through both entry points."""
    x = R.case_input(P, 48, 2)
    for entry in ("kmedoids", "dpcknn"):
        slow, _ = _run_dist(ops, x, entry, 0)
        fast, sqrt_d = _run_dist(ops, x, entry, 1)
        assert torch.equal(slow["dist"].view(torch.int32), fast["dist"].view(torch.int32)), entry
        R.check_dist(fast["dist"], x[:, 1:], sqrt_d, "gram")


def test_workspace_argument(ops):
    """ws=None and a caller-owned workspace give the same bits; a workspace that cannot serve raises ValueError."""
    B, P, D, K = 2, 70, 32, 9
    x, part, noise = R.case_input(P, D, B).cuda(), R.case_weights(P, B).cuda(), torch.rand(B, P).cuda()
    need = ops.cluster_workspace_floats(B, P + 1)
    assert need == B * P * P + B * (3 * P + P + 1) + 64 + B                       # tr_dpcknn_workspace_floats
    for call in (lambda ws: ops.kmedoids(x, part, K, 3, fast_dist=1, ws=ws), lambda ws: ops.kmedoids_equal(x, 5, K, 3, ws=ws),
                 lambda ws: ops.dpcknn_cluster(x, K, noise, k=5, fast_dist=2, ws=ws)):
        want = call(None)
        got = call(torch.empty(need, device="cuda"))
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        for bad in (torch.empty(need - 1, device="cuda"), torch.empty(need, device="cuda", dtype=torch.float64), torch.empty(need),
                    torch.empty(2 * need, device="cuda")[::2]):
            with pytest.raises(ValueError):
                call(bad)


# ------------------------------------------------------------------------------------------------------------------ (b) K-Medoids decisions
def _check_kmedoids(v, x, part, first, K, iters, centers, assign, what):
    return R.check_kmedoids(v, part, first, K, iters, centers.cpu().numpy(), assign.cpu().numpy(), what)


@pytest.mark.parametrize("P", [2, 64, 65, 196, 577, 1024])
def test_kmedoids_decisions(ops, P):
    """Every (K, iters) of the chunk and iteration edges, both distance paths, weighted and equal-weight: medoids and assignment equal
    the replay.  iters = 0 exposes the initialisation alone.  Beyond 196 tokens the equal-weight call takes ONE of the three first
    medoids per combination, in rotation (every value is reached at every length)."""
    B, D = 2, 32
    x, part = R.case_input(P, D, B), R.case_weights(P, B)
    xd, pd = x.cuda(), part.cuda()
    firsts = sorted({0, P - 1, P // 3})
    n = 0
    for K in sorted({k for k in (1, 8, 9, 16, 17, P) if k <= P}):
        for iters in (0, 1, 3):
            for fast in (0, 1):
                w = _Ws(ops, B, P + 1)
                c, a = ops.kmedoids(xd, pd, K, iters, fast_dist=fast, ws=w.ws)
                _check_kmedoids(w.read("kmedoids"), x, part, None, K, iters, c, a, f"weighted P={P} K={K} iters={iters} fast={fast}")
                n += 1
                for first in (firsts if P <= 196 else [firsts[n % len(firsts)]]):
                    w = _Ws(ops, B, P + 1)
                    c, a = ops.kmedoids_equal(xd, first, K, iters, fast_dist=fast, ws=w.ws)
                    _check_kmedoids(w.read("kmedoids"), x, None, first, K, iters, c, a,
                                    f"equal P={P} K={K} iters={iters} fast={fast} first={first}")


@pytest.mark.parametrize("P,D", [(16, 16), (70, 32)])
def test_kmedoids_duplicated_tokens(ops, P, D):
    """The first eight patch rows are identical and, on the weighted path, carry the largest weights: exact ties between the first eight
    medoids (every token goes to the smallest k), empty clusters, the fall to index 0."""
    B, K = 2, 9
    x, part = R.case_input(P, D, B), R.case_weights(P, B)
    x[:, 1:9] = x[:, 1:2]
    part[:, :, :, 1:9] += 1.0
    for iters in (0, 1, 3):
        for fast in (0, 1):
            w = _Ws(ops, B, P + 1)
            c, a = ops.kmedoids(x.cuda(), part.cuda(), K, iters, fast_dist=fast, ws=w.ws)
            v = w.read("kmedoids")
            rep = _check_kmedoids(v, x, part, None, K, iters, c, a, f"duplicates weighted P={P} iters={iters} fast={fast}")
            if iters == 0:
                assert all(set(rep[b][:8]) == set(range(8)) for b in range(B))     # the duplicated rows are the first medoids
                assert not np.isin(a.cpu().numpy(), np.arange(1, 8)).any()          # the tie between them goes to the smallest k
            else:
                assert all((rep[b] == 0).sum() >= 2 for b in range(B)), rep        # empty clusters fell to index 0
            for first in (0, P - 1):
                w = _Ws(ops, B, P + 1)
                c, a = ops.kmedoids_equal(x.cuda(), first, K, iters, fast_dist=fast, ws=w.ws)
                _check_kmedoids(w.read("kmedoids"), x, None, first, K, iters, c, a, f"duplicates equal P={P} iters={iters} fast={fast} first={first}")


# ------------------------------------------------------------------------------------------------------------------ (c) DPC-KNN stages
@pytest.mark.parametrize("P", [26, 208, 209, 256, 257, 288, 576, 1024])
def test_dpcknn_stages(ops, P):
    """Density within its derived bound of float64 on the device's matrix; then bit for bit: row maxima, parent scores, centres, the
    assignment.  256 / 257 is the switch to 16 elements per lane in density_kernel and parent_score_kernel."""
    B, D = 2, 32
    x = R.case_input(P, D, B)
    noise = torch.rand(B, P, generator=torch.Generator().manual_seed(P))
    for k in (1, 5, 8):
        for K in sorted({1, 8, 9, P}):
            for fast in (0, 2):
                what = f"P={P} k={k} K={K} fast={fast}"
                nz = None if (k, K) == (1, 1) else noise                           # one combination without the noise input
                w = _Ws(ops, B, P + 1)
                centers, idx, scores = ops.dpcknn_cluster(x.cuda(), K, None if nz is None else nz.cuda(), k=k, fast_dist=fast, ws=w.ws)
                v = w.read("dpcknn")
                R.check_dpcknn(v, nz, k, K, centers.cpu().numpy(), idx.cpu().numpy(), scores.cpu(), what)


# ------------------------------------------------------------------------------------------------------------------ (d) float64 trajectory
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("P,K,D,iters,seed", R.TRAJ_CASES)
def test_kmedoids_equals_the_float64_trajectory(ops, P, K, D, iters, seed, weighted, fast):
    """On inputs whose float64 trajectory takes every decision with a relative margin of at least 8 x the path's relative distance bound,
    the device's medoids and assignment ARE the float64 trajectory's."""
    x, part = R.traj_inputs(P, D, seed)
    kind = R.kernel_for(P, D, fast)
    need = R.TRAJ_FACTOR * R.trajectory_rel_bound(x[:, 1:], kind)
    for first in ([None] if weighted else [0, P - 1]):
        want_c, want_a, margin = R.traj_reference(P, K, D, iters, seed, weighted, first)
        assert margin >= need, f"the float64 trajectory is not decided: margin {margin:.3e} < {need:.3e}"
        w = _Ws(ops, x.shape[0], P + 1)
        if weighted:
            c, a = ops.kmedoids(x.cuda(), part.cuda(), K, iters, fast_dist=fast, ws=w.ws)
        else:
            c, a = ops.kmedoids_equal(x.cuda(), first, K, iters, fast_dist=fast, ws=w.ws)
        w.read("kmedoids")
        assert np.array_equal(c.cpu().numpy(), want_c), f"medoids differ from the float64 trajectory (margin {margin:.3e})"
        assert np.array_equal(a.cpu().numpy(), want_a), f"assignment differs from the float64 trajectory (margin {margin:.3e})"
