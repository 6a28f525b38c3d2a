"""CPU checks of tests/_cluster_ref.py, the checker behind tests/test_hip_cluster_stages.py: fed the oracle's own float64 distance matrix
the replays reproduce the oracle decision for decision; the float64 trajectory is the oracle's; the checker fails on each kind of damage
it exists to find; the committed constants and trajectory seeds hold."""
import numpy as np
import pytest
import torch

import oracle
from oracle.cluster import kmedoids_init_equal
from tests import _cluster_ref as R

F64 = torch.float64


def _x64(P, D, B, seed=11):
    return torch.randn(B, P, D, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ------------------------------------------------------------------------------------------------------------------ replays == oracle
@pytest.mark.parametrize("P,K,D,iters", [(70, 9, 32, 3), (40, 17, 16, 1), (20, 5, 16, 2), (33, 33, 16, 1), (30, 1, 16, 3)])
def test_replays_reproduce_the_oracle_kmedoids(P, K, D, iters):
    B = 3
    x = _x64(P, D, B)
    w = torch.rand(B, P, 1, generator=torch.Generator().manual_seed(5), dtype=F64)
    dist = torch.cdist(x, x)
    t = torch.sum(dist * w, dim=-1)
    _, want_c, want_a = oracle.kmedoids_fit(x, K, iters, w)
    for b in range(B):
        c0 = R.replay_weighted_init(torch.cat([torch.zeros(1, dtype=F64), w[b, :, 0]]), K)
        c, a = R.replay_kmed_iterate(dist[b], t[b], c0, iters)
        assert np.array_equal(c, want_c[b].numpy()) and np.array_equal(a, want_a[b].numpy())
    for first in (0, P - 1, P // 2):
        want_init = kmedoids_init_equal(x, K, first)
        _, want_c, want_a = oracle.kmedoids_fit(x, K, iters, None, first)
        for b in range(B):
            c0 = R.replay_kmed_init_equal(dist[b], K, first)
            assert np.array_equal(c0, want_init[b].numpy())
            c, a = R.replay_kmed_iterate(dist[b], dist[b].sum(-1), c0, iters)
            assert np.array_equal(c, want_c[b].numpy()) and np.array_equal(a, want_a[b].numpy())


def test_replay_empty_cluster_falls_to_index_0():
    """Two identical first medoids: the second one's cluster is empty (ties go to the smallest k) and its medoid becomes token 0."""
    x = _x64(12, 16, 1)
    x[0, 3] = x[0, 7]
    dist = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist")
    w = torch.ones(1, 12, 1, dtype=F64)
    _, want_c, want_a = oracle.kmedoids_fit(x, 3, 1, w, forced_init=torch.tensor([[3, 7, 9]]))
    c, a = R.replay_kmed_iterate(dist[0], dist[0].sum(-1), [3, 7, 9], 1)
    assert c[1] == 0 and np.array_equal(c, want_c[0].numpy()) and np.array_equal(a, want_a[0].numpy())


@pytest.mark.parametrize("P,K,k", [(60, 9, 5), (26, 26, 1), (20, 1, 8), (130, 8, 5)])
def test_replays_reproduce_the_oracle_dpcknn(P, K, k):
    B, D = 2, 16
    x = _x64(P, D, B)
    noise = torch.rand(B, P, generator=torch.Generator().manual_seed(2), dtype=F64)
    dist = oracle.dpcknn_distances(x)
    density, _, score = oracle.dpcknn_scores(dist, noise, k)
    want64, _ = R.density64(dist, noise, k)
    torch.testing.assert_close(want64, density, rtol=1e-14, atol=0)
    centers = torch.sort(score, dim=-1, descending=True, stable=True).indices[:, :K]
    want_idx = oracle.dpcknn_assign(dist, centers)
    for b in range(B):
        sc = R.replay_parent_score(dist[b], density[b], dist[b].max(-1).values)
        assert np.array_equal(sc, score[b].numpy())
        assert np.array_equal(R.replay_centers(score[b], K), centers[b].numpy())
        assert np.array_equal(R.replay_assign(dist[b], centers[b].numpy()), want_idx[b].numpy())


@pytest.mark.parametrize("P,K,D,iters,seed", R.TRAJ_CASES + [(30, 4, 16, 2, 0)])
def test_trajectory_is_the_oracle_in_float64(P, K, D, iters, seed):
    x, part = R.traj_inputs(P, D, seed)
    xs = x[:, 1:].double()
    w = torch.from_numpy(R.replay_wrow(part))[:, 1:].double().unsqueeze(2)
    _, want_c, want_a = oracle.kmedoids_fit(xs, K, iters, w)
    c, a, margin = R.traj_reference(P, K, D, iters, seed, True)
    assert np.array_equal(c, want_c.numpy()) and np.array_equal(a, want_a.numpy()) and 0 < margin < 1
    for first in (0, P - 1):
        _, want_c, want_a = oracle.kmedoids_fit(xs, K, iters, None, first)
        c, a, margin = R.traj_reference(P, K, D, iters, seed, False, first)
        assert np.array_equal(c, want_c.numpy()) and np.array_equal(a, want_a.numpy()) and 0 < margin < 1


@pytest.mark.parametrize("P,K,D,iters,seed", R.TRAJ_CASES)
def test_committed_trajectory_seeds_are_decided(P, K, D, iters, seed):
    """The smallest relative margin of every trajectory the GPU test runs is at least 8 x the relative distance bound of either path."""
    x = R.traj_inputs(P, D, seed)[0][:, 1:]
    need = R.TRAJ_FACTOR * max(R.trajectory_rel_bound(x, "gram"), R.trajectory_rel_bound(x, "split"))
    margins = [R.traj_reference(P, K, D, iters, seed, True)[2]] + [R.traj_reference(P, K, D, iters, seed, False, f)[2] for f in (0, P - 1)]
    print(f"(P, K, D, iters) = ({P}, {K}, {D}, {iters}) seed {seed}: margins {margins}, needed {need:.3e}")
    assert min(margins) >= need


# ------------------------------------------------------------------------------------------------------------------ constants
def test_committed_constants_cover_the_small_cases():
    """Re-measures the cases of up to 129 tokens (the whole table: `python -m tests._cluster_ref`); none exceeds the committed figure."""
    cases = [(kind, P, D, B, 0) for kind, P, D, B in R.DIST_CASES if kind != "direct" and P <= 129]
    gram, split = R.measure(cases)
    assert gram and split
    for D, v in gram.items():
        assert v <= R.GRAM32[D] * 1.001, (D, v)
    for D, v in split.items():
        assert v <= R.SPLIT_EMU[D] * 1.001, (D, v)
    for kind, P, D, B in R.DIST_CASES:
        if kind != "direct":
            assert 0 < R.dist_coeff(kind, D) < 1e-4
    assert {D for kind, _, D, _ in R.DIST_CASES if kind == "split"} <= set(R.SPLIT_EMU)


def test_workspace_views_follow_the_layout():
    B, N = 2, 6
    P = N - 1
    ws = torch.arange(B * P * P + B * (3 * P + N) + 64 + B, dtype=torch.float32)
    v = R.workspace_views(ws, B, N, "kmedoids")
    assert v["dist"].shape == (B, P, P) and v["nrm"][0, 0] == B * P * P and v["t"][0, 0] == B * P * P + B * P
    assert v["wrow"].shape == (B, N) and v["wrow"][0, 0] == B * P * P + 2 * B * P
    v = R.workspace_views(ws, B, N, "dpcknn")
    assert v["rowmax"][1, 0] == B * P * P + P and v["density"][0, 0] == B * P * P + B * P and v["score_rows"][1, 0] == B * P * P + 2 * B * P + N


def test_skipped_tiles():
    """257 tokens: the second row tile (row 256) skips its first two column tiles; 576: 6 of the 15 tiles."""
    assert not R.skipped_mask(256).any()
    m = R.skipped_mask(257)
    assert m[256, :256].all() and not m[256, 256:].any() and not m[:256].any()
    m = R.skipped_mask(576)
    tiles = {(i // R.GT, j // R.GTN) for i, j in torch.nonzero(m).tolist()}
    assert tiles == {(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3)}
    assert not (m & m.t()).any()                                 # the mirror of a skipped element is computed


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _emulated_split(P, D, B):
    """What a correct split kernel would leave, from the float64 emulation: float32, exactly symmetric."""
    x = R.case_input(P, D, B)[:, 1:]
    q = R.split_emulation(x)
    q = torch.triu(q) + torch.triu(q, 1).transpose(1, 2)
    return x, q.clamp_min(1e-30).sqrt().float()


def test_check_dist_is_sensitive():
    P, D, B = 257, 32, 2
    x, dist = _emulated_split(P, D, B)
    q64 = R.check_dist(dist, x, 1.0, "split")
    bad = dist.clone()
    bad[1, 200, 7] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        R.check_dist(bad, x, 1.0, "split", q64)
    bad = dist.clone()
    bad.view(torch.int32)[1, 256, 5] += 1                        # one ulp, in the region the kernel stores as a mirror image
    with pytest.raises(AssertionError, match="bitwise mirror"):
        R.check_dist(bad, x, 1.0, "split", q64)
    bad = dist.clone()
    bad[0, 3, 90] *= 1.0 + 1e-4                                  # a wrong element outside it
    with pytest.raises(AssertionError, match=r"element \(3, 90\) in tile \(0, 0\)"):
        R.check_dist(bad, x, 1.0, "split", q64)
    # the same matrix is far outside the fp32 kernel's bound: the two bounds are not interchangeable
    with pytest.raises(AssertionError):
        R.check_dist(dist, x, 1.0, "gram", q64)


@pytest.mark.parametrize("drop", ["hl", "lh"])
def test_a_missing_cross_term_exceeds_the_split_bound(drop):
    P, D, B = 129, 128, 2
    x = R.case_input(P, D, B)[:, 1:]
    q64, n = R.sqdist64(x), R.sqnorm64(x)
    err = ((R.split_emulation(x, drop) - q64).abs() / (n[:, :, None] + n[:, None, :])).max().item()
    assert err > 10 * R.dist_coeff("split", D), (err, R.dist_coeff("split", D))
    with pytest.raises(AssertionError, match="against float64"):
        R.check_dist(R.split_emulation(x, drop).clamp_min(1e-30).sqrt().float(), x, 1.0, "split", q64)


def test_direct_bound_and_diagonal():
    P, D, B = 25, 16, 2
    x = R.case_input(P, D, B)[:, 1:]
    dist = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist") / torch.tensor(R.sqrt_d32(D))
    R.check_dist(dist, x, R.sqrt_d32(D), "direct")
    bad = dist.clone()
    bad[0, 4, 4] = 1e-20
    with pytest.raises(AssertionError, match="diagonal"):
        R.check_dist(bad, x, R.sqrt_d32(D), "direct")
    with pytest.raises(AssertionError):                          # the Gram form's diagonal residue is not a direct-kernel result
        R.check_dist(R.gram32_dist(x, 1.0), x, 1.0, "direct")


def _emulated_kmedoids(P, K, D, iters, first=None):
    """The workspace and outputs a correct device would leave, in float32 on the CPU."""
    B = 2
    x, part = R.case_input(P, D, B), R.case_weights(P, B)
    dist = R.gram32_dist(x[:, 1:], 1.0)
    wrow = torch.from_numpy(R.replay_wrow(part)) if first is None else torch.ones(B, P + 1)
    v = {"dist": dist, "wrow": wrow, "t": (dist * wrow[:, 1:, None]).sum(-1)}
    cs, as_ = [], []
    for b in range(B):
        c0 = R.replay_weighted_init(wrow[b], K) if first is None else R.replay_kmed_init_equal(dist[b], K, first)
        c, a = R.replay_kmed_iterate(dist[b], v["t"][b], c0, iters)
        cs.append(c), as_.append(a)
    return v, (part if first is None else None), np.stack(cs), np.stack(as_)


@pytest.mark.parametrize("first", [None, 4])
def test_check_kmedoids_is_sensitive(first):
    P, K, iters = 65, 9, 3
    v, part, c, a = _emulated_kmedoids(P, K, 32, iters, first)
    R.check_kmedoids(v, part, first, K, iters, c, a)
    bad = a.copy()
    bad[1, 64] = (bad[1, 64] + 1) % K                            # one assignment changed
    with pytest.raises(AssertionError, match="assignment differs"):
        R.check_kmedoids(v, part, first, K, iters, c, bad)
    bad = c.copy()
    bad[0, 8] = (bad[0, 8] + 1) % P
    with pytest.raises(AssertionError, match="medoids differ"):
        R.check_kmedoids(v, part, first, K, iters, bad, a)
    vb = dict(v, t=v["t"] * (1 + 1e-4))
    with pytest.raises(AssertionError, match="row cost"):
        R.check_kmedoids(vb, part, first, K, iters, c, a)
    vb = dict(v, wrow=torch.from_numpy(np.nextafter(v["wrow"].numpy(), np.float32(9))))
    with pytest.raises(AssertionError, match="wrow"):
        R.check_kmedoids(vb, part, first, K, iters, c, a)


def test_check_dpcknn_is_sensitive():
    B, P, D, K, k = 2, 70, 32, 9, 5
    x = R.case_input(P, D, B)
    noise = torch.rand(B, P, generator=torch.Generator().manual_seed(1))
    dist = R.gram32_dist(x[:, 1:], R.sqrt_d32(D))
    near = torch.topk(dist, k=k, dim=-1, largest=False).values
    density = (-(near ** 2).mean(-1)).exp() + noise * 1e-6
    rowmax = dist.max(-1).values
    scores = torch.from_numpy(np.stack([R.replay_parent_score(dist[b], density[b], rowmax[b]) for b in range(B)]))
    v = {"dist": dist, "rowmax": rowmax, "density": density, "score_rows": torch.cat([torch.zeros(B, 1), scores], 1)}
    centers = np.stack([R.replay_centers(scores[b], K) for b in range(B)])
    idx = np.stack([R.replay_assign(dist[b], centers[b]) for b in range(B)])
    R.check_dpcknn(v, noise, k, K, centers, idx, scores)
    bad = idx.copy()
    bad[1, 69] = (bad[1, 69] + 1) % K
    with pytest.raises(AssertionError, match="assignment differs"):
        R.check_dpcknn(v, noise, k, K, centers, bad, scores)
    bad = centers.copy()
    bad[0, [7, 8]] = bad[0, [8, 7]]
    with pytest.raises(AssertionError, match="centres"):
        R.check_dpcknn(v, noise, k, K, bad, idx, scores)
    with pytest.raises(AssertionError, match="density"):
        R.check_dpcknn(dict(v, density=density * (1 + 1e-5)), noise, k, K, centers, idx, scores)
    bad = scores.clone()
    bad.view(torch.int32)[0, 3] += 1
    with pytest.raises(AssertionError, match="scores"):
        R.check_dpcknn(v, noise, k, K, centers, idx, bad)
    with pytest.raises(AssertionError, match="row maxima"):
        R.check_dpcknn(dict(v, rowmax=rowmax * 2), noise, k, K, centers, idx, scores)
