"""ATS forward kernels (csrc/tr_ats.hip) at small, tied and long token counts, at op level.

  * decisions on an exact cdf (tests/_ats_ref.py): the device cdf is the constructed one bit for bit, so the ids are held to torch.cdist's
    own choice among near-equidistant entries, on both sides of cdist's 25-row threshold between its direct and its matmul form;
  * plateaus (the first entry of a run of equal values wins), collisions (most grid points on one token) and the dynamic width;
  * every length N = 2 .. 70 and the long ones up to 1025 tokens and 20 heads on random probabilities, cdf within the bound measured in
    tests/_ats_ref.py, ids exact on the device's own cdf;
  * the row gather in both precisions, width / narrow at the 256-thread block edge, and what the entry points refuse.
"""
import numpy as np
import pytest
import torch

import oracle
from tests import _ats_ref as R
from tests._params import assert_valid_sampling

pytestmark = pytest.mark.gpu

TABLES = {"small": R.SMALL, "boundary": R.BOUNDARY, "long": R.LONG}
ALL_CASES = [pytest.param(P, K, seed, id=f"{name}-P{P}-K{K}") for name, table in TABLES.items() for P, K, seed in table]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _sample(ops, cls_rows, qkv, mask, steps, K, f32):
    """-> (ids int64 [B,K], new_mask fp32 [B,K], cdf fp32 [B,P]) on the CPU"""
    ids, new_mask, cdf = ops.ats_sample(cls_rows.cuda(), (qkv if f32 else qkv.bfloat16()).cuda(), None if mask is None else mask.cuda(),
                                        steps.cuda(), K, want_cdf=True)
    return ids.cpu().long(), new_mask.cpu(), cdf.cpu()


def _check_against_oracle(ids, new_mask, cdf_for_ids, steps, K, what):
    want, want_mask = oracle.ats_ids_from_cdf(cdf_for_ids, steps, pad_to=K)
    for b in range(ids.shape[0]):
        assert np.array_equal(ids[b].numpy(), want[b].numpy()), f"{what} image {b}: ids {ids[b].tolist()} != torch.cdist's {want[b].tolist()}"
    assert np.array_equal(new_mask.numpy(), want_mask.float().numpy()), f"{what}: new_mask"
    return want


# ---------------------------------------------------------------------------------------- 3a: decisions on an exact cdf
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("P,K,seed", ALL_CASES)
def test_exact_cdf_decisions(ops, P, K, seed, f32, H):
    """cdf bit for bit, ids and new_mask torch.cdist's: direct form for P <= 25 and <= 25 grid points, matmul form otherwise.  Once padded
    to n_steps + 1 without a mask, once wider with a mask of ones.  (On the kernel that took the matmul form everywhere, all 44 SMALL cases
    with P >= 3 failed here with another token at one of the pairs, and every BOUNDARY and LONG case passed.)"""
    c = R.exact_case(P, K, H, seed)
    ns = len(c["steps"])
    for pad_to, mask in ((ns + 1, None), (ns + 4, c["mask"])):
        ids, new_mask, cdf = _sample(ops, c["cls_rows"], c["qkv"], mask, c["steps"], pad_to, f32)
        assert torch.equal(cdf, c["cdf"]), f"P={P} K={K}: device cdf is not the constructed one ({int((cdf != c['cdf']).sum())} entries differ)"
        _check_against_oracle(ids, new_mask, c["cdf"], c["steps"], pad_to, f"P={P} K={K} H={H} {R.form_of(P, K)} form, padded to {pad_to}")


# ---------------------------------------------------------------------------------------- 3b: plateaus and ties
def _plateau_units(P, K, run=9):
    """[4,P] cdf units: image r holds a run of `run + r` equal entries that starts at an index = r mod 4 and lies one unit above the middle
    grid point, nothing else within a quarter of the grid spacing.  -> (units, first index of the run per image, the grid point's index)"""
    s = oracle.ats_sample_steps(K).double().numpy()
    i = len(s) // 2
    a = int(np.rint(s[i] / R.UNIT)) + 1
    units, first = np.empty((4, P), np.int64), []
    for r in range(4):
        p0, L = 4 + r, run + r
        rest = P - p0 - L
        assert rest >= 1
        below = (np.arange(1, p0 + 1) * (a - R.TOTAL // (2 * K))) // p0                      # up to half a spacing below the run
        above = a + R.TOTAL // (2 * K) + (np.arange(1, rest + 1) * (R.TOTAL - a - R.TOTAL // (2 * K))) // rest
        units[r] = np.concatenate([below, np.full(L, a), above])
        first.append(p0)
    return units, first, i


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("P,K", [(24, 5), (25, 25), (40, 6), (200, 27)])
def test_plateau_takes_its_first_entry(ops, P, K, f32, H):
    """Runs of zero significance of length >= 8 starting at each residue of p mod 4: the grid point next to the run takes the run's FIRST
    entry -- torch's first minimum, the kernel's four-lane lexicographic combine."""
    units, first, i = _plateau_units(P, K)
    c = R.from_units(units, H, np.random.default_rng([P, K, H]))
    steps = oracle.ats_sample_steps(K)
    pad_to = len(steps) + 1
    ids, new_mask, cdf = _sample(ops, c["cls_rows"], c["qkv"], None, steps, pad_to, f32)
    assert torch.equal(cdf, c["cdf"])
    _check_against_oracle(ids, new_mask, c["cdf"], steps, pad_to, f"plateau P={P} K={K}")
    nearest = R.cdist_argmin(c["cdf"].numpy(), steps.numpy())
    for r in range(4):
        assert nearest[r, i] == first[r], "the test's own construction: the middle grid point's nearest value is the run"
        run = set(range(first[r] + 1, first[r] + 1 + 9 + r))                                   # 1-based ids of the run
        assert run & set(ids[r].tolist()) == {first[r] + 1}, f"image {r}: of the run {sorted(run)} the ids hold {sorted(run & set(ids[r].tolist()))}"


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("P,K,seed", [(17, 6, 7), (40, 11, 0)])
def test_all_zero_image(ops, P, K, seed, f32):
    """cls_rows of zeros: cdf exactly 0 everywhere (0 / 1e-6), every grid point takes entry 0."""
    c = R.exact_case(P, K, 3, seed)
    cls = c["cls_rows"].clone()
    cls[1, :, 1:] = 0
    pad_to = len(c["steps"]) + 1
    ids, new_mask, cdf = _sample(ops, cls, c["qkv"], None, c["steps"], pad_to, f32)
    want_cdf = c["cdf"].clone()
    want_cdf[1] = 0
    assert torch.equal(cdf, want_cdf)
    assert ids[1].tolist() == [0, 1] + [0] * (pad_to - 2) and new_mask[1].tolist() == [1.0, 1.0] + [0.0] * (pad_to - 2)
    _check_against_oracle(ids, new_mask, want_cdf, c["steps"], pad_to, f"all-zero image P={P} K={K}")


# ---------------------------------------------------------------------------------------- 3c: collisions, width, narrow
def _collision_units(P):
    """[4,P]: one token with all but a sliver of the mass (2 unique ids), two such tokens (3), an even spread (one id per grid point while
    P allows), and the heavy token in front (1)."""
    sliver = np.arange(1, P + 1, dtype=np.int64)
    t, t2 = P // 3, (2 * P) // 3
    one = np.where(np.arange(P) < t, sliver, R.TOTAL - (P - sliver))
    two = np.where(np.arange(P) < t, sliver, np.where(np.arange(P) < t2, R.TOTAL // 2 + sliver, R.TOTAL - (P - sliver)))
    even = (sliver * R.TOTAL) // P
    front = R.TOTAL - (P - sliver)
    return np.stack([one, two, even, front]), (t, t2)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("P,K,H", [(12, 6, 1), (30, 12, 3), (300, 40, 2)])
def test_collisions_width_narrow(ops, P, K, H, f32):
    units, (t, t2) = _collision_units(P)
    c = R.from_units(units, H, np.random.default_rng([P, K]))
    steps = oracle.ats_sample_steps(K)
    ns = len(steps)
    pad_to = ns + 1
    ids, new_mask, cdf = _sample(ops, c["cls_rows"], c["qkv"], None, steps, pad_to, f32)
    assert torch.equal(cdf, c["cdf"])
    _check_against_oracle(ids, new_mask, c["cdf"], steps, pad_to, f"collisions P={P} K={K}")
    pad = [0] * (pad_to - 4)
    assert ids[0].tolist() == [0, t, t + 1, 0] + pad                    # the last sliver below the heavy token, and the token
    assert ids[3].tolist() == [0, 1, 0, 0] + pad
    counts = (ids != 0).sum(1)
    assert counts[0] == 2 and 3 <= counts[1] < counts[2] <= ns and counts[3] == 1
    for rows in ([0, 1, 2, 3], [3, 0], [3], [0, 1, 3]):                 # batches of different maxima
        m, i = new_mask[rows].contiguous().cuda(), ids[rows].int().contiguous().cuda()
        width = ops.ats_width(m)
        assert width == 1 + int(counts[rows].max())
        ids_n, mask_n = ops.ats_narrow(i, m, width)
        assert ids_n.shape == (len(rows), width) and ids_n.is_contiguous() and mask_n.is_contiguous()
        assert torch.equal(ids_n.cpu().long(), ids[rows][:, :width]) and torch.equal(mask_n.cpu(), new_mask[rows][:, :width])
        assert bool((ids[rows][:, width:] == 0).all())


# ---------------------------------------------------------------------------------------- 3d: every length
def _random_length(ops, N, H, K, masked, f32):
    c = R.random_case(N, H, 0, masked, f32)
    steps = oracle.ats_sample_steps(K)
    pad_to = len(steps) + 1
    want_cdf = R.oracle_cdf(c["cls_rows"], c["qkv"], c["mask"])
    ids, new_mask, cdf = _sample(ops, c["cls_rows"], c["qkv"], c["mask"] if masked else None, steps, pad_to, f32)
    err, bound = float((cdf - want_cdf).abs().max()), R.cdf_bound(N)
    print(f"N={N} H={H} K={K} masked={masked} {'fp32' if f32 else 'bf16'}: cdf off by {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"N={N} H={H}: cdf off by {err:.3e} > {bound:.3e}"
    _check_against_oracle(ids, new_mask, cdf, steps, pad_to, f"N={N} H={H} K={K} masked={masked}")
    assert_valid_sampling((ids[:, 1:] - 1).numpy(), want_cdf.numpy(), steps.numpy(), tol=5e-4)
    if masked:                                                           # a masked (padded) token is never sampled: it lies 0.1 away
        assert bool(torch.gather(c["mask"], 1, ids).all())


@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
def test_every_short_length(ops, f32, masked):
    """N = 2 .. 70, one launch each; masked: one image with a masked tail, one with all but one patch masked."""
    for N in R.SWEEP_N:
        _random_length(ops, N, *R.sweep_shape(N), masked, f32)


@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N,H,K", R.LARGE)
def test_long_lengths(ops, N, H, K, f32, masked):
    """Up to 1025 tokens; 16 heads x 1024 tokens fill the default 64 KiB of dynamic LDS exactly, 20 heads take the raised limit; 63, 64
    and 65 grid points around the rounding of the grid-point loop."""
    _random_length(ops, N, H, K, masked, f32)


# ---------------------------------------------------------------------------------------- 3e: gather
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", [8, 64, 192, 384, 768, 1024])
def test_gather_rows(ops, D, f32):
    """Rows bit for bit torch.gather's; B * K = 21, 10 and 3 rows leave the last four-row block partly empty; ids with zero padding and
    repeated rows."""
    rng = np.random.default_rng([D, int(f32)])
    for B, K in ((3, 7), (2, 5), (1, 3)):
        N = K + 6
        x = torch.from_numpy(rng.standard_normal((B, N, D)).astype(np.float32))
        ao = torch.from_numpy(rng.standard_normal((B * N, D)).astype(np.float32))
        if not f32:
            ao = ao.bfloat16()
        ids = np.zeros((B, K), np.int64)
        for b in range(B):
            n = K - 1 - (b % 2)
            ids[b, 1:1 + n] = np.sort(rng.permutation(N - 1)[:n] + 1)
            ids[b, 2] = ids[b, 1]                                        # a repeated row
        ids[B - 1, K - 1] = N - 1                                        # the last row of the last image
        ids = torch.from_numpy(ids)
        xo, ao2 = ops.ats_gather(x.cuda(), ao.cuda(), ids.int().cuda())
        gi = ids[:, :, None].expand(B, K, D)
        assert xo.shape == (B, K, D) and ao2.shape == (B * K, D) and ao2.dtype == ao.dtype
        assert torch.equal(xo.cpu(), torch.gather(x, 1, gi)), f"x rows, D={D} B={B} K={K}"
        assert torch.equal(ao2.cpu().reshape(B, K, D), torch.gather(ao.reshape(B, N, D), 1, gi)), f"ao rows, D={D} B={B} K={K}"


# ---------------------------------------------------------------------------------------- 3f: width and narrow
@pytest.mark.parametrize("K", [2, 9])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])
def test_width_narrow_block_edges(ops, B, K):
    """One thread per image in blocks of 256: the widest row sits in the LAST image."""
    rng = np.random.default_rng([B, K])
    for widest in (K, max(1, K - 1)):
        n = rng.integers(1, widest + 1, B) if widest > 1 else np.ones(B, np.int64)
        n[:B - 1] = np.minimum(n[:B - 1], max(1, widest - 1))
        n[B - 1] = widest
        new_mask = (torch.arange(K)[None, :] < torch.from_numpy(n)[:, None]).float()
        ids = torch.from_numpy(rng.integers(1, 1000, (B, K))).int() * new_mask.int()
        m, i = new_mask.cuda(), ids.cuda()
        assert ops.ats_width(m) == widest
        for Kw in (1, K):
            ids_n, mask_n = ops.ats_narrow(i, m, Kw)
            assert torch.equal(ids_n.cpu(), ids[:, :Kw]) and torch.equal(mask_n.cpu(), new_mask[:, :Kw])


# ---------------------------------------------------------------------------------------- 3g: refusals
SENTINEL = -7


def _refused_sample(ops, N, H, n_grid, K, match):
    """tr_ats_sample on full-size buffers: an error return with `match` in the message, outputs untouched."""
    from tokenreduction_amd import _lib
    lib = _lib.load()
    cls = torch.full((1, H, N), 1.0 / N, device="cuda")
    qkv = torch.ones(N, 3 * H * 64, dtype=torch.bfloat16, device="cuda")
    steps = torch.linspace(0.1, 0.9, n_grid, device="cuda")
    ids = torch.full((1, K), SENTINEL, dtype=torch.int32, device="cuda")
    new_mask = torch.full((1, K), float(SENTINEL), device="cuda")
    rc = lib.tr_ats_sample(cls.data_ptr(), qkv.data_ptr(), 0, None, steps.data_ptr(), n_grid, ids.data_ptr(), new_mask.data_ptr(), None,
                           1, N, H, K, ops._stream())
    assert rc != 0
    with pytest.raises(RuntimeError, match=match):
        _lib.check(rc, "tr_ats_sample")
    torch.cuda.synchronize()
    assert bool((ids == SENTINEL).all()) and bool((new_mask == SENTINEL).all()), "a refused call wrote its outputs"


@pytest.mark.parametrize("N,H,n_grid,K,match", [(1, 1, 1, 2, r"need 2 <= N <= 1025 \(N=1\)"),
                                                (1026, 1, 4, 5, r"need 2 <= N <= 1025 \(N=1026\)"),
                                                (40, 2, 6, 6, r"6 grid points cannot exceed K-1 = 5"),
                                                (40, 2, 1, 1, r"cannot exceed K-1 = 0"),
                                                (1025, 33, 8, 9, r"33 heads x 1024 tokens do not fit")])
def test_sample_refuses(ops, N, H, n_grid, K, match):
    _refused_sample(ops, N, H, n_grid, K, match)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", [1032, 12])
def test_gather_refuses(ops, D, f32):
    x = torch.zeros(2, 5, D, device="cuda")
    ao = torch.zeros(10, D, device="cuda", dtype=torch.float32 if f32 else torch.bfloat16)
    ids = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=rf"tr_ats_gather: bad shape B=2 N=5 K=3 D={D}"):
        ops.ats_gather(x, ao, ids)


def test_narrow_refuses(ops):
    ids = torch.zeros(4, 3, dtype=torch.int32, device="cuda")
    new_mask = torch.zeros(4, 3, device="cuda")
    with pytest.raises(RuntimeError, match=r"tr_ats_narrow: bad shape B=3 K=3 Kw=4"):
        ops.ats_narrow(ids[:3], new_mask[:3], 4)                         # the fourth row backs what a launch would have read
