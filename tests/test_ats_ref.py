"""CPU checks of tests/_ats_ref.py: the exact-cdf inputs are exact, the two fp32 emulations are torch.cdist's two forms on their own
domains, and every table case can tell a kernel that takes the wrong form from one that takes the right one.  What the GPU tests of
tests/test_hip_ats_edges.py then hold the kernel to is torch.cdist itself; if torch's choice of form ever moves, it shows here."""
import functools

import numpy as np
import pytest
import torch

import oracle
from tests import _ats_ref as R

HEADS = (1, 3)
TABLES = {"small": R.SMALL, "boundary": R.BOUNDARY, "long": R.LONG}
ALL_CASES = [pytest.param(name, P, K, seed, id=f"{name}-P{P}-K{K}") for name, table in TABLES.items() for P, K, seed in table]


@functools.lru_cache(maxsize=None)
def _case(P, K, H, seed):
    return R.exact_case(P, K, H, seed)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def test_tables_hold_what_they_are_for():
    assert {(3, 2), (7, 3), (9, 5), (15, 8), (17, 6), (25, 13), (25, 20), (1, 2), (25, 26)} <= {(P, K) for P, K, _ in R.SMALL}
    assert R.n_steps(26) == 25 and R.n_steps(27) == 27                   # the float arange lets the end point in at K = 27
    assert all(R.form_of(P, K) == "direct" for P, K, _ in R.SMALL)
    assert all(R.form_of(P, K) == "matmul" for P, K, _ in R.BOUNDARY + R.LONG)
    assert any(P == 26 for P, _, _ in R.BOUNDARY) and (25, 27) in {(P, K) for P, K, _ in R.BOUNDARY}
    assert {196, 576, 1024} <= {P for P, _, _ in R.LONG} and (1024, 26) in {(P, K) for P, K, _ in R.LONG}
    assert {R.n_steps(K) for N, _, K in R.LARGE if N == 130} == {63, 64, 65}
    assert set(R.MEASURED) == {R.length_key(N) for N, _, _ in R.random_cases()}


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("name,P,K,seed", ALL_CASES)
def test_exact_cdf(name, P, K, seed, H):
    """The constructed cdf is the oracle's and the kernel restatement's, bit for bit, with fp32 and with bf16 values."""
    c = _case(P, K, H, seed)
    assert c["cdf"].shape == (R.EXACT_B, P) and bool((c["cdf"][:, -1] == 1.0).all())
    assert torch.equal(c["qkv"].bfloat16().float(), c["qkv"])
    want = _bits(c["cdf"])
    assert np.array_equal(_bits(R.oracle_cdf(c["cls_rows"], c["qkv"], c["mask"])), want)
    assert np.array_equal(_bits(R.kernel_cdf(c["cls_rows"], c["qkv"], c["mask"])), want)
    assert np.array_equal(_bits(R.kernel_cdf(c["cls_rows"], c["qkv"], None)), want)


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("name,P,K,seed", ALL_CASES)
def test_emulations_are_cdist_on_their_domains(name, P, K, seed, H):
    c = _case(P, K, H, seed)
    cdf, steps = c["cdf"].numpy(), c["steps"].numpy()
    emu = R.direct_form_argmin if R.form_of(P, K) == "direct" else R.matmul_form_argmin
    assert np.array_equal(emu(cdf, steps), R.cdist_argmin(cdf, steps)), f"torch.cdist does not take its {R.form_of(P, K)} form at P={P}, {len(steps)} grid points"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("N,H,K", [(N, *R.sweep_shape(N)) for N in (2, 3, 17, 26, 27, 70)] + [(130, 6, 65), (257, 16, 129), (1025, 16, 513)])
def test_emulations_on_random_cdfs(N, H, K, masked):
    """The same on the random inputs of the every-length GPU test (the restated kernel cdf, masked plateaus at +0.1 included)."""
    c = R.random_case(N, H, 0, masked, True)
    cdf, steps = R.kernel_cdf(c["cls_rows"], c["qkv"], c["mask"]), oracle.ats_sample_steps(K).numpy()
    emu = R.direct_form_argmin if R.form_of(N - 1, K) == "direct" else R.matmul_form_argmin
    assert np.array_equal(emu(cdf, steps), R.cdist_argmin(cdf, steps))


@pytest.mark.parametrize("H", HEADS)
def test_every_case_tells_the_forms_apart(H):
    """A condition on the inputs, not a measurement: with these a kernel that keeps one form everywhere, or moves the threshold by one,
    gives other ids than torch.cdist.  (P < 3 leaves no room for a pair: module docstring of _ats_ref.)"""
    count = {name: [] for name in TABLES}
    for name, table in TABLES.items():
        for P, K, seed in table:
            c = _case(P, K, H, seed)
            n = R.telling_decisions(c["cdf"].numpy(), c["steps"].numpy(), P, K)
            print(f"{name} P={P} K={K} H={H}: {n} of {R.EXACT_B * len(c['steps'])} decisions differ between the two forms")
            count[name].append(n)
            if P >= 3:
                assert n >= 1, f"{name} (P, K) = ({P}, {K}) seed {seed}: no decision tells the forms apart"
    assert sum(count["small"]) >= R.MIN_SMALL_TOTAL
    assert min(count["long"]) >= R.MIN_LONG_EACH


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("name,P,K,seed", ALL_CASES)
def test_ids_are_sorted_unique_zero_padded(name, P, K, seed, H):
    c = _case(P, K, H, seed)
    ns = len(c["steps"])
    for pad_to in (ns + 1, ns + 4):
        ids, new_mask = oracle.ats_ids_from_cdf(c["cdf"], c["steps"], pad_to=pad_to)
        assert ids.shape == (R.EXACT_B, pad_to) and bool((ids[:, 0] == 0).all()) and bool(new_mask[:, 0].all())
        for row, m in zip(ids[:, 1:].numpy(), new_mask[:, 1:].numpy()):
            n = int((row != 0).sum())
            assert n >= 1 and (row[:n] >= 1).all() and (row[:n] <= P).all() and (np.diff(row[:n]) > 0).all() and (row[n:] == 0).all()
            assert np.array_equal(m, row != 0)


def test_measured_table_is_the_measurement():
    """MEASURED is not stale: on the lengths that are quick to redo, `python -m tests._ats_ref` still gives about the committed figures (a
    few roundings of a value near 1 either way: another CPU's softmax and sums may differ in the last bit)."""
    cases = [(N, H, K) for N, H, K in R.random_cases() if N <= 257]
    got = R.measure(cases)
    for key, v in got.items():
        assert 0.5 * R.MEASURED[key] <= v <= 1.5 * R.MEASURED[key], (key, v, R.MEASURED[key])
