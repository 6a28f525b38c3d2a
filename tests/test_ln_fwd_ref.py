"""CPU checks of tests/_ln_fwd_ref.py, the reference tests/test_hip_layernorm_fwd_edges.py holds the forward LayerNorm kernels against:
the float64 closed form is torch.nn.functional.layer_norm, constant rows give exactly beta, plain float32 evaluation stays within a quarter
of the bound the GPU test applies (what makes that bound mean something: a family that breaks it fails HERE, not on the GPU), and the tables
name what they claim to name."""
import pytest
import torch

import oracle
from tests import _ln_fwd_ref as R

_CASES = sorted(set(R.ln_cases()))


def _by_shape():
    out = {}
    for M, D, o, kind in _CASES:
        out.setdefault((M, D), []).append((o, kind))
    return [pytest.param(shape, rest, id=f"{shape[0]}x{shape[1]}") for shape, rest in sorted(out.items())]


@pytest.mark.parametrize("shape,rest", _by_shape())
def test_ln_ref_is_layer_norm_in_float64(shape, rest):
    M, D = shape
    for o, kind in rest:
        c = R.ln_case(M, D, o)
        s = R.stream_of(c, kind)
        for eps in R.LN_EPS:
            want = torch.nn.functional.layer_norm(s.double(), (D,), c["gamma"].double(), c["beta"].double(), R.eps32(eps))
            got = R.ln_ref(s, c["gamma"], c["beta"], eps)
            assert got.dtype == torch.float64
            assert float((got - want).abs().max()) <= 1e-12, f"M = {M}, D = {D}, offset {o}, stream {kind}, eps {eps}"


@pytest.mark.parametrize("shape,rest", _by_shape())
def test_constant_rows_give_exactly_beta(shape, rest):
    M, D = shape
    for o, kind in rest:
        if kind != "x":
            continue
        c = R.ln_case(M, D, o)
        rows = [r for r, f in enumerate(c["fam"]) if f == "const"]
        for r in rows:
            assert float(c["x"][r].min()) == float(c["x"][r].max()) and float(c["x"][r, 0]) in R.CONSTS
        for eps in R.LN_EPS:
            assert torch.equal(R.ln_ref(c["x"], c["gamma"], c["beta"], eps)[rows], c["beta"].double().expand(len(rows), D))
            assert torch.equal(R.ln_f32(c["x"], c["gamma"], c["beta"], eps)[rows], c["beta"].expand(len(rows), D))


def test_every_constant_and_every_family_position_is_reached():
    seen = {float(R.ln_case(R.LN_M_ALL, 128)["x"][r, 0]) for r, f in enumerate(R.ln_case(R.LN_M_ALL, 128)["fam"]) if f == "const"}
    assert seen == set(R.CONSTS)
    for r in range(8):
        assert {R.family_of(r, o) for o in R.OFFSETS} == set(R.FAMILIES)


@pytest.mark.parametrize("shape,rest", _by_shape())
def test_float32_stays_within_a_quarter_of_the_bound(shape, rest):
    M, D = shape
    assert R.LN_FWD_BOUND == 4 * R.LN_F32_WORST
    for o, kind in rest:
        for eps in R.LN_EPS:
            rel = R.ln_f32_cost(M, D, o, kind, eps)
            r = int(rel.argmax())
            assert float(rel[r]) <= R.LN_FWD_BOUND / 4, (f"row {r} (family {R.ln_case(M, D, o)['fam'][r]}) of M = {M}, D = {D}, offset {o}, stream {kind}, "
                                                         f"eps {eps}: float32 is off by {float(rel[r]):.2e}")


@pytest.mark.parametrize("B,N,K", R.GATHER_CASES)
def test_fused_row_in_float32_stays_within_a_quarter_of_its_bound(B, N, K):
    assert R.FUSE_BOUND == 4 * R.FUSE_F32_WORST
    for D in R.GATHER_D:
        for delta in (None, "bf16", "f32"):
            rel = R.fuse_f32_cost(B, N, K, D, delta)
            assert float(rel.max()) <= R.FUSE_BOUND / 4, f"D = {D}, delta {delta}: float32 is off by {float(rel.max()):.2e}"


def test_gather_cases_are_what_their_table_says():
    for B, N, K in R.GATHER_CASES:
        assert 1 <= K <= N - 2 and N <= 600 and B <= 2
        c = R.gather_case(B, N, K, 4)
        idx, compl, w = c["idx"], c["compl"], c["scores"]
        for b in range(B):
            assert sorted(idx[b].tolist() + compl[b].tolist()) == list(range(N - 1)), "kept and dropped tokens partition the patches"
            wc = w[b, compl[b]]
            assert float(wc.max()) == 40.0 and int((wc == 40.0).sum()) == 1
            assert N - 1 - K <= 2 or bool((wc == 0).any())
        assert torch.equal(oracle.evit_fuse(c["x"], idx, w)[1], compl)
    dropped = sorted({N - 1 - K for _, N, K in R.GATHER_CASES})
    assert dropped == [1, 2, 3, 4, 5, 11, 14, 255, 256, 257, 259, 288, 513]
    assert {K + 1 for _, _, K in R.GATHER_CASES} >= {2, 4, 5, 8}
    # a wave's tokens per trip, cnt = min(64, ceil((c - wave) / 4) - 64 trip): every remainder of the four-row step, and 1, 2 and 3 trips
    cnts = {min(64, (c - wv + 3) // 4 - i0) % 4 for c in dropped for wv in range(4) for i0 in range(0, (c - wv + 3) // 4, 64)}
    assert cnts == {0, 1, 2, 3}
    assert {((c + 3) // 4 + 63) // 64 for c in dropped} == {1, 2, 3}
    for B, N, D in R.GATHER_KEPT_ALL:
        assert R.gather_case(B, N, N - 1, D)["compl"].shape == (B, 0)


def test_tables_meet_the_c_abi_and_name_every_chunk_count():
    """tr_layernorm_*: D % 4 == 0, D <= 1024 (strides % 4 == 0 follow from D and the gaps the GPU test adds); every NCH = ceil(D / 256) at its
    narrowest and widest row, the D next to every NCH boundary, the half kernel's D, and row counts around both workgroup heights."""
    every_d = set(R.LN_D) | set(R.LN_FORM_D) | set(R.GATHER_D) | {D for _, _, D in R.GATHER_ALL_ROWS} | {D for _, _, D in R.GATHER_KEPT_ALL}
    for D in every_d:
        assert D > 0 and D % 4 == 0 and D <= 1024
    for nch, (lo, hi) in R.LN_NCH_ENDS.items():
        assert lo in R.LN_D and hi in R.LN_D and (lo + 255) // 256 == nch and (hi + 255) // 256 == nch
        assert (lo - 4 + 255) // 256 == nch - 1 and ((hi + 4 + 255) // 256 == nch + 1 or hi == 1024)
        assert hi - 4 in R.LN_D or nch == 1 and 252 in R.LN_D
    assert R.LN_HALF_D in R.LN_D and R.LN_HALF_D in R.LN_FORM_D and R.LN_HALF_D in R.GATHER_D
    assert {(D + 255) // 256 for D in R.LN_FORM_D if D != R.LN_HALF_D} == {1, 2, 3, 4}
    assert {(D + 255) // 256 for _, _, D in R.GATHER_ALL_ROWS} == {1, 2, 3, 4}
    assert {1, 3, 4, 5} <= set(R.LN_M_WAVE) and {1, 7, 8, 9} <= set(R.LN_M_HALF)
    assert R.LN_M_ALL >= 16 and max(M for M, _, _ in R.LN_SHAPES) <= 1000
    assert {M for M, D, _ in R.LN_SHAPES if D == R.LN_HALF_D} == set(R.LN_M_HALF) | {R.LN_M_ALL}
    assert all(len(o) == len(R.FAMILIES) for M, _, o in R.LN_SHAPES if M != R.LN_M_ALL)
