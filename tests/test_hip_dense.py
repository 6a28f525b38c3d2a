"""tr_dense_gather and tr_dense_index at op level (GPU tier): synthetic inputs, no model; every comparison is bit equality with the numpy
restatement (tests/_dense_ref.py).
Gather: a sampled cross product (48 cases) of B in {1, 3}, P in {1, 4, 9, 63, 64, 65, 196, 1024} (one patch, P % 4 != 0, the 64-patch tile
and one more and one less, several tiles), D in {4, 60, 64, 68, 128, 384, 768, 1024} (one 16-byte chunk, the 64-channel tile and its
neighbours, the widest row), n_rows in {2, P/2 + 1, P + 1}, both layouts, both dtypes, fill in {0, -7.5} and six index patterns.
Index: synthetic record-form tables of every kind with 1 to 3 stages, n_in up to 1025."""
import numpy as np
import pytest
import torch

from tests import _dense_ref as ref
from tests import _launches

pytestmark = pytest.mark.gpu

PS = [1, 4, 9, 63, 64, 65, 196, 1024]
DS = [4, 60, 64, 68, 128, 384, 768, 1024]
PATTERNS = ["identity", "none", "one_row", "reversed", "random", "outside"]
INT32_MIN = -2 ** 31


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _gather_cases():
    """48 cases, six sweeps over P: every P meets six different D and all four (layout, dtype) pairs, every D meets both layouts; the rest
    cycles at periods of its own."""
    cases = []
    for i in range(48):
        j, s = i % 8, i // 8
        P, D = PS[j], DS[(j + s + s // 3) % 8]
        rows = (2, P // 2 + 1, P + 1)[i % 3]
        cases.append((1 if i % 5 == 0 else 3, P, D, rows, ("NCHW", "NHWC")[(s + j) % 2], ("fp32", "bf16")[(s // 2 + j) % 2],
                      (0.0, -7.5)[(i // 3) % 2], PATTERNS[(i + i // 6) % 6]))
    return cases


def _tokens(B, n_rows, D, rng, bf16):
    t = rng.standard_normal((B, n_rows, D)).astype(np.float32)
    flat = t.reshape(-1)
    # +-0, +-inf, fp32 denormals, and values half way between two bf16 neighbours (even and odd below: the tie goes both ways)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -3e-39, 1.1754942e-38, 1.00390625, 1.01171875, -1.00390625, -1.01171875, 65280.0,
                        3.3961775e38], dtype=np.float32)
    at = rng.permutation(flat.size)[:min(flat.size, 4 * special.size)]
    flat[at] = np.resize(special, at.size)
    if not bf16:
        flat[rng.integers(flat.size)] = np.nan
    return t


def _index(pattern, B, P, n_rows, rng):
    if pattern == "identity":
        idx = np.tile(np.arange(1, P + 1), (B, 1))             # (rows past n_rows - 1 come out as fill)
    elif pattern == "none":
        idx = np.full((B, P), -1)
    elif pattern == "one_row":
        idx = np.tile(rng.integers(0, n_rows, size=(B, 1)), (1, P))
    elif pattern == "reversed":
        idx = np.tile(np.arange(P, 0, -1) % n_rows, (B, 1))
    else:
        idx = rng.integers(0, n_rows, size=(B, P))
        idx[rng.random((B, P)) < 0.3] = -1
        if pattern == "outside":
            bad = np.array([n_rows, n_rows + 5, -2, INT32_MIN, 2 ** 31 - 1])
            where = rng.random((B, P)) < 0.3
            idx[where] = np.resize(bad, int(where.sum()))
            idx.reshape(-1)[0] = INT32_MIN
    return idx.astype(np.int32)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("B,P,D,n_rows,layout,dtype,fill,pattern", _gather_cases())
def test_gather_is_the_restatement_bit_for_bit(B, P, D, n_rows, layout, dtype, fill, pattern):
    from tokenreduction_amd import ops
    rng = np.random.default_rng(P * 131 + D)
    tokens, index = _tokens(B, n_rows, D, rng, dtype == "bf16"), _index(pattern, B, P, n_rows, rng)
    want = ref.dense_gather(tokens, index, layout, dtype, fill)
    want = want if dtype == "bf16" else want.view(np.uint32)
    t, i = torch.from_numpy(tokens).cuda(), torch.from_numpy(index).cuda()
    tdtype = torch.bfloat16 if dtype == "bf16" else torch.float32
    # a buffer with a canary behind it, pre-filled with a value the gather never writes: every element is written, none behind the end
    buf = torch.full((B * P * D + 64,), 123.0, dtype=tdtype, device="cuda")
    got = ops.dense_gather(t, i, layout=layout, dtype=tdtype, fill=fill, out=buf[:B * P * D])
    assert got.shape == ((B, D, P) if layout == "NCHW" else (B, P, D))
    np.testing.assert_array_equal(_bits(got), want)
    assert (buf[B * P * D:] == 123.0).all()
    again = ops.dense_gather(t, i, layout=layout, dtype=tdtype, fill=fill)
    assert np.array_equal(_bits(again), want)                   # the same launch twice: the same bits
    if dtype == "bf16":
        f32 = ops.dense_gather(t, i, layout=layout, dtype=torch.float32, fill=fill)
        assert torch.equal(f32.to(torch.bfloat16).view(torch.int16), again.view(torch.int16))
    assert _launches.labels(lambda: ops.dense_gather(t, i, layout=layout, dtype=tdtype, fill=fill)) == ["tr_dense_gather"]


def test_gather_refuses_what_the_header_refuses():
    from tokenreduction_amd import ops
    t, i = torch.zeros(2, 5, 8, device="cuda"), torch.zeros(2, 4, dtype=torch.int32, device="cuda")

    def refused(exc, match, *args, **kw):
        def fn():
            with pytest.raises(exc, match=match):
                ops.dense_gather(*args, **kw)
        assert _launches.labels(fn) == []
    refused(ValueError, "layout", t, i, layout="CHWN")
    refused(ValueError, "dtype", t, i, dtype=torch.float16)
    refused(RuntimeError, r"code -1\)", torch.zeros(2, 5, 6, device="cuda"), i)                     # D % 4
    refused(RuntimeError, r"code -1\)", t, torch.zeros(2, 1025, dtype=torch.int32, device="cuda"))  # P > 1024
    refused(RuntimeError, r"code -2\)", torch.zeros(2 * 5 * 8 + 1, device="cuda")[1:].view(2, 5, 8), i)
    torch.cuda.synchronize()


# ---- the index -------------------------------------------------------------------------------------------------------------------------
def _run_index(dec, stages, B, P0, n_last):
    """Device index (the flat buffers laid out by ops.decision_table) and the restatement's."""
    from tokenreduction_amd import ops
    table, layout, kept_n, assign_n, _ = ops.decision_table(stages, B)
    kept, assign = np.full(max(1, kept_n), 77, np.int32), np.full(max(1, assign_n), 77, np.int32)
    for blk, _, W, koff, A, aoff in layout:
        if W:
            kept[koff: koff + B * W] = np.asarray(dec["kept"][blk]).reshape(-1)
        if A:
            assign[aoff: aoff + B * A] = np.asarray(dec["assign"][blk]).reshape(-1)
    k, a = torch.from_numpy(kept).cuda(), torch.from_numpy(assign).cuda()
    got = ops.dense_index(k, a, stages, B, P0, n_last, table=table)
    again = ops.dense_index(k, a, stages, B, P0, n_last)
    assert torch.equal(got, again) and got.dtype == torch.int32
    want = ref.dense_index(dec, stages, B, P0, n_last)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    return want


def _kept_chain(kind, P0, B, ks, rng, spoil=False):
    """Absolute kept lists [B, W] of up to three stages, each drawn from the stage before."""
    dec, stages, n_in = {"kept": {}, "assign": {}}, [], P0 + 1
    alive = [np.arange(P0) for _ in range(B)]
    for blk, k in zip((0, 2, 5), ks):
        W = ref.n_out(kind, n_in, k)
        rows = np.full((B, W), -1, dtype=np.int64)
        for b in range(B):
            take = rng.permutation(alive[b])[:min(W, len(alive[b]))]
            if kind == ref.ATS:
                take = np.sort(take)[:rng.integers(0, len(take) + 1)] if b else np.sort(take)      # image 0: count == W where it can
            rows[b, :len(take)] = take
            if kind == ref.EVIT and W > 3:
                rows[b, [1, W // 2, W - 1]] = -1                 # fused tokens: this stage's and survivors of the stages before
            alive[b] = rows[b][rows[b] >= 0]
        if spoil and W > 4:
            rows[0, 3] = rows[0, 0]                              # a duplicate: the lowest j wins
            rows[-1, 2] = -2
            rows[-1, 4] = P0                                     # one past the grid
        dec["kept"][blk] = rows
        stages.append((blk, kind, n_in, k))
        n_in = W + 1
    return dec, stages, n_in


@pytest.mark.parametrize("kind", [ref.PRUNE, ref.EVIT, ref.ATS])
@pytest.mark.parametrize("P0,B", [(196, 3), (576, 1), (1024, 3)])
def test_index_of_kept_list_chains(kind, P0, B):
    rng = np.random.default_rng(P0 + kind)
    lo = 2 if kind == ref.ATS else 1
    for n, ks in enumerate(([P0 - 1 - (kind == ref.EVIT)], [P0 * 7 // 10, 257 if P0 > 400 else 64], [300 if P0 > 400 else 137, 65, lo])):
        dec, stages, n_in = _kept_chain(kind, P0, B, ks, rng, spoil=n == 1)
        index = _run_index(dec, stages, B, P0, n_in)
        last = dec["kept"][stages[-1][0]]
        for b in range(B):
            assert (index[b] >= 0).sum() == len(set(last[b][(last[b] >= 0) & (last[b] < P0)].tolist()))
        if n == 1:
            first = dec["kept"][0]
            assert first[0, 3] == first[0, 0]                    # (the duplicate was written)
    if kind == ref.ATS:                                          # count == 0: an image whose list is all padding
        dec, stages, n_in = _kept_chain(kind, P0, B, [100], rng)
        dec["kept"][0][-1] = -1
        index = _run_index(dec, stages, B, P0, n_in)
        assert (index[-1] == -1).all()


def _tome_map(n_in, r, B, rng):
    P_in, out = n_in - 1, n_in - 1 - r
    return np.stack([rng.permutation(np.concatenate([np.arange(out), rng.integers(0, out, size=P_in - out)])) for _ in range(B)])


@pytest.mark.parametrize("P0,B", [(196, 3), (576, 1), (1024, 3)])
def test_index_of_map_chains(P0, B):
    rng = np.random.default_rng(P0)
    # ToMe: r = 1, r = 16, and the largest r (the op clips k to (n_in - 1) // 2)
    dec, stages, n_in = {"kept": {}, "assign": {}}, [], P0 + 1
    for blk, k in zip((0, 1, 3), (1, 16, None)):
        k = n_in - 1 if k is None else k
        r = min(k, (n_in - 1) // 2)
        dec["assign"][blk] = _tome_map(n_in, r, B, rng)
        stages.append((blk, ref.TOME, n_in, k))
        n_in -= r
    index = _run_index(dec, stages, B, P0, n_in)
    assert (index >= 1).all() and all(set(index[b].tolist()) == set(range(1, n_in)) for b in range(B))
    # SOFT / CENTRES: clusters that own nothing, k = 1 at the end; a -2 and an id one past the clusters in the first map
    for kind in (ref.SOFT, ref.CENTRES):
        dec, stages, n_in = {"kept": {}, "assign": {}}, [], P0 + 1
        for blk, k in zip((0, 2, 5), (P0 // 2, 70, 1)):
            a = rng.integers(0, k, size=(B, n_in - 1))
            if k > 8:
                a[a == 5] = 6                                    # cluster 5 owns nothing
                a[0, 0], a[-1, 7] = -2, k
            dec["assign"][blk] = a
            if kind == ref.CENTRES:
                dec["kept"][blk] = rng.integers(0, P0, size=(B, k))          # the centre list: present, not used
            stages.append((blk, kind, n_in, k))
            n_in = k + 1
        index = _run_index(dec, stages, B, P0, n_in)
        assert set(np.unique(index).tolist()) == {-1, 1} and index[0, 0] == -1
    # a pruning stage in front of a merge stage
    kdec, stages, n_in = _kept_chain(ref.PRUNE, P0, B, [P0 * 7 // 10], rng)
    r = 16
    kdec["assign"][4] = _tome_map(n_in, r, B, rng)
    stages.append((4, ref.TOME, n_in, r))
    index = _run_index(kdec, stages, B, P0, n_in - r)
    assert ((index >= 1).sum(axis=1) == P0 * 7 // 10).all()


def test_no_stage_writes_the_identity_and_a_bad_table_launches_nothing():
    from tokenreduction_amd import _lib, ops
    got = ops.dense_index(None, None, [], 3, 196, 197)
    assert torch.equal(got.cpu(), torch.arange(1, 197, dtype=torch.int32).expand(3, 196))
    kept = torch.zeros(2 * 137, dtype=torch.int32, device="cuda")

    def refused(code, *args):
        def fn():
            with pytest.raises(RuntimeError, match=rf"code {code}\)"):
                ops.dense_index(*args)
        assert _launches.labels(fn) == []
    refused(-1, kept, None, [(0, _lib.TR_DECISION_PRUNE, 197, 137)], 2, 196, 137)                  # the chain ends at 137 patch rows, not 136
    refused(-1, kept[:-1], None, [(0, _lib.TR_DECISION_PRUNE, 197, 137)], 2, 196, 138)             # the list leaves its buffer
    refused(-3, kept, None, [(0, _lib.TR_DECISION_TOME, 197, 16)], 2, 196, 181)                    # a map stage without maps
    assert _launches.labels(lambda: ops.dense_index(kept, None, [(0, _lib.TR_DECISION_PRUNE, 197, 137)], 2, 196, 138)) == ["tr_dense_index"]
    torch.cuda.synchronize()
