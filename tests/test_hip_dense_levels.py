"""tr_dense_index_levels and tr_dense_gather_levels at op level (GPU tier): synthetic inputs, no model; every comparison is bit equality
with the numpy restatement (tests/_dense_levels_ref.py), and with the single-level ops on the same data.
Index: chains of every stage kind (stages at blocks 2 / 4 / 7) at P0 in {9, 196, 1024}, B in {1, 3}, under level sets with a level in front
of every stage, one at every stage boundary, two between the same pair of stages, L in {1, 5, 9, 32}.
Gather: a sampled cross product (42 cases) of P in {1, 9, 63, 64, 65, 196, 225} (both P % 4 paths, the 64-patch tile edge), D in {4, 60, 64,
68, 128, 384}, L in {1, 2, 5} with differing rows per level (n_rows = 1 among them), both layouts, both dtypes, the index patterns and special
values of tests/test_hip_dense.py."""
import numpy as np
import pytest
import torch

from tests import _dense_levels_ref as lref
from tests import _dense_ref as ref
from tests import _launches
from tests.test_hip_dense import PATTERNS, _bits, _index, _tokens, _tome_map

pytestmark = pytest.mark.gpu

PS = [1, 9, 63, 64, 65, 196, 225]
DS = [4, 60, 64, 68, 128, 384]
STAGE_BLOCKS = (2, 4, 7)
LEVEL_SETS = [[0], [31], [1, 2, 3, 7, 20], list(range(9)), list(range(32))]
CHAINS = ["prune", "evit", "ats", "tome", "soft", "centres", "prune_tome"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- the index -------------------------------------------------------------------------------------------------------------------------
def _kept_stage(kind, P0, B, n_in, k, alive, rng, spoil):
    W = ref.n_out(kind, n_in, k)
    rows = np.full((B, W), -1, dtype=np.int64)
    for b in range(B):
        take = rng.permutation(alive[b])[:min(W, len(alive[b]))]
        if kind == ref.ATS:
            take = np.sort(take)[:rng.integers(0, len(take) + 1)] if b else np.sort(take)
        rows[b, :len(take)] = take
        if kind == ref.EVIT and W > 3:
            rows[b, [1, W - 1]] = -1                             # fused tokens
        alive[b] = rows[b][rows[b] >= 0]
    if spoil and W > 4:
        rows[0, 3] = rows[0, 0]                                  # a duplicate: the lowest j wins
        rows[-1, 2], rows[-1, 4] = -2, P0                        # an invalid entry, one past the grid
    return rows, W


def _chain(name, P0, B, rng):
    """Three stages at STAGE_BLOCKS: (dec, stages)."""
    dec, stages, n_in = {"kept": {}, "assign": {}}, [], P0 + 1
    alive = [np.arange(P0) for _ in range(B)]
    kinds = {"prune": [ref.PRUNE] * 3, "evit": [ref.EVIT] * 3, "ats": [ref.ATS] * 3, "tome": [ref.TOME] * 3, "soft": [ref.SOFT] * 3,
             "centres": [ref.CENTRES] * 3, "prune_tome": [ref.PRUNE, ref.PRUNE, ref.TOME]}[name]
    for i, (blk, kind) in enumerate(zip(STAGE_BLOCKS, kinds)):
        P_in = n_in - 1
        if kind == ref.TOME:
            k = max(1, P_in // 4)
            r = min(k, P_in // 2)
            dec["assign"][blk] = _tome_map(n_in, r, B, rng)
            n_out = P_in - r
        elif kind in (ref.SOFT, ref.CENTRES):
            k = max(1, P_in * 2 // 3)
            a = rng.integers(0, k, size=(B, P_in))
            if k > 8:
                a[a == 5] = 6                                    # cluster 5 owns nothing
                a[0, 0], a[-1, 7] = -2, k
            dec["assign"][blk] = a
            if kind == ref.CENTRES:
                dec["kept"][blk] = rng.integers(0, P0, size=(B, k))
            n_out = k
        else:
            k = max(2 if kind == ref.ATS else 1, P_in * 2 // 3) + (1 if kind == ref.ATS else 0)
            k = min(k, n_in - 1)
            dec["kept"][blk], n_out = _kept_stage(kind, P0, B, n_in, k, alive, rng, spoil=i == 1)
        stages.append((blk, kind, n_in, k))
        assert n_out == ref.n_out(kind, n_in, k) and n_out >= 1
        n_in = n_out + 1
    return dec, stages


def _device_decisions(dec, stages, B):
    from tokenreduction_amd import ops
    table, layout, kept_n, assign_n, _ = ops.decision_table(stages, B)
    kept, assign = np.full(max(1, kept_n), 77, np.int32), np.full(max(1, assign_n), 77, np.int32)
    for blk, _, W, koff, A, aoff in layout:
        if W:
            kept[koff: koff + B * W] = np.asarray(dec["kept"][blk]).reshape(-1)
        if A:
            assign[aoff: aoff + B * A] = np.asarray(dec["assign"][blk]).reshape(-1)
    return torch.from_numpy(kept).cuda(), torch.from_numpy(assign).cuda(), table


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("P0,B", [(9, 1), (9, 3), (196, 3), (196, 1), (1024, 3), (1024, 1)])
def test_level_indices_are_the_restatement(name, P0, B):
    from tokenreduction_amd import ops
    rng = np.random.default_rng(P0 * 7 + B + len(name))
    dec, stages = _chain(name, P0, B, rng)
    k, a, table = _device_decisions(dec, stages, B)
    every = lref.dense_index_levels(dec, stages, B, P0, list(range(32)))      # the restatement of each block's level, computed once
    for blocks in LEVEL_SETS:
        rows = [lref.level_rows(stages, P0, b) for b in blocks]
        want = every[blocks]
        L = len(blocks)
        buf = torch.full((L * B * P0 + 64,), 12345, dtype=torch.int32, device="cuda")      # a canary behind the buffer
        got = ops.dense_index_levels(k, a, stages, B, P0, blocks, rows, table=table, out=buf[:L * B * P0])
        assert got.shape == (L, B, P0) and got.dtype == torch.int32
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert (buf[L * B * P0:] == 12345).all()
        for l, blk in enumerate(blocks):
            if blk < STAGE_BLOCKS[0]:                            # in front of every stage: the identity
                assert (want[l] == np.arange(1, P0 + 1)).all()
            if l and not set(range(blocks[l - 1] + 1, blk + 1)) & set(STAGE_BLOCKS):       # two levels between the same pair of stages
                np.testing.assert_array_equal(want[l], want[l - 1])
    # with every stage before the one level it is tr_dense_index
    n_last = lref.level_rows(stages, P0, 31)
    single = ops.dense_index(k, a, stages, B, P0, n_last, table=table)
    assert torch.equal(ops.dense_index_levels(k, a, stages, B, P0, [STAGE_BLOCKS[-1]], [n_last])[0], single)
    assert torch.equal(got[-1], single)
    assert _launches.labels(lambda: ops.dense_index_levels(k, a, stages, B, P0, [1, 2, 3, 7, 20], [lref.level_rows(stages, P0, b) for b in
                                                                                                  (1, 2, 3, 7, 20)])) == ["tr_dense_index_levels"]


def test_no_stage_is_the_identity_at_every_level_and_bad_levels_launch_nothing():
    from tokenreduction_amd import _lib, ops
    got = ops.dense_index_levels(None, None, [], 3, 196, [0, 5, 11], [197, 197, 197])
    assert torch.equal(got.cpu(), torch.arange(1, 197, dtype=torch.int32).expand(3, 3, 196))
    kept = torch.zeros(2 * 137, dtype=torch.int32, device="cuda")
    stages = [(3, _lib.TR_DECISION_PRUNE, 197, 137)]

    def refused(code, *args):
        def fn():
            with pytest.raises(RuntimeError, match=rf"code {code}\)"):
                ops.dense_index_levels(*args)
        assert _launches.labels(fn) == []
    refused(-1, kept, None, stages, 2, 196, [2, 3], [197, 137])                # block 3's stream has 138 tokens
    refused(-1, kept, None, stages, 2, 196, [2, 3], [138, 138])                # block 2 is in front of the stage
    refused(-5, kept, None, stages, 2, 196, [3, 2], [138, 197])                # not ascending
    refused(-5, kept, None, stages, 2, 196, [3, 32], [138, 138])
    assert _launches.labels(lambda: ops.dense_index_levels(kept, None, stages, 2, 196, [2, 3], [197, 138])) == ["tr_dense_index_levels"]
    torch.cuda.synchronize()


# ---- the gather ------------------------------------------------------------------------------------------------------------------------
def _gather_cases():
    """42 cases, six sweeps over P: every P meets every D, both layouts, both dtypes and two of the three L."""
    cases = []
    for i in range(42):
        j, s = i % 7, i // 7
        cases.append((1 if i % 4 == 0 else 3, PS[j], DS[(j + s) % 6], (1, 2, 5)[(i + s) % 3], ("NCHW", "NHWC")[(s + j) % 2],
                      ("fp32", "bf16")[(s // 2 + j) % 2], (0.0, -7.5)[(i // 3) % 2], i))
    return cases


def _level_rows(P, L, i):
    pool = [1, P + 1, 2, P // 2 + 1, 3]
    return [pool[(i + l) % 5] for l in range(L)] if L > 1 else [pool[i % 5]]


@pytest.mark.parametrize("B,P,D,L,layout,dtype,fill,i", _gather_cases())
def test_level_gather_is_the_restatement_bit_for_bit(B, P, D, L, layout, dtype, fill, i):
    from tokenreduction_amd import ops
    rng = np.random.default_rng(P * 131 + D + L)
    rows = _level_rows(P, L, i)
    stride = B * max(rows) * D + (8 if i % 2 else 0)            # slabs as large as the largest level, or with room behind it
    tokens = [_tokens(B, n, D, rng, dtype == "bf16") for n in rows]
    index = np.stack([_index(PATTERNS[(i + l) % 6], B, P, rows[l], rng) for l in range(L)])
    bad = [-1, -2, rows[-1], -2 ** 31][:B * P]                  # (whatever the pattern: the four indices no row answers to)
    index[-1].reshape(-1)[:len(bad)] = bad
    want = lref.dense_gather_levels(tokens, index, layout, dtype, fill)
    want = want if dtype == "bf16" else want.view(np.uint32)
    flat = np.full(L * stride, 555.0, dtype=np.float32)         # between the levels' rows: values no index may reach
    for l in range(L):
        flat[l * stride: l * stride + B * rows[l] * D] = tokens[l].reshape(-1)
    t, ix = torch.from_numpy(flat).cuda(), torch.from_numpy(index).cuda()
    tdtype = torch.bfloat16 if dtype == "bf16" else torch.float32
    n = B * P * D
    buf = torch.full((L * n + 64,), 123.0, dtype=tdtype, device="cuda")                    # a canary behind the whole buffer
    got = ops.dense_gather_levels(t, stride, rows, ix, D, layout=layout, dtype=tdtype, fill=fill, out=buf[:L * n])
    assert got.shape == ((L, B, D, P) if layout == "NCHW" else (L, B, P, D))
    np.testing.assert_array_equal(_bits(got), want)
    assert (buf[L * n:] == 123.0).all()
    again = ops.dense_gather_levels(t, stride, rows, ix, D, layout=layout, dtype=tdtype, fill=fill)
    assert np.array_equal(_bits(again), want)                   # the same launch twice: the same bits
    for l in range(L):
        # every level alone, through both entry points, into a buffer with a canary right behind that level's output
        tl = t[l * stride: l * stride + B * rows[l] * D].view(B, rows[l], D)
        one = torch.full((n + 64,), 123.0, dtype=tdtype, device="cuda")
        single = ops.dense_gather(tl, ix[l].clone(), layout=layout, dtype=tdtype, fill=fill, out=one[:n])
        assert np.array_equal(_bits(single), _bits(got[l])) and (one[n:] == 123.0).all(), l
        one.fill_(123.0)
        alone = ops.dense_gather_levels(tl.reshape(-1), tl.numel(), [rows[l]], ix[l:l + 1].clone(), D, layout=layout, dtype=tdtype, fill=fill,
                                        out=one[:n])
        assert np.array_equal(_bits(alone[0]), _bits(got[l])) and (one[n:] == 123.0).all(), l
    assert _launches.labels(lambda: ops.dense_gather_levels(t, stride, rows, ix, D, layout=layout, dtype=tdtype, fill=fill)) == [
        "tr_dense_gather_levels"]


def test_level_gather_refuses_what_the_header_refuses():
    from tokenreduction_amd import ops
    t, ix = torch.zeros(2 * 2 * 5 * 8, device="cuda"), torch.zeros(2, 2, 4, dtype=torch.int32, device="cuda")

    def refused(exc, match, *args, **kw):
        def fn():
            with pytest.raises(exc, match=match):
                ops.dense_gather_levels(*args, **kw)
        assert _launches.labels(fn) == []
    refused(ValueError, "layout", t, 80, [5, 3], ix, 8, layout="CHWN")
    refused(ValueError, "dtype", t, 80, [5, 3], ix, 8, dtype=torch.float16)
    refused(ValueError, "index", t, 80, [5, 3, 2], ix, 8)
    refused(ValueError, "tokens holds", t, 80, [5, 6], ix, 8)
    refused(RuntimeError, r"code -1\)", t, 64, [4, 5], ix, 8)                               # level 1's rows leave its slab
    refused(RuntimeError, r"code -1\)", torch.zeros(2 * 2 * 5 * 6, device="cuda"), 60, [5, 3], ix, 6)      # D % 4
    refused(RuntimeError, r"code -2\)", torch.zeros(200, device="cuda"), 82, [5, 3], ix, 8)                # slabs not 16-byte aligned
    assert _launches.labels(lambda: ops.dense_gather_levels(t, 80, [5, 3], ix, 8)) == ["tr_dense_gather_levels"]
    torch.cuda.synchronize()
