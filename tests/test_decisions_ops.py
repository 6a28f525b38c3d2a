"""tr_stage_decisions at op level (GPU tier): synthetic slabs, no model.  Every comparison is equality with the numpy restatement
(tests/_decisions_ref.py).  Shapes: N0 in {197, 577, 1025} (224, 384, 512 inputs), B in {1, 3, 5}, three chained stages; the stage widths
sit on the kernel's loop edges -- a wave (64), the workgroup (256), one more and one less."""
import numpy as np
import pytest
import torch

from tests import _decisions_ref as ref
from tests import _launches

pytestmark = pytest.mark.gpu

BLOCKS = (0, 2, 5)                       # the three stages' blocks: slabs that are not adjacent
DEPTH = 6
EDGES = [1, 63, 64, 65, 137, 255, 256, 257, 576]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _run(kept, compl, soft, stages, B, N0):
    """(device result as int64 numpy, numpy restatement) of one table."""
    from tokenreduction_amd import ops
    dev = ops.stage_decisions(torch.from_numpy(kept).cuda(), None if compl is None else torch.from_numpy(compl).cuda(),
                              None if soft is None else torch.from_numpy(soft).cuda(), stages, B, N0)
    torch.cuda.synchronize()
    got = {"stages": dev["stages"], **{key: {blk: t.cpu().numpy().astype(np.int64) for blk, t in dev[key].items()}
                                       for key in ("kept", "kept_count", "assign")}}
    want = ref.stage_decisions(kept, kept if compl is None else compl, np.zeros(0, np.float32) if soft is None else soft, stages, B, N0)
    return got, want


def _equal(got, want):
    assert got["stages"] == want["stages"]
    for key in ("kept", "kept_count", "assign"):
        assert sorted(got[key]) == sorted(want[key]), key
        for blk in want[key]:
            np.testing.assert_array_equal(got[key][blk], want[key][blk], err_msg=f"{key}[{blk}]")


def _slabs(B, N0, fill=7):
    # entries no stage reads hold a value that would show if one did
    return np.full(DEPTH * B * N0, fill, dtype=np.int32)


def _put(arr, blk, B, N0, rows, at=0):
    flat = np.asarray(rows, dtype=np.int32).reshape(-1)
    arr[blk * B * N0 + at: blk * B * N0 + at + flat.size] = flat


def _chains(N0):
    """Descending triples of the edge widths that fit below N0, the last one padded with 1."""
    ks = sorted((k for k in EDGES if k < N0), reverse=True)
    ks += [1] * (-len(ks) % 3)
    return [tuple(ks[i: i + 3]) for i in range(0, len(ks), 3)]


def _prune_chain(kind, N0, B, ks, rng):
    kept, stages, n_in, length = _slabs(B, N0), [], N0, N0 - 1
    for blk, k in zip(BLOCKS, ks):
        rel = np.stack([rng.permutation(length)[:k] for _ in range(B)])
        if kind == ref.EVIT and k > 2:
            rel[:, 1] = -1                                      # the fused token's own index
            if length > N0 - 1 or blk != BLOCKS[0]:
                rel[:, 2] = length - 1                          # ... and the trailing entry of the list before
        _put(kept, blk, B, N0, rel)
        stages.append((blk, kind, n_in, k))
        length = k + 1 if kind == ref.EVIT else k
        n_in = length + 1
    return kept, stages


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("N0", [197, 577, 1025])
def test_pruning_chains(N0, B):
    rng = np.random.default_rng(N0 * 10 + B)
    for ks in _chains(N0):
        for kind in (ref.PRUNE, ref.EVIT):
            if kind == ref.EVIT and ks[0] + 2 > N0:
                continue                                        # (EViT leaves K + 2 tokens: K <= N - 2)
            kept, stages = _prune_chain(kind, N0, B, ks, rng)
            got, want = _run(kept, None, None, stages, B, N0)
            _equal(got, want)
            last = got["kept"][BLOCKS[2]]
            assert last.shape == (B, ks[2] + (kind == ref.EVIT)) and last.min() >= -1 and last.max() < N0 - 1
            if kind == ref.EVIT:
                assert (last[:, -1] == -1).all()


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("N0", [197, 577, 1025])
def test_centres_chain_copies_the_assignment(N0, B):
    rng = np.random.default_rng(N0 * 20 + B)
    ks = _chains(N0)[0]
    kept, stages = _prune_chain(ref.CENTRES, N0, B, ks, rng)
    compl = _slabs(B, N0, fill=9)
    for (blk, _, n_in, k) in stages:
        _put(compl, blk, B, N0, rng.integers(0, k, size=(B, n_in - 1)))
    got, want = _run(kept, compl, None, stages, B, N0)
    _equal(got, want)
    assert sorted(got["assign"]) == list(BLOCKS)


def _ats_chain(N0, B, widths, counts, rng, gaps=False):
    """counts[s][b]: valid ids of image b at stage s (clipped to what the stage can hold and what the list before offers)."""
    kept, stages, n_in = _slabs(B, N0), [], N0
    avail = np.full(B, N0 - 1)
    for s, (blk, K) in enumerate(zip(BLOCKS, widths)):
        ids = np.zeros((B, K), dtype=np.int64)
        here = np.zeros(B, dtype=np.int64)
        for b in range(B):
            c = int(min(counts[s][b], K - 1, avail[b]))
            pick = 1 + np.sort(rng.permutation(avail[b])[:c])
            cols = 1 + (np.sort(rng.permutation(K - 1)[:c]) if gaps else np.arange(c))
            ids[b, cols] = pick
            here[b] = c
        _put(kept, blk, B, N0, ids)
        stages.append((blk, ref.ATS, n_in, K))
        avail = (np.full(B, K - 1) if s == 0 else here) if gaps else here      # (with gaps the first list keeps its padding: any slot is an index)
        n_in = K
    return kept, stages


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("N0", [197, 577, 1025])
def test_ats_chains(N0, gaps):
    rng = np.random.default_rng(N0 + gaps)
    full = 10 ** 6
    widths = {197: (139, 98, 70), 577: (404, 300, 259), 1025: (1024, 600, 300)}[N0]
    # B = 5: every id valid / one valid id / the scan's wave boundary; B = 3: the workgroup boundary, or no valid id at all
    batches = [[full, 1, 63, 64, 65], [255, 256, 257] if N0 > 197 else [0, 65, full], [full]]
    for first in batches:
        B = len(first)
        counts = [first, first, [c if c == full else max(c - 1, 0) for c in first]]      # (clipped to what each stage can hold)
        kept, stages = _ats_chain(N0, B, widths, counts, rng, gaps)
        got, want = _run(kept, None, None, stages, B, N0)
        _equal(got, want)
        c0 = got["kept_count"][BLOCKS[0]]
        assert c0.tolist() == [min(c, widths[0] - 1) for c in first]
        for blk in BLOCKS[1:]:                                   # -1 exactly behind the valid entries
            rows, cnt = got["kept"][blk], got["kept_count"][blk]
            for b in range(B):
                assert (rows[b, cnt[b]:] == -1).all() and (gaps or (rows[b, :cnt[b]] >= 0).all())


def _tome_chain(N0, B, rs, rng):
    kept, stages, n_in = _slabs(B, N0), [], N0
    for blk, k in zip(BLOCKS, rs):
        na, nb = (n_in + 1) // 2, n_in // 2
        r = min(k, (n_in - 1) // 2)
        unm, src, dst = np.zeros((B, na - r), np.int64), np.zeros((B, r), np.int64), np.zeros((B, r), np.int64)
        for b in range(B):
            order = rng.permutation(na)
            src[b], unm[b] = order[:r], order[r:]
            dst[b] = rng.integers(0, nb, size=r)
        _put(kept, blk, B, N0, unm)
        _put(kept, blk, B, N0, src, B * (na - r))
        _put(kept, blk, B, N0, dst, B * na)
        stages.append((blk, ref.TOME, n_in, k))
        n_in -= r
    return kept, stages


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("N0", [197, 577, 1025])
def test_tome_chains(N0, B):
    rng = np.random.default_rng(N0 * 30 + B)
    # odd n_in first (N0), even behind an odd r; r = 1, r = 16, and an r the op clips to (n_in - 1) // 2
    for rs in ((1, 16, N0 - 20), (16, 1, 16), (N0 - 1, 15, 1)):
        kept, stages = _tome_chain(N0, B, rs, rng)
        assert {st[2] % 2 for st in stages} == {0, 1}
        got, want = _run(kept, None, None, stages, B, N0)
        _equal(got, want)
        for (blk, _, n_in, k) in stages:
            m = got["assign"][blk]
            assert m.shape == (B, n_in - 1) and m.min() >= -1 and m.max() < n_in - min(k, (n_in - 1) // 2) - 1


@pytest.mark.parametrize("values", ["fp32", "bf16", "ties"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("P", [196, 576])
def test_soft_argmax_first_maximum_wins(P, B, values):
    rng = np.random.default_rng(P + B)
    N0, stages, parts, n_in = P + 1, [], [], P + 1
    for blk, K in zip(BLOCKS, (137, 7, 1)):
        a = rng.standard_normal((B, K, n_in - 1)).astype(np.float32)
        if values == "bf16":
            a = torch.from_numpy(a).bfloat16().float().numpy()
        elif values == "ties":
            a = rng.integers(0, 3, size=a.shape).astype(np.float32)          # three levels: nearly every column has its maximum twice
            if K > 1:
                assert ((a == a.max(axis=1, keepdims=True)).sum(axis=1) > 1).any()
        parts.append(a.reshape(-1))
        stages.append((blk, ref.SOFT, n_in, K))
        n_in = K + 1
    soft = np.concatenate(parts)
    got, want = _run(_slabs(B, N0), None, soft, stages, B, N0)
    _equal(got, want)
    assert not got["kept"] and (got["assign"][BLOCKS[2]] == 0).all()


def test_indices_just_outside_their_list_come_back_as_minus_two():
    rng = np.random.default_rng(5)
    B, N0, ks = 3, 197, (137, 65, 64)
    kept, stages = _prune_chain(ref.PRUNE, N0, B, ks, rng)
    clean, _ = _run(kept, None, None, stages, B, N0)
    bad = kept.copy()
    base1, base2 = BLOCKS[1] * B * N0, BLOCKS[2] * B * N0
    bad[BLOCKS[0] * B * N0 + 5] = N0 - 1                          # one past the input grid
    bad[base1 + 1 * ks[1] + 7] = ks[0]                            # image 1: one past the list before
    bad[base1 + 2 * ks[1] + 9] = -2
    bad[base2 + 0 * ks[2] + 63] = ks[1]
    bad[base2 + 2 * ks[2] + 0] = -1                               # -1 is a padding only under EViT
    got, want = _run(bad, None, None, stages, B, N0)
    _equal(got, want)
    marks = {BLOCKS[0]: [(0, 5)], BLOCKS[1]: [(1, 7), (2, 9)], BLOCKS[2]: [(0, 63), (2, 0)]}
    for blk, cells in marks.items():
        hit = np.zeros_like(got["kept"][blk], dtype=bool)
        for cell in cells:
            assert got["kept"][blk][cell] == -2, (blk, cell)
            hit[cell] = True
        if blk == BLOCKS[0]:
            np.testing.assert_array_equal(got["kept"][blk][~hit], clean["kept"][blk][~hit])       # the neighbours are intact
    # the -2 of stage 0 travels: whoever picks that slot later shows it, nobody else does
    later = got["kept"][BLOCKS[1]] != clean["kept"][BLOCKS[1]]
    assert set(zip(*np.nonzero(later))) <= {(1, 7), (2, 9)} | set(zip(*np.nonzero(kept[base1: base1 + B * ks[1]].reshape(B, ks[1]) == 5)))
    # ATS: an id one past the list before, a negative id; ToMe: positions outside the table
    kept, stages = _ats_chain(N0, B, (139, 98, 70), [[100, 64, 65], [60, 64, 10], [30, 30, 5]], rng)
    kept[BLOCKS[1] * B * N0 + 0 * 98 + 3] = 139                    # the first stage's list has 138 slots (padding included): id 139 is index 138
    kept[BLOCKS[2] * B * N0 + 2 * 70 + 1] = 11                     # image 2 kept 10 entries at the stage before: id 11 is index 10
    kept[BLOCKS[1] * B * N0 + 1 * 98 + 2] = -1
    kept[BLOCKS[0] * B * N0 + 2 * 139 + 4] = N0
    got, want = _run(kept, None, None, stages, B, N0)
    _equal(got, want)
    assert got["kept"][BLOCKS[1]][0, 2] == -2 and got["kept"][BLOCKS[1]][1, 1] == -2 and got["kept"][BLOCKS[0]][2, 3] == -2
    assert got["kept"][BLOCKS[2]][2, 0] == -2
    assert got["kept_count"][BLOCKS[1]].tolist() == [60, 64, 10] and got["kept_count"][BLOCKS[2]].tolist() == [30, 30, 5]
    kept, stages = _tome_chain(N0, B, (16, 16, 16), rng)
    na = (N0 + 1) // 2
    kept[BLOCKS[0] * B * N0 + 3] = na                              # unm of image 0: one past the table
    kept[BLOCKS[0] * B * N0 + B * (na - 16) + 16 + 2] = -1         # src of image 1
    kept[BLOCKS[0] * B * N0 + B * na + 2 * 16 + 5] = N0 // 2       # dst of image 2: one past the b set
    got, want = _run(kept, None, None, stages, B, N0)
    _equal(got, want)
    assert [(got["assign"][BLOCKS[0]][b] == -2).sum() for b in range(B)] == [1, 1, 1]


def test_a_bad_stage_table_is_refused_and_nothing_is_launched():
    from tokenreduction_amd import _lib, ops
    B, N0 = 2, 197
    kept = torch.zeros(DEPTH * B * N0 + 4, dtype=torch.int32, device="cuda")
    good = [(0, _lib.TR_DECISION_PRUNE, N0, 137)]

    def refused(code, *args):
        def fn():
            with pytest.raises(RuntimeError, match=rf"code {code}\)"):
                ops.stage_decisions(*args)
        assert _launches.labels(fn) == []
    refused(-1, kept[:-4], None, None, [(0, _lib.TR_DECISION_PRUNE, N0, N0)], B, N0)                   # k >= n_in
    refused(-1, kept[:-4], None, None, [(0, _lib.TR_DECISION_PRUNE, N0 + 1, 137)], B, N0)              # n_in > N0
    refused(-5, kept[:-4], None, None, [(0, _lib.TR_DECISION_PRUNE, N0, 1)] * 33, B, N0)               # 33 stages
    refused(-2, kept[1:-3], None, None, good, B, N0)                                                   # a pointer at 4 bytes
    refused(-1, kept[:B * N0], None, None, [(1, _lib.TR_DECISION_PRUNE, N0, 137)], B, N0)              # a slab behind the buffer
    refused(-3, kept[:-4], None, None, [(0, _lib.TR_DECISION_SOFT, N0, 8)], B, N0)                     # a soft stage without its matrix
    assert _launches.labels(lambda: ops.stage_decisions(kept[:-4], None, None, good, B, N0)) == ["tr_stage_decisions"]
    assert _launches.labels(lambda: ops.stage_decisions(kept[:-4], None, None, [], B, N0)) == []     # no stage: no launch
    torch.cuda.synchronize()
