"""tr_dense_scatter_levels, tr_level_tap_norm and tr_stream_grad_add at op level (GPU tier): synthetic inputs, no model; every comparison is
bit equality.

The scatter of L levels is compared with the numpy restatement (tests/_dense_train_levels_ref.dense_scatter_levels: fp32 additions,
sequential, ascending p) AND with L separate tr_dense_scatter launches on the same slabs.  One test per (P, D) of P in {1, 63, 64, 65, 196,
1023, 1024} x D in {4, 68, 384, 1024} at B = 3; inside it L in {1, 2, 4, 32}, each under one of the eight (layout, input dtype, output dtype)
combinations -- the combination moves on by one from L to L and starts one further on from test to test, so every L meets every
combination.  The levels' rows differ (1, P + 1 and values between), their indices cycle through the patterns (identity, pruning holes, every
patch on one row, entries -2 / n_rows that own nothing, merges that leave rows unnamed); with L >= 4 some levels have no gradient (NULL).
The output is pre-filled with NaN and has a canary behind it: a present level writes exactly its [B, rows, D], a NULL level's slab stays
untouched.  The launch runs twice."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _dense_ref as ref
from tests import _dense_train_levels_ref as lref
from tests import _dense_train_ref as tref
from tests import _launches
from tests.test_hip_dense import _bits

pytestmark = pytest.mark.gpu

PS = [1, 63, 64, 65, 196, 1023, 1024]
DS = [4, 68, 384, 1024]
LS = [1, 2, 4, 32]
PATTERNS = ["identity", "holes", "one_row", "outside", "merge"]
COMBOS = [(layout, src, dst) for layout in ("NCHW", "NHWC") for src in ("fp32", "bf16") for dst in ("fp32", "bf16")]
B = 3
OK, SHAPE, ALIGN, NULL, CONFIG = 0, -1, -2, -3, -5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _index(pattern, P, n_rows, rng):
    if pattern == "identity":
        idx = np.tile(np.arange(1, P + 1), (B, 1))              # (rows past n_rows - 1 own nothing)
    elif pattern == "holes":                                     # pruning: a permutation of some rows, -1 elsewhere
        idx = np.full((B, P), -1)
        for b in range(B):
            keep = rng.permutation(P)[:min(P, max(1, n_rows - 1))]
            idx[b, keep] = 1 + rng.permutation(len(keep))
    elif pattern == "one_row":                                   # the longest sum: every patch of an image on one row
        idx = np.tile(rng.integers(0, n_rows, size=(B, 1)), (1, P))
    elif pattern == "outside":                                   # -2 and n_rows own nothing
        idx = rng.integers(0, n_rows, size=(B, P))
        where = rng.random((B, P)) < 0.4
        idx[where] = np.resize(np.array([n_rows, -2, -1, n_rows + 5]), int(where.sum()))
        idx.reshape(-1)[0], idx.reshape(-1)[-1] = -2, n_rows
    else:                                                        # merging: many patches to one row, the upper half of the rows unnamed
        idx = rng.integers(0, max(1, n_rows // 2 + 1), size=(B, P))
    return idx.astype(np.int32)


def _dmap(P, D, layout, src, rng):
    g = rng.standard_normal((B, D, P) if layout == "NCHW" else (B, P, D)).astype(np.float32)
    flat = g.reshape(-1)
    special = np.array([0.0, -0.0, 1e-45, -3e-39, 1.00390625, 1.01171875, 65280.0, -1e30, 1e-30], dtype=np.float32)
    at = rng.permutation(flat.size)[:min(flat.size, 2 * special.size)]
    flat[at] = np.resize(special, at.size)
    if src == "bf16":
        bits = ref.to_bf16_bits(g)
        return bits, torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    return g, torch.from_numpy(g).cuda()


def _level_rows(L, P):
    pool = [P + 1, 1, max(1, P // 2), 2, max(1, P - 1), 3]
    return [min(pool[l % len(pool)], P + 1) for l in range(L)]


def _absent(L):
    return {1} if L == 4 else {1, 7, 30, 31} if L == 32 else set()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", PS)
def test_scatter_levels_is_the_restatement_and_the_single_level_kernel_bit_for_bit(P, D):
    from tokenreduction_amd import ops
    rng = np.random.default_rng(P * 131 + D)
    step = PS.index(P) * len(DS) + DS.index(D)
    for L in LS:
        layout, src, dst = COMBOS[step % len(COMBOS)]
        step += 1
        rows, absent = _level_rows(L, P), _absent(L)
        pool = [_dmap(P, D, layout, src, rng) for _ in range(min(L, 3))]             # (levels may share a map: the pointers travel per level)
        index = np.stack([_index(PATTERNS[(l + step) % len(PATTERNS)], P, rows[l], rng) for l in range(L)])
        host = [None if l in absent else pool[l % len(pool)][0] for l in range(L)]
        dev = [None if l in absent else pool[l % len(pool)][1] for l in range(L)]
        want = lref.dense_scatter_levels(host, index, rows, layout, dst)
        tdtype = torch.bfloat16 if dst == "bf16" else torch.float32
        stride = (B * (P + 1) * D + 7) // 8 * 8
        i = torch.from_numpy(index).cuda()
        buf = torch.full((L * stride + 64,), float("nan"), dtype=tdtype, device="cuda")
        what = (L, layout, src, dst)
        recs = _launches.labels(lambda: ops.dense_scatter_levels(dev, i, rows, stride, layout=layout, dtype=tdtype, out=buf[:L * stride]))
        assert recs == ["tr_dense_scatter_levels"], (what, recs)                      # ONE launch for all levels
        first = buf.clone()
        for l in range(L):
            slab, n = buf[l * stride: (l + 1) * stride], B * rows[l] * D
            if l in absent:
                assert torch.isnan(slab).all(), (what, l)                             # no gradient: the slab is not touched
                continue
            got = slab[:n].view(B, rows[l], D)
            assert not torch.isnan(got).any(), (what, l)                              # every element of a present level is written
            w = want[l] if dst == "bf16" else want[l].view(np.uint32)
            np.testing.assert_array_equal(_bits(got), w, err_msg=str((what, l)))
            single = ops.dense_scatter(dev[l], i[l].clone(), rows[l], layout=layout, dtype=tdtype)
            assert np.array_equal(_bits(single), _bits(got)), (what, l)               # the single-level kernel's bits
            assert torch.isnan(slab[n:]).all(), (what, l)                             # ... and nothing behind its rows
        assert torch.isnan(buf[L * stride:]).all(), what
        buf2 = torch.full_like(buf, float("nan"))
        ops.dense_scatter_levels(dev, i, rows, stride, layout=layout, dtype=tdtype, out=buf2[:L * stride])
        assert torch.equal(_bits_t(buf2), _bits_t(first)), what                       # the same launch twice: the same bits


def _bits_t(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def test_no_level_with_a_gradient_launches_nothing():
    from tokenreduction_amd import ops
    i = torch.zeros(2, B, 8, dtype=torch.int32, device="cuda")
    out = torch.full((2 * 3 * 9 * 8,), 5.0, device="cuda")
    assert _launches.labels(lambda: ops.dense_scatter_levels([None, None], i, [9, 4], 3 * 9 * 8, out=out)) == []
    assert (out == 5.0).all()


def test_scatter_levels_refusals_return_their_codes_without_a_launch():
    from tokenreduction_amd import _lib
    lib = _lib.load()
    P, D = 64, 8
    stride = B * (P + 1) * D
    g = torch.zeros(B * D * P + 4, device="cuda")
    i = torch.zeros(33 * B * P + 4, dtype=torch.int32, device="cuda")
    out = torch.zeros(33 * stride + 4, device="cuda")
    codes = []

    def call(L=2, layout=_lib.TR_LAYOUT_NCHW, maps=None, index=None, dst=None, stride=stride, rows=None):
        maps = [g.data_ptr()] * max(L, 1) if maps is None else maps
        rows = [P + 1] * max(L, 1) if rows is None else rows
        ptrs, r = (C.c_void_p * len(maps))(*maps), (C.c_int32 * len(rows))(*rows)
        codes.append(lib.tr_dense_scatter_levels(ptrs, i.data_ptr() if index is None else index, out.data_ptr() if dst is None else dst, stride, r, L,
                                                 layout, 0, 0, B, P, D, torch.cuda.current_stream().cuda_stream))

    def all_refused():
        call(L=0)
        call(L=33)
        call(layout=7)
        call(maps=[g.data_ptr(), g.data_ptr() + 4])
        call(index=i.data_ptr() + 4)
        call(dst=out.data_ptr() + 8)
        call(stride=stride - 8)
        call(stride=stride + 2)
    assert _launches.labels(all_refused) == []
    assert codes == [CONFIG, CONFIG, CONFIG, ALIGN, ALIGN, ALIGN, SHAPE, ALIGN], codes
    assert not out.any()


# ---- the two-output level tap -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 384, 1024])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 3 * 197])
def test_level_tap_norm_is_cls_tap_and_final_tokens_in_one_launch(M, D):
    from tokenreduction_amd import ops
    g = torch.Generator().manual_seed(M * 7 + D)
    x = (torch.randn(M, D, generator=g) * 3).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
    for delta in (torch.bfloat16, torch.float32):
        d1, d2 = torch.randn(M, D, generator=g).cuda().to(delta), torch.randn(M, D, generator=g).cuda().to(delta)
        for pending in ((None, None), (d1, None), (d1, d2)):
            keep = x.clone()
            recs = _launches.labels(lambda: ops.level_tap_norm(x, gamma, beta, 1e-6, *pending))
            assert recs == ["tr_level_tap_norm"], recs
            total, y = ops.level_tap_norm(x, gamma, beta, 1e-6, *pending)
            want_total = ops.cls_tap(x, D, M, D, pending[0], D, pending[1], D)
            want_y = ops.final_tokens_f32(x, gamma, beta, 1e-6, *pending)
            what = (M, D, delta, sum(p is not None for p in pending))
            assert torch.equal(_bits_t(total), _bits_t(want_total)), what
            assert torch.equal(_bits_t(y), _bits_t(want_y)), what
            assert torch.equal(_bits_t(x), _bits_t(keep)), what                        # x is not written


@pytest.mark.parametrize("D", [4, 384, 1024])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 3 * 197])
def test_stream_grad_add_is_the_fp32_sum_and_its_bf16_rounding(M, D):
    from tokenreduction_amd import ops
    rng = np.random.default_rng(M * 11 + D)
    g, d = rng.standard_normal((M, D)).astype(np.float32), rng.standard_normal((M, D)).astype(np.float32)
    g.reshape(-1)[:4], d.reshape(-1)[:4] = [1.0, 1.0, -0.0, 65280.0], [2.0 ** -8, 3 * 2.0 ** -8, 0.0, 128.0]      # ties of the bf16 rounding
    want = g + d
    tg, td = torch.from_numpy(g).cuda(), torch.from_numpy(d).cuda()
    tb = torch.full((M * D + 8,), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert _launches.labels(lambda: ops.stream_grad_add(td, tg, tb[:M * D])) == ["tr_stream_grad_add"]
    np.testing.assert_array_equal(_bits(tg), want.view(np.uint32))
    np.testing.assert_array_equal(_bits(tb[:M * D].view(M, D)), ref.to_bf16_bits(want))
    assert torch.isnan(tb[M * D:]).all()
    np.testing.assert_array_equal(_bits(td), d.view(np.uint32))
    ops.stream_grad_add(td, tg)                                  # without the bf16 copy
    np.testing.assert_array_equal(_bits(tg), (want + d).view(np.uint32))
