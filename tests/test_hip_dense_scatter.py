"""tr_dense_scatter at op level (GPU tier): synthetic inputs, no model; every comparison is bit equality with the numpy restatement
(tests/_dense_train_ref.py), whose additions are fp32, sequential, in ascending p.
One test per (P, D) of P in {1, 3, 63, 64, 65, 196, 1024} x D in {4, 64, 68, 128, 384}; inside it n_rows in {1, 2, P + 1} x the seven index
patterns, each under one of the eight (layout, input dtype, output dtype) combinations -- the combination moves on by one from case to case
and starts one further on from test to test, so that every pattern and every n_rows meets every combination.  The output buffer is
pre-filled with NaN and has a canary behind it; the launch runs twice."""
import numpy as np
import pytest
import torch

from tests import _dense_ref as ref
from tests import _dense_train_ref as tref
from tests import _launches
from tests.test_hip_dense import _bits

pytestmark = pytest.mark.gpu

PS = [1, 3, 63, 64, 65, 196, 1024]
DS = [4, 64, 68, 128, 384]
PATTERNS = ["identity", "none", "holes", "merge", "one_row", "zeros", "outside"]
COMBOS = [(layout, src, dst) for layout in ("NCHW", "NHWC") for src in ("fp32", "bf16") for dst in ("fp32", "bf16")]
INT32_MIN = -2 ** 31
B = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _index(pattern, P, n_rows, rng):
    if pattern == "identity":
        idx = np.tile(np.arange(1, P + 1), (B, 1))              # (rows past n_rows - 1 own nothing)
    elif pattern == "none":
        idx = np.full((B, P), -1)
    elif pattern == "holes":                                     # pruning: a permutation of some rows, -1 elsewhere
        idx = np.full((B, P), -1)
        for b in range(B):
            keep = rng.permutation(P)[:min(P, max(1, n_rows - 1))]
            idx[b, keep] = 1 + rng.permutation(len(keep))
    elif pattern == "merge":                                     # merging: many patches to one row, some rows nobody names
        idx = rng.integers(0, max(1, n_rows // 2 + 1), size=(B, P))
    elif pattern == "one_row":                                   # the longest list: every patch of an image in one row
        idx = np.tile(rng.integers(0, n_rows, size=(B, 1)), (1, P))
    elif pattern == "zeros":                                     # row 0 is a row like any other
        idx = rng.integers(0, n_rows, size=(B, P))
        idx[rng.random((B, P)) < 0.5] = 0
    else:
        idx = rng.integers(0, n_rows, size=(B, P))
        bad = np.array([n_rows, n_rows + 5, -2, -1, INT32_MIN, 2 ** 31 - 1])
        where = rng.random((B, P)) < 0.4
        idx[where] = np.resize(bad, int(where.sum()))
        idx.reshape(-1)[0] = -2
        idx.reshape(-1)[-1] = n_rows
    return idx.astype(np.int32)


def _dmap(P, D, layout, src, rng):
    g = rng.standard_normal((B, D, P) if layout == "NCHW" else (B, P, D)).astype(np.float32)
    flat = g.reshape(-1)
    # +-0, fp32 denormals, values half way between two bf16 neighbours, a large and a tiny magnitude (no inf: inf - inf has no one NaN)
    special = np.array([0.0, -0.0, 1e-45, -3e-39, 1.1754942e-38, 1.00390625, 1.01171875, -1.00390625, 65280.0, -1e30, 1e-30], dtype=np.float32)
    at = rng.permutation(flat.size)[:min(flat.size, 3 * special.size)]
    flat[at] = np.resize(special, at.size)
    if src == "bf16":
        bits = ref.to_bf16_bits(g)
        return bits, torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    return g, torch.from_numpy(g).cuda()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", PS)
def test_scatter_is_the_restatement_bit_for_bit(P, D):
    from tokenreduction_amd import ops
    rng = np.random.default_rng(P * 131 + D)
    step = PS.index(P) * len(DS) + DS.index(D)
    maps = {}
    for n_rows in (1, 2, P + 1):
        for pattern in PATTERNS:
            layout, src, dst = COMBOS[step % len(COMBOS)]
            step += 1
            if (layout, src) not in maps:
                maps[layout, src] = _dmap(P, D, layout, src, rng)
            host, dev = maps[layout, src]
            index = _index(pattern, P, n_rows, rng)
            want = tref.dense_scatter(host, index, n_rows, layout, dst)
            want = want if dst == "bf16" else want.view(np.uint32)
            assert not np.isnan(want.view(np.float32) if dst == "fp32" else tref.bf16_bits_to_f32(want)).any()
            i = torch.from_numpy(index).cuda()
            tdtype = torch.bfloat16 if dst == "bf16" else torch.float32
            n = B * n_rows * D
            buf = torch.full((n + 64,), float("nan"), dtype=tdtype, device="cuda")
            got = ops.dense_scatter(dev, i, n_rows, layout=layout, dtype=tdtype, out=buf[:n])
            what = (pattern, n_rows, layout, src, dst)
            assert got.shape == (B, n_rows, D)
            assert not torch.isnan(got).any(), what                   # every element written
            np.testing.assert_array_equal(_bits(got), want, err_msg=str(what))
            assert torch.isnan(buf[n:]).all(), what                    # nothing behind the end
            again = ops.dense_scatter(dev, i, n_rows, layout=layout, dtype=tdtype)
            assert np.array_equal(_bits(again), want), what            # the same launch twice: the same bits


def test_scatter_is_one_launch_and_the_gathers_adjoint_on_the_device():
    """<gather(T), G> == <T, scatter(G)> exactly on integer-valued arrays, with the device's gather and the device's scatter."""
    from tokenreduction_amd import ops
    rng = np.random.default_rng(5)
    P, D, n_rows = 196, 68, 120
    index = _index("merge", P, n_rows, rng)
    index[rng.random((B, P)) < 0.2] = -1
    i = torch.from_numpy(index).cuda()
    T = torch.from_numpy(rng.integers(-8, 9, size=(B, n_rows, D)).astype(np.float32)).cuda()
    for layout in ("NCHW", "NHWC"):
        G = torch.from_numpy(rng.integers(-8, 9, size=(B, D, P) if layout == "NCHW" else (B, P, D)).astype(np.float32)).cuda()
        lhs = (ops.dense_gather(T, i, layout=layout, fill=0.0).double() * G.double()).sum()
        rhs = (T.double() * ops.dense_scatter(G, i, n_rows, layout=layout).double()).sum()
        assert lhs.item() == rhs.item()
        assert _launches.labels(lambda: ops.dense_scatter(G, i, n_rows, layout=layout)) == ["tr_dense_scatter"]


def test_scatter_refuses_what_the_header_refuses():
    from tokenreduction_amd import ops
    g, i = torch.zeros(2, 8, 4, device="cuda"), torch.zeros(2, 4, dtype=torch.int32, device="cuda")

    def refused(exc, match, *args, **kw):
        def fn():
            with pytest.raises(exc, match=match):
                ops.dense_scatter(*args, **kw)
        assert _launches.labels(fn) == []
    refused(ValueError, "layout", g, i, 5, layout="CHWN")
    refused(ValueError, "dtype", g, i, 5, dtype=torch.float16)
    refused(ValueError, "dtype", g.half(), i, 5)
    refused(ValueError, r"\[B, P\]", g, i[:1], 5)
    refused(RuntimeError, r"code -1\)", torch.zeros(2, 6, 4, device="cuda"), i, 5)                              # D % 4
    refused(RuntimeError, r"code -1\)", torch.zeros(2, 8, 1025, device="cuda"), torch.zeros(2, 1025, dtype=torch.int32, device="cuda"), 5)
    refused(RuntimeError, r"code -2\)", torch.zeros(2 * 8 * 4 + 1, device="cuda")[1:].view(2, 8, 4), i, 5)
    torch.cuda.synchronize()
