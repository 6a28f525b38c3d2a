"""GPU tests of the norm prologue of tr_mlp_fused_ln_bf16 as the wave pair shares it (csrc/tr_mlp_fused.hip): at a workgroup's FIRST block
the fc1 wave normalises rows 0..15 of its 32-row slice and its fc2 partner rows 16..31, which cross LDS through ring slot 2; later blocks
of the workgroup are normalised by the fc1 wave alone.  Everything is compared BIT FOR BIT with tr_layernorm2_bf16 followed by
tr_mlp_fused_bf16 (the per-row arithmetic is the LayerNorm kernel's, whichever wave runs it), so no tolerance appears below.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

D, HD = 384, 1536


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _randn(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


@pytest.fixture(scope="module")
def mlp(ops):
    """One set of Mlp and norm parameters for every case of this file."""
    rng = np.random.default_rng(1234)
    w1, w2 = _randn(rng, HD, D, scale=0.05).bfloat16().cuda(), _randn(rng, D, HD, scale=0.05).bfloat16().cuda()
    b1, b2 = _randn(rng, HD, scale=0.1).cuda(), _randn(rng, D, scale=0.1).cuda()
    g, bt = (1.0 + 0.2 * _randn(rng, D)).cuda(), (0.1 * _randn(rng, D)).cuda()
    return {"pk": ops.mlp_pack(w1, w2, b2), "b1": b1, "g": g, "bt": bt}


def _stream_rows(M, seed):
    """The fp32 stream and the pending bf16 residual of M rows: per-row spreads from 1e-3 to 50 (small and large variance), every seventh
    row with a common offset that dwarfs its spread, a constant row; a nonzero delta of unit spread."""
    rng = np.random.default_rng(seed)
    spread = torch.tensor([1e-3, 1.0, 50.0, 0.05, 7.0])[torch.arange(M) % 5].unsqueeze(1)
    x = spread * _randn(rng, M, D)
    x[::7] += 300.0
    if M > 3:
        x[3] = 1.25
    delta = _randn(rng, M, D).bfloat16()
    return x.cuda(), delta.cuda()


@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257])
def test_split_prologue_is_bit_identical_to_layernorm_then_mlp(ops, mlp, M):
    """One row to three blocks: the edges of the 16-row group one wave of a pair normalises (15, 16, 17), of the pair's 32-row slice
    (31, 32, 33), of the 128-row block (127, 128, 129) and a ragged third block (257).  Rows beyond M are clamped to the last row on
    both waves and their results dropped: the guard rows behind the output stay untouched; the inputs are not written."""
    x, delta = _stream_rows(M, 100 + M)
    x0, d0 = x.clone(), delta.clone()
    want = ops.mlp_fused(ops.layernorm2(x, mlp["g"], mlp["bt"], 1e-6, delta, write_x=False), mlp["pk"], mlp["b1"])
    for streamk in (True, False):
        guard = torch.full((M + 3, D), float("nan"), dtype=torch.bfloat16, device="cuda")
        got = ops.mlp_fused_ln(x, delta, mlp["g"], mlp["bt"], 1e-6, mlp["pk"], mlp["b1"], out=guard[:M], streamk=streamk)
        diff = got.view(torch.int16) != want.view(torch.int16)
        assert not bool(diff.any()), (f"streamk={streamk}: {int(diff.sum())} of {got.numel()} elements differ from LayerNorm + fused Mlp, rows "
                                      f"{diff.any(dim=1).nonzero().flatten()[:12].tolist()}")
        assert torch.isnan(guard[M:].float()).all(), "rows beyond M were written"
    assert torch.equal(x, x0) and torch.equal(delta.view(torch.int16), d0.view(torch.int16)), "an input was written"
    ops.mlp_fused_status()


_GRID_WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["TR_ROOT"])
import torch
from tokenreduction_amd import ops
D, Hd = 384, 1536
M = 5 * 128 + 3
g0 = torch.Generator().manual_seed(11)
x = 2.0 * torch.randn(M, D, generator=g0)
x[::7] += 300.0
x[1::5] *= 1e-3
x, delta = x.cuda(), torch.randn(M, D, generator=g0).bfloat16().cuda()
w1, w2 = (0.05 * torch.randn(Hd, D, generator=g0)).bfloat16().cuda(), (0.05 * torch.randn(D, Hd, generator=g0)).bfloat16().cuda()
b1, b2 = (0.1 * torch.randn(Hd, generator=g0)).cuda(), (0.1 * torch.randn(D, generator=g0)).cuda()
g, bt = (1.0 + 0.2 * torch.randn(D, generator=g0)).cuda(), (0.1 * torch.randn(D, generator=g0)).cuda()
pk = ops.mlp_pack(w1, w2, b2)
xn = ops.layernorm2(x, g, bt, 1e-6, delta, write_x=False)
want = ops.mlp_fused(xn, pk, b1, streamk=False)
# (the reference itself against the two GEMM launches, so that it does not lean on the launch under test's sibling alone)
pair = ops.gemm(ops.gemm(xn, w1, b1, ops.TR_EPI_GELU_BF16), w2, b2, ops.TR_EPI_BF16)
assert torch.equal(want.view(torch.int16), pair.view(torch.int16)), "reference: fused Mlp differs from the GEMM pair"
for streamk in (True, False):
    for it in range(3):
        guard = torch.full((M + 3, D), float("nan"), dtype=torch.bfloat16, device="cuda")
        got = ops.mlp_fused_ln(x, delta, g, bt, 1e-6, pk, b1, out=guard[:M], streamk=streamk)
        diff = got.view(torch.int16) != want.view(torch.int16)
        assert not bool(diff.any()), (streamk, it, int(diff.sum()), diff.any(dim=1).nonzero().flatten()[:12].tolist())
        assert torch.isnan(guard[M:].float()).all(), "rows beyond M were written"
    ops.mlp_fused_status()
print("grid ok")
"""


@pytest.mark.parametrize("grid", [2, 3, 4])
def test_split_prologue_then_reload_path_on_a_smaller_grid(ops, tmp_path, grid):
    """Six blocks (5 x 128 + 3 rows) on 2, 3 and 4 workgroups (TR_MLP_FUSED_GRID, read at library load -> a subprocess): a workgroup's
    first block takes the split prologue, its later ones the fc1 wave's own norm -- with the whole-block schedule and with the
    hand-over scratch given.  On 2 and 3 workgroups the stream-K ranges are whole blocks (3 and 2 each); on 4 they are 1.5 blocks, so
    a workgroup's first segment is the HEAD of a block another workgroup finishes (split prologue on a block that is handed over) and
    its last a tail (the fc1 wave's own norm, the accumulator taken over).  Three launches each, the last block ragged."""
    script = tmp_path / "ln_pair_grid_worker.py"
    script.write_text(_GRID_WORKER)
    env = dict(os.environ, TR_ROOT=ROOT, TR_MLP_FUSED_GRID=str(grid))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "grid ok" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.parametrize("M", [128, 129])
def test_split_prologue_back_to_back_launches(ops, mlp, M):
    """Race screen of the hand-over through ring slot 2: 200 launches enqueued back to back with no host synchronisation between them,
    each into its own output; every result must equal the first bit for bit (and the first the LayerNorm + fused Mlp pair).  One block
    (every wave pair full) and two (the second block holds one row: all other rows of its slices are clamped copies)."""
    x, delta = _stream_rows(M, 900 + M)
    want = ops.mlp_fused(ops.layernorm2(x, mlp["g"], mlp["bt"], 1e-6, delta, write_x=False), mlp["pk"], mlp["b1"])
    outs = torch.full((200, M, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    for it in range(200):
        ops.mlp_fused_ln(x, delta, mlp["g"], mlp["bt"], 1e-6, mlp["pk"], mlp["b1"], out=outs[it])
    torch.cuda.synchronize()
    bits = outs.view(torch.int16)
    differing = (bits != bits[0]).flatten(1).any(dim=1).nonzero().flatten().tolist()
    assert not differing, f"{len(differing)} of 200 launches differ from the first: launches {differing[:10]}"
    assert torch.equal(bits[0], want.view(torch.int16)), "the first launch differs from LayerNorm + fused Mlp"
    ops.mlp_fused_status()
