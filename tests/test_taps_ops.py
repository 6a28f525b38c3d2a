"""The two tap kernels (csrc/tr_taps.hip) against a restatement, bitwise.

tr_cls_tap: out[b] = (x[b] + d1[b]) + d2[b] -- torch's fp32 additions in that order (IEEE, so equal or wrong).
tr_final_tokens_f32: the same sums through ops.layernorm_f32 (tr_layernorm_f32), the two-launch sequence the kernel replaces.
Shapes: every NCH instantiation (D 64 ... 1024, with D = 192 / 384 / 768 leaving lanes of the last chunk idle), one row, rows that do
not fill the 4-row workgroup (B = 1, 3; M = 2 ... 594), both row strides of every operand, zero / one / two pending operands of either type."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS = [64, 128, 192, 384, 768, 1024]
GUARD = -12345.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _rows(t, B, ld, D):
    """The B rows of D that a kernel reads from flat tensor t at row stride ld, as fp32."""
    return torch.as_strided(t, (B, D), (ld, 1)).float()


def _operand(g, B, ld, D, dtype, scale):
    """A flat operand holding B rows at stride ld (the rest of a [B, N, D] slab is there too and must not be read)."""
    return (scale * torch.randn(B * ld, generator=g)).to(dtype).cuda()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", DIMS)
def test_cls_tap_is_the_two_additions_in_order(ops, D, dtype):
    g = torch.Generator().manual_seed(1000 + D)
    for B, N, full_x, full_d, nops, nblk in itertools.product((1, 3), (2, 197, 198), (True, False), (True, False), (0, 1, 2), (1, 4)):
        ldx, ldd = (N * D if full_x else D), (N * D if full_d else D)
        x = _operand(g, B, ldx, D, torch.float32, 2.0)
        d = [_operand(g, B, ldd, D, dtype, 1.0) for _ in range(nops)]
        want = _rows(x, B, ldx, D)
        for t in d:
            want = want + _rows(t, B, ldd, D)
        col = nblk - 2 if nblk > 1 else 0                       # a middle column of the image's taps
        out = torch.full((B + 2, nblk, D), GUARD, dtype=torch.float32, device="cuda")       # a guard row on either side
        ops.cls_tap(x, ldx, B, D, d[0] if nops > 0 else None, ldd, d[1] if nops > 1 else None, ldd, out=out, ldo=nblk * D,
                    offset=(nblk + col) * D)
        what = (B, N, ldx, ldd, nops, nblk)
        assert torch.equal(out[1:B + 1, col], want), what
        keep = torch.ones(B + 2, nblk, dtype=torch.bool)
        keep[1:B + 1, col] = False
        assert bool((out[keep.cuda()] == GUARD).all()), what


def test_cls_tap_addition_order_is_observable():
    """The restatement above would also pass for x + (d1 + d2) if the two orders agreed on the test data: they do not."""
    g = torch.Generator().manual_seed(7)
    x, d1, d2 = 2.0 * torch.randn(3, 384, generator=g), torch.randn(3, 384, generator=g).bfloat16().float(), torch.randn(3, 384, generator=g).bfloat16().float()
    assert not torch.equal((x + d1) + d2, x + (d1 + d2))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", DIMS)
def test_final_tokens_is_the_snapshot_followed_by_layernorm_f32(ops, D, dtype):
    g = torch.Generator().manual_seed(2000 + D)
    gamma, beta = (1.0 + 0.2 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
    for B, N, nops in itertools.product((1, 3), (2, 197, 198), (0, 1, 2)):
        M = B * N
        x = (2.0 * torch.randn(M, D, generator=g) + 0.3).cuda()
        d = [torch.randn(M, D, generator=g).to(dtype).cuda() for _ in range(nops)]
        summed = x.clone()
        for t in d:
            summed = summed + t.float()
        want = ops.layernorm_f32(summed, gamma, beta, 1e-6)
        x_before = x.clone()
        got = ops.final_tokens_f32(x, gamma, beta, 1e-6, d[0] if nops > 0 else None, d[1] if nops > 1 else None)
        assert got.shape == (M, D) and torch.equal(got, want), (B, N, nops)
        assert torch.equal(x, x_before), (B, N, nops)                 # the stream is not written


def test_argument_checks(ops):
    x = torch.zeros(2 * 64, device="cuda")
    d = torch.zeros(2 * 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="tr_cls_tap"):
        ops.cls_tap(x, 64, 2, 62)                                 # D % 4
    with pytest.raises(RuntimeError, match="tr_cls_tap"):
        ops.cls_tap(x, 32, 2, 64)                                 # row stride below D
    with pytest.raises(RuntimeError, match="second pending operand"):
        ops.cls_tap(x, 64, 2, 64, None, 0, d, 64)
    with pytest.raises(TypeError):
        ops.cls_tap(x, 64, 2, 64, d, 64, d.float(), 64)           # one dtype for both operands
    g = torch.ones(64, device="cuda")
    with pytest.raises(RuntimeError, match="second pending operand"):
        ops.final_tokens_f32(x.view(2, 64), g, g, 1e-6, None, d.view(2, 64))
