"""GPU parity tests, op level, for the lengths of 448 x 448 and 512 x 512 inputs (N = 785 and 1025 tokens incl. CLS): the entry points
that refused these shapes -- ToMe matching above 600 tokens, fp32 attention above 640, split attention above 1024, Sinkhorn with more
than 640 centres once K x P exceeds the LDS -- against the oracle on the same inputs, and the launch labels that show the kernels of
the shorter lengths are still the ones selected there."""
import numpy as np
import pytest
import torch

import oracle
from tests._launches import labels as _labels          # launch labels of the entry-point calls fn makes on the current stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _randn(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


# ---------------------------------------------------------------------------------------- ToMe bipartite matching
def _tome_case(N, H, f32, seed):
    qkv = _randn(seed, 2 * N, 3 * H * 64)
    if not f32:
        qkv = qkv.bfloat16().float()
    k = qkv.reshape(2, N, 3, H, 64)[:, :, 1].permute(0, 2, 1, 3)
    metric = k.mean(1)
    m = metric / metric.norm(dim=-1, keepdim=True)
    sc = m[:, ::2] @ m[:, 1::2].transpose(-1, -2)
    top2 = sc[:, 1:].topk(2, dim=-1).values
    # tie-free decision inputs: the row maxima's gap to the runner-up and the gaps between row maxima are far above fp32 noise
    assert (top2[..., 0] - top2[..., 1]).min() > 2e-6
    rowmax = top2[..., 0].sort(dim=-1).values
    assert (rowmax[:, 1:] - rowmax[:, :-1]).min() > 1e-7
    return qkv, metric


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("N,H,r,seed", [(601, 6, 150, 2), (785, 6, 196, 0), (785, 2, 392, 5), (1025, 6, 256, 0), (1025, 12, 7, 0),
                                        (1024, 3, 300, 0)])
def test_tome_match_long(ops, f32, N, H, r, seed):
    """N > 600: the odd rows in LDS, the even rows streamed in chunks (tr_tome_match_long); maps bit-exact against the oracle.
    (seed: the first seed whose decision inputs are tie-free in both precisions.)"""
    qkv, metric = _tome_case(N, H, f32, 7000 + N + H + seed)
    unm_w, src_w, dst_w = oracle.tome_match(metric, r)
    labels = []

    def run():
        labels.append(ops.tome_match((qkv if f32 else qkv.bfloat16()).cuda(), 2, N, H, r))

    assert _labels(run) == ["tr_tome_match_long"]
    unm, src, dst = labels[0]
    np.testing.assert_array_equal(unm.cpu().numpy(), unm_w.numpy())
    np.testing.assert_array_equal(src.cpu().numpy(), src_w.numpy())
    np.testing.assert_array_equal(dst.cpu().numpy(), dst_w.numpy())


@pytest.mark.parametrize("N", [197, 577, 600])
def test_tome_match_short_keeps_its_kernel(ops, N):
    """Up to 600 tokens the launch is the all-in-LDS kernel, as before."""
    qkv = _randn(N, 2 * N, 3 * 6 * 64)
    for f32 in (False, True):
        x = (qkv if f32 else qkv.bfloat16()).cuda()
        assert _labels(lambda: ops.tome_match(x, 2, N, 6, N // 4)) == ["tr_tome_match"]


def test_tome_match_refuses_beyond_1025(ops):
    with pytest.raises(RuntimeError, match="N <= 1025"):
        ops.tome_match(torch.zeros(1026, 3 * 64, device="cuda"), 1, 1026, 1, 4)


# ---------------------------------------------------------------------------------------- attention, fp32 and split-bf16
def _attn_want(qkv, B, N, H, size):
    q, k, v = qkv.double().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * 0.125
    if size is not None:
        s = s + size.double().log()[:, None, None, :]
    attn = s.softmax(-1)
    return attn, (attn @ v).transpose(1, 2).reshape(B * N, H * 64)


@pytest.mark.parametrize("B,N,H", [(1, 641, 2), (2, 785, 3), (1, 1025, 2), (1, 1088, 1)])
@pytest.mark.parametrize("with_size", [False, True])
def test_attention_f32_long(ops, B, N, H, with_size):
    """tr_attention_f32 beyond 640 keys, with CLS rows, the key bias (+ log size) and column sums, at the tolerances of test_hip_fp32.py."""
    qkv = _randn(N + H, B * N, 3 * H * 64, scale=1.5)
    size = (1 + torch.from_numpy(np.random.default_rng(N).integers(0, 4, (B, N)).astype(np.float32))) if with_size else None
    attn, want = _attn_want(qkv, B, N, H, size)
    colsum = torch.zeros(B, H, 4, N, device="cuda")
    res = []
    labels = _labels(lambda: res.append(ops.attention_f32(qkv.cuda(), B, N, H, want_cls=True, size=None if size is None else size.cuda(),
                                                          colsum_part=colsum)))
    assert labels == ["tr_attention_f32_long"]
    got, cls = res[0]
    torch.testing.assert_close(got.cpu(), want.float(), atol=2e-5, rtol=2e-5)
    torch.testing.assert_close(cls.cpu(), attn[:, :, 0, :].float(), atol=1e-7, rtol=2e-5)
    torch.testing.assert_close(colsum.sum((1, 2)).cpu().double(), attn.sum((1, 2)), atol=1e-4, rtol=2e-5)


def test_attention_f32_short_keeps_its_kernel(ops):
    qkv = _randn(3, 640, 3 * 64)
    assert _labels(lambda: ops.attention_f32(qkv.cuda(), 1, 640, 1)) == ["tr_attention_f32"]
    with pytest.raises(RuntimeError, match="N <= 1088"):
        ops.attention_f32(torch.zeros(1089, 3 * 64, device="cuda"), 1, 1089, 1)


@pytest.mark.parametrize("B,N,H", [(1, 1025, 2), (2, 1088, 1), (1, 1025, 6)])
@pytest.mark.parametrize("with_size", [False, True])
def test_attention_split_long(ops, B, N, H, with_size):
    """The chunked split-bf16 kernel past 1024 keys (nine chunks), at test_hip_split.py's tolerances; it no longer hands these
    lengths to tr_attention_f32."""
    qkv = _randn(N + H, B * N, 3 * H * 64, scale=1.5)
    size = (1 + torch.from_numpy(np.random.default_rng(N).integers(0, 4, (B, N)).astype(np.float32))) if with_size else None
    attn, want = _attn_want(qkv, B, N, H, size)
    colsum = torch.zeros(B, H, 4, N, device="cuda")
    res = []
    labels = _labels(lambda: res.append(ops.attention_f32(qkv.cuda(), B, N, H, want_cls=True, size=None if size is None else size.cuda(),
                                                          colsum_part=colsum, split=True)))
    assert labels == ["attention_split_long"]
    got, cls = res[0]
    torch.testing.assert_close(got.cpu().double(), want, atol=1e-4, rtol=3e-5)
    torch.testing.assert_close(cls.cpu().double(), attn[:, :, 0, :], atol=2e-6, rtol=2e-4)
    torch.testing.assert_close(colsum.sum((1, 2)).cpu().double(), attn.sum((1, 2)), atol=2e-4, rtol=1e-4)


# ---------------------------------------------------------------------------------------- Sinkhorn
@pytest.mark.parametrize("B,N,K,ldl,iters", [(2, 785, 641, 648, 3), (1, 1025, 921, 928, 3), (1, 1025, 1024, 1024, 2), (2, 1025, 705, 712, 0)])
def test_sinkhorn_many_centres(ops, B, N, K, ldl, iters):
    """K > 640 centres with K x P beyond the LDS (tr_sinkhorn_xl), at test_hip_ops.py's Sinkhorn tolerances."""
    scores = _randn(40 + N + K, B, N, ldl, scale=0.5).clamp(-1, 1)
    want = oracle.sinkhorn_transport(scores[:, 1:, :K].transpose(1, 2).contiguous(), 0.7, iters)
    res = []
    assert _labels(lambda: res.append(ops.sinkhorn(scores.cuda(), K, 0.7, iters, want_soft=True))) == ["tr_sinkhorn_xl"]
    wt, soft = res[0]
    torch.testing.assert_close(soft.cpu(), want, atol=1e-6, rtol=2e-5)
    torch.testing.assert_close(wt.cpu()[:, 1:, :K], want.transpose(1, 2), atol=1e-6, rtol=2e-5)


def test_sinkhorn_640_keeps_its_kernel(ops):
    scores = _randn(5, 1, 577, 640, scale=0.5).clamp(-1, 1)
    assert _labels(lambda: ops.sinkhorn(scores.cuda(), 640, 0.7, 1)) == ["tr_sinkhorn"]
    with pytest.raises(RuntimeError, match="K=1025"):
        ops.sinkhorn(torch.zeros(1, 1100, 1032, device="cuda"), 1025, 0.7, 1)
