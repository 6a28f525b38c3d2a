"""Per-block comparison of the attention-backward kernels (tests/test_hip_backward.py) and the CPU measurement its bounds come from.

The kernels are tiled by 16-row query blocks and 64-key blocks, so they are held per block: dq per 16 queries, dk / dv per 64 keys, each per
(image, head), each against the reference's norm over the same slice.  The bound is measured from the reference alone: a float64
restatement of the backward that rounds P (in the P^T dO product) and dS (in the dS K and dS^T Q products) to bf16 where the kernels do,
against the unrounded float64 gradient, per block, over the tests' own shapes and seeds.  `python -m tests._attn_bwd_ref` prints the worst
block of every test; the kernels are allowed 2 x that (their bf16 output rounding, 2^-9 per element, and fp32 order)."""
import torch

import oracle

QB, KB = 16, 64            # query rows per block of dq, keys per block of dk / dv
SMALL = 1e-3               # blocks below this share of the tensor's norm are compared absolutely
MAX_SMALL_SHARE = 0.02
# (B, N, H) of the attention-backward tests: shared by their parametrize marks and by the measurement below
SHAPES = {"bwd": [(2, 197, 6), (3, 50, 3), (1, 224, 2), (2, 17, 1), (2, 139, 12), (1, 64, 1), (4, 98, 3)],
          "long": [(2, 577, 3), (1, 290, 2), (2, 197, 6), (1, 65, 1), (3, 64, 2), (1, 640, 1), (2, 17, 1)],
          "policy": [(2, 577, 2), (1, 300, 3), (2, 197, 6), (2, 138, 2), (1, 40, 1), (1, 640, 1)]}
# one N per count of 32-key blocks, 1..7: every instantiation the register-resident kernels are dispatched to (plain, bias and policy form)
SHAPES["bwd_blocks"] = SHAPES["policy_blocks"] = [(2, 17, 1), (1, 50, 2), (1, 81, 2), (1, 98, 2), (1, 139, 2), (1, 177, 2), (1, 197, 2)]


class _RoundGrad(torch.autograd.Function):
    """Identity whose GRADIENT is rounded to bf16: dS as the kernels feed it to the matrix cores."""
    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return oracle.round_bf16(g).to(g.dtype)


class _RoundValue(torch.autograd.Function):
    """bf16 rounding of the value, identity gradient: P as the kernels feed it to the matrix cores."""
    @staticmethod
    def forward(ctx, t):
        return oracle.round_bf16(t).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def attention(qkv, B, N, H, size=None, policy=None, rounded=False):
    """softmax(q k^T / 8 [+ log size]) v, or DyViT's softmax_with_policy (policy [B,N]) -> (out [B*N, H*64], p [B,H,N,N]).  rounded: with
    the kernels' bf16 roundings of P and dS placed in the backward."""
    q, k, v = qkv.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    if rounded:
        s = _RoundGrad.apply(s)
    if policy is not None:
        p = oracle.dyvit_softmax_with_policy(s, policy.unsqueeze(-1))
    else:
        if size is not None:
            s = s + size.log()[:, None, None, :]
        p = s.softmax(-1)
    out = ((_RoundValue.apply(p) if rounded else p) @ v).transpose(1, 2).reshape(B * N, H * 64)
    return out, p


def block_errors(got, want, B, N, H):
    """got, want: d qkv [B*N, 3*H*64].  -> {"q" | "k" | "v": (rel, abs_rel, small, nonzero)}: per block, the error norm over the reference's
    norm of the same slice; the error norm over the whole tensor's norm; whether the block is `small` (reference norm < SMALL of the
    tensor's, but not zero); and whether a block whose reference is exactly zero (dk / dv of a block of masked keys only) is not."""
    got = got.detach().double().cpu().view(B, N, 3, H, 64)
    want = want.detach().double().cpu().view(B, N, 3, H, 64)
    res = {}
    for i, nm in enumerate("qkv"):
        blk = QB if nm == "q" else KB
        nb = (N + blk - 1) // blk
        pad = nb * blk - N
        g, w = (torch.nn.functional.pad(t[:, :, i].permute(0, 2, 1, 3), (0, 0, 0, pad)).reshape(B, H, nb, blk * 64) for t in (got, want))
        err, ref = (g - w).norm(dim=-1), w.norm(dim=-1)
        whole = want[:, :, i].norm()
        res[nm] = (err / ref.clamp_min(1e-300), err / whole, (ref < SMALL * whole) & (ref > 0), (ref == 0) & (err > 0))
    return res


def assert_blocks(got, want, B, N, H, bound, what=""):
    """Every block of dq / dk / dv within `bound` of the reference's block (relative L2); small blocks within bound * SMALL of the tensor's
    norm instead, and at most MAX_SMALL_SHARE of the blocks may be small; a block whose reference is exactly zero must be exactly zero.  Prints the worst block before it asserts."""
    n_small = n_all = 0
    for nm, (rel, abs_rel, small, nonzero) in block_errors(got, want, B, N, H).items():
        assert not bool(nonzero.any()), f"{what} d{nm}: a block whose reference gradient is exactly zero is not zero"
        n_small += int(small.sum())
        n_all += small.numel()
        rel = torch.where(abs_rel == 0, torch.zeros_like(rel), rel)            # exact blocks (the zero ones among them)
        worst = float(rel[~small].max()) if bool((~small).any()) else 0.0
        print(f"{what} d{nm}: worst block rel L2 {worst:.3e} (bound {bound[nm]:.1e}), {int(small.sum())} of {small.numel()} blocks small")
        if bool((~small).any()):
            idx = int(torch.where(small, torch.zeros_like(rel), rel).argmax())
            b, h, j = idx // (rel.shape[1] * rel.shape[2]), idx // rel.shape[2] % rel.shape[1], idx % rel.shape[2]
            assert worst <= bound[nm], f"{what} d{nm}: image {b} head {h} block {j}: rel L2 {worst:.3e} > {bound[nm]:.1e}"
        if bool(small.any()):
            assert float(abs_rel[small].max()) <= bound[nm] * SMALL, f"{what} d{nm}: a small block is off by {float(abs_rel[small].max()):.3e} of the tensor"
    assert n_small <= MAX_SMALL_SHARE * n_all, f"{what}: {n_small} of {n_all} blocks are compared absolutely (> {MAX_SMALL_SHARE:.0%})"


# ------------------------------------------------------------------------------------------------------------------ the measurement (CPU)
def _randn(seed, *shape, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _grads(qkv, dout, B, N, H, size, dcls, policy, rounded):
    qf = qkv.double().requires_grad_(True)
    out, p = attention(qf, B, N, H, None if size is None else size.double(), None if policy is None else policy.double(), rounded)
    loss = (out * dout.double()).sum()
    if dcls is not None:
        loss = loss + (p[:, :, 0, :].mean(1) * dcls.double()).sum()
    loss.backward()
    return qf.grad


def _worst(cases):
    worst = {"q": 0.0, "k": 0.0, "v": 0.0}
    small = total = 0
    for qkv, dout, B, N, H, size, dcls, policy in cases:
        a = _grads(qkv, dout, B, N, H, size, dcls, policy, True)
        w = _grads(qkv, dout, B, N, H, size, dcls, policy, False)
        for nm, (rel, abs_rel, sm, _) in block_errors(a, w, B, N, H).items():
            rel = torch.where(abs_rel == 0, torch.zeros_like(rel), rel)
            if bool((~sm).any()):
                worst[nm] = max(worst[nm], float(rel[~sm].max()))
            small += int(sm.sum())
            total += sm.numel()
    return worst, small, total


def _size(B, N):
    size = (torch.rand(B, N, generator=torch.Generator().manual_seed(3)) * 3 + 1).floor()
    size[:, -1] = 0.0 if N > 20 else 1.0
    return size


def _bwd_cases(group):
    return [(_randn(20, B * N, 3 * H * 64, dtype=torch.bfloat16), _randn(21, B * N, H * 64, dtype=torch.bfloat16), B, N, H,
             _size(B, N) if bias else None, None, None) for B, N, H in SHAPES[group] for bias in (False, True)]


def _policy_cases(group):
    cases = []
    for B, N, H in SHAPES[group]:
        policy = (torch.rand(B, N, generator=torch.Generator().manual_seed(5)) > 0.4).float()
        policy[:, 0] = 1.0
        cases.append((_randn(40, B * N, 3 * H * 64, dtype=torch.bfloat16), _randn(41, B * N, H * 64, dtype=torch.bfloat16), B, N, H, None, None, policy))
    return cases


def _measure():
    print("test_attention_bwd:", _worst(_bwd_cases("bwd")))
    print("test_attention_bwd_blocks:", _worst(_bwd_cases("bwd_blocks")))
    B, N, H = 2, 139, 6
    dcls = _randn(24, B, N)
    dcls[:, 0] = 0
    print("test_attention_bwd_cls_gradient:", _worst([(_randn(22, B * N, 3 * H * 64, dtype=torch.bfloat16),
                                                       _randn(23, B * N, H * 64, scale=0.1, dtype=torch.bfloat16), B, N, H, None, dcls, None)]))
    cases = []
    for B, N, H in SHAPES["long"]:
        for bias in (False, True):
            dcls = _randn(32, B, N, scale=0.5)
            dcls[:, 0] = 0
            cases.append((_randn(30, B * N, 3 * H * 64, dtype=torch.bfloat16), _randn(31, B * N, H * 64, dtype=torch.bfloat16), B, N, H,
                          _size(B, N) if bias else None, dcls, None))
    print("test_attention_bwd_long:", _worst(cases))
    print("test_attention_policy_bwd:", _worst(_policy_cases("policy")))
    print("test_attention_policy_bwd_blocks:", _worst(_policy_cases("policy_blocks")))


if __name__ == "__main__":
    _measure()
