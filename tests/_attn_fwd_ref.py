"""Per-block comparison of the forward attention kernels (tests/test_hip_attention_fwd_edges.py, the attention tests of tests/test_hip_ops.py)
and the CPU measurement its bounds come from: the forward counterpart of tests/_attn_bwd_ref.py.

The kernels are tiled by 16- or 32-row query blocks, so `out` is held per block of 16 queries and per (image, head), against the norm of the
unrounded float64 reference over the same slice.  The bound is measured from the reference alone: a float64 restatement that rounds where
the kernels round (csrc/tr_attention.hip: the unnormalised P to bf16 for P.V, the normaliser the sum of the UNrounded exponentials, the
output to bf16) against the unrounded one, per block, over the tests' own shapes, seeds and input kinds.  `python -m tests._attn_fwd_ref`
prints the worst block of every test group; the kernels are allowed MARGIN x that (their fp32 exp and summation order flip a rounding of P
here and there, which the emulation does not hold).  No block is exempt: a reference block below SMALL of the tensor's norm is a defect of
the case (change its seed), not a reason to compare absolutely.

Gaussian inputs cannot show a leaking key -- a padded or masked key then carries an average weight, one key among 197 -- so the builders
below also make inputs on which the softmax's invariance to a per-query shift turns such a leak into an error of the whole output."""
import functools

import numpy as np
import torch

import oracle

QB = 16                    # query rows per block of `out`
SMALL = 1e-3               # no reference block may be below this share of the tensor's norm
MARGIN = 1.5               # the kernels' allowance over the measured rounding noise
EPS = 1e-6                 # dyvit.py:39-51

# ---------------------------------------------------------------------------------------------------------------- the tests' token counts
NS_16Q = [1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 208, 209, 223, 224]   # every NP 1..7
NS_FLASH = [225, 255, 256, 257, 288, 289, 384, 385, 513, 577, 608, 609, 1025]      # B = 1, H = 2; 1025 at H = 1
NS_TWOPASS = [225, 256, 257, 385, 577, 608]
NS_POLICY32 = [2, 31, 32, 33, 64, 65, 96, 97, 128, 129, 161, 193, 224]            # every NKB 1..7 of the 32-query kernel
NS_POLICY_FLASH = [225, 257, 385, 577]
NS_CLS = [1, 16, 17, 32, 33, 224, 225, 256, 257, 1025]
NS_TWIN = [17, 33, 197, 224, 225, 257, 577]
KINDS = ("gaussian", "shift_neg", "shift_pos")


def shape_of(N):
    """(B, H) of a case: B = 2, H = 3 (a head stride that is no power of two) up to 224 tokens, B = 1, H = 2 beyond, H = 1 at 1025"""
    return (2, 3) if N <= 224 else (1, 1) if N >= 1025 else (1, 2)


# (B, N, H) per group: shared by the parametrize marks and by the measurement below
SHAPES = {"16q": [(*shape_of(N)[:1], N, shape_of(N)[1]) for N in NS_16Q],
          "flash": [(*shape_of(N)[:1], N, shape_of(N)[1]) for N in NS_FLASH],
          "twopass": [(*shape_of(N)[:1], N, shape_of(N)[1]) for N in NS_TWOPASS],
          "policy32": [(*shape_of(N)[:1], N, shape_of(N)[1]) for N in NS_POLICY32],
          "policy_flash": [(*shape_of(N)[:1], N, shape_of(N)[1]) for N in NS_POLICY_FLASH],
          # the attention tests of tests/test_hip_ops.py, on their own seeds
          "sweep": [(2, N, 2) for N in sorted(set(list(range(2, 225, 5)) + [31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161,
                                                                          191, 192, 193, 223, 224]))],
          "proportional": [(2, 197, 6), (2, 138, 2), (3, 98, 3), (1, 7, 1)],
          "key_mask": [(2, 197, 6), (3, 138, 2), (1, 40, 3)],
          "long": [(2, 577, 12), (1, 577, 3), (2, 225, 2), (1, 300, 1), (1, 608, 2)],
          "policy": [(2, 197, 6), (2, 138, 2), (1, 40, 3), (1, 224, 1), (2, 577, 2), (1, 257, 1)],
          "beyond": [(1, 785, 2), (2, 1025, 1)]}

# Worst block (relative L2 of `out` per 16 queries, image and head) of the rounded float64 restatement against the unrounded one, per test
# group, printed by `python -m tests._attn_fwd_ref` (CPU).  tests/test_attn_fwd_ref.py fails if the measurement gives more than these now.
# Worst ratio of a kernel's block to these, observed on an MI355X: 1.00 for the register-resident 16-query kernel, the 32-query policy kernel
# and the two-pass kernel (exp(s - max) is what they round, as the restatement does); 1.28 for the online-softmax kernel (785 tokens) and
# 0.78 for its policy form -- its reference point is ceil(max) in the log2 domain, so it rounds 2^frac x the restatement's P: another draw
# of the same noise.  MARGIN = 1.5 holds all of them.
MEASURED = {"16q": 2.82e-3, "flash": 2.84e-3, "twopass": 2.80e-3, "policy32": 5.48e-3, "policy_flash": 4.50e-3,
            "sweep": 2.63e-3, "proportional": 2.05e-3, "key_mask": 2.12e-3, "long": 2.65e-3, "policy": 2.55e-3, "beyond": 2.54e-3}


# ------------------------------------------------------------------------------------------------------------------------- input builders
def _seed(kind, N):
    return 1000 * (1 + ("gaussian", "shift_neg", "shift_pos", "masked_dominant", "policy_dominant").index(kind)) + N


def gaussian(B, N, H, seed):
    """qkv [B*N, 3*H*64] at scale 1.5, bf16-valued (the inputs of the older attention tests)"""
    g = torch.Generator().manual_seed(seed)
    return (1.5 * torch.randn(B * N, 3 * H * 64, generator=g)).bfloat16()


def _set63(qkv, B, N, H, q63, k63):
    """head dimension 63 of every q := q63, of every k := k63 (a number, or [B, N]): every logit moves by q63 * k63 / 8"""
    t = qkv.float().view(B, N, 3, H, 64).clone()
    t[:, :, 0, :, 63] = q63
    t[:, :, 1, :, 63] = k63 if not torch.is_tensor(k63) else k63[:, :, None].expand(B, N, H)
    return t.view(B * N, 3 * H * 64).bfloat16()


def shift_neg(B, N, H, seed):
    """gaussian with q63 = 10, k63 = -10: every real logit moves by exactly -12.5 and the true softmax does not, but a zero-filled padded
    key (logit 0) would carry e^12.5 times a real key's weight"""
    return _set63(gaussian(B, N, H, seed), B, N, H, 10.0, -10.0)


def shift_pos(B, N, H, seed):
    """q63 = k63 = 27: logits move by +91.125, which overflows fp32 exp unless the row maximum is subtracted before every exponentiation, in
    every key chunk"""
    return _set63(gaussian(B, N, H, seed), B, N, H, 27.0, 27.0)


def sizes(B, N, seed):
    """ToMe's token sizes 1..5 (tome.py:48-49), no key masked"""
    return torch.randint(1, 6, (B, N), generator=torch.Generator().manual_seed(seed + 7)).float()


def masked_dominant(B, N, H, seed):
    """-> (qkv, size).  shift_neg with zeros in `size` at key 1, at the middle key, at the last key and over the whole trailing third (whole
    trailing key blocks masked); the masked keys get k63 = +10, 25 above every real key, and must still weigh exactly nothing (ats.py:117-120
    masked_fill(-finfo.max); log 0 in the heuristic masks).  Key 0 stays; the other sizes are 1..5.  N >= 2."""
    assert N >= 2
    size = sizes(B, N, seed)
    size[:, 1] = 0
    size[:, N // 2] = 0
    size[:, N - 1] = 0
    size[:, N - N // 3:] = 0
    size[:, 0] = size[:, 0].clamp_min(1)
    assert bool((size[:, 0] > 0).all())
    k63 = torch.where(size == 0, torch.tensor(10.0), torch.tensor(-10.0))
    return _set63(gaussian(B, N, H, seed), B, N, H, 10.0, k63), size


def policy_dominant(B, N, H, seed):
    """-> (qkv, policy).  The same construction for the dropped keys of a DyViT keep policy: q63 = 8, k63 = -8 on the kept and +8 on the
    dropped keys (-+8 on the logits), so the kept keys' exponentials are e^-16 ~ 1e-7 of the dropped ones and the eps = 1e-6 smoothing of
    softmax_with_policy matters beside them.  policy[:, 0] = 1 (dyvit.py:226)."""
    policy = _policy(B, N, seed)
    k63 = torch.where(policy == 0, torch.tensor(8.0), torch.tensor(-8.0))
    return _set63(gaussian(B, N, H, seed), B, N, H, 8.0, k63), policy


def _policy(B, N, seed):
    policy = (torch.rand(B, N, generator=torch.Generator().manual_seed(seed + 11)) > 0.4).float()
    policy[:, N - 1] = 0.0                       # at least one dropped key, and the last one (a padded-key neighbour)
    policy[:, 0] = 1.0
    return policy


def policy_plain(B, N, H, seed):
    return gaussian(B, N, H, seed), _policy(B, N, seed)


def build(kind, B, N, H, bias=False):
    """-> (qkv bf16, size [B,N] | None) of one case of the plain / bias / column-sum tests"""
    if kind == "masked_dominant":
        return masked_dominant(B, N, H, _seed(kind, N))
    qkv = {"gaussian": gaussian, "shift_neg": shift_neg, "shift_pos": shift_pos}[kind](B, N, H, _seed(kind, N))
    return qkv, (sizes(B, N, _seed(kind, N)) if bias else None)


def build_policy(kind, B, N, H):
    return (policy_dominant if kind == "policy_dominant" else policy_plain)(B, N, H, _seed("policy_dominant", N))


# ------------------------------------------------------------------------------------------------------------------------------ reference
FAULTS = ("pad_key", "masked_leak", "drop_last")


def attention(qkv, B, N, H, size=None, policy=None, rounded=False, fault=None):
    """softmax(q k^T / 8 [+ log size]) v, or DyViT's softmax_with_policy (policy [B,N]), in float64
    -> (out [B*N, H*64], CLS rows attn[:, :, 0, :] [B,H,N], column sums sum_h sum_q attn [B,N]).
    rounded: the kernels' rounding points -- the unnormalised P = exp(s - max) to bf16 for P.V, the normaliser the sum of the unrounded P,
    the output to bf16; with a policy, P = exp(s - max) * pol + eps / N up to 224 tokens, and beyond (online softmax) exp(s - max) * pol with
    eps / N * sum_k v_k added unrounded.  The side outputs are fp32 in the kernels: never rounded here.
    fault (tests/test_attn_fwd_ref.py): "pad_key" one zero-logit key with a zero value row joins the softmax; "masked_leak" the middle masked
    key gets the weight it would have unmasked; "drop_last" the last key is left out."""
    q, k, v = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    size = None if size is None else size.double()
    if fault == "drop_last":
        k, v = k[:, :, :-1], v[:, :, :-1]
        size = None if size is None else size[:, :-1]
    if fault == "pad_key":
        k, v = (torch.cat([t, torch.zeros(B, H, 1, 64, dtype=torch.float64)], 2) for t in (k, v))
        size = None if size is None else torch.cat([size, torch.ones(B, 1, dtype=torch.float64)], 1)
    if fault == "masked_leak":
        size = size.clone()
        assert bool((size[:, N // 2] == 0).all())
        size[:, N // 2] = 1
    s = (q @ k.transpose(-1, -2)) * 0.125
    if policy is not None:
        assert fault is None
        pol = policy.double()[:, None, None, :]
        pol = pol + (1 - pol) * torch.eye(N, dtype=torch.float64)
        e = (s - s.amax(-1, keepdim=True)).exp() * pol
        den = e.sum(-1, keepdim=True) + EPS
        if not rounded:
            # the oracle's restatement (its exp is fp32: 6e-8); the float64 form above is proven against it in tests/test_attn_fwd_ref.py
            p = oracle.dyvit_softmax_with_policy(s, policy.double().unsqueeze(-1))
            o = p @ v
        elif N <= 224:
            p = (e + EPS / N) / den
            o = (oracle.round_bf16((e + EPS / N).float()).double() @ v) / den
        else:
            p = (e + EPS / N) / den
            o = (oracle.round_bf16(e.float()).double() @ v + EPS / N * v.sum(2, keepdim=True)) / den
    else:
        if size is not None:
            s = s + size.log()[:, None, None, :]
        e = (s - s.amax(-1, keepdim=True)).exp()
        den = e.sum(-1, keepdim=True)
        p = e / den
        o = ((oracle.round_bf16(e.float()).double() if rounded else e) @ v) / den
    p = p[..., :N]
    if fault == "drop_last":
        p = torch.cat([p, torch.zeros(B, H, N, 1, dtype=torch.float64)], -1)
    out = o.transpose(1, 2).reshape(B * N, H * 64)
    if rounded:
        out = oracle.round_bf16(out.float()).double()
    return out, p[:, :, 0, :], p.sum(dim=(1, 2))


@functools.lru_cache(maxsize=None)
def case(kind, B, N, H, bias=False):
    """One case of the plain / bias / column-sum tests with its unrounded reference, computed once: (qkv, size, out, cls, colsum)"""
    qkv, size = build(kind, B, N, H, bias)
    return (qkv, size) + attention(qkv, B, N, H, size)


@functools.lru_cache(maxsize=None)
def policy_case(kind, B, N, H):
    qkv, policy = build_policy(kind, B, N, H)
    return qkv, policy, attention(qkv, B, N, H, policy=policy)[0]


# -------------------------------------------------------------------------------------------------------------------- per-block comparison
def block_errors(got, want, B, N, H):
    """got, want: out [B*N, H*64] -> (rel [B,H,nb], share [B,H,nb]): per block of QB queries, image and head, the error's norm over the
    reference's norm of the same slice, and the reference's norm of the slice over the whole tensor's"""
    nb = (N + QB - 1) // QB
    g, w = (torch.nn.functional.pad(t.detach().double().cpu().view(B, N, H, 64).permute(0, 2, 1, 3), (0, 0, 0, nb * QB - N))
            .reshape(B, H, nb, QB * 64) for t in (got, want))
    err, ref = (g - w).norm(dim=-1), w.norm(dim=-1)
    return err / ref.clamp_min(1e-300), ref / want.detach().double().norm().clamp_min(1e-300)


def worst_block(got, want, B, N, H):
    """-> (worst relative L2, (image, head, block)); every reference block must carry at least SMALL of the tensor's norm"""
    rel, share = block_errors(got, want, B, N, H)
    assert float(share.min()) >= SMALL, f"a reference block holds {float(share.min()):.1e} of the tensor's norm: change the case's seed"
    idx = int(rel.argmax())
    return float(rel.max()), (idx // (rel.shape[1] * rel.shape[2]), idx // rel.shape[2] % rel.shape[1], idx % rel.shape[2])


def assert_blocks(got, want, B, N, H, measured, what="", margin=MARGIN, log=None):
    """Every block of `out` within margin x measured of the reference's block (relative L2).  Prints the worst block and its ratio to the
    measured rounding noise before it asserts; `log` (a list) collects the ratios."""
    assert not bool(got.float().isnan().any()) and bool(got.float().isfinite().all()), f"{what}: out has a NaN or an infinity"
    worst, (b, h, j) = worst_block(got, want, B, N, H)
    print(f"{what} B={B} N={N} H={H}: worst block rel L2 {worst:.3e} (image {b} head {h} block {j}), bound {margin * measured:.2e} = "
          f"{margin} x {measured:.2e}, ratio to measured {worst / measured:.2f}")
    if log is not None:
        log.append(worst / measured)
    assert worst <= margin * measured, f"{what} N={N}: image {b} head {h} block {j}: rel L2 {worst:.3e} > {margin * measured:.2e}"


# ------------------------------------------------------------------------------------------------------------------ the measurement (CPU)
def _np_randn(rng, *shape, scale=1.0):
    return oracle.round_bf16(torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)))


def ops_cases(group):
    """The inputs of the attention tests of tests/test_hip_ops.py, drawn as they draw them: yields (qkv fp32 bf16-valued, B, N, H, size, policy)"""
    if group == "sweep":
        rng = np.random.default_rng(123)
        for B, N, H in SHAPES[group]:
            yield _np_randn(rng, B * N, 3 * H * 64, scale=1.2), B, N, H, None, None
        return
    for B, N, H in SHAPES[group]:
        rng = np.random.default_rng({"proportional": 70 + N, "key_mask": 800 + N, "long": 5000 + N + H, "policy": 9000 + N, "beyond": 5100 + N}[group])
        qkv = _np_randn(rng, B * N, 3 * H * 64, scale=1.5)
        if group == "proportional":
            yield qkv, B, N, H, torch.from_numpy(rng.integers(1, 6, size=(B, N)).astype(np.float32)), None
        elif group == "key_mask":
            mask = torch.ones(B, N)
            for b in range(B):
                mask[b, N - 1 - rng.integers(3, N // 2):] = 0
            yield qkv, B, N, H, mask, None
        elif group == "long":
            size = torch.from_numpy(rng.integers(1, 5, size=(B, N)).astype(np.float32))
            size[:, N - 7:] = 0
            size[:, 0] = 1
            tail = size.clone()
            tail[:, N // 2:] = 0
            for sz in (None, size, tail):
                yield qkv, B, N, H, sz, None
        elif group == "policy":
            policy = torch.from_numpy((rng.random((B, N)) > 0.4).astype(np.float32))
            policy[:, 0] = 1.0
            yield qkv, B, N, H, None, policy
        else:
            yield qkv, B, N, H, None, None


def group_cases(group):
    """yields (qkv, B, N, H, size, policy) of one test group of tests/test_hip_attention_fwd_edges.py"""
    for B, N, H in SHAPES[group]:
        if group in ("policy32", "policy_flash"):
            for kind in ("gaussian", "policy_dominant"):
                qkv, policy = build_policy(kind, B, N, H)
                yield qkv, B, N, H, None, policy
            continue
        for kind in KINDS:
            for bias in ((True,) if group == "twopass" else (False, True)):
                qkv, size = build(kind, B, N, H, bias)
                yield qkv, B, N, H, size, None
        if N >= 2:
            qkv, size = build("masked_dominant", B, N, H)
            yield qkv, B, N, H, size, None


def measure(group):
    """worst block of the rounded restatement against the unrounded one over a group's cases"""
    worst = 0.0
    for qkv, B, N, H, size, policy in (group_cases(group) if group in ("16q", "flash", "twopass", "policy32", "policy_flash") else ops_cases(group)):
        a = attention(qkv, B, N, H, size, policy, rounded=True)[0]
        w = attention(qkv, B, N, H, size, policy)[0]
        worst = max(worst, worst_block(a, w, B, N, H)[0])
    return worst


def fault_margins(kind, fault, ns):
    """-> {N: worst block of the faulty unrounded reference against the sound one}, on the designed input `kind`"""
    res = {}
    for N in ns:
        B, H = shape_of(N)
        qkv, size = build(kind, B, N, H)
        res[N] = worst_block(attention(qkv, B, N, H, size, fault=fault)[0], attention(qkv, B, N, H, size)[0], B, N, H)[0]
    return res


FAULT_INPUT = {"pad_key": "shift_neg", "masked_leak": "masked_dominant", "drop_last": "shift_neg"}


def _measure():
    for group in SHAPES:
        m = measure(group)
        print(f"{group}: measured {m:.3e}, committed {MEASURED.get(group, float('nan')):.3e}")
    bound = MARGIN * max(MEASURED[g] for g in ("16q", "flash", "twopass")) if MEASURED else float("nan")
    for fault in FAULTS:
        res = fault_margins(FAULT_INPUT[fault], fault, [N for N in sorted(set(NS_16Q + NS_FLASH)) if N >= 2 or fault == "pad_key"])
        N, low = min(res.items(), key=lambda kv: kv[1])
        print(f"fault {fault} on {FAULT_INPUT[fault]}: smallest worst-block error {low:.3e} at N = {N}: {low / bound:.1f} x the bound {bound:.2e}")


if __name__ == "__main__":
    _measure()
