"""The float64 forward-attention reference of tests/_attn_fwd_ref.py, its input builders and its committed measurement (no GPU): the
reference against torch's scaled_dot_product_attention in float64, the shift invariance the designed inputs rest on, the policy form
against the oracle's softmax_with_policy, three injected faults that the GPU tests' per-block bound must catch with a factor of ten to
spare at every token count of their lists, and the committed constants against what the measurement gives now.  This proves the reference
and the bound before tests/test_hip_attention_fwd_edges.py compares the kernels with them."""
import pytest
import torch

import oracle
from tests import _attn_fwd_ref as R

F64 = torch.float64
NS = sorted(set(R.NS_16Q + R.NS_FLASH))
MAX_MARGIN = 2.0                 # the most the kernels' allowance over the measured noise may ever be raised to


def _sdpa(qkv, B, N, H, size):
    q, k, v = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    mask = None if size is None else size.double().log()[:, None, None, :].expand(B, H, N, N)
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    return o.transpose(1, 2).reshape(B * N, H * 64)


@pytest.mark.parametrize("N", [1, 2, 17, 33, 97, 197, 224, 225, 257, 577])
def test_reference_equals_sdpa_and_ignores_the_shift(N):
    B, H = R.shape_of(N)
    for kind in ("gaussian", "shift_neg", "shift_pos") + (("masked_dominant",) if N >= 2 else ()):
        for bias in (False, True):
            qkv, size = R.build(kind, B, N, H, bias)
            assert qkv.dtype == torch.bfloat16 and qkv.shape == (B * N, 3 * H * 64)
            out, cls, colsum = R.attention(qkv, B, N, H, size)
            assert out.dtype == F64 and cls.shape == (B, H, N) and colsum.shape == (B, N)
            assert float((out - _sdpa(qkv, B, N, H, size)).abs().max()) <= 1e-12, kind
            assert float((cls.sum(-1) - 1).abs().max()) <= 1e-12 and float((colsum.sum(-1) - H * N).abs().max()) <= 1e-9
            if size is not None:
                assert bool((cls[(size == 0)[:, None, :].expand(B, H, N)] == 0).all()) and bool((colsum[size == 0] == 0).all())
            if kind in ("shift_neg", "shift_pos"):
                # the same keys and values with q63 = 0: every logit of a query lies lower (higher) by exactly the shift, the softmax is the same
                t = qkv.float().view(B, N, 3, H, 64).clone()
                shift = float(t[0, 0, 0, 0, 63] * t[0, 0, 1, 0, 63]) / 8
                assert shift == (-12.5 if kind == "shift_neg" else 91.125)
                t[:, :, 0, :, 63] = 0
                flat, cls0, _ = R.attention(t.view(B * N, 3 * H * 64), B, N, H, size)
                assert float((out - flat).abs().max()) <= 1e-10 and float((cls - cls0).abs().max()) <= 1e-10


@pytest.mark.parametrize("N", [2, 33, 97, 224, 225, 385])
def test_masked_dominant_builder(N):
    B, H = R.shape_of(N)
    qkv, size = R.build("masked_dominant", B, N, H)
    masked = size == 0
    assert bool(masked[:, 1].all() and masked[:, N // 2].all() and masked[:, N - 1].all() and masked[:, N - N // 3:].all())
    assert not bool(masked[:, 0].any()) and bool((~masked).any(1).all())
    if N >= 97:
        assert N // 3 >= 32 and not bool(masked[:, 2:N // 2].any())          # whole trailing key blocks, and real keys between the single ones
    q, k, _ = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    part = q[..., 63:] @ k[..., 63:].transpose(-1, -2) * 0.125
    assert bool((part[masked[:, None, None, :].expand(B, H, N, N)] == 12.5).all()) and bool((part[~masked[:, None, None, :].expand(B, H, N, N)] == -12.5).all())


@pytest.mark.parametrize("N", [2, 33, 161, 224, 225, 577])
def test_policy_reference_is_the_oracles(N):
    B, H = R.shape_of(N)
    for kind in ("gaussian", "policy_dominant"):
        qkv, policy = R.build_policy(kind, B, N, H)
        assert bool((policy[:, 0] == 1).all()) and 0 < float(policy.mean()) < 1
        q, k, v = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        s = q @ k.transpose(-1, -2) * 0.125
        want = (oracle.dyvit_softmax_with_policy(s, policy.double().unsqueeze(-1)) @ v).transpose(1, 2).reshape(B * N, H * 64)
        out, cls, _ = R.attention(qkv, B, N, H, policy=policy)
        assert torch.equal(out, want)
        # the float64 restatement that carries the rounding points, unrounded: the oracle's exp is fp32
        pol = policy.double()[:, None, None, :] + (1 - policy.double()[:, None, None, :]) * torch.eye(N, dtype=F64)
        e = (s - s.amax(-1, keepdim=True)).exp() * pol
        mine = (((e + R.EPS / N) / (e.sum(-1, keepdim=True) + R.EPS)) @ v).transpose(1, 2).reshape(B * N, H * 64)
        assert R.worst_block(mine, want, B, N, H)[0] <= 1e-6               # 2^-24 = 6e-8 per weight
        if kind == "policy_dominant" and N >= 33:
            # a kept query's kept keys weigh about as much as the eps smoothing: both matter
            kept_sum = (e * policy.double()[:, None, None, :])[policy.bool()[:, None, :, None].expand(B, H, N, 1).squeeze(-1)].sum(-1)
            assert 1e-9 < float(kept_sum.median()) < 1e-4


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_faults_exceed_the_bound_tenfold(fault):
    """at EVERY token count of the register-resident and online-softmax lists, on the designed input"""
    ns = [N for N in NS if N >= 2 or fault == "pad_key"]
    res = R.fault_margins(R.FAULT_INPUT[fault], fault, ns)
    for N, err in res.items():
        bound = MAX_MARGIN * R.MEASURED["16q" if N <= 224 else "flash" if N not in R.NS_TWOPASS else "twopass"]
        print(f"{fault} N={N}: worst block {err:.3e} = {err / bound:.0f} x the bound")
        assert err >= 10 * bound, (fault, N, err, bound)


def test_a_leak_hides_in_gaussian_inputs():
    """why the designed inputs: the same zero-logit key on gaussian inputs stays inside the old whole-tensor tolerance of 3e-2 at 197 tokens"""
    B, H, N = 2, 3, 197
    qkv, _ = R.build("gaussian", B, N, H)
    bad, good = R.attention(qkv, B, N, H, fault="pad_key")[0], R.attention(qkv, B, N, H)[0]
    assert float((bad - good).abs().max()) < 3e-2


@pytest.mark.parametrize("group", list(R.SHAPES))
def test_committed_constants_hold(group):
    m = R.measure(group)
    print(f"{group}: measured {m:.3e}, committed {R.MEASURED[group]:.3e}")
    assert m <= R.MEASURED[group], f"{group}: the measurement gives {m:.3e}, more than the committed {R.MEASURED[group]:.3e}"
    assert R.MEASURED[group] <= 1.02 * m, f"{group}: the committed {R.MEASURED[group]:.3e} is more than the rounded-up measurement {m:.3e}"


def test_tables_cover_every_kernel_variant():
    assert {(N + 31) // 32 for N in R.NS_16Q} == set(range(1, 8)) and {(N + 31) // 32 for N in R.NS_POLICY32} == set(range(1, 8))
    assert max(R.NS_16Q) == 224 and min(R.NS_FLASH) == 225 and max(R.NS_TWOPASS) == 608 and 609 in R.NS_FLASH
    assert set(R.MEASURED) == set(R.SHAPES) and R.MARGIN <= MAX_MARGIN
    for N in R.NS_16Q:
        assert R.shape_of(N) == (2, 3)
