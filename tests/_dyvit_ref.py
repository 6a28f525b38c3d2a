"""Float64 restatements of the DyViT training pieces (dyvit.py:108-119, 221-224) that tests/test_hip_dyvit_train_ops.py holds the HIP
kernels against, and the comparison helpers those tests share.  tests/test_dyvit_train_ref.py pins these restatements on torch.autograd
over the oracle (oracle.dyvit_predictor_logprob / oracle.dyvit_train_forward), which tests/test_oracle_grad.py pins on the reference's
recorded gradients: reference -> oracle -> restatement -> kernel.

Every function takes and returns float64 CPU tensors; the callers feed the bf16-rounded operands the kernels see.  Where a kernel rounds
an intermediate to bf16 by design the restatement rounds at the same point (`rb`: oracle.round_bf16 with an identity gradient)."""
import torch

import oracle


class _RoundBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return oracle.round_bf16(t).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def rb(t):
    """oracle.round_bf16 (nearest even) with an identity gradient in the tensor's own precision.  (Differentiating through the cast
    itself would round the GRADIENT to bf16 as well: autograd hands a bf16 tensor a bf16 gradient.)"""
    return _RoundBf16.apply(t)


def bf16_ulp(want):
    """Spacing of bf16 at |want| (float64 tensor): 2^(floor(log2 |want|) - 7); the smallest normal's spacing at zero."""
    e = torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def bf16_ulp_excess(got, want, rows_dim=-1, nulp=1.0):
    """max over the elements of (|got - want| - tolerance) / tolerance-scale, <= 0 when `got` (bf16 values) is within `nulp` bf16 ulp of
    the float64 `want`.  The tolerance is nulp * ulp(want) + 2^-20 * max|want| over `rows_dim` (the row): the kernels evaluate in fp32
    and round once, so they are within half an ulp of their own fp32 value, and that value is within the fp32 evaluation error of the
    terms that cancel -- bounded by 2^-20 of the row's largest entry (sums of <= 600 fp32 terms: 600 * 2^-24 < 2^-14 relative to the terms,
    which the bf16 ulp of a result that is not itself cancelled covers; the floor is for the entries that are)."""
    got, want = got.double(), want.double()
    tol = nulp * bf16_ulp(want) + 2.0 ** -20 * want.abs().amax(dim=rows_dim, keepdim=True)
    return float(((got - want).abs() - tol).max())


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------ pool_policy
def pool_policy_ref(h, pol, eps=1e-6, precision="bf16", stored_glob=False, stored_value=None):
    """PredictorLG.forward dyvit.py:115-118 on rows [B,N,C] whose row 0 is the CLS token (not pooled; it receives the broadcast like every
    row): cat = [h[..., :C/2] | bf16(sum_p h[p, C/2:] pol[p] / sum_p pol[p] + eps)].  pol [B,N], entry 0 not read.
    stored_glob: the gradient wrt pol uses the STORED broadcast value in place of the unrounded mean, d glob / d pol_p =
    (h[p] - stored) / S, as tr_pool_policy_bwd documents (the value and the gradient wrt h are unchanged); stored_value [B,1,C/2]: that
    value when it is not this forward's own."""
    B, N, C = h.shape
    Ch = C // 2
    p = pol[:, 1:, None]
    S = p.sum(dim=1, keepdim=True)
    num = (h[:, 1:, Ch:] * p).sum(dim=1, keepdim=True)
    if stored_glob:
        st = (rb(num / S + eps) if precision == "bf16" else num / S + eps).detach() if stored_value is None else stored_value
        glob = (num - st * S) / S.detach() + st
    else:
        glob = num / S
    g = glob + eps
    g = rb(g) if precision == "bf16" else g
    return torch.cat([h[:, :, :Ch], g.expand(-1, N, -1)], dim=-1)


def pool_policy_bwd_ref(dcat, pre0, pol, eps=1e-6, stored_glob=True, round_h0=True, stored_value=None):
    """Gradients of sum(cat[:, 1:] * dcat[:, 1:]) (the CLS row takes no gradient) with cat = pool_policy_ref(h0, pol), h0 =
    bf16(gelu_erf(pre0)): -> (d h0 [B,N,C], d pol [B,N] with entry 0 zero, cat)."""
    h0 = oracle.gelu_erf(pre0)
    h0 = (rb(h0) if round_h0 else h0).detach().requires_grad_(True)
    p = pol.clone().requires_grad_(True)
    cat = pool_policy_ref(h0, p, eps, "bf16", stored_glob, stored_value)
    (cat[:, 1:] * dcat[:, 1:]).sum().backward()
    return h0.grad, p.grad, cat.detach()


# ------------------------------------------------------------------------------------------------------------ decide
def decide_ref(h2, w, b, gumbel, prev, forced_hard=None):
    """out_conv.4 + LogSoftmax + F.gumbel_softmax(hard=True)[..., 0:1] * prev_decision (dyvit.py:108-109, 223-224) on the patch rows.
    h2 [B,N,C] (row 0 = CLS, unused), w [2,C], b [2], gumbel [B,N-1,2], prev [B,N] -> dict of [B,N-1] tensors: keep (differentiable,
    straight-through), ysoft0, sm0 = softmax(z)_0, hard0 (first index on a tie, torch.max), margin = |t0 - t1|."""
    z = h2[:, 1:] @ w.t() + b
    s = torch.log_softmax(z, dim=-1)
    t = s + gumbel
    ysoft = torch.softmax(t, dim=-1)
    hard0 = (t[..., 0] >= t[..., 1]).to(z.dtype) if forced_hard is None else forced_hard.to(z.dtype)
    y0 = hard0.detach() - ysoft[..., 0].detach() + ysoft[..., 0]
    return {"keep": y0 * prev[:, 1:], "ysoft0": ysoft[..., 0], "sm0": torch.exp(s[..., 0]), "hard0": hard0.detach(),
            "margin": (t[..., 0] - t[..., 1]).abs().detach()}


def decide_bwd_ref(dkeep, h2, w, b, gumbel, prev, forced_hard=None):
    """Gradients of sum(keep * dkeep[:, 1:]): -> (d h2 [B,N,C] (CLS rows zero), d prev [B,N] (entry 0 zero), dW3 [2,C], db3 [2], fwd)."""
    h2 = h2.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    prev = prev.clone().requires_grad_(True)
    fwd = decide_ref(h2, w, b, gumbel, prev, forced_hard)
    (fwd["keep"] * dkeep[:, 1:]).sum().backward()
    return h2.grad, prev.grad, w.grad, b.grad, fwd


# ------------------------------------------------------------------------------------------------------------ a whole predictor stage (CPU link)
def predictor_stage_ref(x_sp, prev_sp, p, j, gumbel, forced_hard=None):
    """One stage of the training forward from the pieces above, without rounding points (x_sp [B,P,D] patch rows, prev_sp [B,P,1]):
    LayerNorm(1e-5) -> Linear + GELU -> pool_policy -> two Linear + GELU -> decide.  -> (log-probabilities [B,P,2], keep [B,P,1]); what
    oracle.dyvit_predictor_logprob and the straight-through step of oracle.dyvit_train_forward compute in fp32 precision."""
    pre = f"score_predictor.{j}."
    B, P, D = x_sp.shape
    h = torch.nn.functional.layer_norm(x_sp, (D,), p[pre + "in_conv.0.weight"], p[pre + "in_conv.0.bias"], 1e-5)
    h0 = oracle.gelu_erf(h @ p[pre + "in_conv.1.weight"].t() + p[pre + "in_conv.1.bias"])
    pad = lambda t: torch.cat([torch.zeros_like(t[:, :1]), t], dim=1)           # a CLS row in front: the kernels' [B,N,.] layout
    cat = pool_policy_ref(pad(h0), pad(prev_sp[..., 0]), 1e-6, "fp32")[:, 1:]
    h1 = oracle.gelu_erf(cat @ p[pre + "out_conv.0.weight"].t() + p[pre + "out_conv.0.bias"])
    h2 = oracle.gelu_erf(h1 @ p[pre + "out_conv.2.weight"].t() + p[pre + "out_conv.2.bias"])
    w3, b3 = p[pre + "out_conv.4.weight"], p[pre + "out_conv.4.bias"]
    fwd = decide_ref(pad(h2), w3, b3, gumbel, pad(prev_sp[..., 0]), forced_hard)
    return torch.log_softmax(h2 @ w3.t() + b3, dim=-1), fwd["keep"].unsqueeze(-1)
