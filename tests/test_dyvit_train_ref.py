"""CPU link of the chain reference -> oracle -> restatement -> kernel: the float64 restatements in tests/_dyvit_ref.py, which the GPU tests
of the DyViT training kernels trust, agree with torch.autograd over the oracle (oracle.dyvit_predictor_logprob and the straight-through
step of oracle.dyvit_train_forward) in fp32 precision, values and gradients, to 1e-5 relative.  tests/test_oracle_grad.py pins that
oracle on the reference's recorded gradients."""
import torch

import oracle
from tests import _dyvit_ref as R
from tests._params import case_params, make_images

CASE = dict(family="dyvit", embed_dim=64, depth=1, num_heads=1, num_classes=8, img_size=64, keep_rate=[0.7], reduction_loc=[0], batch=3,
            wseed=31, xseed=32, qkv_gain=1.0)
TOL = 1e-5


def _leaves(params, dtype):
    return {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}


def _close(got, want, what):
    r = R.rel_l2(got, want)
    assert r <= TOL, f"{what}: relative L2 {r:.3e} > {TOL}"


def test_predictor_logprob_and_its_gradients_match_the_oracle():
    """Random 0/1 policy and a fractional one: log-probabilities, d x, d policy and every predictor parameter's gradient."""
    cfg, params = case_params(CASE)
    B, P, D = 3, cfg.num_patches, cfg.embed_dim
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, P, D, generator=g)
    dscore = torch.randn(B, P, 2, generator=g)
    for kind in ("binary", "fractional"):
        pol = (torch.rand(B, P, 1, generator=g) < 0.6).float() if kind == "binary" else torch.rand(B, P, 1, generator=g) + 0.05
        pol[:, 0] = 1.0
        lo, xo, po = _leaves(params, torch.float32), x.clone().requires_grad_(True), pol.clone().requires_grad_(True)
        so = oracle.dyvit_predictor_logprob(xo, po, lo, 0, "fp32")
        (so * dscore).sum().backward()
        lr, xr, pr = _leaves(params, torch.float64), x.double().requires_grad_(True), pol.double().requires_grad_(True)
        sr, _ = R.predictor_stage_ref(xr, pr, lr, 0, torch.zeros(B, P, 2, dtype=torch.float64))
        (sr * dscore.double()).sum().backward()
        _close(sr, so, f"{kind}: log-probabilities")
        _close(xr.grad, xo.grad, f"{kind}: d x")
        _close(pr.grad, po.grad, f"{kind}: d policy")
        for k in lo:
            if k.startswith("score_predictor.0."):
                _close(lr[k].grad, lo[k].grad, f"{kind}: d {k}")


def test_straight_through_step_matches_the_oracle_train_forward():
    """The first stage's keep decision (out_pred_prob[0] of oracle.dyvit_train_forward: embedding -> predictor -> Gumbel straight-through)
    and its gradients wrt the predictor's parameters, against the restatement fed the same embedded tokens and the same noise."""
    cfg, params = case_params(CASE)
    B, P = CASE["batch"], cfg.num_patches
    x = make_images(B, CASE["img_size"], CASE["xseed"])
    g = torch.Generator().manual_seed(9)
    gumbel = -torch.empty(B, P, 2).exponential_(generator=g).log()
    dkeep = torch.randn(B, P, generator=g)
    lo = _leaves(params, torch.float32)
    out_pred = oracle.dyvit_train_forward(lo, x, cfg, {0: gumbel}, "fp32")[3]
    (out_pred[0] * dkeep).sum().backward()
    lr = _leaves(params, torch.float64)
    tok = oracle.embed_tokens(oracle.patch_embed(x.double(), lr["patch_embed.proj.weight"], lr["patch_embed.proj.bias"], cfg.patch_size, "fp32"),
                              lr["cls_token"], lr["pos_embed"])
    _, keep = R.predictor_stage_ref(tok[:, 1:], torch.ones(B, P, 1, dtype=torch.float64), lr, 0, gumbel.double())
    (keep[..., 0] * dkeep.double()).sum().backward()
    assert torch.equal(keep[..., 0].detach().float(), out_pred[0].detach()), "hard decisions differ"
    assert 0 < float(keep.detach().sum()) < B * P, "degenerate decisions: the case does not exercise both branches"
    for k in lo:
        if k.startswith("score_predictor.0.") or k.startswith("patch_embed"):
            _close(lr[k].grad, lo[k].grad, f"d {k}")


def test_pool_policy_gradient_with_the_stored_broadcast_value():
    """pool_policy_bwd_ref's `stored_glob` form (what tr_pool_policy_bwd computes) differs from plain autograd ONLY in d policy, and there by
    the substitution of bf16(glob + eps) for glob: d h0 identical, d policy equal to the closed form sum_c G_c (h0[p,c] - stored_c) / S."""
    B, N, C = 2, 23, 48
    g = torch.Generator().manual_seed(3)
    pre0 = torch.randn(B, N, C, generator=g).bfloat16().double()
    dcat = torch.randn(B, N, C, generator=g).bfloat16().double()
    pol = (torch.rand(B, N, generator=g) < 0.6).double()
    pol[:, 1] = 1.0
    dh_s, dp_s, cat = R.pool_policy_bwd_ref(dcat, pre0, pol, stored_glob=True)
    dh_p, dp_p, cat_p = R.pool_policy_bwd_ref(dcat, pre0, pol, stored_glob=False)
    assert torch.equal(dh_s, dh_p) and torch.equal(cat, cat_p)
    h0 = R.rb(oracle.gelu_erf(pre0))
    G = dcat[:, 1:, C // 2:].sum(1)
    S = pol[:, 1:].sum(1, keepdim=True)
    want = ((h0[:, 1:, C // 2:] - cat[:, 1:2, C // 2:]) * G[:, None, :]).sum(-1) / S
    _close(dp_s[:, 1:], want, "d policy, stored form")
    assert float(dp_s[:, 0].abs().max()) == 0.0 and float(dh_s[:, 0].abs().max()) == 0.0
    assert 1e-5 < R.rel_l2(dp_s, dp_p) < 1e-2          # the two forms differ by the bf16 rounding of the broadcast value
