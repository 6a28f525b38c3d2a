"""Reference arithmetic of the average-pooled head (global_pool='avg'): plain torch on the CPU, fp64 unless said otherwise.

    v_n   = (x_n + d_attn_n) + d_mlp_n          n = 1 .. N-1: the stream after the last block (row 0, the CLS token, is left out)
    pool  = sum_n w_n v_n / sum_n w_n           0 where the weights sum to 0
    feat  = LayerNorm(pool; norm.weight, norm.bias, eps)      pool first, then norm (timm's fc_norm)
    out   = head(feat), or feat itself for a headless model

Op level: pool() / pool_bound() / pool_bwd().  Model level: final_stream() composes the block functions oracle/ exports (block_forward,
tome_block_forward, ats_block_forward) into the stream after the last block and the pool's weights -- ToMe's token sizes, the ATS padding
mask, None (ones) for every other family -- and pooled_logits() puts the head on it.  With precision="bf16" and the device's decisions
forced, the same composition is the differentiable fp32 restatement of the training step (autograd_step), the way tests/_input_grad_ref.py
restates the CLS head's."""
import torch

from oracle import vit as ovit
from oracle.ats import ats_block_forward, ats_sample_counts


# ------------------------------------------------------------------------------------------------------------------------- op level
def stream(x, d1=None, d2=None):
    """(x + d1) + d2 in fp64 from the operands as stored (bf16 / fp32 values are exact in fp64)."""
    v = x.double()
    if d1 is not None:
        v = v + d1.double()
    if d2 is not None:
        v = v + d2.double()
    return v


def pool(v, w=None):
    """[B, D] fp64: the weighted mean of rows 1 .. N-1 of v [B, N, D]; w [B, N] or None (ones); an image without weight pools to 0."""
    v = v.double()
    w = torch.ones(v.shape[:2], dtype=torch.float64) if w is None else w.double()
    num = (w[:, 1:, None] * v[:, 1:]).sum(1)
    den = w[:, 1:].sum(1, keepdim=True)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num))


def pool_bound(v, w=None):
    """[B, D] fp64: (N + 4) * 2^-24 * (sum_n w_n |v_n| / sum_n w_n), the per-element error bound of an fp32 pool over N - 1 rows: N - 2
    additions of the sum, the two additions behind v, the product and the division, each at most half an ulp of a partial result that
    sum_n w_n |v_n| bounds."""
    N = v.shape[1]
    return (N + 4) * 2.0 ** -24 * pool(v.double().abs(), w)


def pool_bwd(gpool, N, w=None):
    """[B, N, D] fp64: the gradient of pool() with respect to v for the upstream gradient gpool [B, D]; row 0 is zero."""
    B, D = gpool.shape
    w = torch.ones(B, N, dtype=torch.float64) if w is None else w.double()
    den = w[:, 1:].sum(1, keepdim=True)
    coef = torch.where(den > 0, w / den.clamp_min(1e-300), torch.zeros_like(w))
    coef[:, 0] = 0
    return coef[:, :, None] * gpool.double()[:, None, :]


def norm_head(pooled, params, eps, headless=False):
    """fp64: LayerNorm(pooled) and, unless headless, the classifier on it."""
    p = {k: params[k].double() for k in ("norm.weight", "norm.bias")}
    feat = torch.nn.functional.layer_norm(pooled.double(), (pooled.shape[-1],), p["norm.weight"], p["norm.bias"], eps)
    if headless:
        return feat
    return feat @ params["head.weight"].double().t() + params["head.bias"].double()


# ---------------------------------------------------------------------------------------------------------------------- model level
def final_stream(params, x, cfg, precision="fp32", forced=None):
    """(h [B, N_last, D], w [B, N_last] or None, decisions {blk: ...}) of the oracle's blocks on image x: the stream after the last block, the
    pool's weights and what every reducing block decided (Top-K: idx; ToMe: the Assignment_Maps entry; ATS: ids [B, K] with the CLS id 0
    first, 0 = padding, padded to the static bound like the executor).  forced: the decisions to use instead, in the form
    training.train_decisions gives them.  Differentiable when called under torch.enable_grad()."""
    p = params
    tok = ovit.patch_embed(x, p["patch_embed.proj.weight"], p["patch_embed.proj.bias"], cfg.patch_size, precision)
    h = ovit.embed_tokens(tok, p["cls_token"], p["pos_embed"])
    forced = forced or {}
    dec, w = {}, None
    fam = cfg.family
    if fam in ("deit", "topk", "evit"):
        keeps = ovit.stage_keep_counts(cfg) if fam != "deit" else {}
        for i in range(cfg.depth):
            h, idx, _ = ovit.block_forward(h, p, i, cfg, keeps.get(i), precision, forced.get(i))
            if idx is not None:
                dec[i] = idx
    elif fam == "tome":
        sched, size = ovit.tome_schedule(cfg), None
        for i in range(cfg.depth):
            h, size, assign = ovit.tome_block_forward(h, size, p, i, cfg, sched.get(i, 0), precision, forced.get(i))
            if assign is not None:
                dec[i] = assign
        w = None if size is None else size[..., 0]
    elif fam == "ats":
        counts = ats_sample_counts(cfg)
        mask = torch.ones(h.shape[0], h.shape[1], dtype=torch.bool)
        for i in range(cfg.depth):
            h, mask, ids, _ = ats_block_forward(h, mask, p, i, cfg, counts.get(i, 0), precision, True, forced.get(i))
            if ids is not None:
                dec[i] = ids
        w = mask.to(h.dtype) if dec else None
    else:
        raise ValueError(f"no block composition for family {fam!r}")
    return h, w, dec


def pooled_logits(params, x, cfg, headless=False):
    """fp64 head on the oracle's fp32 stream (the reference's arithmetic for the blocks, the issue's semantics above it):
    (out [B, C] or [B, D], decisions)."""
    with torch.no_grad():
        h, w, dec = final_stream(params, x, cfg)
    return norm_head(pool(h, w), params, cfg.ln_eps, headless), dec


def autograd_step(params, x, cfg, labels, forced=None, headless_grad=None):
    """One training step of the pooled model restated in fp32 torch with the HIP rounding points (precision="bf16": round_bf16 is
    autograd-transparent) on the given decisions: (loss, logits, {name: parameter gradient}, dx).  The pool's weights carry no gradient.
    headless_grad [B, D]: the model is headless; the features are the output and this is their upstream gradient."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    img = x.detach().to(torch.float32).clone().requires_grad_(True)
    with torch.enable_grad():
        h, w, _ = final_stream(leaves, img, cfg, "bf16", forced)
        w = torch.ones(h.shape[:2]) if w is None else w.detach().to(torch.float32)
        pooled = (w[:, 1:, None] * h[:, 1:]).sum(1) / w[:, 1:].sum(1, keepdim=True)
        if headless_grad is not None:
            out = torch.nn.functional.layer_norm(pooled, (pooled.shape[-1],), leaves["norm.weight"], leaves["norm.bias"], cfg.ln_eps)
            loss = (out * headless_grad).sum()
        else:
            feat = ovit.layer_norm(pooled, leaves["norm.weight"], leaves["norm.bias"], cfg.ln_eps, "bf16")
            out = feat @ ovit.round_bf16(leaves["head.weight"]).t() + leaves["head.bias"]
            loss = torch.nn.functional.cross_entropy(out, labels)
        loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return loss.item(), out.detach(), grads, img.grad.detach()
