"""Reference of the multi-level dense feature maps in training (model.forward_dense_train(x, blocks=...)): plain torch / numpy on the CPU.

streams_after_blocks() composes the block and stage functions oracle/ exports into the stream after EVERY block, the way
tests/_pool_ref.final_stream does for five families, for the ten families of tests/test_dense_train_gpu.py::CASES; its last stream and the
logits on it are the oracle's own *_forward(..., return_viz=True) output bit for bit (tests/test_dense_train_levels_ref.py), which pins the
composition on the oracle.  Under torch.enable_grad(), with precision="bf16" (round_bf16 is autograd-transparent) and the device's decisions
forced, it is the differentiable restatement of the training forward whose gradients the GPU tier compares with.
level_maps() puts levels on the grid by given indices; dense_scatter_levels() is tests/_dense_train_ref.dense_scatter per level."""
import numpy as np
import torch

import oracle
from oracle import vit as ovit
from tests import _dense_train_ref as tref

FAMILIES = ("deit", "topk", "evit", "tome", "ats", "dpcknn", "kmedoids", "sit", "patchmerger", "sinkhorn")


def streams_after_blocks(params, x, cfg, precision="fp32", forced=None, noise=None):
    """[h_0, ..., h_{depth-1}]: h_i [B, N_i, D] is the stream after block i (every residual added) of the oracle's blocks and stages on image
    x.  forced {blk: decision} in the form training.train_decisions gives them (Top-K / EViT: idx; ToMe: (unm, src, dst); ATS: ids; DPC-KNN:
    (centres, assignment); K-Medoids: medoid ids); noise: DPC-KNN's density draws {blk: [B, P_in]}.  The soft families take no decisions.
    Differentiable under torch.enable_grad(); the discrete decisions carry no gradient, as in the oracle."""
    p, fam = params, cfg.family
    assert fam in FAMILIES, fam
    forced = forced or {}
    tok = ovit.patch_embed(x, p["patch_embed.proj.weight"], p["patch_embed.proj.bias"], cfg.patch_size, precision)
    h = ovit.embed_tokens(tok, p["cls_token"], p["pos_embed"])
    out = []
    if fam in ("deit", "topk", "evit"):
        keeps = ovit.stage_keep_counts(cfg) if fam != "deit" else {}
        for i in range(cfg.depth):
            h, _, _ = ovit.block_forward(h, p, i, cfg, keeps.get(i), precision, forced.get(i))
            out.append(h)
    elif fam == "tome":
        sched, size = ovit.tome_schedule(cfg), None
        for i in range(cfg.depth):
            h, size, _ = ovit.tome_block_forward(h, size, p, i, cfg, sched.get(i, 0), precision, forced.get(i))
            out.append(h)
    elif fam == "ats":
        counts = oracle.ats_sample_counts(cfg)
        mask = torch.ones(h.shape[0], h.shape[1], dtype=torch.bool)
        for i in range(cfg.depth):
            h, mask, _, _ = oracle.ats_block_forward(h, mask, p, i, cfg, counts.get(i, 0), precision, False, forced.get(i))
            out.append(h)
    elif fam == "kmedoids":
        counts, attn = oracle.dpcknn_cluster_counts(cfg), None
        for i in range(cfg.depth):
            if i in counts:
                if i in forced:
                    centers = forced[i]
                else:
                    with torch.no_grad():
                        _, centers, _ = oracle.kmedoids_fit(h[:, 1:].detach(), counts[i], 3, oracle.kmedoids_token_weights(attn.detach()))
                xs = torch.gather(h[:, 1:], 1, centers[:, :, None].expand(-1, -1, h.shape[-1]))
                h = torch.cat([h[:, :1], xs], dim=1)
            h, attn = oracle.kmedoids_block_forward(h, p, i, cfg, precision)
            out.append(h)
    else:
        counts = oracle.sit_cluster_counts(cfg) if fam in ("sit", "patchmerger") else oracle.dpcknn_cluster_counts(cfg)
        j = 0
        for i in range(cfg.depth):
            if i in counts:
                if fam == "dpcknn":
                    xs, _, _, _ = oracle.dpcknn_ctm(h[:, 1:], p, j, counts[i], noise[i], 5, forced.get(i))
                elif fam == "sit":
                    xs, _ = oracle.sit_slim(h[:, 1:], p, j, precision)
                elif fam == "patchmerger":
                    xs, _ = oracle.patchmerger_merge(h[:, 1:], p, j, precision)
                else:
                    xs, _ = oracle.sinkhorn_layer(h[:, 1:], p[f"cluster_layers.{j}.v"], 1.0, 3, precision)
                h = torch.cat([h[:, :1], xs], dim=1)
                j += 1
            h, _, _ = ovit.block_forward(h, p, i, cfg, None, precision)
            out.append(h)
    return out


def logits_of(params, h, cfg, precision="fp32"):
    """The oracle's head on the last stream."""
    p = params
    return ovit.head(h, p["norm.weight"], p["norm.bias"], p["head.weight"], p["head.bias"], cfg.ln_eps, precision)


def oracle_forward(params, x, cfg, precision="fp32", forced=None, noise=None):
    """(logits, viz) of the oracle's own forward of cfg.family with return_viz=True, undecorated (the caller picks the grad mode)."""
    fam = cfg.family
    if fam == "kmedoids":
        return oracle.kmedoids_forward.__wrapped__(params, x, cfg, precision, True, 3, forced)
    if fam == "tome":
        return oracle.tome_forward.__wrapped__(params, x, cfg, precision, True, forced)
    if fam == "dpcknn":
        return oracle.dpcknn_forward.__wrapped__(params, x, cfg, noise, precision, True, forced)
    if fam == "ats":
        return oracle.ats_forward.__wrapped__(params, x, cfg, precision, True, False, forced)
    if fam in ("sit", "patchmerger", "sinkhorn"):
        return getattr(oracle, fam + "_forward").__wrapped__(params, x, cfg, precision, True)
    return oracle.vit_forward.__wrapped__(params, x, cfg, precision, True, forced)


def level_rows(h, params, cfg, norm):
    """A level's rows [B, N, D] as the map shows them: the model's final norm in fp32 arithmetic (norm=True) or the stream as it stands."""
    if not norm:
        return h
    return torch.nn.functional.layer_norm(h, (h.shape[-1],), params["norm.weight"], params["norm.bias"], cfg.ln_eps)


def level_map(rows, index, fill):
    """[B, P0, D]: rows [B, N, D] gathered by index [B, P0] (the row that stands for a patch), `fill` where index < 0.  Differentiable."""
    index = torch.as_tensor(index).long()
    D = rows.shape[-1]
    got = torch.gather(rows, 1, index.clamp_min(0)[:, :, None].expand(-1, -1, D))
    return torch.where((index >= 0)[:, :, None], got, torch.full_like(got, fill))


def dense_scatter_levels(dmaps, index, level_rows_, layout, dtype="fp32"):
    """dmaps: a list of L arrays as tests/_dense_train_ref.dense_scatter takes them, or None for a level without a gradient; index int
    [L, B, P]; level_rows_ the rows of each level.  -> a list of L results [B, rows_l, D], None where the level has no gradient (the
    kernel does not touch its slab)."""
    assert len(dmaps) == len(level_rows_) == index.shape[0]
    return [None if g is None else tref.dense_scatter(g, index[l], int(level_rows_[l]), layout, dtype) for l, g in enumerate(dmaps)]


def dense_gather_f64(tokens, index, layout):
    """The gather in fp64 with fill 0 (the adjoint identity's left side): tokens [B, n_rows, D], index [B, P]."""
    B, P = index.shape
    D = tokens.shape[-1]
    out = np.zeros((B, P, D), dtype=np.float64)
    for b in range(B):
        for q in range(P):
            r = int(index[b, q])
            if 0 <= r < tokens.shape[1]:
                out[b, q] = tokens[b, r]
    return out.transpose(0, 2, 1) if layout == "NCHW" else out
