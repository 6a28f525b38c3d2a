"""LayerScale references for the tests (tests/test_layerscale.py, test_hip_layerscale_ops.py, test_layerscale_gpu.py), written from timm's
definition (timm.models.vision_transformer.Block with init_values):

    x = x + drop_path(ls1(attn(norm1(x))))          ls(y) = y * gamma
    x = x + drop_path(ls2(mlp(norm2(x))))

  * RefBlock: that block in torch (run it in fp64), with or without the two gammas;
  * fold / unfold: the identities the package rests on -- gamma o (W h + b) = (diag(gamma) W) h + gamma o b, and for the gradients of the
    folded operands dW', db':  dW = gamma[:, None] * dW',  db = gamma * db',  dgamma = sum_k dW' * W + db' * b;
  * fold_ref / unfold_ref: the arithmetic of csrc/tr_layerscale.hip in numpy fp32, rounding by rounding (bf16: round to nearest, ties to even);
  * make_model / folded_twin: a micro model of a golden case with the options on, and the plain model of the same family and configuration
    whose proj / fc2 weights and biases are the fp32 products (with no_embed_class its pos_embed is [0; pos]); everything else is copied.
"""
import types

import numpy as np
import torch
import torch.nn as nn

FAM = {"deit": "VisionTransformer", "topk": "TopKVisionTransformer", "evit": "EfficientVisionTransformer", "tome": "ToMeVisionTransformer",
       "dyvit": "DynamicVisionTransformer", "sit": "SelfSlimmedVisionTransformer", "dpcknn": "DPCKNNVisionTransformer", "ats": "ATSVisionTransformer"}


class RefBlock(nn.Module):
    """timm's ViT block (pre-norm, GELU Mlp, qkv_bias) with LayerScale when `gammas`."""

    def __init__(self, dim, heads, gammas=True, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.heads = heads
        self.norm1, self.norm2 = nn.LayerNorm(dim, eps=1e-6), nn.LayerNorm(dim, eps=1e-6)
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.fc1, self.fc2 = nn.Linear(dim, 4 * dim), nn.Linear(4 * dim, dim)
        for p in self.parameters():
            p.data = torch.randn(p.shape, generator=g) * (0.3 if p.dim() == 1 else p.shape[1] ** -0.5)
        self.gamma_1 = self.gamma_2 = None
        if gammas:
            self.gamma_1 = nn.Parameter(torch.rand(dim, generator=g) - 0.4)         # both signs
            self.gamma_2 = nn.Parameter(torch.rand(dim, generator=g) - 0.4)

    def forward(self, x):
        B, N, D = x.shape
        q, k, v = self.qkv(self.norm1(x)).reshape(B, N, 3, self.heads, D // self.heads).permute(2, 0, 3, 1, 4)
        a = ((q @ k.transpose(-2, -1)) * (D // self.heads) ** -0.5).softmax(dim=-1)
        y = self.proj((a @ v).transpose(1, 2).reshape(B, N, D))
        x = x + (y if self.gamma_1 is None else y * self.gamma_1)
        y = self.fc2(nn.functional.gelu(self.fc1(self.norm2(x))))
        return x + (y if self.gamma_2 is None else y * self.gamma_2)


def fold(w, b, gamma):
    """(gamma[d] * w[d, k], gamma o b) in the operands' own precision (torch)."""
    return gamma[:, None] * w, gamma * b


def unfold(dw_f, db_f, w, b, gamma):
    """(dW, db, dgamma) from the gradients of the folded operands (torch, the operands' own precision)."""
    return gamma[:, None] * dw_f, gamma * db_f, (dw_f * w).sum(dim=1) + db_f * b


def folded_block(blk: RefBlock) -> RefBlock:
    """The block without gammas whose proj / fc2 are the folded ones of `blk`; every other parameter is copied."""
    twin = RefBlock(blk.proj.in_features, blk.heads, gammas=False)
    twin = twin.to(next(blk.parameters()).dtype)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items() if not k.startswith("gamma")}
    sd["proj.weight"], sd["proj.bias"] = fold(blk.proj.weight.detach(), blk.proj.bias.detach(), blk.gamma_1.detach())
    sd["fc2.weight"], sd["fc2.bias"] = fold(blk.fc2.weight.detach(), blk.fc2.bias.detach(), blk.gamma_2.detach())
    twin.load_state_dict(sd)
    return twin


# ---- the kernels' arithmetic in numpy ------------------------------------------------------------------------------------------
def bf16_rne(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bits (uint16), round to nearest, ties to even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def fold_ref(w, b, gamma):
    """(fp32 product [rows, cols], its bf16 bits, fp32 folded bias) of tr_layerscale_fold: one fp32 rounding, then one to bf16."""
    prod = (gamma.astype(np.float32)[:, None] * w.astype(np.float32)).astype(np.float32)
    return prod, bf16_rne(prod), (gamma.astype(np.float32) * b.astype(np.float32)).astype(np.float32)


def unfold_ref(dw_f, db_f, gamma, old_dw=None, old_db=None):
    """(dW, db) of tr_layerscale_unfold_grad in fp32: fl(gamma * x), and with old values fl(old + fl(gamma * x)) -- two roundings."""
    dw = (gamma[:, None].astype(np.float32) * dw_f.astype(np.float32)).astype(np.float32)
    db = (gamma.astype(np.float32) * db_f.astype(np.float32)).astype(np.float32)
    if old_dw is not None:
        dw = (old_dw.astype(np.float32) + dw).astype(np.float32)
    if old_db is not None:
        db = (old_db.astype(np.float32) + db).astype(np.float32)
    return dw, db


def dgamma_ref(dw_f, db_f, w, b):
    """(dgamma in fp64, the bound of an fp32 sum of cols + 1 products in any order: (cols + 2) * 2^-24 * (sum_k |dW' W| + |db' b|))."""
    t = dw_f.astype(np.float64) * w.astype(np.float64)
    tb = db_f.astype(np.float64) * b.astype(np.float64)
    return t.sum(axis=1) + tb, (dw_f.shape[1] + 2) * 2.0 ** -24 * (np.abs(t).sum(axis=1) + np.abs(tb))


# ---- micro models ------------------------------------------------------------------------------------------------------------------
def make_model(case, gamma_seed=None, **extra):
    """The micro model of a golden case (tests/_params.GOLDEN_CASES) with extra constructor keywords (init_values, no_embed_class, ...), the
    case's parameters loaded; gamma_seed: the gammas are drawn in [0.5, 1.5] * 1e-1 so that the branches matter.  On the CPU, train mode off."""
    import tokenreduction_amd as tra
    from tests._params import case_params
    args = types.SimpleNamespace(keep_rate=list(case["keep_rate"]), reduction_loc=list(case["reduction_loc"]), viz_mode=False,
                                 dyvit_distill=False, k_neighbors=5, equal_weight=False, sinkhorn_eps=1.0, cluster_iters=3,
                                 heuristic_pattern="l2", not_contiguous=False, min_radius=None)
    m = getattr(tra, FAM[case["family"]])(img_size=case.get("img_size", 224), patch_size=16, embed_dim=case["embed_dim"], depth=case["depth"],
                                          num_heads=case["num_heads"], mlp_ratio=4, qkv_bias=True, num_classes=case["num_classes"],
                                          drop_path_rate=float(case.get("drop_path", 0.0)), drop_rate=float(case.get("drop_rate", 0.0)), args=args,
                                          **extra)
    _cfg, params = case_params(dict(case, num_classes=case["num_classes"] or 16))
    params = {k: v for k, v in params.items() if isinstance(m.head, nn.Linear) or not k.startswith("head.")}      # (headless: no classifier)
    if m.no_embed_class:
        params["pos_embed"] = params["pos_embed"][:, 1:]
    missing, unexpected = m.load_state_dict(params, strict=False)
    assert not unexpected and all(k.endswith((".ls1.gamma", ".ls2.gamma")) for k in missing), (missing, unexpected)
    if gamma_seed is not None:
        g = torch.Generator().manual_seed(gamma_seed)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith(".gamma"):
                    p.copy_((0.5 + torch.rand(p.shape, generator=g)) * 1e-1)
    return m.eval()


def twin_state_dict(model):
    """State dict of the folded twin of `model`: no gammas, proj / fc2 folded in fp32 (one rounding), [0; pos] for a no_embed_class table."""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for i in range(model.depth):
        pre = f"blocks.{i}."
        for lin, ls in (("attn.proj", "ls1"), ("mlp.fc2", "ls2")):
            gamma = sd.pop(pre + ls + ".gamma", None)
            if gamma is not None:
                sd[pre + lin + ".weight"], sd[pre + lin + ".bias"] = fold(sd[pre + lin + ".weight"], sd[pre + lin + ".bias"], gamma)
    if model.no_embed_class:
        sd["pos_embed"] = torch.cat((torch.zeros_like(sd["pos_embed"][:, :1]), sd["pos_embed"]), dim=1)
    return sd


def folded_twin(model, case, **extra):
    """The plain model (no LayerScale, class row in the position table) of the same family and configuration that computes what `model` does."""
    twin = make_model(case, **extra)
    twin.load_state_dict(twin_state_dict(model), strict=True)
    return twin.to(model.pos_embed.device)
