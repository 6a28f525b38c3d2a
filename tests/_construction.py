"""What a constructor leaves behind, as plain JSON: shared by tests/golden/gen_model_construction.py (which records it) and
tests/test_model_construction.py (which compares against the record).

Per (factory name, keep_rate, reduction_loc): one digest of the parameter names and shapes in registration order (= the positional keys
of an optimizer state_dict) and of the state_dict keys, the keep schedule, the reference helper surface, every public instance attribute the family's constructor adds to the trunk's, and a digest of
torch's CPU generator state after construction under torch.manual_seed(0) (pins the NUMBER of random draws); for the tiny width also a
digest of all parameter bytes (pins their order and values)."""
from __future__ import annotations

import hashlib
import json
import types

import torch

import tokenreduction_amd as tra

RATIO_FAMILIES = ("topk", "evit", "dyvit")
SCHEDULES = [([0.7], [3, 6, 9]), ([0.5], [1, 5]), ([0.9], [0, 4, 8, 11])]      # test_boundary.test_stage_schedules_match_the_oracle


def _args(kr, loc, **kw):
    base = dict(keep_rate=list(kr), reduction_loc=list(loc), viz_mode=False, dyvit_distill=False, k_neighbors=5, equal_weight=False,
                cluster_iters=3, sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None, distillation_type="none")
    base.update(kw)
    return types.SimpleNamespace(**base)


def cases():
    """[(key, factory name, args)] -- every registered name with the three geometric schedules and one explicit list (ratios for
    topk / evit / dyvit, absolute counts for the others; heuristic: the listed-blocks variant).  The dense names take no schedule."""
    out = []
    for name in tra.list_models():
        fam = name.split("_")[0]
        if fam == "deit" or name.endswith("_teacher"):
            out.append((name, name, _args([0.7], [3, 6, 9])))
            continue
        scheds = [(kr, loc, {}) for kr, loc in SCHEDULES if not (fam == "kmedoids" and 0 in loc)]
        if fam in RATIO_FAMILIES:
            scheds.append(([0.8, 0.5, 0.3], [2, 5, 8], {}))
        elif fam == "ats":
            scheds.append(([120, 60, 30], [2, 5, 8], {}))
        elif fam == "heuristic":
            scheds.append(([0.7], [2, 5, 8], {"not_contiguous": True}))
        else:
            scheds.append(([150, 100, 40], [2, 5, 8], {}))
        for kr, loc, extra in scheds:
            key = f"{name}|{kr}|{loc}" + "".join(f"|{k}={v}" for k, v in extra.items())
            out.append((key, name, _args(kr, loc, **extra)))
    return out


MISMATCH_CASES = {"topk": ("topk_tiny_patch16_224", [0.7, 0.5], [3, 6, 9]), "cluster": ("sit_tiny_patch16_224", [150, 100], [2, 5, 8]),
                  "ats": ("ats_tiny_patch16_224", [120, 60], [2, 5, 8])}


def mismatch_message(which):
    name, kr, loc = MISMATCH_CASES[which]
    try:
        tra.create_model(name, pretrained=False, num_classes=10, img_size=224, args=_args(kr, loc))
    except AssertionError as e:
        return str(e)
    raise RuntimeError(f"{name} accepted {kr} for {loc}")


def _sha(b: bytes):
    return hashlib.sha256(b).hexdigest()


def _plain(v):
    """JSON form of a public attribute, or None for what has none (modules, callables)."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if torch.is_tensor(v):
        out = {"tensor_shape": list(v.shape)}
        if v.numel() <= 64:
            out["values"] = [round(float(t), 5) for t in v.reshape(-1)]
        return out
    if isinstance(v, (list, tuple)):
        items = [_plain(t) for t in v]
        return None if any(t is None and s is not None for t, s in zip(items, v)) else items
    if isinstance(v, dict):
        return {str(k): _plain(t) for k, t in v.items()}
    return None


# what the dense trunk's constructor sets (dimensions, drop rates, precision, ...): the same for every family, not part of a schedule
_TRUNK_ATTRS = set(vars(tra.VisionTransformer(embed_dim=64, depth=1, num_heads=1)))


def snapshot(name, args):
    torch.manual_seed(0)
    m = tra.create_model(name, pretrained=False, num_classes=10, img_size=224, args=args)
    rng = _sha(torch.get_rng_state().numpy().tobytes())
    attrs = {}
    for k, v in vars(m).items():
        if k.startswith("_") or k in _TRUNK_ATTRS or k == "default_cfg":          # (default_cfg: the registry's, the same for every name)
            continue
        p = _plain(v)
        if p is not None or v is None:
            attrs[k] = p
    # parameter names and shapes in order + the state_dict keys: 300 to 400 strings per model, so the record keeps their digest
    structure = [[[n, list(p.shape)] for n, p in m.named_parameters()], list(m.state_dict().keys())]
    snap = dict(n_params=len(structure[0]), structure_sha256=_sha(json.dumps(structure).encode()),
                keep={str(i): int(k) for i, k in enumerate(m._keep) if k}, reduction_count=_plain(m.get_reduction_count()),
                new_module_names=list(m.get_new_module_names()), attrs=attrs,
                block_keep_rate={str(i): b.attn.keep_rate for i, b in enumerate(m.blocks) if b.attn.keep_rate != 1.0},
                block_r={str(i): b.r for i, b in enumerate(m.blocks) if hasattr(b, "r")}, rng_sha256=rng)
    if "_tiny_" in name:
        h = hashlib.sha256()
        for p in m.parameters():
            h.update(p.detach().contiguous().numpy().tobytes())
        snap["param_sha256"] = h.hexdigest()
    return snap

