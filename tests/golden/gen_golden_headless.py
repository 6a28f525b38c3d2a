#!/usr/bin/env python3
"""Golden vectors of headless models (num_classes = 0) by RUNNING THE REFERENCE (build container only):

    python tests/golden/gen_golden_headless.py [case ... | state_keys]

writes tests/golden/<case>.npz for tests/_headless_params.py -- gen_golden.run_case (imported, not edited) on the micro cases at
num_classes = 0, whose "logits" are then the reference's final-normed CLS rows [B, D] -- and tests/golden/headless_state_keys.json, the
state_dict keys of every factory name built by the reference's create_model at num_classes = 0."""
import contextlib
import io
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402  (sets up the reference import path and the timm stand-in)

from tests._headless_params import HEADLESS_CASES, drop_head  # noqa: E402

_make_params = gen_golden.make_params


def _make_params_headless(cfg, seed, qkv_gain=1.0):
    """gen_golden.build_reference loads strictly: a headless reference model has no head.* keys (same trunk draws: the head comes last)."""
    p = _make_params(cfg, seed, qkv_gain)
    return drop_head(p) if cfg.num_classes == 0 else p


def run_state_keys():
    import tokenreduction_amd as tra
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False, dyvit_distill=False, k_neighbors=5, equal_weight=False,
                                 sinkhorn_eps=1.0, cluster_iters=3, heuristic_pattern="l2", not_contiguous=False, min_radius=None,
                                 distillation_type="none")
    sets, models = [], {}
    for name in tra.list_models():
        with contextlib.redirect_stdout(io.StringIO()):
            m = gen_golden.create_model(name, pretrained=False, num_classes=0, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None,
                                        img_size=224, args=args)
        keys = list(m.state_dict().keys())
        if keys not in sets:
            sets.append(keys)
        models[name] = sets.index(keys)
    out = os.path.join(gen_golden.HERE, "headless_state_keys.json")
    with open(out, "w") as f:
        json.dump({"key_sets": sets, "models": models}, f, separators=(",", ":"))
    print(f"headless_state_keys.json: {len(models)} factory names, {len(sets)} distinct key lists")


if __name__ == "__main__":
    only = sys.argv[1:]
    gen_golden.make_params = _make_params_headless
    if not only or "state_keys" in only:
        run_state_keys()
    for name, case in HEADLESS_CASES.items():
        if only and name not in only:
            continue
        gen_golden.run_case(name, case)
