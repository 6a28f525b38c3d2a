#!/usr/bin/env python3
"""Record which parameters the reference's --attn-only leaves trainable (build container only):
    REFERENCE_ROOT=<reference checkout> python tests/golden/gen_attn_only.py

Executes the reference's own lines (train.py, the `if args.attn_only:` block) on the reference's own models (test-only timm stand-in,
see gen_golden.py) and writes tests/golden/attn_only_names.json: per factory the trainable and the frozen parameter names."""
import contextlib
import io
import json
import os
import sys
import textwrap
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["REFERENCE_ROOT"]
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "timm_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

with contextlib.redirect_stdout(io.StringIO()):
    import models_act  # noqa: E402,F401
from timm.models import create_model  # noqa: E402

from tests.test_finetune import case_args  # noqa: E402

FACTORIES = ["deit_small_patch16_224_local", "topk_small_patch16_224", "evit_small_patch16_224", "tome_small_patch16_224",
             "dyvit_small_patch16_224", "sit_small_patch16_224", "dpcknn_small_patch16_224", "ats_small_patch16_224",
             "sinkhorn_small_patch16_224", "kmedoids_small_patch16_224", "patchmerger_small_patch16_224",
             "heuristic_small_patch16_224"]

# the block of train.py that --attn-only runs: from `if args.attn_only:` to the line before `model.to(device)`
lines = open(os.path.join(REF, "train.py")).read().split("\n")
first = next(i for i, l in enumerate(lines) if l.strip() == "if args.attn_only:")
last = next(i for i in range(first, len(lines)) if lines[i].strip() == "model.to(device)")
block = compile(textwrap.dedent("\n".join(lines[first:last])), "train.py --attn-only", "exec")

out = {}
for factory in FACTORIES:
    with contextlib.redirect_stdout(io.StringIO()):
        model = create_model(factory, pretrained=False, num_classes=10, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None,
                             img_size=224, args=case_args())
    exec(block, {"args": types.SimpleNamespace(attn_only=True), "model": model})
    out[factory] = {"trainable": [n for n, p in model.named_parameters() if p.requires_grad],
                    "frozen": [n for n, p in model.named_parameters() if not p.requires_grad]}
with open(os.path.join(HERE, "attn_only_names.json"), "w") as f:
    json.dump(out, f, indent=1)
print({k: (len(v["trainable"]), len(v["frozen"])) for k, v in out.items()})
