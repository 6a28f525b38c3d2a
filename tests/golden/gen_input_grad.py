#!/usr/bin/env python3
"""Input-gradient fixtures by RUNNING THE REFERENCE (build container only):

    python tests/golden/gen_input_grad.py [case ...]

writes tests/golden/input_grad_<case>.npz for every GRAD_CASES entry whose gradient fixture grad_<case>.npz was recorded without random
draws (no rand_*, gumbel_* or dropkeep entries: DPC-KNN's density noise, DropPath, DyViT's Gumbel noise and nn.Dropout would have to be
replayed inside the reference).  The reference model (gen_golden.build_reference, imported, not edited) runs in train mode on the case's
batch with the image as an autograd leaf, cross-entropy on grad_labels, loss.backward() -- plain torch.autograd, which returns the input's
gradient for free.  Recorded, by the norm-plus-samples convention of the parameter gradients (never the full tensor): the L2 norm of dx,
its grad_sample_index entries, and the per-patch norms [B, P]; logits and loss as a check that the run is the one grad_<case>.npz holds."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402  (sets up the reference import path and the timm stand-in)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests._input_grad_ref import patch_norms  # noqa: E402
from tests._params import GOLDEN_CASES, GRAD_CASES, grad_labels, grad_sample_index, make_images  # noqa: E402


def deterministic(name):
    g = np.load(os.path.join(gen_golden.HERE, f"grad_{name}.npz"))
    return not any(k.startswith(("rand_", "gumbel_")) or k == "dropkeep" for k in g.files)


def run_input_grad_case(name, case):
    m, _ = gen_golden.build_reference(case)
    m.train()
    m.viz_mode = False
    x = make_images(case["batch"], case.get("img_size", 224), case["xseed"]).requires_grad_(True)
    torch.manual_seed(case["xseed"])
    out = m(x)
    logits = out[0] if isinstance(out, (tuple, list)) else out
    loss = torch.nn.functional.cross_entropy(logits, grad_labels(case))
    loss.backward()
    g = np.load(os.path.join(gen_golden.HERE, f"grad_{name}.npz"))
    assert np.array_equal(logits.detach().numpy(), g["logits"]) and loss.item() == float(g["loss"]), f"{name}: not the run of grad_{name}.npz"
    dx = x.grad.detach()
    flat = dx.reshape(-1)
    rec = {"logits": logits.detach().numpy(), "loss": np.array(loss.item(), dtype=np.float64),
           "norm": np.array(flat.double().norm().item(), dtype=np.float64),
           "sample": flat[torch.from_numpy(grad_sample_index(flat.numel()))].numpy().astype(np.float32),
           "patch_norms": patch_norms(dx).numpy().astype(np.float32), "shape": np.array(dx.shape, dtype=np.int64)}
    np.savez_compressed(os.path.join(gen_golden.HERE, f"input_grad_{name}.npz"), **rec)
    print(f"input_grad_{name}: loss {loss.item():.5f}  |dx| {float(rec['norm']):.4e}  {tuple(dx.shape)}")


if __name__ == "__main__":
    only = sys.argv[1:]
    for name in GRAD_CASES:
        if (only and name not in only) or not deterministic(name):
            continue
        run_input_grad_case(name, GOLDEN_CASES[name])
