"""CPU: the oracle's gradient with respect to the input image, pinned on the REFERENCE's own.

tests/golden/input_grad_<case>.npz were recorded by tests/golden/gen_input_grad.py from the reference model in train mode with the image
as an autograd leaf: the L2 norm of dx, its grad_sample_index entries and the per-patch norms [B, P].  tests/_input_grad_ref.py runs the
oracle step of tests/_params.oracle_param_grads with the image as one more leaf:
  (1) that changes nothing above the patch embedding: loss, logits and every parameter gradient are the bits of oracle_param_grads;
  (2) its fp32 dx reproduces the fixture by the norm-and-samples rule of tests/test_oracle_grad.py, with dx as one more parameter (fp32 on
      both sides: 1e-4 relative to the gradient's norm, 3e-3 at DeiT-B width; measured relative L2 of the whole tensor 2.8e-6 .. 5.2e-6
      on the micro cases) -- for EVERY recorded fixture.
The GPU tests then compare the HIP input gradient with this oracle on the device's own decisions (tests/test_input_grad_gpu.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from tests._input_grad_ref import oracle_input_grads, patch_norms
from tests._params import GOLDEN_CASES, GRAD_CASES, dropout_masks, grad_sample_index, oracle_param_grads
from tests.test_oracle_grad import fixture_inputs

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORDED = sorted(os.path.basename(p)[len("input_grad_"):-len(".npz")] for p in glob.glob(os.path.join(HERE, "input_grad_*.npz")))


def _deterministic(name):
    g = np.load(os.path.join(HERE, f"grad_{name}.npz"))
    return not any(k.startswith(("rand_", "gumbel_")) or k == "dropkeep" for k in g.files)


def test_every_deterministic_gradient_case_has_an_input_gradient_fixture():
    assert RECORDED == sorted(n for n in GRAD_CASES if _deterministic(n))
    assert {"deit_micro", "topk_micro", "evit_micro", "tome_micro", "topk_small_kr07", "deit_base"} <= set(RECORDED)


@pytest.mark.parametrize("name", ["topk_micro", "dpcknn_micro", "dyvit_micro_train", "topk_micro_droppath", "topk_micro_dropout", "sit_micro"])
def test_the_image_as_a_leaf_leaves_the_oracle_step_unchanged(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"grad_{name}.npz"))
    forced, noise = fixture_inputs(GOLDEN_CASES[name], g)
    want_loss, want_logits, want = oracle_param_grads(GOLDEN_CASES[name], forced=forced, noise=noise, dropout=dropout_masks(g))
    loss, logits, grads, dx = oracle_input_grads(GOLDEN_CASES[name], forced=forced, noise=noise, dropout=dropout_masks(g))
    assert loss == want_loss and torch.equal(logits, want_logits)
    assert set(grads) == set(want)
    for n in want:
        assert torch.equal(grads[n], want[n]), n
    case = GOLDEN_CASES[name]
    size = case.get("img_size", 224)
    assert dx.shape == (case["batch"], 3, size, size) and dx.dtype == torch.float32
    assert bool(torch.isfinite(dx).all()) and float(dx.norm()) > 0


@pytest.mark.parametrize("name", RECORDED)          # every committed fixture, the DeiT-S and DeiT-B widths included
def test_oracle_input_gradient_matches_the_reference(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"grad_{name}.npz"))
    r = np.load(os.path.join(golden_dir, f"input_grad_{name}.npz"))
    forced, noise = fixture_inputs(GOLDEN_CASES[name], g)
    loss, logits, grads, dx = oracle_input_grads(GOLDEN_CASES[name], forced=forced, noise=noise, dropout=dropout_masks(g))
    assert abs(loss - float(r["loss"])) <= 1e-5 * max(1.0, abs(float(r["loss"])))
    assert tuple(dx.shape) == tuple(int(v) for v in r["shape"])
    wide = GOLDEN_CASES[name]["embed_dim"] >= 768
    rel = 3e-3 if wide else 1e-4
    ref_norm = float(r["norm"])
    # dx as one more parameter of tests/test_oracle_grad.py's rule: `total` is the norm of the whole gradient, dx included
    total = (sum(float(g["norm:" + str(n)]) ** 2 for n in g["param_names"]) + ref_norm ** 2) ** 0.5
    flat = dx.reshape(-1)
    got_norm = float(flat.double().norm())
    print(f"\n[{name}] |dx| {got_norm:.6e} (reference {ref_norm:.6e})")
    assert abs(got_norm - ref_norm) <= rel * ref_norm + 1e-7 * total, (got_norm, ref_norm)
    smp = flat[torch.from_numpy(grad_sample_index(flat.numel()))].numpy()
    err = np.abs(smp - r["sample"]).max()
    assert err <= (rel * ref_norm + 1e-7 * total) / np.sqrt(max(1, flat.numel())) * 30 + 1e-9, (err, ref_norm)
    # the per-patch norms: a patch's norm is 1-Lipschitz in the patch, so the vector of their differences is no longer than dx's own error
    pn = patch_norms(dx).numpy()
    assert pn.shape == r["patch_norms"].shape
    # (the fixture stores them in fp32: 6e-8 relative each, far below rel)
    assert float(np.linalg.norm(pn - r["patch_norms"].astype(np.float64))) <= rel * ref_norm + 1e-7 * total


def test_oracle_input_gradient_at_another_image():
    """x=: the oracle differentiates at the caller's image (what a module in front of the model hands it), not at the case's own batch."""
    case = GOLDEN_CASES["deit_micro"]
    from tests._params import make_images
    x0 = make_images(case["batch"], 224, case["xseed"])
    _, logits0, _, dx0 = oracle_input_grads(case)
    _, logits1, _, dx1 = oracle_input_grads(case, x=x0)
    assert torch.equal(logits0, logits1) and torch.equal(dx0, dx1)
    _, logits2, _, dx2 = oracle_input_grads(case, x=0.5 * x0 + 0.1)
    assert not torch.equal(logits0, logits2) and not torch.equal(dx0, dx2)
