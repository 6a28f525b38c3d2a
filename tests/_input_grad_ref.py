"""The oracle's gradient with respect to the INPUT image, beside its parameter gradients.

tests/_params.oracle_param_grads runs torch.autograd over the oracle's functional forward with the parameters as leaves and the image as
a constant.  Here the very same call runs with the image as one more leaf: the graph above the patch embedding is the same graph (the
parameter gradients and the loss come out bit for bit, tests/test_input_grad.py), and `x.grad` is what the reference's plain autograd
hands a caller whose input requires a gradient.  round_bf16 is autograd-transparent, so precision="bf16" gives the gradient of the HIP
rounding points with fp32 backward arithmetic, as for the parameters (tests/test_hip_train.py).

How the image becomes a leaf: tests/_params.py is a yardstick and stays as it is, and its _oracle_param_grads builds the image itself, so
this module replaces `tests._params.make_images` for the duration of one call.  That leans on _oracle_param_grads looking make_images up
as a module global exactly once per step (asserted: one image per call) and is NOT re-entrant or thread-safe: one oracle_input_grads call
at a time.  Should _oracle_param_grads ever take the image as an argument, pass the leaf there and delete _leaf_image."""
import contextlib

import torch

from tests import _params


@contextlib.contextmanager
def _leaf_image(x):
    """While active, the image tests/_params._oracle_param_grads builds for its case is the leaf `holder[0]`: the case's own image
    (make_images on the case's seed) with requires_grad set, or the caller's `x` (detached: a leaf of this graph)."""
    holder = []
    make = _params.make_images

    def leaf(*a, **kw):
        img = (make(*a, **kw) if x is None else x.detach().to(torch.float32).clone()).requires_grad_(True)
        holder.append(img)
        return img

    _params.make_images = leaf
    try:
        yield holder
    finally:
        _params.make_images = make


def oracle_input_grads(case: dict, forced=None, precision: str = "fp32", noise=None, dropout=None, x=None):
    """(loss, logits, {name: parameter gradient}, dx) of the case's oracle step -- oracle_param_grads with the image as a leaf.
    x: another image [B, C, H, W] to differentiate at (default: the case's own batch)."""
    with _leaf_image(x) as holder:
        loss, logits, grads = _params.oracle_param_grads(case, forced=forced, precision=precision, noise=noise, dropout=dropout)
    assert len(holder) == 1, "the oracle step builds its image exactly once"
    img = holder[0]
    assert img.grad is not None, "the oracle's forward does not carry the input's gradient"
    return loss, logits, grads, img.grad.detach()


def patch_norms(dx: torch.Tensor, patch: int = 16) -> torch.Tensor:
    """[B, P] L2 norm of dx over every patch (all channels), patches in the model's row-major token order."""
    B, C, H, W = dx.shape
    t = dx.double().reshape(B, C, H // patch, patch, W // patch, patch)
    return t.pow(2).sum(dim=(1, 3, 5)).sqrt().reshape(B, -1)
