"""GPU: the gradient with respect to the input image (tr_vit_backward_dx; training._VitTrainFn returns it in x's slot).

When `x.requires_grad` is set, or something learnable sits in front of the model, `loss.backward()` hands autograd the input's gradient:
the patch projection's data gradient (tr_patch_embed_dgrad on the bf16 gradient of the embedded stream) folded back into [B, C, H, W].
  * parity: x.grad against the oracle's dx (tests/_input_grad_ref.py, precision="bf16", the DEVICE's own decisions, the reference's draws
    replayed as tests/test_hip_train.py does) for every gradient case.  Bound: whole-tensor relative L2 below 2 x grad_tol(case) -- the
    project's worst-single-parameter bound: dx and patch_embed.proj.weight.grad are both linear images of the same bf16 stream gradient,
    which has crossed the whole depth, so dx belongs with the worst parameter, not with the whole-model average.
  * nothing else moves: logits, loss and every parameter gradient are the same bits with and without x.requires_grad; the extra launch
    appears exactly once and only then; dx is the same bits run after run and through torch.autograd.grad.
  * frozen parameters, the gradient reducer's block-range calls, a learnable module in front of the model, inputs that cannot take a gradient.
Every parity and composition test fails without the feature: x.grad is None there."""
import os

import numpy as np
import pytest
import torch

from tests import _launches
from tests._input_grad_ref import oracle_input_grads
from tests._params import GOLDEN_CASES, GRAD_CASES, dyvit_train_loss, grad_labels, make_images
from tests.test_hip_model import build_model
from tests.test_hip_train import _dropout, _noise, _rel, grad_tol

pytestmark = pytest.mark.gpu

DGRAD = "patch_embed_dgrad_kernel"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _model(case, noise=None, dropout=None):
    """The case's model in train mode with every draw fixed, as tests/test_hip_train.py::_train_step sets them."""
    model, _, _ = build_model(case)
    model.viz_mode = False
    model.train()
    if dropout is not None:
        model.dropout_draws = dropout
    if noise is not None and case.get("drop_path"):
        model.drop_path_draws = noise
    elif noise is not None and case["family"] == "dyvit":
        model.gumbel_noise = noise
    elif noise is not None:
        model.density_noise = noise
    return model


def _image(case):
    return make_images(case["batch"], case.get("img_size", 224), case["xseed"]).cuda()


def _loss(case, out):
    y = grad_labels(case).cuda()
    return dyvit_train_loss(out, y, case) if case["family"] == "dyvit" else torch.nn.functional.cross_entropy(out, y)


def _step(case, model, x, record=False):
    """forward + loss + backward.  (logits, loss, {name: grad clone or None}, x.grad clone or None, launch labels of the backward)."""
    model.zero_grad(set_to_none=True)
    x.grad = None
    out = model(x)
    logits = out[0] if isinstance(out, tuple) else out
    loss = _loss(case, out)
    labels = _launches.labels(loss.backward) if record else loss.backward()
    torch.cuda.synchronize()
    return (logits.detach().clone(), loss.detach().clone(), {n: None if p.grad is None else p.grad.clone() for n, p in model.named_parameters()},
            None if x.grad is None else x.grad.clone(), labels)


# ------------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", GRAD_CASES)
def test_input_gradient_matches_the_oracle_on_the_device_decisions(golden_dir, name):
    from tokenreduction_amd import training
    case = GOLDEN_CASES[name]
    noise, dropout = _noise(case, golden_dir), _dropout(case, golden_dir)
    model = _model(case, noise, dropout)
    x = _image(case).requires_grad_(True)
    logits, loss, grads, dx, _ = _step(case, model, x)
    assert dx is not None, "x.requires_grad is set but loss.backward() delivered no input gradient"
    assert dx.shape == x.shape and dx.dtype == torch.float32 and bool(torch.isfinite(dx).all())
    decisions = training.train_decisions(model)
    forced = {blk: (tuple(t.cpu() for t in d) if isinstance(d, tuple) else d.cpu()) for blk, d in decisions.items()}
    if case["family"] == "dyvit":          # the oracle indexes DyViT's stages 0..S-1
        forced = {j: forced[blk] for j, blk in enumerate(sorted(forced))}
    o_loss, o_logits, o_grads, o_dx = oracle_input_grads(case, forced=forced or None, precision="bf16", noise=noise, dropout=dropout)
    rl, rd = _rel(logits.cpu(), o_logits), _rel(dx.cpu(), o_dx)
    rp = _rel(grads["patch_embed.proj.weight"].cpu(), o_grads["patch_embed.proj.weight"])
    print(f"\n[{name}] loss {loss.item():.5f} (oracle {o_loss:.5f}); logits rel L2 {rl:.3e}; dx rel L2 {rd:.3e} "
          f"(patch_embed.proj.weight.grad {rp:.3e}); |dx| {float(o_dx.norm()):.4e}")
    assert rl < 3e-2
    assert rd < 2 * grad_tol(case), rd


# ---------------------------------------------------------------------------------------------------------- nothing else moves
@pytest.mark.parametrize("name", ["topk_micro", "dpcknn_micro", "dyvit_micro_train"])
def test_nothing_else_moves(golden_dir, name):
    case = GOLDEN_CASES[name]
    model = _model(case, _noise(case, golden_dir))
    x = _image(case)
    logits0, loss0, grads0, dx0, labels0 = _step(case, model, x, record=True)
    assert dx0 is None and DGRAD not in labels0
    xg = x.clone().requires_grad_(True)
    logits1, loss1, grads1, dx1, labels1 = _step(case, model, xg, record=True)
    assert dx1 is not None and labels1.count(DGRAD) == 1
    assert [a for a in labels1 if a != DGRAD] == labels0          # the one extra launch, nothing else
    assert labels1[-1] == DGRAD                                    # ... after the embedding's own gradients
    assert torch.equal(logits1, logits0) and torch.equal(loss1, loss0)
    for n in grads0:
        assert grads0[n] is not None and torch.equal(grads1[n], grads0[n]), n
    # the same bits run after run, and through torch.autograd.grad
    _, _, _, dx2, _ = _step(case, model, xg)
    assert torch.equal(dx2, dx1)
    model.zero_grad(set_to_none=True)
    (dx3,) = torch.autograd.grad(_loss(case, model(xg)), xg)
    assert torch.equal(dx3, dx1)
    # x.grad accumulates like any leaf's (autograd's own accumulation: the executor overwrites its dx buffer)
    xg.grad = None
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        _loss(case, model(xg)).backward()
    assert torch.equal(xg.grad, dx1 + dx1)


def test_no_grad_eval_and_plain_inputs_are_as_before():
    case = GOLDEN_CASES["topk_micro"]
    model = _model(case)
    x = _image(case)
    xg = x.clone().requires_grad_(True)
    with torch.no_grad():
        want = model(x)
        rec0 = _launches.labels(lambda: model(x))
        got = model(xg)
        rec1 = _launches.labels(lambda: model(xg))
    assert torch.equal(got, want) and rec1 == rec0 and not got.requires_grad and got.grad_fn is None
    model.eval()                                                   # eval stays non-differentiable
    e0, e1 = model(x), model(xg)
    e0, e1 = (e0[0], e1[0]) if isinstance(e0, tuple) else (e0, e1)
    assert torch.equal(e0, e1) and not e1.requires_grad


# ------------------------------------------------------------------------------------------------------------ frozen interplay
@pytest.mark.parametrize("name", ["topk_micro", "dpcknn_micro", "dyvit_micro_train"])
def test_fully_frozen_model_still_delivers_the_input_gradient(golden_dir, name):
    """An adversarial step on fixed weights: no unit takes a gradient, the walk still goes all the way down."""
    case = GOLDEN_CASES[name]
    model = _model(case, _noise(case, golden_dir))
    xg = _image(case).requires_grad_(True)
    _, loss_all, _, dx_all, _ = _step(case, model, xg)
    for p in model.parameters():
        p.requires_grad = False
    model.zero_grad(set_to_none=True)
    st = model._train_state()
    stage = {n for names in (st._stage_names or {}).values() for n in names}
    before = st.flat.clone()
    _, loss, grads, dx, labels = _step(case, model, xg, record=True)
    assert torch.equal(loss, loss_all) and torch.equal(dx, dx_all)
    assert all(g is None for g in grads.values())
    assert labels.count(DGRAD) == 1 and "tr_embed_bwd" not in labels
    for n, _ in st.order:                                           # a reached stage's slices are computed and discarded; nothing else is written
        if n not in stage:
            assert torch.equal(st.views[n], before[st.offsets[n]: st.offsets[n] + st.views[n].numel()].view_as(st.views[n])), n


def test_head_only_with_the_input_gradient_walks_to_the_bottom():
    case = GOLDEN_CASES["topk_micro"]
    model = _model(case)
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("head.")
    x = _image(case)
    _, loss0, grads0, dx0, labels0 = _step(case, model, x, record=True)
    assert dx0 is None and DGRAD not in labels0 and len(labels0) <= 6          # the classifier step alone
    xg = x.clone().requires_grad_(True)
    _, loss1, grads1, dx1, labels1 = _step(case, model, xg, record=True)
    assert torch.equal(loss1, loss0)
    assert len(labels1) > len(labels0) + 4 * case["depth"] and labels1[-1] == DGRAD      # every block is walked
    for n in grads0:
        assert (grads1[n] is None) == (grads0[n] is None), n
        if grads0[n] is not None:
            assert n.startswith("head.") and torch.equal(grads1[n], grads0[n]), n
    for p in model.parameters():
        p.requires_grad = True
    _, _, _, dx_all, _ = _step(case, model, xg)
    assert torch.equal(dx1, dx_all)


# ------------------------------------------------------------------------------------------------------------------- reducer
@pytest.mark.parametrize("name", ["evit_micro", "dpcknn_micro"])
def test_input_gradient_under_the_gradient_reducer(name):
    """World-1 RCCL, the backward in per-bucket block ranges (tests/test_hip_train.py::test_gradient_reducer_on_rccl_world1): every range
    call takes dx, only the last one (blk_lo == 0) writes it -- the bits of the single-call dx."""
    import torch.distributed as dist
    from tokenreduction_amd.dp import FlatGradReducer
    case = GOLDEN_CASES[name]
    noise = None
    if case["family"] == "dpcknn":
        probe, *_ = build_model(case)
        noise = {blk: torch.zeros(case["batch"], P) for blk, _, P in probe._stage_shapes()}
    model = _model(case, noise)
    xg = _image(case).requires_grad_(True)
    _, loss, want, dx, _ = _step(case, model, xg)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29577")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        red = FlatGradReducer(bucket_bytes=512 * 1024).attach(model)
        red.broadcast_parameters(model)
        _, loss2, got, dx2, labels = _step(case, model, xg, record=True)
        assert len(red.launched) >= 3 and red.launched[-1][1] == model._train_state().flat.numel()
        assert labels.count(DGRAD) == 1
        assert torch.equal(loss2, loss) and torch.equal(dx2, dx)
        for n in want:
            assert torch.equal(got[n], want[n]), n
    finally:
        model._grad_reducer = None
        dist.destroy_process_group()


# --------------------------------------------------------------------------------------------------------------- composition
class _ChannelAffine(torch.nn.Module):
    """A learnable per-channel affine in front of the model: the smallest module that trains only through the input gradient."""

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor([1.10, 0.90, 1.05]))
        self.shift = torch.nn.Parameter(torch.tensor([0.05, -0.03, 0.02]))

    def forward(self, x):
        return x * self.scale.view(1, -1, 1, 1) + self.shift.view(1, -1, 1, 1)


def test_a_module_in_front_of_the_model_trains():
    from tokenreduction_amd import training
    case = GOLDEN_CASES["topk_micro"]
    model = _model(case)
    stem = _ChannelAffine().cuda()
    x = _image(case)
    y = stem(x)
    _loss(case, model(y)).backward()
    torch.cuda.synchronize()
    assert stem.scale.grad is not None and stem.shift.grad is not None, "the module in front of the model received no gradient"
    decisions = training.train_decisions(model)
    forced = {blk: d.cpu() for blk, d in decisions.items()}
    # the oracle at the image the model saw, then plain autograd through the same affine on the CPU
    ref = _ChannelAffine()
    y_ref = ref(x.cpu())
    _, _, _, o_dx = oracle_input_grads(case, forced=forced, precision="bf16", x=y_ref)
    y_ref.backward(o_dx)
    for got, want, what in ((stem.scale.grad, ref.scale.grad, "scale"), (stem.shift.grad, ref.shift.grad, "shift")):
        r = _rel(got.cpu(), want)
        print(f"\n[affine.{what}] {got.cpu().tolist()} vs {want.tolist()}: rel L2 {r:.3e}")
        assert r < 2 * grad_tol(case), (what, r)


# ----------------------------------------------------------------------------------------------------------- unaffected inputs
def test_uint8_pixels_and_augmented_batches_train_as_before():
    from tests.test_device_augment import u8_batch
    from tokenreduction_amd import augment
    case = dict(GOLDEN_CASES["topk_micro"], batch=4)
    u8 = u8_batch(4, 3, 224, 9).cuda()
    runs = []
    for batch in (u8, augment.AugmentedBatch(u8, augment.empty_table(4))):
        model = _model(case)
        model.set_pixel_input()
        loss = _loss(case, model(batch))
        labels = _launches.labels(loss.backward)
        torch.cuda.synchronize()
        assert DGRAD not in labels and all(p.grad is not None for p in model.parameters())
        runs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_an_unsupported_width_raises_instead_of_dropping_the_gradient():
    """embed_dim 64 trains, but tr_patch_embed_dgrad has no kernel for it: an input that requires a gradient is refused at the forward."""
    case = dict(GOLDEN_CASES["deit_micro"], embed_dim=64, num_heads=1)
    model = _model(case)
    x = _image(case)
    _, _, grads, dx, labels = _step(case, model, x, record=True)
    assert dx is None and DGRAD not in labels and all(g is not None for g in grads.values())
    with pytest.raises(NotImplementedError, match="input gradient"):
        model(x.clone().requires_grad_(True))
    with torch.no_grad():                                          # nothing to differentiate: no refusal
        model(x.clone().requires_grad_(True))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
def test_input_gradient_comes_back_in_the_input_dtype(dtype):
    case = GOLDEN_CASES["topk_micro"]
    model = _model(case)
    xw = _image(case).to(dtype)                     # the values the executor reads are xw.float()
    xf = xw.float().requires_grad_(True)
    _, loss32, _, dx32, _ = _step(case, model, xf)
    xw.requires_grad_(True)
    _, loss, _, dx, _ = _step(case, model, xw)
    assert torch.equal(loss, loss32)
    assert dx.dtype == dtype and dx.shape == xw.shape and torch.equal(dx, dx32.to(dtype))
