"""Device-side mixup / cutmix / random erasing, GPU tier.  Every comparison is torch.equal against `restate` (tests/test_device_augment.py):
the torch restatement of the specified arithmetic, here run on the device -- never augment.py's fallback, never tr_pixels_augment_f32.
Shapes are tiny: what can go wrong is addressing (boxes against 8-pixel runs and patch borders, partners, noise offsets), not size."""
import numpy as np
import pytest
import torch

from tests._params import GOLDEN_CASES, dyvit_train_loss
from tests.test_device_augment import MEAN, STD, make_table, restate, u8_batch
from tests.test_hip_model import build_model
from tokenreduction_amd import _lib, augment, pixels

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def tables(S, C):
    """name -> (table of 4 records, noise): one hand-written table per property"""
    g = torch.Generator().manual_seed(S + C)
    blend = dict(kind=1, lam=F(0.3), oml=F(1.0 - 0.3))                     # timm's batch mode: float32(lam), float32(1.0 - lam)
    paste = dict(kind=2, yl=5, yh=29, xl=3, xh=21)                        # neither 8- nor 16-aligned, crosses patch borders
    e0 = dict(erased=1, ey=3, eh=13, ex=5, ew=18, noise_off=0)
    e3 = dict(erased=1, ey=10, eh=12, ex=9, ew=7, noise_off=C * 13 * 18)
    n03 = C * (13 * 18 + 12 * 7)
    edge = dict(erased=1, ey=S - 9, eh=9, ex=S - 11, ew=11, noise_off=5)   # touches the right and the bottom edge; a block not at 0
    lams = [F(0.25), F(0.6180339887), F(0.999)]
    return {
        "none": ([{}, {}, {}, {}], torch.zeros(0)),
        "blend": ([blend] * 4, torch.zeros(0)),
        "paste": ([paste] * 4, torch.zeros(0)),
        "empty_box": ([dict(kind=2, yl=7, yh=7, xl=3, xh=21), dict(kind=2, yl=3, yh=9, xl=11, xh=11), dict(kind=2, yl=0, yh=0, xl=0, xh=0),
                       dict(kind=2, yl=S, yh=S, xl=S, xh=S)], torch.zeros(0)),
        "whole_image": ([dict(kind=2, yl=0, yh=S, xl=0, xh=S)] * 4, torch.zeros(0)),
        # elem mode: image 1 drew lam == 1 (kind 0), the others distinct factors with oml = float32(1) - float32(lam); image 3 pastes
        "elem": ([dict(kind=1, lam=lams[0], oml=F(1) - lams[0]), {}, dict(kind=1, lam=lams[1], oml=F(1) - lams[1]),
                  dict(kind=2, yl=1, yh=S - 1, xl=S - 9, xh=S)], torch.zeros(0)),
        # image 0 and its partner 3 both erased, image 0's paste box over both erase boxes; image 3 blends with the erased image 0
        "erase_pixel": ([dict(e0, **paste), {}, blend, dict(e3, **blend)], torch.randn(n03, generator=g)),
        "erase_const": ([dict(e0, **blend), blend, blend, dict(e3, **blend)], torch.zeros(n03)),
        "erase_edge": ([{}, dict(edge, kind=2, yl=S - 20, yh=S, xl=S - 13, xh=S - 2), dict(edge, noise_off=5 + C * 99, **blend), {}],
                       torch.randn(5 + 2 * C * 99 + 3, generator=g)),
    }


def _device_batch(u8, layout):
    d = u8.cuda()
    return d if layout == "nchw" else d.contiguous(memory_format=torch.channels_last)


# ---- ops --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,C,layout", [(32, 3, "nchw"), (32, 3, "nhwc"), (48, 3, "nchw"), (48, 3, "nhwc"), (32, 1, "nhwc"), (48, 1, "nhwc")])
def test_pixels_and_columns_equal_the_restatement(S, C, layout):
    from tokenreduction_amd import ops
    u8 = u8_batch(4, C, S, 100 + S + C)
    img = _device_batch(u8, layout)
    lut = pixels.pixel_lut(MEAN[:C], STD[:C]).cuda()
    lay = _lib.TR_LAYOUT_NHWC if layout == "nhwc" else _lib.TR_LAYOUT_NCHW      # (one channel: the same bytes, the NHWC kernel)
    for name, (rows, noise) in tables(S, C).items():
        table = make_table(rows)
        augment.validate_table(table, C, S, S, noise.numel())
        want = restate(u8.cuda(), lut, table, noise.cuda())
        dev_table = torch.from_numpy(table.view(np.uint8).copy()).cuda()
        for patch in (8, 16):
            got = ops.pixels_augment(img, lut, dev_table, noise.cuda(), patch=patch, layout=lay)
            assert got.shape == want.shape and got.is_contiguous()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, patch, float((got - want).abs().max()))
            cols = ops.im2col_u8_aug(img, lut, dev_table, noise.cuda(), patch, layout=lay)
            assert torch.equal(cols.view(torch.int16), ops.im2col(want, patch).view(torch.int16)), (name, patch)
        if name == "none":       # ... which are the bits of today's uint8 path
            assert torch.equal(ops.im2col_u8_aug(img, lut, dev_table, noise.cuda(), 16, layout=lay).view(torch.int16),
                               ops.im2col_u8(img, lut, 16).view(torch.int16))


def test_augmented_batch_float_and_to():
    u8 = u8_batch(4, 3, 32, 1)
    rows, noise = tables(32, 3)["erase_pixel"]
    host = augment.AugmentedBatch(u8, make_table(rows), noise)
    batch = host.to("cuda", non_blocking=True)
    assert batch.is_cuda and batch.table.is_cuda and batch.noise.is_cuda and tuple(batch.shape) == (4, 3, 32, 32) and not host.is_cuda
    want = restate(u8.cuda(), pixels.pixel_lut(MEAN, STD).cuda(), make_table(rows), noise.cuda())
    assert torch.equal(batch.float(), want) and batch.float() is batch.float()
    strided = augment.AugmentedBatch(u8.cuda().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), make_table(rows), noise.cuda())
    assert torch.equal(strided.float(), want)


# ---- models -----------------------------------------------------------------------------------------------------------------------

def _case(name):
    case = dict(GOLDEN_CASES[name])
    case["batch"] = 4 if case["batch"] % 2 else case["batch"]
    return case


def _labels(case):
    return torch.randint(0, case["num_classes"], (case["batch"],), generator=torch.Generator().manual_seed(case["xseed"] + 7))


def _train(case, x):
    model, _, _ = build_model(case)
    model.viz_mode = False
    model.set_pixel_input()
    model.train()
    torch.manual_seed(3)                  # Gumbel draws
    np.random.seed(3)
    out = model(x)
    if case["family"] == "dyvit":
        assert isinstance(out, tuple) and len(out) == 4
        logits, loss = out[0], dyvit_train_loss(out, _labels(case).cuda(), case)
    else:
        logits, loss = out, torch.nn.functional.cross_entropy(out, _labels(case).cuda())
    loss.backward()
    return logits.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _model_table(name, S):
    if name == "blend":
        return tables(S, 3)["blend"]
    # paste + erase at the model's size: image 0 and its partner erased, paste boxes over both, one image left alone
    paste = dict(kind=2, yl=37, yh=S - 50, xl=21, xh=S - 3)
    e0 = dict(erased=1, ey=30, eh=61, ex=45, ew=83, noise_off=0)
    eL = dict(erased=1, ey=S - 70, eh=70, ex=S - 99, ew=99, noise_off=3 * 61 * 83)
    rows = [dict(e0, **paste), paste, {}, dict(eL, **paste)][:4]
    return rows, torch.randn(3 * (61 * 83 + 70 * 99), generator=torch.Generator().manual_seed(S))


@pytest.mark.parametrize("table_name", ["blend", "paste_erase"])
@pytest.mark.parametrize("name", ["topk_micro", "dyvit_micro_train", "topk_micro_384"])
def test_model_logits_and_gradients_equal_the_float_image(name, table_name):
    case = _case(name)
    S, B = case.get("img_size", 224), case["batch"]
    u8 = u8_batch(B, 3, S, case["xseed"])
    rows, noise = _model_table(table_name, S)
    rows = rows[:B] if B == 4 else [rows[0], rows[3]]
    table = make_table(rows)
    want_l, want_g = _train(case, restate(u8.cuda(), pixels.pixel_lut(MEAN, STD).cuda(), table, noise.cuda()))
    assert "patch_embed.proj.weight" in want_g
    for layout in ("nchw", "nhwc"):
        batch = augment.AugmentedBatch(_device_batch(u8, layout), table, noise.cuda())
        got_l, got_g = _train(case, batch)
        assert torch.equal(got_l, want_l), layout
        assert sorted(got_g) == sorted(want_g)
        for n in want_g:
            assert torch.equal(got_g[n], want_g[n]), (layout, n)


def test_none_table_gives_the_uint8_path():
    case = _case("topk_micro")
    u8 = u8_batch(4, 3, 224, 9)
    want_l, want_g = _train(case, u8.cuda())                                          # tr_vit_forward_train_pixels
    got_l, got_g = _train(case, augment.AugmentedBatch(u8.cuda(), augment.empty_table(4)))      # tr_vit_forward_train_aug
    assert torch.equal(got_l, want_l) and sorted(got_g) == sorted(want_g)
    for n in want_g:
        assert torch.equal(got_g[n], want_g[n]), n


def test_other_consumers_materialize_the_batch():
    """The teacher (eval executor whatever its mode), an eval model and a model without pixel input return what they return for the
    restated float image; a model whose normalization differs from the batch's refuses it."""
    import tokenreduction_amd as tra
    case = _case("dyvit_micro_train")
    torch.manual_seed(1)
    teacher = tra.VisionTransformerTeacher(patch_size=16, embed_dim=case["embed_dim"], depth=case["depth"], num_heads=case["num_heads"],
                                           mlp_ratio=4, qkv_bias=True, num_classes=case["num_classes"]).cuda().eval()
    u8 = u8_batch(4, 3, 224, 2)
    rows, noise = _model_table("paste_erase", 224)
    table = make_table(rows)
    xf = restate(u8.cuda(), pixels.pixel_lut(MEAN, STD).cuda(), table, noise.cuda())
    with torch.no_grad():
        want = [t.clone() for t in teacher(xf)]
        for pixel_input in (False, True):
            teacher.set_pixel_input(*((MEAN, STD) if pixel_input else (None, None)))
            got = teacher(augment.AugmentedBatch(u8.cuda(), table, noise.cuda()))
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), pixel_input
    model, _, _ = build_model(_case("topk_micro"))
    model.viz_mode = False
    model.eval()
    batch = augment.AugmentedBatch(u8.cuda(), table, noise.cuda())
    want = model(xf).clone()
    assert torch.equal(model(batch), want) and torch.equal(model.forward_async(batch).result(), want)
    model.train()                                                   # pixel input off: the float training path on the materialized image
    assert torch.equal(model(batch), model(xf))
    model.set_pixel_input((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
    with pytest.raises(ValueError, match="mean"):
        model(batch)


# ---- harness ------------------------------------------------------------------------------------------------------------------------

def test_train_one_epoch_uint8_loader_equals_the_float_loader():
    """harness.train_one_epoch over three batches with grad_accum_steps = 2 -- two FusedAdamW steps (after batch 2, and at the end of the
    loader) -- with DeviceAugment as mixup_fn, elem mode so that one batch holds blends, pastes and untouched images, erasing on: the uint8
    loader (AugmentedBatch -> tr_vit_forward_train_aug) against the normalized float loader (DeviceAugment's torch path) with the same seeds."""
    import random
    from tokenreduction_amd import harness
    from tokenreduction_amd.optim import FusedAdamW
    case = _case("topk_micro")
    batches = [u8_batch(4, 3, 224, 70 + i) for i in range(3)]
    targets = [torch.randint(0, case["num_classes"], (4,), generator=torch.Generator().manual_seed(i)) for i in range(3)]
    lut = pixels.pixel_lut(MEAN, STD)
    normalized = [torch.stack([lut[c][b[:, c].long()] for c in range(3)], dim=1) for b in batches]
    runs = []
    for loader in ([(x, t) for x, t in zip(normalized, targets)], [(b, t) for b, t in zip(batches, targets)],
                   [(b.contiguous(memory_format=torch.channels_last), t) for b, t in zip(batches, targets)]):
        model, _, _ = build_model(case)
        model.viz_mode = False
        model.set_pixel_input()
        opt = FusedAdamW(list(model.parameters()), lr=2e-3, weight_decay=0.05, model=model)
        mix = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", prob=0.7, label_smoothing=0.1, num_classes=case["num_classes"],
                                    re_prob=0.5, re_mode="pixel")
        losses, kinds = [], []

        def crit(samples, output, soft, m):
            if isinstance(samples, augment.AugmentedBatch):
                kinds.extend(samples.host_table["kind"].tolist())
            loss = torch.sum(-soft * torch.nn.functional.log_softmax(output.float(), dim=-1), dim=-1).mean()
            losses.append(loss.item())
            return loss
        random.seed(4)
        np.random.seed(4)
        torch.manual_seed(4)
        stats, total = harness.train_one_epoch(model, crit, loader, opt, torch.device("cuda"), 0, mixup_fn=mix, grad_accum_steps=2)
        assert total == 2 and len(losses) == 3 and np.isfinite(losses).all()
        runs.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()}, kinds))
    assert set(runs[1][2]) == {0, 1, 2}                       # the uint8 runs went through the table, with every kind in it
    for losses, params, _ in runs[1:]:
        assert losses == runs[0][0], (losses, runs[0][0])
        for n, p in params.items():
            assert torch.equal(p, runs[0][1][n]), n
