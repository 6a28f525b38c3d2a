"""GPU, model level: LayerScale (init_values) and no_embed_class against the FOLDED TWIN -- the plain model of the same family whose proj / fc2
weights and biases are the fp32 products gamma o W, gamma o b (tests/_layerscale_ref.py).  The executor of a LayerScale model reads exactly
those operands (one fp32 rounding, then the cast every operand takes), so logits and every gradient the executor produces are the twin's
BITS; the gradients of proj / fc2 are the numpy unfold of the twin's (bitwise: fl(gamma * x), under accumulation fl(old + fl(gamma * x))) and
those of gamma lie within the bound of an fp32 sum in any order, (cols + 2) * 2^-24 * (sum_k |dW' W| + |db' b|) (+ one addition per further
micro-step).  Draws (Gumbel, DropPath, ...) are device draws: the seed is set before every forward."""
import os

import numpy as np
import pytest
import torch

from tests import _launches
from tests._layerscale_ref import dgamma_ref, folded_twin, make_model, unfold_ref
from tests._params import GOLDEN_CASES, make_images

pytestmark = pytest.mark.gpu

FAMILIES = ["deit_micro", "topk_micro", "tome_micro", "ats_micro", "sit_micro", "dyvit_micro"]
FOLD, UNFOLD = "tr_layerscale_fold", "tr_layerscale_unfold_grad"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _pair(name, **extra):
    case = GOLDEN_CASES[name]
    plain = {k: v for k, v in extra.items() if k not in ("init_values", "no_embed_class")}
    model = make_model(case, gamma_seed=case["wseed"] + 1, **dict(dict(init_values=1e-6), **extra)).cuda()
    return case, model, folded_twin(model, case, **plain)


def _x(case, k=0):
    return make_images(case["batch"], case.get("img_size", 224), case["xseed"] + 1000 * k).cuda()


def _logits(out):
    return out[0] if isinstance(out, (tuple, list)) else out


def _target(case, model, k=0):
    g = torch.Generator().manual_seed(77 + k)
    return torch.randn(case["batch"], model._out_cols, generator=g).cuda()


def _train(model, case, steps=(0,), x_grad=False):
    """Forward + backward over the micro-steps `steps` (gradients accumulate from the second on): (logits per step, {name: grad}, x.grad)."""
    model.train()
    model.zero_grad(set_to_none=True)
    outs, xg = [], None
    for k in steps:
        x = _x(case, k).requires_grad_(x_grad)
        torch.manual_seed(500 + k)
        out = _logits(model(x))
        (out * _target(case, model, k)).sum().backward()
        outs.append(out.detach().clone())
        xg = None if x.grad is None else x.grad.clone()
    torch.cuda.synchronize()
    return outs, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, xg


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(_np(a).view(np.int32), _np(b).view(np.int32))


def _check_grads(model, got, twin_steps, twin_acc, trainable=None):
    """got: the LayerScale model's gradients; twin_steps: the twin's single-step gradients per micro-step; twin_acc: the twin's accumulated."""
    named = dict(model.named_parameters())
    has_ls = hasattr(model.blocks[0], "ls1")
    for n, g in got.items():
        if has_ls and (".ls1." in n or ".ls2." in n or ".attn.proj." in n or ".mlp.fc2." in n):
            continue
        want = twin_acc[n][:, 1:] if n == "pos_embed" and model.no_embed_class else twin_acc[n]
        assert torch.equal(g, want), n
    for i in range(model.depth if has_ls else 0):
        for lin, ls in (("attn.proj", "ls1"), ("mlp.fc2", "ls2")):
            wn, bn, gn = f"blocks.{i}.{lin}.weight", f"blocks.{i}.{lin}.bias", f"blocks.{i}.{ls}.gamma"
            gamma = _np(named[gn])
            dw = db = None
            want_dg, bound_dg = 0.0, 0.0
            for s, step in enumerate(twin_steps):
                if wn not in step:          # the twin skipped a frozen pair the LayerScale model needs for gamma: not comparable here
                    break
                dw, db = unfold_ref(_np(step[wn]), _np(step[bn]), gamma, dw, db)
                w64, b64 = dgamma_ref(_np(step[wn]), _np(step[bn]), _np(named[wn]), _np(named[bn]))
                want_dg, bound_dg = want_dg + w64, bound_dg + b64 + (2.0 ** -24 * np.abs(want_dg + w64) if s else 0.0)
            else:
                if wn in got:
                    assert np.array_equal(_np(got[wn]).view(np.int32), dw.view(np.int32)), wn
                    assert np.array_equal(_np(got[bn]).view(np.int32), db.view(np.int32)), bn
                if gn in got:
                    err = np.abs(_np(got[gn]).astype(np.float64) - want_dg)
                    assert (err <= bound_dg).all(), (gn, float(err.max()), float(bound_dg.min()))
                    assert float(np.abs(want_dg).max()) > 0
    if trainable is not None:
        assert sorted(got) == sorted(trainable)


# ---------------------------------------------------------------------------------------------------------------------------- eval
@pytest.mark.parametrize("name", FAMILIES)
def test_eval_logits_are_the_folded_twins_bits(name):
    case, model, twin = _pair(name)
    x = _x(case)
    for precision in ("bf16", "bf16x3", "fp32"):
        model.precision = twin.precision = precision
        torch.manual_seed(3)
        want = _logits(twin(x))
        torch.manual_seed(3)
        got = _logits(model(x))                       # captures
        assert _same_bits(got, want), precision
        torch.manual_seed(3)
        assert _same_bits(_logits(model(x)), want), precision          # graph replay
        torch.manual_seed(3)
        assert _same_bits(_logits(model.forward_async(x).result()), want), precision
        model.use_graph = False
        torch.manual_seed(3)
        assert _same_bits(_logits(model(x)), want), precision          # plain launches
        model.use_graph = True
    assert float(want.abs().max()) > 0


def test_gammas_matter_and_init_values_one_is_the_plain_model():
    case, model, twin = _pair("topk_micro")
    plain = make_model(case).cuda()
    one = make_model(case, init_values=1.0).cuda()
    x = _x(case)
    assert _same_bits(one(x), plain(x))
    assert not torch.equal(model(x), plain(x))
    outs1, g1, _ = _train(one, case)
    outsp, gp, _ = _train(plain, case)
    assert _same_bits(outs1[0], outsp[0])
    for n, g in gp.items():
        assert torch.equal(g1[n], g), n          # gamma == 1: fl(1 * x) = x


# ------------------------------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("name", FAMILIES)
def test_train_forward_and_gradients(name):
    case, model, twin = _pair(name)
    outs, got, _ = _train(model, case)
    touts, tg, _ = _train(twin, case)
    assert _same_bits(outs[0], touts[0])
    assert all(f"blocks.{i}.{ls}.gamma" in got for i in range(model.depth) for ls in ("ls1", "ls2"))
    _check_grads(model, got, [tg], tg)


@pytest.mark.parametrize("name", ["deit_micro", "topk_micro", "dyvit_micro"])
def test_gradient_accumulation_over_two_micro_steps(name):
    case, model, twin = _pair(name)
    outs, got, _ = _train(model, case, steps=(0, 1))
    _, t0, _ = _train(twin, case, steps=(0,))
    _, t1, _ = _train(twin, case, steps=(1,))
    touts, tacc, _ = _train(twin, case, steps=(0, 1))
    assert _same_bits(outs[0], touts[0]) and _same_bits(outs[1], touts[1])
    _check_grads(model, got, [t0, t1], tacc)
    # ... and a third step after zero_grad overwrites again: nothing of the accumulated steps is left in the scratch
    _, again, _ = _train(model, case, steps=(0,))
    _check_grads(model, again, [t0], t0)


@pytest.mark.parametrize("name", ["topk_micro", "sit_micro"])
def test_freeze_attn_only_and_input_gradient(name):
    from tokenreduction_amd import finetune
    case, model, twin = _pair(name)
    names = finetune.freeze_attn_only(model)
    finetune.freeze_attn_only(twin)
    assert not any("gamma" in n for n in names) and "blocks.0.attn.proj.weight" in names
    outs, got, xg = _train(model, case, x_grad=True)
    touts, tg, txg = _train(twin, case, x_grad=True)
    assert _same_bits(outs[0], touts[0]) and xg is not None and torch.equal(xg, txg)
    _check_grads(model, got, [tg], tg, trainable=names)
    assert not any(".mlp.fc2." in n or "gamma" in n for n in got)
    # gamma alone trainable in a branch whose Linear is frozen: the pair still reaches the executor, only dgamma is written
    for p in model.parameters():
        p.requires_grad = False
    model.blocks[1].ls2.gamma.requires_grad = True
    model.head.weight.requires_grad = model.head.bias.requires_grad = True
    for p in twin.parameters():
        p.requires_grad = False
    for p in (twin.blocks[1].mlp.fc2.weight, twin.blocks[1].mlp.fc2.bias, twin.head.weight, twin.head.bias):
        p.requires_grad = True
    _, got, _ = _train(model, case)
    _, tg, _ = _train(twin, case)
    assert sorted(got) == ["blocks.1.ls2.gamma", "head.bias", "head.weight"]
    _check_grads(model, got, [tg], tg)


# -------------------------------------------------------------------------------------------------------------- stale-copy guard
def _fresh_copy(model, case, **extra):
    new = make_model(case, **extra).cuda()
    new.load_state_dict(model.state_dict(), strict=True)
    return new


@pytest.mark.parametrize("opt_name", ["FusedAdamW", "torch"])
@pytest.mark.parametrize("name,classes", [("deit_micro", 32), ("deit_micro", 16), ("topk_micro", 16), ("sit_micro", 16)])
def test_no_stale_operands_after_an_optimizer_step(name, classes, opt_name):
    from tokenreduction_amd.optim import FusedAdamW
    case = dict(GOLDEN_CASES[name], num_classes=classes)
    extra = dict(init_values=1e-6, no_embed_class=True)
    model = make_model(case, gamma_seed=5, **extra).cuda()
    x = _x(case)
    model.eval()
    before = model(x).clone()                                            # operands packed, graph captured
    opt = FusedAdamW(model.parameters(), lr=1e-2, weight_decay=0.05, model=model) if opt_name == "FusedAdamW" else \
        torch.optim.AdamW(model.parameters(), lr=1e-2, weight_decay=0.05, fused=True)
    for _ in range(2):                                                  # (the second step runs with the optimizer's table built)
        _train(model, case)
        opt.step()
    fresh = _fresh_copy(model, case, **extra)
    torch.manual_seed(9)
    want_train = _logits(fresh.train()(x)).detach().clone()
    torch.manual_seed(9)
    got_train = _logits(model.train()(x)).detach().clone()
    assert _same_bits(got_train, want_train)
    got, want = model.eval()(x), fresh.eval()(x)
    assert _same_bits(got, want) and not torch.equal(got, before)
    # a gamma edited in place + weights_changed(): the replayed graph follows
    with torch.no_grad():
        model.blocks[0].ls1.gamma.mul_(3.0)
        model.pos_embed.add_(0.01)
    model.weights_changed()
    fresh = _fresh_copy(model, case, **extra)
    got2, want2 = model(x), fresh.eval()(x)
    assert _same_bits(got2, want2) and not torch.equal(got2, got)


# ------------------------------------------------------------------------------------------------------------------ no_embed_class
@pytest.mark.parametrize("name", ["deit_micro", "tome_micro"])
@pytest.mark.parametrize("ls", [False, True])
def test_no_embed_class(name, ls):
    case, model, twin = _pair(name, no_embed_class=True, init_values=1e-6 if ls else None)
    P, D = model.patch_embed.num_patches, case["embed_dim"]
    assert tuple(model.pos_embed.shape) == (1, P, D) and tuple(twin.pos_embed.shape) == (1, P + 1, D)
    x = _x(case)
    for precision in ("bf16", "bf16x3", "fp32"):
        model.precision = twin.precision = precision
        assert _same_bits(model(x), twin(x)), precision
    model.precision = twin.precision = "bf16"
    outs, got, _ = _train(model, case, steps=(0, 1))
    touts, tacc, _ = _train(twin, case, steps=(0, 1))
    _, t0, _ = _train(twin, case, steps=(0,))
    _, t1, _ = _train(twin, case, steps=(1,))
    assert _same_bits(outs[1], touts[1])
    g = model.pos_embed.grad
    assert tuple(g.shape) == (1, P, D) and g.is_contiguous() and g.data_ptr() % 256 == 0
    assert torch.equal(g, tacc["pos_embed"][:, 1:]) and torch.equal(got["cls_token"], tacc["cls_token"])
    _check_grads(model, got, [t0, t1], tacc)


# ---------------------------------------------------------------------------------------------------------------- block ranges
def test_flat_grad_reducer_world1_gives_the_single_calls_gradients():
    import torch.distributed as dist
    from tokenreduction_amd.dp import FlatGradReducer
    case, model, _twin = _pair("topk_micro", no_embed_class=True)
    _, want, _ = _train(model, case)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29577")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        red = FlatGradReducer(bucket_bytes=256 * 1024).attach(model)
        recs = []
        model.train()
        model.zero_grad(set_to_none=True)
        torch.manual_seed(500)
        out = _logits(model(_x(case)))
        recs = _launches.labels(lambda: (out * _target(case, model)).sum().backward())
        torch.cuda.synchronize()
        assert len(red.launched) >= 2
        assert recs.count(UNFOLD) == len(red.launched)                 # one launch behind every block range
        for n, p in model.named_parameters():
            assert torch.equal(p.grad, want[n]), n
    finally:
        model._grad_reducer = None
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------ launch accounting
def _step_labels(model, case, opt):
    model.train()
    model.zero_grad(set_to_none=True)
    x, t = _x(case), _target(case, model)
    out = []
    fwd = _launches.labels(lambda: out.append(_logits(model(x))))
    bwd = _launches.labels(lambda: (out[0] * t).sum().backward())
    step = _launches.labels(opt.step)
    return fwd, bwd, step


def test_launch_accounting():
    from tokenreduction_amd.optim import FusedAdamW
    case = dict(GOLDEN_CASES["deit_micro"], num_classes=32)             # (a classifier large enough for the fused cast table)
    plain = make_model(case).cuda()
    model = make_model(case, gamma_seed=1, init_values=1e-6).cuda()
    for m, ls in ((plain, False), (model, True)):
        opt = FusedAdamW(m.parameters(), lr=1e-3, model=m)
        _step_labels(m, case, opt)                                       # first step: tables are built, the optimizer sees the pack table
        fwd, bwd, step = _step_labels(m, case, opt)
        fwd3, _bwd3, _step3 = _step_labels(m, case, opt)
        everything = fwd + bwd + step + fwd3
        if not ls:
            assert FOLD not in everything and UNFOLD not in everything
            assert _launches.labels(lambda: m.eval()(_x(case))).count(FOLD) == 0
            continue
        assert step.count(FOLD) == 1 and step.count("tr_adamw_step") == 1 and step.index(FOLD) > step.index("tr_adamw_step")
        assert bwd.count(UNFOLD) == 1 and FOLD not in bwd and UNFOLD not in fwd + step
        assert FOLD not in fwd3 and "tr_cast_pack_bf16" not in fwd3      # the step left every operand fresh: the next forward packs nothing
    # another optimizer: the refresh is the repack of the next forward -- one cast launch, one fold launch
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True)
    _step_labels(model, case, opt)
    fwd, bwd, _ = _step_labels(model, case, opt)
    assert fwd.count(FOLD) == 1 and fwd.count("tr_cast_pack_bf16") == 1 and bwd.count(UNFOLD) == 1


# ----------------------------------------------------------------------------------------------------- what must keep working
def _same_tree(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return sorted(a, key=str) == sorted(b, key=str) and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_tree(u, v) for u, v in zip(a, b))
    return a == b


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro", "sit_micro"])
def test_taps_decisions_pixels_and_copies(name):
    import copy
    case, model, twin = _pair(name, no_embed_class=True)
    x = _x(case)
    assert _same_tree(model.forward_taps(x, cls_blocks=(0, 2), final_tokens=True), twin.forward_taps(x, cls_blocks=(0, 2), final_tokens=True))
    assert _same_tree(model.forward_decisions(x), twin.forward_decisions(x))
    assert _same_tree(model.forward_async(x, cls_blocks=(1,), decisions=True).result(), twin.forward_async(x, cls_blocks=(1,), decisions=True).result())
    u8 = torch.randint(0, 256, tuple(x.shape), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).cuda()
    assert _same_bits(model.set_pixel_input()(u8), twin.set_pixel_input()(u8))
    ema = copy.deepcopy(model)                      # (ModelEma: a deep copy that is then driven through its state dict)
    ema.load_state_dict(model.state_dict())
    assert _same_bits(ema(u8), model(u8))


@pytest.mark.parametrize("extra", [dict(num_classes=0), dict(global_pool="avg"), dict(num_classes=0, global_pool="avg")])
def test_headless_and_average_pooled_heads(extra):
    case = dict(GOLDEN_CASES["topk_micro"])
    kw = {k: v for k, v in extra.items() if k != "num_classes"}
    if "num_classes" in extra:
        case["num_classes"] = 0
    model = make_model(case, gamma_seed=3, init_values=1e-6, no_embed_class=True, **kw).cuda()
    twin = folded_twin(model, case, **kw)
    x = _x(case)
    assert _same_bits(model(x), twin(x))
    outs, got, _ = _train(model, case)
    touts, tg, _ = _train(twin, case)
    assert _same_bits(outs[0], touts[0])
    _check_grads(model, got, [tg], tg)


@pytest.mark.parametrize("name", ["topk_micro_droppath", "topk_micro_dropout"])
def test_drop_path_and_dropout_commute_with_the_scale(name):
    case, model, twin = _pair(name)
    outs, got, _ = _train(model, case, steps=(0, 1))
    _, t0, _ = _train(twin, case, steps=(0,))
    _, t1, _ = _train(twin, case, steps=(1,))
    touts, tacc, _ = _train(twin, case, steps=(0, 1))
    assert _same_bits(outs[0], touts[0]) and _same_bits(outs[1], touts[1])
    _check_grads(model, got, [t0, t1], tacc)
