"""GPU, model level: global_pool='avg' -- the head (or a headless model's output) reads LayerNorm(weighted mean of the patch tokens after the
last block) instead of the final-normed CLS row -- in eval (three precisions), through every entry point, in training and its backward.

Expectations (tests/_pool_ref.py, fp64 on the CPU):
  * unweighted families (DeiT, Top-K, EViT, DPC-KNN, SiT): the same weights with CLS pooling and viz_mode give the stream after the last block,
    viz_data["Features"][depth-1]; the pooled model's stream is that stream bit for bit (asserted), so only pool, norm and head differ:
    LN(mean(Features[depth-1][:, 1:], 1)) -> head.  fp32 within 2e-5 (DPC-KNN 3e-5), bf16x3 within 1e-4 (DPC-KNN 2e-4): the bounds
    tests/test_headless_gpu.py holds headless features to; bf16 logits within relative L2 3e-2, tests/test_hip_model.py's teacher-forced bound.
  * ToMe (token sizes) and ATS (padding mask), fp32: the oracle's blocks composed into the final stream and the weights, 2e-5 -- given that
    the oracle and the device decided alike, which the test asserts.
  * training: one step (drop rates 0) against torch.autograd through the fp32 restatement with the HIP rounding points on the tape's
    decisions; logits relative L2 < 3e-2, gradients within grad_tol / 2 x grad_tol of tests/test_hip_train.py, x.grad within 2 x grad_tol of
    tests/test_input_grad_gpu.py.
Every test here fails without the feature (the attribute did not exist; reset_classifier ignored the argument)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import _launches, _pool_ref
from tests._params import GOLDEN_CASES, case_params, grad_labels, make_images
from tests.test_hip_model import FORCED_TOL, build_model
from tests.test_hip_train import _rel, grad_tol

pytestmark = pytest.mark.gpu

UNWEIGHTED = ["deit_micro", "topk_micro", "evit_micro", "dpcknn_micro", "sit_micro", "topk_small_kr07"]          # the last one: DeiT-S width
ABS_TOL = {"fp32": (2e-5, 3e-5), "bf16x3": (1e-4, 2e-4)}          # (every family, DPC-KNN): tests/test_headless_gpu.py
LAUNCH_CASES = ["deit_micro", "topk_micro", "tome_micro", "deit_small"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _model(case, pool="avg", viz=False, precision="bf16", **over):
    m, params, cfg = build_model(dict(case, **over))
    m.global_pool = pool
    m.viz_mode = viz
    m.precision = precision
    if hasattr(m, "density_noise"):          # DPC-KNN draws its density noise per forward: the same (zero) draws for every model of a test
        m.density_noise = {blk: torch.zeros(case["batch"], P) for blk, _, P in m._stage_shapes()}
    return m, params, cfg


def _image(case):
    return make_images(case["batch"], case.get("img_size", 224), case["xseed"]).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ eval, unweighted families
@pytest.fixture(scope="module")
def cls_streams():
    """{(case, precision): (Features[depth-1] of the CLS-pooled model under viz_mode, its params)}: computed once, shared, never written."""
    return {}


def _cls_stream(cache, name, precision):
    if (name, precision) not in cache:
        case = GOLDEN_CASES[name]
        cl, params, cfg = _model(case, pool="", viz=True, precision=precision)
        _, viz = cl(_image(case))
        cache[(name, precision)] = (viz["Features"][cfg.depth - 1].copy(), params, cfg)
    return cache[(name, precision)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", UNWEIGHTED)
def test_eval_matches_the_pooled_cls_stream(cls_streams, name, precision):
    case = GOLDEN_CASES[name]
    feats, params, cfg = _cls_stream(cls_streams, name, precision)
    x = _image(case)
    av, _, _ = _model(case, viz=True, precision=precision)
    logits, viz = av(x)
    np.testing.assert_array_equal(viz["Features"][cfg.depth - 1], feats)           # the stream does not know how it will be pooled
    av.viz_mode = False
    assert torch.equal(_bits(av(x)), _bits(logits))
    pooled = _pool_ref.pool(torch.from_numpy(feats))
    want = _pool_ref.norm_head(pooled, params, cfg.ln_eps)
    av.reset_classifier(0)                                                          # headless: the pooling stays, the output is feat
    assert av.global_pool == "avg"
    f = av(x)
    want_f = _pool_ref.norm_head(pooled, params, cfg.ln_eps, headless=True)
    assert f.shape == want_f.shape == (case["batch"], case["embed_dim"]) and f.dtype == torch.float32
    dl, df = (logits.cpu().double() - want).abs().max().item(), (f.cpu().double() - want_f).abs().max().item()
    rl, rf = _rel(logits.cpu(), want), _rel(f.cpu(), want_f)
    print(f"\n[{name}] {precision}: max|logits - expected| = {dl:.2e} (rel L2 {rl:.2e}), max|feat - expected| = {df:.2e} (rel L2 {rf:.2e}); "
          f"|feat| <= {want_f.abs().max().item():.2f}")
    if precision == "bf16":
        assert rl < FORCED_TOL and rf < FORCED_TOL, (rl, rf)
    else:
        tol = ABS_TOL[precision][1 if case["family"] == "dpcknn" else 0]
        assert dl <= tol and df <= tol, (dl, df)
    # ... and the check tells the two poolings apart: the CLS head's logits miss the bound the pooled ones were just held to
    cl, _, _ = _model(case, pool="token", precision=precision)
    c = cl(x).cpu()
    if precision == "bf16":
        assert _rel(c, want) > FORCED_TOL
    else:
        assert (c.double() - want).abs().max().item() > tol


# ----------------------------------------------------------------------------------------------------------- eval, ToMe and ATS (weighted)
def _same_ids(a, b):
    """Two id tables with -1 padding, possibly of different width."""
    a, b = np.asarray(a), np.asarray(b)
    w = max(a.shape[1], b.shape[1])
    pad = lambda t: np.pad(t, ((0, 0), (0, w - t.shape[1])), constant_values=-1)
    return a.shape[0] == b.shape[0] and bool((pad(a) == pad(b)).all())


@pytest.mark.parametrize("name", ["tome_micro", "ats_micro"])
def test_eval_weighted_pool_matches_the_oracle_composition(name):
    case = GOLDEN_CASES[name]
    av, params, cfg = _model(case, viz=True, precision="fp32")
    x = _image(case)
    logits, viz = av(x)
    want, dec = _pool_ref.pooled_logits(params, x.cpu(), cfg)
    assert dec, "the fixture reduces tokens"
    if case["family"] == "tome":          # the same merges: the oracle's Assignment_Maps are the device's
        assert sorted(viz["Assignment_Maps"]) == sorted(dec)
        for blk, a in dec.items():
            np.testing.assert_array_equal(viz["Assignment_Maps"][blk], a.numpy())
    else:                                  # the same samples (ids [B, K]: CLS id 0 first, 0 = padding -> Kept_Tokens = ids[:, 1:] - 1)
        assert sorted(viz["Kept_Tokens"]) == sorted(dec)
        for blk, ids in dec.items():
            assert _same_ids(viz["Kept_Tokens"][blk], (ids[:, 1:] - 1).numpy()), f"block {blk}: the oracle and the device sampled other ids"
        assert any(bool((ids[:, 1:] == 0).any()) for ids in dec.values()), "the fixture pads no row: the mask would not matter"
    d = (logits.cpu().double() - want).abs().max().item()
    # the weights matter: an unweighted mean of the same stream is somewhere else
    h, w, _ = _pool_ref.final_stream(params, x.cpu(), cfg)
    plain = _pool_ref.norm_head(_pool_ref.pool(h), params, cfg.ln_eps)
    print(f"\n[{name}] fp32: max|logits - expected| = {d:.2e}; |expected - unweighted| = {(plain - want).abs().max().item():.2e}")
    assert d <= 2e-5, d
    assert (plain - want).abs().max().item() > 100 * 2e-5
    av.reset_classifier(0)
    av.viz_mode = False
    want_f, _ = _pool_ref.pooled_logits(params, x.cpu(), cfg, headless=True)
    df = (av(x).cpu().double() - want_f).abs().max().item()
    assert df <= 2e-5, df


@pytest.mark.parametrize("precision", ["bf16", "fp32", "bf16x3"])
def test_tome_that_merges_nothing_is_the_dense_model(precision):
    case = GOLDEN_CASES["tome_micro"]
    tome, _, _ = _model(case, precision=precision, keep_rate=[1.0])
    deit, _, _ = _model(case, precision=precision, family="deit", keep_rate=[1.0], reduction_loc=[])
    x = _image(case)
    a, b = tome(x), deit(x)
    assert tome._last_tokens == deit._last_tokens == [197] * case["depth"]
    assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------ headless and pooled
@pytest.mark.parametrize("name", ["topk_micro", "tome_micro", "ats_micro"])
def test_headless_pooled_features_are_the_identity_heads_operand(name):
    case = GOLDEN_CASES[name]
    D = case["embed_dim"]
    hl, _, _ = _model(case, num_classes=D)
    hl.reset_classifier(0, global_pool="avg")
    cl, _, _ = _model(case, num_classes=D)
    with torch.no_grad():
        cl.head.weight.copy_(torch.eye(D))
        cl.head.bias.zero_()
    x = _image(case)
    f, l = hl(x), cl(x)
    assert f.shape == (case["batch"], D)
    assert torch.equal(l, f.bfloat16().float()) and not torch.equal(f, f.bfloat16().float())
    hl.precision = cl.precision = "fp32"
    f32, l32 = hl(x), cl(x)
    assert torch.equal(_bits(l32), _bits(f32))
    hl.precision = cl.precision = "bf16x3"
    f3, l3 = hl(x), cl(x)
    assert bool(((l3 - f3).abs() <= 1e-5 * f3.abs()).all())


# --------------------------------------------------------------------------------------------------------- the same bits, every entry point
@pytest.mark.parametrize("name", ["deit_micro", "topk_micro", "tome_micro", "ats_micro", "deit_small"])
def test_entry_points_agree_bit_for_bit(name):
    case = GOLDEN_CASES[name]
    depth = case["depth"]
    av, _, _ = _model(case)
    cl, _, _ = _model(case, pool="")
    x = _image(case)
    first = av(x)                                                   # plain launches (the workspace's first forward) ...
    assert torch.equal(_bits(av(x)), _bits(first))                  # ... then a captured graph ...
    assert torch.equal(_bits(av(x)), _bits(first))                  # ... replayed
    av.use_graph = False
    assert torch.equal(_bits(av(x)), _bits(first))
    av.use_graph = True
    h1, h2 = av.forward_async(x), av.forward_async(x)               # two in flight, each on its own workspace
    assert torch.equal(_bits(h1.result()), _bits(first)) and torch.equal(_bits(h2.result()), _bits(first))
    logits, taps = av.forward_taps(x, cls_blocks=(depth - 1,), final_tokens=True)
    assert torch.equal(_bits(logits), _bits(first))
    c_logits, c_taps = cl.forward_taps(x, cls_blocks=(depth - 1,), final_tokens=True)
    assert not torch.equal(c_logits, first)
    assert torch.equal(_bits(taps["cls"]), _bits(c_taps["cls"]))                    # a CLS tap stays the CLS row of the stream
    assert torch.equal(_bits(taps["final_tokens"]), _bits(c_taps["final_tokens"]))  # final_tokens stays the norm of every row
    logits2, taps2 = av.forward_taps(x, cls_blocks=(0, depth - 1))                  # without final_tokens: still no CLS tail under the pool
    assert torch.equal(_bits(logits2), _bits(first)) and torch.equal(_bits(taps2["cls"][:, 1]), _bits(taps["cls"][:, 0]))
    out = av.forward_decisions(x)
    assert torch.equal(_bits(out[0]), _bits(first))
    h3 = av.forward_async(x, cls_blocks=(depth - 1,), decisions=True).result()
    assert torch.equal(_bits(h3[0]), _bits(first)) and torch.equal(_bits(h3[1]["cls"]), _bits(taps["cls"]))
    av.viz_mode = True
    assert torch.equal(_bits(av(x)[0]), _bits(first))
    av.viz_mode = False
    # uint8 pixels: normalized inside the patch embedding, bitwise as if the normalized fp32 image had been passed
    from tokenreduction_amd import pixels
    u8 = torch.randint(0, 256, (case["batch"], 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    av.set_pixel_input()
    lut = pixels.pixel_lut(*av.pixel_input).cuda()
    xf = torch.stack([lut[c][u8[:, c].long()] for c in range(3)], dim=1)
    assert torch.equal(_bits(av(u8)), _bits(av(xf)))
    # switching the pooling on one model: no stale workspace or graph
    av.set_pixel_input(None)
    av.reset_classifier(case["num_classes"], global_pool="")
    cl2, _, _ = _model(case, pool="")
    cl2.head.load_state_dict(av.head.state_dict())
    assert torch.equal(_bits(av(x)), _bits(cl2(x)))


# ----------------------------------------------------------------------------------------------------------------- the unchanged default
def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("name", LAUNCH_CASES)
def test_default_pooling_launches_and_bits_are_the_recorded_ones(golden_dir, name):
    """tests/golden/avg_pool_default.json: the launch labels (tests/_launches.forward_launches, tr_set_cls_tail untouched) and the sha256 of
    the logits of the CLS-pooled model, recorded on the commit before global_pool existed."""
    from tokenreduction_amd import ops
    rec = json.load(open(os.path.join(golden_dir, "avg_pool_default.json")))[name]
    case = GOLDEN_CASES[name]
    x = _image(case)
    cl, _, _ = _model(case, pool="")
    labels = [r[0] for r in _launches.forward_launches(cl, x)]
    assert labels == rec["labels"]
    assert _digest(cl(x)) == rec["logits_sha256"]
    tok, _, _ = _model(case, pool="token")
    assert [r[0] for r in _launches.forward_launches(tok, x)] == rec["labels"] and _digest(tok(x)) == rec["logits_sha256"]
    av, _, _ = _model(case)
    pooled = [r[0] for r in _launches.forward_launches(av, x)]
    assert pooled.count("tr_token_pool") == 1 and not any("<cls>" in l for l in pooled)          # no CLS-tail launch (attention_kernel<cls>)
    # what the pooled forward costs: the full-width last block (the CLS forward with its CLS tail off) plus the one pool launch
    was = ops.set_cls_tail(False)
    try:
        full, _, _ = _model(case, pool="")
        full_labels = [r[0] for r in _launches.forward_launches(full, x)]
    finally:
        ops.set_cls_tail(was)
    i = pooled.index("tr_token_pool")
    assert pooled[:i] + pooled[i + 1:] == full_labels
    assert "tr_token_pool" not in labels


# ------------------------------------------------------------------------------------------------------------------------------ training
def _train_model(case, pool="avg"):
    m, params, cfg = _model(case, pool=pool)
    m.train()
    return m, params, cfg


def _step(case, model, x):
    model.zero_grad(set_to_none=True)
    x.grad = None
    logits = model(x)
    loss = torch.nn.functional.cross_entropy(logits, grad_labels(case).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), loss.item(), {n: None if p.grad is None else p.grad.clone() for n, p in model.named_parameters()}, \
        None if x.grad is None else x.grad.clone()


@pytest.fixture(scope="module")
def train_steps():
    return {}


def _full_step(cache, name):
    """One pooled training step of the case, every parameter and the image taking a gradient: computed once, shared, never written."""
    if name not in cache:
        from tokenreduction_amd import training
        case = GOLDEN_CASES[name]
        model, params, cfg = _train_model(case)
        x = _image(case).requires_grad_(True)
        logits, loss, grads, dx = _step(case, model, x)
        decisions = training.train_decisions(model)
        forced = {blk: (tuple(t.cpu() for t in d) if isinstance(d, tuple) else d.cpu()) for blk, d in decisions.items()}
        cache[name] = dict(model=model, params=params, cfg=cfg, x=x, logits=logits, loss=loss, grads=grads, dx=dx, forced=forced)
    return cache[name]


@pytest.mark.parametrize("name", ["deit_micro", "topk_micro", "tome_micro", "ats_micro"])
def test_training_step_matches_autograd_on_the_tape_decisions(train_steps, name):
    case = GOLDEN_CASES[name]
    s = _full_step(train_steps, name)
    o_loss, o_logits, o_grads, o_dx = _pool_ref.autograd_step(s["params"], s["x"].detach().cpu(), s["cfg"], grad_labels(case), s["forced"] or None)
    rl = _rel(s["logits"].cpu(), o_logits)
    gnorm = float(torch.cat([g.reshape(-1) for g in o_grads.values()]).double().norm())
    errs = []
    for n, g in s["grads"].items():
        assert g is not None and bool(torch.isfinite(g).all()), n
        d = float((g.cpu().double() - o_grads[n].double()).norm())
        errs.append((d / max(float(o_grads[n].double().norm()), 1e-3 * gnorm), n))
    errs.sort(reverse=True)
    total = _rel(torch.cat([g.reshape(-1).cpu() for g in s["grads"].values()]), torch.cat([o_grads[n].reshape(-1) for n in s["grads"]]))
    rd = _rel(s["dx"].cpu(), o_dx)
    print(f"\n[{name}] loss {s['loss']:.5f} (restatement {o_loss:.5f}); logits rel L2 {rl:.3e}; gradients: whole-model rel L2 {total:.3e}, worst "
          f"{[(n, round(e, 4)) for e, n in errs[:4]]}; dx rel L2 {rd:.3e}")
    assert rl < FORCED_TOL, rl
    assert total < grad_tol(case), total
    assert errs[0][0] < 2 * grad_tol(case), errs[0]
    assert rd < 2 * grad_tol(case), rd
    assert float(s["grads"]["cls_token"].abs().max()) > 0          # the CLS token is not pooled but still feeds every attention
    # ... and the check tells the two heads apart: the CLS model's classifier gradient on the same batch
    cl, _, _ = _train_model(case, pool="")
    _, _, cgrads, _ = _step(case, cl, _image(case).requires_grad_(True))
    assert _rel(cgrads["head.weight"].cpu(), o_grads["head.weight"]) > 2 * grad_tol(case)          # it misses the bound held above


def test_training_logits_are_the_eval_models(train_steps):
    """No decision anywhere (DeiT): the training forward's pooled logits against the eval forward's, the two bf16 executors."""
    case = GOLDEN_CASES["deit_micro"]
    s = _full_step(train_steps, "deit_micro")
    ev, _, _ = _model(case)
    r = _rel(s["logits"].cpu(), ev(_image(case)).cpu())
    assert r < FORCED_TOL, r


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro"])
def test_head_only_probe_updates_only_the_head(train_steps, name):
    case = GOLDEN_CASES[name]
    s = _full_step(train_steps, name)
    model, _, _ = _train_model(case)
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("head.")
    x = _image(case)
    model.zero_grad(set_to_none=True)
    loss = torch.nn.functional.cross_entropy(model(x), grad_labels(case).cuda())
    labels = _launches.labels(loss.backward)
    torch.cuda.synchronize()
    assert "tr_token_pool_bwd" not in labels and len(labels) <= 6          # the classifier step alone
    for n, p in model.named_parameters():
        if n.startswith("head."):
            assert torch.equal(_bits(p.grad), _bits(s["grads"][n])), n
        else:
            assert p.grad is None, n
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.1).step()
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n]) != n.startswith("head."), n


def test_frozen_blocks_stop_the_walk_behind_the_final_norm(train_steps):
    """Head and final norm train, every block is frozen: the norm's backward runs on the pooled rows and nothing is spread over the tokens."""
    case = GOLDEN_CASES["topk_micro"]
    s = _full_step(train_steps, "topk_micro")
    model, _, _ = _train_model(case)
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith(("head.", "norm."))
    model.zero_grad(set_to_none=True)
    loss = torch.nn.functional.cross_entropy(model(_image(case)), grad_labels(case).cuda())
    labels = _launches.labels(loss.backward)
    torch.cuda.synchronize()
    assert "tr_token_pool_bwd" not in labels
    for n in ("head.weight", "head.bias", "norm.weight", "norm.bias"):
        assert torch.equal(_bits(dict(model.named_parameters())[n].grad), _bits(s["grads"][n])), n


class _BlockRanges:
    """What training._VitTrainFn.backward asks of a gradient reducer, without a process group: the backward runs as one tr_vit_backward call
    per block and nothing is reduced."""
    sync = True

    def plan(self, block_slices, depth):
        return [(blk, blk, 0, 0) for blk in range(depth - 1, -1, -1)]

    def begin(self, flat):
        self.launched = []

    def reduce_slice(self, flat, start, stop):
        self.launched.append((start, stop))

    def finish(self, flat):
        pass


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro", "ats_micro"])
def test_block_range_backward_is_the_single_call_bit_for_bit(train_steps, name):
    case = GOLDEN_CASES[name]
    s = _full_step(train_steps, name)
    model, _, _ = _train_model(case)
    model._grad_reducer = red = _BlockRanges()
    try:
        logits, loss, grads, dx = _step(case, model, _image(case).requires_grad_(True))
    finally:
        model._grad_reducer = None
    assert len(red.launched) == case["depth"]
    assert torch.equal(_bits(logits), _bits(s["logits"])) and torch.equal(_bits(dx), _bits(s["dx"]))
    for n, g in grads.items():
        assert torch.equal(_bits(g), _bits(s["grads"][n])), n


def test_headless_pooled_training(train_steps):
    """num_classes = 0: the features carry the upstream gradient; against the same restatement, and the launches of the pooled backward."""
    case = GOLDEN_CASES["tome_micro"]
    from tokenreduction_amd import training
    model, params, cfg = _train_model(case)
    model.reset_classifier(0)
    x = _image(case).requires_grad_(True)
    G = torch.randn(case["batch"], case["embed_dim"], generator=torch.Generator().manual_seed(4)).cuda()
    f = model(x)
    labels = _launches.labels(lambda: f.backward(G))
    torch.cuda.synchronize()
    assert labels.count("tr_token_pool_bwd") == 1
    forced = {blk: tuple(t.cpu() for t in d) for blk, d in training.train_decisions(model).items()}
    params = {k: v for k, v in params.items() if not k.startswith("head.")}
    _, o_f, o_grads, o_dx = _pool_ref.autograd_step(params, x.detach().cpu(), cfg, None, forced, headless_grad=G.cpu())
    assert _rel(f.detach().cpu(), o_f) < FORCED_TOL
    total = _rel(torch.cat([p.grad.reshape(-1).cpu() for _, p in model.named_parameters()]),
                 torch.cat([o_grads[n].reshape(-1) for n, _ in model.named_parameters()]))
    assert total < grad_tol(case), total
    assert _rel(x.grad.cpu(), o_dx) < 2 * grad_tol(case)


def test_dyvit_pools_in_eval_and_refuses_in_training():
    case = GOLDEN_CASES["dyvit_micro"]
    cl, params, cfg = _model(case, pool="", viz=True, precision="fp32")
    x = _image(case)
    _, viz = cl(x)
    av, _, _ = _model(case, precision="fp32")
    want = _pool_ref.norm_head(_pool_ref.pool(torch.from_numpy(viz["Features"][cfg.depth - 1])), params, cfg.ln_eps)
    d = (av(x).cpu().double() - want).abs().max().item()
    assert d <= 2e-5, d                                                              # eval removes tokens: pooled like Top-K
    av.precision = "bf16"
    av.train()
    with pytest.raises(NotImplementedError, match="DyViT in train mode"):
        av(x)
