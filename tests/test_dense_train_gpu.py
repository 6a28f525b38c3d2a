"""Dense feature maps in training at model level (model.forward_dense_train), GPU tier, on the micro fixtures of every family but DyViT.

Forward: `out` is model(x)'s in train mode bit for bit; the index is the numpy composition (tests/_decisions_ref.py, tests/_dense_ref.py) of
the decisions read back from the TAPE on the host (the slabs the executor copied on the device are not looked at; the soft families'
assignments are not on the tape in slab form: theirs are the soft output the forward wrote); the map is the restated gather of the token
rows the same forward wrote; against the oracle -- LayerNorm(viz["Final_Tokens"]) of the undecorated oracle forward with the HIP rounding
points and the device's decisions, gathered by the device's index -- the patch rows hold the logits' bound of tests/test_hip_train.py.
Gradients: torch autograd over that oracle forward, for cross_entropy(out) + (features * G).sum() and for the map term alone, under
tests/test_hip_train.py's bounds: grad_tol(case) on the whole gradient vector, twice that on the worst parameter (floor: 1e-3 of the whole
norm), twice that on x.grad.  G is seeded N(0, 1) / (B * P0): the map term is then a mean over images and patches like the cross-entropy
is a mean over images, and the token gradients of the two terms have the same order of magnitude (about sqrt(D / (B * P0)) against about
1 / sqrt(B) at the logits), so neither hides the other."""
import numpy as np
import pytest
import torch

from tests import _decisions_ref as dref
from tests import _dense_ref as ref
from tests import _launches, _pool_ref
from tests._params import GOLDEN_CASES, grad_labels, make_images
from tests.test_avg_pool_gpu import _BlockRanges
from tests.test_hip_model import FORCED_TOL, build_model
from tests.test_hip_train import _noise, _rel, grad_tol

pytestmark = pytest.mark.gpu

CASES = ["topk_micro", "evit_micro", "tome_micro", "dpcknn_micro", "ats_micro", "kmedoids_micro", "sit_micro", "sinkhorn_micro",
         "patchmerger_micro", "deit_micro"]
DX_CASES = ("topk_micro", "tome_micro")
FILL = -7.5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def steps():
    return {}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _image(case):
    return make_images(case["batch"], case.get("img_size", 224), case["xseed"]).cuda()


def _train_model(case, noise=None, pool="", headless=False):
    m, params, cfg = build_model(case)
    m.viz_mode = False
    if pool:
        m.global_pool = pool
    if headless:
        m.reset_classifier(0)
        params = {k: v for k, v in params.items() if not k.startswith("head.")}
    if noise is not None:
        m.density_noise = noise                                  # DPC-KNN: the recorded density draws, the same for every forward
    m.train()
    return m, params, cfg


def _map_weights(case, model):
    B, D, P0 = case["batch"], model.embed_dim, model.patch_embed.num_patches
    g = torch.Generator().manual_seed(case["xseed"] + 23)
    return torch.randn(B, D, P0, generator=g) / (B * P0)


def _head_loss(case, out, G_out):
    """The term on `out`: cross-entropy on logits, a seeded linear form on a headless model's features."""
    if G_out is not None:
        return (out * G_out.to(out.device)).sum()
    return torch.nn.functional.cross_entropy(out, grad_labels(case).to(out.device))


def _tape_slabs(model):
    """The decision slots of the tape as the eval slab format, read back on the host: (kept, compl) int32 [depth * B * N0]."""
    from tokenreduction_amd import training
    st = model._train_state()
    n = st.B * (model.patch_embed.num_patches + 1)
    kept, compl = np.full(model.depth * n, -77, np.int32), np.full(model.depth * n, -77, np.int32)
    for blk in range(model.depth):
        lay = training.tape_layout(model, blk)
        if lay["kk"] > 0:
            kept[blk * n: (blk + 1) * n] = st.tape[lay["idx"]: lay["idx"] + 4 * n].view(torch.int32).cpu().numpy()
            compl[blk * n: (blk + 1) * n] = st.tape[lay["idx2"]: lay["idx2"] + 4 * n].view(torch.int32).cpu().numpy()
    return kept, compl


def _grads(model):
    return {n: None if p.grad is None else p.grad.detach().clone() for n, p in model.named_parameters()}


def _device_step(case, model, x, G, G_out, head_term=True):
    model.zero_grad(set_to_none=True)
    x.grad = None
    out, dense = model.forward_dense_train(x, fill=FILL)
    loss = (dense["features"].reshape(G.shape) * G).sum()
    if head_term:
        loss = loss + _head_loss(case, out, G_out)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), dense, _grads(model), None if x.grad is None else x.grad.detach().clone()


def _oracle_stream(case, leaves, img, cfg, forced, noise):
    """(out or None, h): the oracle's logits and the stream entering the final norm, bf16 rounding points, the device's decisions."""
    import oracle
    fam = case["family"]
    if fam == "kmedoids":
        return oracle.kmedoids_forward.__wrapped__(leaves, img, cfg, "bf16", True, 3, forced)
    if fam == "tome":
        return oracle.tome_forward.__wrapped__(leaves, img, cfg, "bf16", True, forced)
    if fam == "dpcknn":
        return oracle.dpcknn_forward.__wrapped__(leaves, img, cfg, noise, "bf16", True, forced)
    if fam == "ats":
        return oracle.ats_forward.__wrapped__(leaves, img, cfg, "bf16", True, False, forced)
    if fam in ("sit", "patchmerger", "sinkhorn"):
        return getattr(oracle, fam + "_forward").__wrapped__(leaves, img, cfg, "bf16", True)
    return oracle.vit_forward.__wrapped__(leaves, img, cfg, "bf16", True, forced)


def oracle_step(case, params, cfg, x, forced, noise, index, G, G_out=None, pool=""):
    """torch autograd over the oracle forward: {"out", "rows", "mixed": (grads, dx), "map": (grads, dx)}.  rows [B, P0, D] are the oracle's
    final-normed rows gathered by the device's index (FILL where it is negative)."""
    from oracle import vit as ovit
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    img = x.detach().cpu().to(torch.float32).clone().requires_grad_(True)
    index = torch.as_tensor(index).long()
    with torch.enable_grad():
        if pool or G_out is not None:                            # the head variants (Top-K): the head restated on the block composition
            h, w, _ = _pool_ref.final_stream(leaves, img, cfg, "bf16", forced)
            assert w is None
            D = h.shape[-1]
            first = h[:, 1:].mean(1) if pool else h[:, 0]
            if G_out is not None:
                out = torch.nn.functional.layer_norm(first, (D,), leaves["norm.weight"], leaves["norm.bias"], cfg.ln_eps)
            else:
                out = ovit.layer_norm(first, leaves["norm.weight"], leaves["norm.bias"], cfg.ln_eps, "bf16") @ ovit.round_bf16(leaves["head.weight"]).t() \
                    + leaves["head.bias"]
        else:
            out, viz = _oracle_stream(case, leaves, img, cfg, forced, noise)
            h = viz["Final_Tokens"]
        D = h.shape[-1]
        normed = torch.nn.functional.layer_norm(h, (D,), leaves["norm.weight"], leaves["norm.bias"], cfg.ln_eps)      # fp32, like tokens_out
        rows = torch.gather(normed, 1, index.clamp_min(0)[:, :, None].expand(-1, -1, D))
        rows = torch.where((index >= 0)[:, :, None], rows, torch.full_like(rows, FILL))
        map_term = (rows.permute(0, 2, 1) * G).sum()
        result = {"out": out.detach(), "rows": rows.detach()}
        names = list(leaves)
        for key, loss in (("mixed", map_term + _head_loss(case, out, G_out)), ("map", map_term)):
            gs = torch.autograd.grad(loss, [leaves[n] for n in names] + [img], retain_graph=True, allow_unused=True)
            grads = {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, gs[:-1])}
            result[key] = (grads, gs[-1])
    return result


def _full(cache, name, pool="", headless=False, golden_dir=None):
    """Device steps (mixed loss, map loss) and the oracle's of one case: computed once, shared, never written."""
    key = (name, pool, headless)
    if key in cache:
        return cache[key]
    from tokenreduction_amd import training
    case = GOLDEN_CASES[name]
    noise = _noise(case, golden_dir) if case["family"] == "dpcknn" else None
    model, params, cfg = _train_model(case, noise, pool, headless)
    x = _image(case)
    if name in DX_CASES:
        x.requires_grad_(True)
    B, D, P0 = case["batch"], model.embed_dim, model.patch_embed.num_patches
    G = _map_weights(case, model)
    G_out = torch.randn(B, D, generator=torch.Generator().manual_seed(4)) if headless else None
    plain = model(x).detach().clone()                            # the plain training forward first: same noise, same bits
    out, dense, grads, dx = _device_step(case, model, x, G.cuda(), G_out)
    st = model._train_state()
    n_last = model._last_tokens[-1]
    tokens = st.dense["tokens"][:B * n_last * D].view(B, n_last, D).cpu().numpy()
    soft = st.dense["plan"]["soft"]
    kept, compl = _tape_slabs(model)
    decisions = training.train_decisions(model)
    forced = {blk: (tuple(t.cpu() for t in d) if isinstance(d, tuple) else d.cpu()) for blk, d in decisions.items()}
    _, _, grads_map, dx_map = _device_step(case, model, x, G.cuda(), G_out, head_term=False)
    o = oracle_step(case, params, cfg, x, forced or None, noise, dense["index"].cpu(), G, G_out, pool)
    cache[key] = dict(case=case, model=model, x=x, G=G, G_out=G_out, plain=plain, out=out, dense=dense, grads=grads, dx=dx, grads_map=grads_map,
                      dx_map=dx_map, tokens=tokens, n_last=n_last, kept=kept, compl=compl, soft=None if soft is None else soft.cpu().numpy(),
                      oracle=o)
    return cache[key]


def _check_grads(what, case, grads, dx, o_grads, o_dx):
    names = list(grads)
    gnorm = float(torch.cat([o_grads[n].reshape(-1) for n in names]).double().norm())
    errs = []
    for n in names:
        assert grads[n] is not None and bool(torch.isfinite(grads[n]).all()), n
        d = float((grads[n].cpu().double() - o_grads[n].double()).norm())
        errs.append((d / max(float(o_grads[n].double().norm()), 1e-3 * gnorm), n))
    errs.sort(reverse=True)
    total = _rel(torch.cat([grads[n].reshape(-1).cpu() for n in names]), torch.cat([o_grads[n].reshape(-1) for n in names]))
    rd = None if dx is None else _rel(dx.cpu(), o_dx)
    print(f"\n[{what}] gradients: whole-model rel L2 {total:.3e}, worst {[(n, round(e, 4)) for e, n in errs[:4]]}; dx rel L2 {rd}")
    assert total < grad_tol(case), (what, total)
    assert errs[0][0] < 2 * grad_tol(case), (what, errs[0])
    if dx is not None:
        assert rd < 2 * grad_tol(case), (what, rd)


@pytest.mark.parametrize("name", CASES)
def test_forward_is_the_plain_training_forward_plus_the_restated_map(steps, golden_dir, name):
    s = _full(steps, name, golden_dir=golden_dir)
    case, model, dense = s["case"], s["model"], s["dense"]
    B, D = case["batch"], model.embed_dim
    h, w = model.patch_embed.grid_size
    P0 = h * w
    assert torch.equal(_bits(s["out"]), _bits(s["plain"]))
    assert dense["grid"] == (h, w) and dense["features"].shape == (B, D, h, w) and dense["features"].dtype == torch.float32
    assert dense["index"].shape == (B, P0) and dense["index"].dtype == torch.int32 and not dense["index"].requires_grad
    assert dense["features"].requires_grad
    # the index: the tape's decisions composed on the host
    stages = model._decision_stages()
    dec = dref.stage_decisions(s["kept"], s["compl"], s["soft"], stages, B, P0 + 1)
    index = ref.dense_index(dec, stages, B, P0, s["n_last"])
    np.testing.assert_array_equal(dense["index"].cpu().numpy(), index)
    family = case["family"]
    if family == "deit":
        assert not stages and (index == np.arange(1, P0 + 1)).all()
    elif family in ("topk", "evit", "ats"):
        assert (index < 0).any()
    else:
        assert (index >= 1).all()
    # the map: the restated gather of the rows this forward wrote
    want = ref.dense_gather(s["tokens"], index, "NCHW", "fp32", FILL)
    np.testing.assert_array_equal(dense["features"].detach().cpu().numpy().reshape(B, D, P0).view(np.uint32), want.view(np.uint32))
    # against the oracle: out, and the patch rows that have a row
    o = s["oracle"]
    assert _rel(s["out"].cpu(), o["out"]) < FORCED_TOL
    got = dense["features"].detach().cpu().reshape(B, D, P0).permute(0, 2, 1)
    has = torch.from_numpy(index >= 0)
    r = _rel(got[has], o["rows"][has])
    print(f"\n[{name}] out rel L2 {_rel(s['out'].cpu(), o['out']):.3e}; patch rows rel L2 {r:.3e} ({int(has.sum())} of {has.numel()} patches have a row)")
    assert r < 3e-2, r
    assert (got[~has] == FILL).all()


def test_out_and_the_map_are_two_outputs_of_one_autograd_node():
    model, _, _ = _train_model(GOLDEN_CASES["topk_micro"])
    out, dense = model.forward_dense_train(_image(GOLDEN_CASES["topk_micro"]))
    assert out.grad_fn is not None and out.grad_fn is dense["features"].grad_fn and "_VitTrainFn" in type(out.grad_fn).__name__
    assert dense["index"].grad_fn is None and not dense["index"].requires_grad


@pytest.mark.parametrize("name", CASES)
def test_gradients_of_the_mixed_loss_and_of_the_map_alone_match_autograd_over_the_oracle(steps, golden_dir, name):
    s = _full(steps, name, golden_dir=golden_dir)
    o = s["oracle"]
    _check_grads(name + " mixed", s["case"], s["grads"], s["dx"], *o["mixed"])
    _check_grads(name + " map", s["case"], s["grads_map"], s["dx_map"], *o["map"])
    assert (s["dx"] is not None) == (name in DX_CASES)
    # the two losses differ where the head's gradient goes: the map alone gives the classifier none
    if "head.weight" in s["grads_map"]:
        assert float(s["grads_map"]["head.weight"].abs().max()) == 0 and float(s["grads"]["head.weight"].abs().max()) > 0


@pytest.mark.parametrize("pool,headless", [("avg", False), ("", True)])
def test_head_variants(steps, golden_dir, pool, headless):
    s = _full(steps, "topk_micro", pool, headless, golden_dir)
    o = s["oracle"]
    assert torch.equal(_bits(s["out"]), _bits(s["plain"])) and _rel(s["out"].cpu(), o["out"]) < FORCED_TOL
    assert s["out"].shape[1] == (s["model"].embed_dim if headless else s["case"]["num_classes"])
    what = f"topk_micro pool={pool!r} headless={headless}"
    _check_grads(what + " mixed", s["case"], s["grads"], s["dx"], *o["mixed"])
    _check_grads(what + " map", s["case"], s["grads_map"], s["dx_map"], *o["map"])


def test_frozen_trunk_the_map_still_reaches_the_final_norm(steps, golden_dir):
    s = _full(steps, "topk_micro", golden_dir=golden_dir)
    case = s["case"]
    model, _, _ = _train_model(case)
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("norm.")
    x = _image(case)
    _, dense = model.forward_dense_train(x, fill=FILL)
    loss = (dense["features"].reshape(s["G"].shape) * s["G"].cuda()).sum()
    labels = _launches.labels(loss.backward)
    torch.cuda.synchronize()
    # the scatter, then the final norm's backward twice (the CLS rows', whose gradient is zero here, and the pass over every row)
    assert labels.count("tr_dense_scatter") == 1 and labels.count("ln_bwd_kernel") == 2, labels
    assert not [l for l in labels if "gemm" in l or "attention" in l or "linear_bwd" in l], labels      # no block kernel
    o_grads = s["oracle"]["map"][0]
    for n, p in model.named_parameters():
        if n.startswith("norm."):
            assert _rel(p.grad.cpu(), o_grads[n]) < 2 * grad_tol(case), n
            # the trunk's gradient does not feed the norm's parameters: the full step's map-only gradient is the same work
            assert _rel(p.grad, s["grads_map"][n]) < 1e-5, n
        else:
            assert p.grad is None, n


def test_two_dense_micro_steps_accumulate(steps, golden_dir):
    s = _full(steps, "tome_micro", golden_dir=golden_dir)
    case, G = s["case"], s["G"].cuda()
    model, _, _ = _train_model(case)
    x = _image(case)

    def micro(shift, head):
        out, dense = model.forward_dense_train(x + shift, fill=FILL)
        loss = (dense["features"].reshape(G.shape) * G).sum()
        (loss + _head_loss(case, out, None) if head else loss).backward()

    singles = []
    for shift, head in ((0.0, True), (0.25, False)):
        model.zero_grad(set_to_none=True)
        micro(shift, head)
        singles.append(_grads(model))
    model.zero_grad(set_to_none=True)
    micro(0.0, True)
    micro(0.25, False)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        want = singles[0][n] + singles[1][n]
        # the accumulate path adds in fp32 where the fresh path writes: two roundings of values of the sum's size (test_hip_train.py's rtol)
        assert torch.allclose(p.grad, want, rtol=1e-5, atol=1e-7 + 2.0 ** -22 * float(want.abs().max())), n


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro"])
def test_block_range_backward_is_the_single_call_bit_for_bit(steps, golden_dir, name):
    s = _full(steps, name, golden_dir=golden_dir)
    case = s["case"]
    model, _, _ = _train_model(case)
    model._grad_reducer = red = _BlockRanges()
    try:
        out, _, grads, dx = _device_step(case, model, _image(case).requires_grad_(True), s["G"].cuda(), None)
    finally:
        model._grad_reducer = None
    assert len(red.launched) == case["depth"]
    assert torch.equal(_bits(out), _bits(s["out"])) and torch.equal(_bits(dx), _bits(s["dx"]))
    for n, g in grads.items():
        assert torch.equal(_bits(g), _bits(s["grads"][n])), n


def test_other_layout_other_dtype_and_no_map_gradient(steps, golden_dir):
    s = _full(steps, "tome_micro", golden_dir=golden_dir)
    case, f32 = s["case"], s["dense"]["features"].detach()
    model, _, _ = _train_model(case)
    x = _image(case)
    B, D = f32.shape[:2]
    G = s["G"].cuda()
    want = None
    for fmt, dtype in (("NCHW", torch.float32), ("NHWC", torch.float32), ("NCHW", torch.bfloat16), ("NHWC", torch.bfloat16)):
        model.zero_grad(set_to_none=True)
        out, dense = model.forward_dense_train(x, output_fmt=fmt, dtype=dtype, fill=FILL)
        feat = dense["features"]
        assert feat.dtype == dtype and torch.equal(dense["index"], s["dense"]["index"]) and torch.equal(_bits(out), _bits(s["out"]))
        nchw = feat.detach() if fmt == "NCHW" else feat.detach().permute(0, 3, 1, 2)
        assert torch.equal(_bits(nchw), _bits(f32.to(dtype)))
        Gf = G.reshape(f32.shape) if fmt == "NCHW" else G.reshape(f32.shape).permute(0, 2, 3, 1)
        (feat.float() * Gf).sum().backward()                     # (bf16 map: autograd hands the node a bf16 gradient)
        grads = _grads(model)
        if want is None:
            want = grads
            for n in grads:
                assert torch.equal(_bits(grads[n]), _bits(s["grads_map"][n])), n
        elif dtype == torch.float32:
            for n in grads:                                      # the same sums in the other layout: the same bits
                assert torch.equal(_bits(grads[n]), _bits(want[n])), (fmt, n)
        else:
            total = _rel(torch.cat([g.reshape(-1) for g in grads.values()]), torch.cat([want[n].reshape(-1) for n in grads]))
            assert total < 2.0 ** -7, (fmt, total)               # G rounded to bf16 on its way in: 2^-9 per element
    # no gradient for the map: the head's term alone is model(x)'s step
    model.zero_grad(set_to_none=True)
    out, dense = model.forward_dense_train(x)
    labels = _launches.labels(_head_loss(case, out, None).backward)
    assert "tr_dense_scatter" not in labels
    head_only = _grads(model)
    model.zero_grad(set_to_none=True)
    _head_loss(case, model(x), None).backward()
    for n, p in model.named_parameters():
        assert torch.equal(_bits(p.grad), _bits(head_only[n])), n


def _plain_step_labels(case, model, x):
    model.zero_grad(set_to_none=True)
    fwd = []

    def forward():
        fwd.append(torch.nn.functional.cross_entropy(model(x), grad_labels(case).cuda()))
    labels = _launches.labels(forward)
    return labels, _launches.labels(fwd[0].backward), _grads(model)


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro", "sit_micro"])
def test_the_plain_training_step_keeps_its_launches_and_bits(steps, golden_dir, name):
    s = _full(steps, name, golden_dir=golden_dir)
    case = s["case"]
    model, _, _ = _train_model(case)
    x = _image(case)
    before = _plain_step_labels(case, model, x)
    dense_fwd, dense_bwd = [], []

    def dense_forward():
        out, dense = model.forward_dense_train(x)
        dense_fwd.append((dense["features"].reshape(s["G"].shape) * s["G"].cuda()).sum() + _head_loss(case, out, None))
    model.zero_grad(set_to_none=True)
    fl = _launches.labels(dense_forward)
    bl = _launches.labels(dense_fwd[0].backward)
    after = _plain_step_labels(case, model, x)
    assert before[0] == after[0] and before[1] == after[1]
    for n in before[2]:
        assert torch.equal(_bits(before[2][n]), _bits(after[2][n])), n
    # the dense step: the plain forward's launches, the two of the row output in front of the final norm, then the eval path's three (no
    # tr_stage_decisions for a model without stages); the plain backward's launches plus the scatter and the norm's pass over every row
    from collections import Counter
    extra_f, extra_b = Counter(fl) - Counter(before[0]), Counter(bl) - Counter(before[1])
    assert not Counter(before[0]) - Counter(fl) and not Counter(before[1]) - Counter(bl)
    assert fl[-2:] == ["tr_dense_index", "tr_dense_gather"] and bl[0] == "tr_dense_scatter"
    assert extra_f == Counter({"layernorm_kernel": 2, "tr_stage_decisions": 1, "tr_dense_index": 1, "tr_dense_gather": 1}), extra_f
    assert extra_b == Counter({"tr_dense_scatter": 1, "ln_bwd_kernel": 1, "tr_layernorm_bwd (reduce)": 1}), extra_b


def test_refusals(steps, golden_dir):
    case = GOLDEN_CASES["topk_micro"]
    model, _, _ = _train_model(case)
    x = _image(case)

    def refused(exc, match, fn):
        def call():
            with pytest.raises(exc, match=match):
                fn()
        assert _launches.labels(call) == []
    model.eval()
    refused(RuntimeError, r"model\.train\(\).*forward_dense", lambda: model.forward_dense_train(x))
    model.train()
    with pytest.raises(RuntimeError, match="eval feature"):      # forward_dense itself stays an eval entry
        model.forward_dense(x)
    model.viz_mode = True
    refused(RuntimeError, "viz_mode", lambda: model.forward_dense_train(x))
    model.viz_mode = False
    refused(RuntimeError, "no CPU path", lambda: model.forward_dense_train(x.cpu()))
    refused(ValueError, "output_fmt", lambda: model.forward_dense_train(x, output_fmt="CHW"))
    refused(ValueError, "dtype", lambda: model.forward_dense_train(x, dtype=torch.float16))
    model.precision = "fp32"
    refused(NotImplementedError, "bf16", lambda: model.forward_dense_train(x))
    model.precision = "bf16"
    ats, _, _ = _train_model(GOLDEN_CASES["ats_micro"])
    ats.dynamic_width = True
    refused(RuntimeError, "dynamic_width", lambda: ats.forward_dense_train(x))
    dyvit, _, _ = _train_model(GOLDEN_CASES["dyvit_micro_train"])
    refused(NotImplementedError, "DyViT", lambda: dyvit.forward_dense_train(x))
    # one tape per model: a second dense forward makes the first one's backward stale
    G = _map_weights(case, model).cuda()
    first = (model.forward_dense_train(x)[1]["features"].reshape(G.shape) * G).sum()
    second = (model.forward_dense_train(x + 0.5)[1]["features"].reshape(G.shape) * G).sum()
    with pytest.raises(RuntimeError, match="overwritten"):
        first.backward()
    second.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())


def _map_matches_its_rows(model, dense, B):
    """The map is the restated gather of the rows this forward wrote, by the index it returned."""
    st = model._train_state()
    D, P0, n_last = model.embed_dim, model.patch_embed.num_patches, model._last_tokens[-1]
    tokens = st.dense["tokens"][:B * n_last * D].view(B, n_last, D).cpu().numpy()
    want = ref.dense_gather(tokens, dense["index"].cpu().numpy(), "NCHW", "fp32", FILL)
    np.testing.assert_array_equal(dense["features"].detach().cpu().numpy().reshape(B, D, P0).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("kind", ["uint8", "uint8_channels_last", "augmented"])
def test_uint8_and_augmented_input_go_through_the_same_entry(kind):
    """The superset entry's other two inputs: `out` is model(x)'s for the same input, the map is made of the rows of that forward, and the
    map's gradient reaches every parameter."""
    from tokenreduction_amd import augment
    case = GOLDEN_CASES["tome_micro"]
    model, _, _ = _train_model(case)
    model.set_pixel_input()
    B = 4
    u8 = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(9)).cuda()
    if kind == "uint8_channels_last":
        u8 = u8.contiguous(memory_format=torch.channels_last)
    x = u8
    if kind == "augmented":
        np.random.seed(3)
        torch.manual_seed(3)
        x, _ = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=case["num_classes"])(u8, torch.arange(B).cuda() % case["num_classes"])
        assert isinstance(x, augment.AugmentedBatch)
    plain = model(x).detach().clone()
    out, dense = model.forward_dense_train(x, fill=FILL)
    assert torch.equal(_bits(out), _bits(plain))
    _map_matches_its_rows(model, dense, B)
    G = torch.randn(dense["features"].shape, generator=torch.Generator().manual_seed(2)).cuda() / (B * 196)
    model.zero_grad(set_to_none=True)
    (dense["features"] * G).sum().backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        assert n.startswith("head.") or float(p.grad.abs().max()) > 0, n
    # the float image the pixels stand for gives the same map (uint8 input is bitwise the fp32 tensor of ToTensor + Normalize)
    if kind != "augmented":
        from tokenreduction_amd import pixels
        mean, std = model.pixel_input
        lut = pixels.pixel_lut(mean, std).cuda()                      # [C, 256]
        xf = torch.stack([lut[c][u8[:, c].long()] for c in range(3)], dim=1).contiguous()
        out_f, dense_f = model.forward_dense_train(xf, fill=FILL)
        assert torch.equal(_bits(out_f), _bits(out)) and torch.equal(_bits(dense_f["features"].detach()), _bits(dense["features"].detach()))


def test_droppath_and_dropout_draw_as_for_the_plain_forward_and_the_map_path_stays_linear():
    case = dict(GOLDEN_CASES["topk_micro"], drop_path=0.1, drop_rate=0.1)
    model, _, _ = _train_model(case)
    x = _image(case)
    B = case["batch"]
    G = _map_weights(case, model).cuda()

    def step(head, map_):
        torch.manual_seed(11)                                    # the same DropPath draws and dropout masks for every forward
        model.zero_grad(set_to_none=True)
        out, dense = model.forward_dense_train(x, fill=FILL)
        loss = 0
        if head:
            loss = loss + _head_loss(case, out, None)
        if map_:
            loss = loss + (dense["features"].reshape(G.shape) * G).sum()
        loss.backward()
        return out.detach().clone(), dense, _grads(model)
    torch.manual_seed(11)
    model.zero_grad(set_to_none=True)
    plain = model(x)
    _head_loss(case, plain, None).backward()
    plain_grads = _grads(model)
    out, dense, head_only = step(True, False)
    assert torch.equal(_bits(out), _bits(plain.detach()))
    _map_matches_its_rows(model, dense, B)
    for n in plain_grads:                                        # no gradient for the map: model(x)'s step, bit for bit
        assert torch.equal(_bits(head_only[n]), _bits(plain_grads[n])), n
    _, _, map_only = step(False, True)
    _, _, both = step(True, True)
    # one backward of the sum against the sum of two backwards: the same masks and scales on both paths.  Each of the three passes is the
    # exact backward, which is linear in the output gradients, up to the bf16 rounding of every gradient GEMM operand -- the error
    # tests/test_hip_train.py bounds by grad_tol(case) on the whole vector; so does the difference here
    total = _rel(torch.cat([both[n].reshape(-1) for n in both]), torch.cat([(head_only[n] + map_only[n]).reshape(-1) for n in both]))
    print(f"\n[droppath + dropout] mixed against head-only + map-only: whole-vector rel L2 {total:.3e}")
    assert total < grad_tol(case), total
    assert float(torch.cat([map_only[n].reshape(-1) for n in map_only if not n.startswith("head.")]).norm()) > 0
