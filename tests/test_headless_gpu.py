"""GPU tests of headless models (num_classes = 0, deit_viz.py:142,182: head = nn.Identity()): the model returns the fp32 final-normed
CLS row [B, D] wherever it returns logits.

1. Reference parity on tests/golden/headless_*.npz (tests/golden/gen_golden_headless.py) in the three eval precisions.  fp32 and bf16x3
   run the fixture tests of test_hip_fp32.py / test_hip_split.py on the headless model (their decision checks, unchanged) and then hold
   the features to 2e-5 / 1e-4 (DPC-KNN 3e-5 in fp32, DyViT and DPC-KNN 2e-4 in bf16x3: measured, see below); bf16 holds the relative L2
   bounds of test_hip_model.py.
2. Identity-head equivalence, the strict check: a classifier with num_classes = D, head.weight = I, head.bias = 0 on the same trunk.  In bf16
   its logits are bf16(features) bit for bit (the head GEMM multiplies the bf16 operand by exact ones and adds exact zeros); fp32 is
   bit-exact for the same reason; bf16x3 splits the operand into hi + lo and the identity returns hi + bf16(lo), within 2^-17 relative.
3. Training equivalence: the same two models, the same draws, upstream gradient G as d logits on one and d features on the other: every
   trunk gradient (norm.* included) bit-identical -- the classifier's data gradient of an identity head is bf16(G), which is what the
   headless backward feeds the final norm's backward.
4. Training with parts: a torch head on the headless trunk under optim.FusedAdamW (bit-identical to torch's fused AdamW), FlatGradReducer on
   RCCL world 1, the tape guard.
5. Classifier <-> headless switches on one model, checked against fresh models (no stale workspace or captured graph)."""
import os
import types

import numpy as np
import pytest
import torch

import tokenreduction_amd as tra
from tests import _params, test_hip_fp32, test_hip_split
from tests._headless_params import HEADLESS_CASES
from tests._params import GOLDEN_CASES, grad_labels, make_images
from tests.test_hip_model import build_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _headless(case):
    """The case's trunk and reduction modules (weights from its seeds), the classifier removed by reset_classifier(0)."""
    m, _, _ = build_model(dict(case, num_classes=case["embed_dim"]))
    m.reset_classifier(0)
    return m


def _pair(case):
    """(headless model, classifier with num_classes = D, head.weight = I, head.bias = 0) on the same trunk."""
    D = case["embed_dim"]
    cl, _, _ = build_model(dict(case, num_classes=D))
    with torch.no_grad():
        cl.head.weight.copy_(torch.eye(D))
        cl.head.bias.zero_()
    return _headless(case), cl


def _same_draws(models, B):
    """DPC-KNN draws its density noise per forward: give both models the same (zero) draws."""
    for m in models:
        if hasattr(m, "density_noise"):
            m.density_noise = {blk: torch.zeros(B, P) for blk, _, P in m._stage_shapes()}


def _assert_viz_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert sorted(a[k]) == sorted(b[k]), k
        for blk in a[k]:
            np.testing.assert_array_equal(np.asarray(a[k][blk]), np.asarray(b[k][blk]), err_msg=f"{k}[{blk}]")


# ---- 1. reference parity ----------------------------------------------------------------------------------------------------------

def _recording_builder(outs):
    def build(case):
        m = _headless(case)
        fwd = m.forward

        def forward(x):
            out = fwd(x)
            outs.append(out)
            return out
        m.forward = forward
        return m, None, None
    return build


def _check_features(golden_dir, name, out, tol, label):
    case = HEADLESS_CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    feats, viz = out
    ref = torch.from_numpy(g["logits"])
    assert feats.shape == ref.shape == (case["batch"], case["embed_dim"])
    d = (feats.cpu() - ref).abs().max().item()
    kept = [k for k in g.files if k.startswith("kept_")]
    same_ids = all(viz["Kept_Tokens"][int(k.split("_")[1])].shape == g[k].shape and bool((viz["Kept_Tokens"][int(k.split("_")[1])] == g[k]).all())
                   for k in kept)
    print(f"\n[{name}] {label}: max|features - reference| = {d:.2e} (|features| <= {ref.abs().max().item():.2f}); kept ids as the reference's: {same_ids}")
    if case["family"] == "ats" and not same_ids:
        # a sample moved to the neighbouring token on a cdf plateau changes every later block (test_hip_fp32._check_ats_fp32): the fixture
        # test above held that case to its own bound
        return
    assert d <= tol, d


@pytest.mark.parametrize("name", list(HEADLESS_CASES))
def test_fp32_headless_matches_reference(golden_dir, name, monkeypatch):
    outs = []
    monkeypatch.setitem(_params.GOLDEN_CASES, name, HEADLESS_CASES[name])
    monkeypatch.setattr(test_hip_fp32, "build_model", _recording_builder(outs))
    test_hip_fp32.test_model_fp32_matches_reference_golden(golden_dir, name)
    # DPC-KNN: measured 2.25e-5 at |features| <= 3.1 with every centre and assignment the reference's -- the merge weights exp(x . w)
    # and the cluster sums come out of the reference's CPU in another summation order
    _check_features(golden_dir, name, outs[0], 3e-5 if HEADLESS_CASES[name]["family"] == "dpcknn" else 2e-5, "fp32")


@pytest.mark.parametrize("name", list(HEADLESS_CASES))
def test_bf16x3_headless_matches_reference(golden_dir, name, monkeypatch):
    outs = []
    monkeypatch.setitem(_params.GOLDEN_CASES, name, HEADLESS_CASES[name])
    monkeypatch.setattr(test_hip_split, "build_model", _recording_builder(outs))
    test_hip_split.test_model_bf16x3_free_running_against_reference_golden(golden_dir, name)
    # DyViT (three predictor Linears per stage) and DPC-KNN (the merge above): measured 1.4e-4 / 1.5e-4 at |features| <= 3.5 with the
    # reference's decisions; every other family <= 7e-5
    _check_features(golden_dir, name, outs[0], 2e-4 if HEADLESS_CASES[name]["family"] in ("dyvit", "dpcknn") else 1e-4, "bf16x3")


@pytest.mark.parametrize("name", list(HEADLESS_CASES))
def test_bf16_headless_matches_reference(golden_dir, name):
    """bf16 against the reference's fp32 features, free-running: test_hip_model.test_model_parity's bounds (relative L2 5 % at micro size,
    DyViT's 0.35 regression bound).  The selections are the classifier path's, bit for bit -- the ones test_hip_model.py pins against the
    oracle on the device's own scores."""
    case = HEADLESS_CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    hl, cl = _pair(case)
    noise = {int(k.split("_")[1]): torch.from_numpy(g[k]) for k in g.files if k.startswith("noise_")}
    if noise:
        hl.density_noise = cl.density_noise = noise
    x = make_images(case["batch"], 224, case["xseed"]).cuda()
    np.random.seed(case["xseed"])
    f, viz = hl(x)
    np.random.seed(case["xseed"])
    l, vizc = cl(x)
    assert f.shape == (case["batch"], case["embed_dim"]) and f.dtype == torch.float32
    _assert_viz_equal(viz, vizc)
    assert torch.equal(l, f.bfloat16().float())
    ref = torch.from_numpy(g["logits"])
    rel = ((f.cpu() - ref).norm() / ref.norm()).item()
    kept = [k for k in g.files if k.startswith("kept_")]
    same_ids = all(viz["Kept_Tokens"][int(k.split("_")[1])].shape == g[k].shape and bool((viz["Kept_Tokens"][int(k.split("_")[1])] == g[k]).all())
                   for k in kept)
    print(f"\n[{name}] bf16: relative L2 |features - reference| = {rel:.3e}; kept ids as the reference's: {same_ids}")
    if case["family"] in ("ats", "kmedoids") and not same_ids:
        # bf16 scores move an ATS sample or a medoid, and every later block sees other tokens (measured 0.45 relative L2 once that happens).
        # test_model_parity holds these two families teacher-forced; free-running, what is held here is coarse.  ATS: the first stage's ids
        # are valid samples of the REFERENCE's cdf at test_model_parity's bf16 tolerance (2e-2).  K-Medoids: the medoid SETS stay the
        # reference's for the most part (first stage >= 0.9, every stage >= 0.5; measured 0.99 / 0.88 / 0.77).  Both: the features within
        # 0.6 relative L2 -- a regression bound like DyViT's below: it fails when the selections fork from the first stage on
        blks = sorted(int(k.split("_")[1]) for k in kept)
        if case["family"] == "ats":
            import oracle
            from tests._params import assert_valid_sampling, case_config
            counts = oracle.ats_sample_counts(case_config(case))
            assert_valid_sampling(viz["Kept_Tokens"][blks[0]], g[f"cdf_{blks[0]}"], oracle.ats_sample_steps(counts[blks[0]]).numpy(), tol=2e-2)
        else:
            ov = [_overlap(viz["Kept_Tokens"][b], g[f"kept_{b}"]) for b in blks]
            print(f"   medoid-set overlap with the reference per stage: {ov}")
            assert ov[0] >= 0.9 and min(ov) >= 0.5, ov
        assert rel < 0.6, rel
        return
    assert rel < (0.35 if case["family"] == "dyvit" else 0.05), rel


def _overlap(a, b):
    """Mean over the images of |A & B| / |B|."""
    return float(np.mean([len({int(v) for v in x} & {int(v) for v in y}) / len(y) for x, y in zip(np.asarray(a), np.asarray(b))]))


# ---- 2. identity-head equivalence (eval) -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(HEADLESS_CASES))
def test_identity_head_equivalence_eval(name):
    case = HEADLESS_CASES[name]
    B = case["batch"]
    hl, cl = _pair(case)
    _same_draws((hl, cl), B)
    x = make_images(B, 224, case["xseed"]).cuda()
    hl.viz_mode = cl.viz_mode = False
    # bf16, one forward at a time (a captured graph from the second call on) and through forward_async
    f, l = hl(x), cl(x)
    assert f.shape == (B, case["embed_dim"])
    assert torch.equal(l, f.bfloat16().float())
    assert not torch.equal(f, f.bfloat16().float())          # the features are the norm's fp32 values, not its bf16 rounding
    assert torch.equal(hl(x), f) and torch.equal(cl(x), l)
    fa, la = hl.forward_async(x), cl.forward_async(x)
    fa, la = fa.result(), la.result()
    torch.cuda.synchronize()
    assert torch.equal(fa, f) and torch.equal(la, l)
    # fp32: the identity GEMM multiplies by exact ones and adds exact zeros
    hl.precision = cl.precision = "fp32"
    f32, l32 = hl(x), cl(x)
    assert torch.equal(l32, f32), (l32 - f32).abs().max().item()
    # bf16x3: the identity product of the split operand is hi + bf16(lo), the operand to 2^-17 relative
    hl.precision = cl.precision = "bf16x3"
    f3, l3 = hl(x), cl(x)
    assert bool(((l3 - f3).abs() <= 1e-5 * f3.abs()).all()), ((l3 - f3).abs() / f3.abs()).max().item()
    # viz_mode: (features, viz_data) with viz_data identical
    hl.precision = cl.precision = "bf16"
    hl.viz_mode = cl.viz_mode = True
    (fv, v), (lv, w) = hl(x), cl(x)
    assert torch.equal(lv, fv.bfloat16().float()) and torch.equal(fv, f)
    _assert_viz_equal(v, w)


def test_identity_head_equivalence_ats_dynamic_width_and_kmedoids_equal_weight():
    for name in ("ats_micro", "kmedoids_micro_equal"):
        case = dict(GOLDEN_CASES[name], batch=2)
        hl, cl = _pair(case)
        hl.viz_mode = cl.viz_mode = False
        if case["family"] == "ats":
            hl.dynamic_width = cl.dynamic_width = True
        x = make_images(2, 224, case["xseed"]).cuda()
        np.random.seed(5)
        f = hl(x)
        np.random.seed(5)
        l = cl(x)
        assert f.shape == (2, case["embed_dim"])
        assert torch.equal(l, f.bfloat16().float()), name
        assert hl._last_tokens == cl._last_tokens, name


def test_headless_dyvit_teacher_returns_cls_and_token_features():
    """dyvit.py:319-336 with head = nn.Identity(): (cls features [B, D], final-normed patch tokens [B, P, D])."""
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False, dyvit_distill=False)
    torch.manual_seed(0)
    t = tra.create_model("dyvit_tiny_patch16_224_teacher", pretrained=False, num_classes=0, args=args)
    c = tra.create_model("dyvit_tiny_patch16_224_teacher", pretrained=False, num_classes=192, args=args)
    c.load_state_dict(t.state_dict(), strict=False)
    with torch.no_grad():
        c.head.weight.copy_(torch.eye(192))
        c.head.bias.zero_()
    t, c = t.cuda().eval(), c.cuda().eval()
    x = make_images(2, 224, 3).cuda()
    (fh, th), (fl, tl) = t(x), c(x)
    assert fh.shape == (2, 192) and th.shape == (2, 196, 192)
    assert torch.equal(fl, fh.bfloat16().float()) and torch.equal(th, tl)


# ---- 3. training equivalence -------------------------------------------------------------------------------------------------------

TRAIN_CASES = ["deit_micro", "topk_micro", "evit_micro", "tome_micro", "dyvit_micro_train", "sit_micro", "dpcknn_micro", "ats_micro", "sinkhorn_micro",
               "kmedoids_micro", "patchmerger_micro", "heuristic_micro_l2"]


def _train_grads(model, x, G, G2, noise):
    model.viz_mode = False
    model.train()
    if model._family == tra.models._lib.TR_FAMILY_DYVIT:
        model.gumbel_noise = noise
    elif hasattr(model, "density_noise"):
        model.density_noise = noise
    model.zero_grad(set_to_none=True)
    out = model(x)
    first = out[0] if isinstance(out, tuple) else out
    if isinstance(out, tuple) and len(out) == 4:           # DyViT distillation: (x, token features, prev_decision, preds)
        torch.autograd.backward([first, out[1]], [G, G2])
    else:
        first.backward(G)
    torch.cuda.synchronize()
    return out, first.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if not n.startswith("head.")}


@pytest.mark.parametrize("name,batch", [(n, None) for n in TRAIN_CASES] + [("topk_small_kr07", 64)])
def test_training_identity_head_equivalence(name, batch):
    case = dict(GOLDEN_CASES[name])
    if batch:
        case["batch"] = batch
    B, D = case["batch"], case["embed_dim"]
    hl, cl = _pair(case)
    x = make_images(B, 224, case["xseed"]).cuda()
    gen = torch.Generator().manual_seed(case["xseed"] + 11)
    G = torch.randn(B, D, generator=gen).cuda()
    P = hl.patch_embed.num_patches
    G2 = torch.randn(B, P, D, generator=gen).cuda()
    if case["family"] == "dyvit":
        noise = {j: torch.empty(B, P, 2).exponential_(generator=gen).log_().neg_() for j in range(len(hl.pruning_loc))}
    elif case["family"] == "dpcknn":
        noise = {blk: torch.zeros(B, Pin) for blk, _, Pin in hl._stage_shapes()}
    else:
        noise = None
    out_h, f, gh = _train_grads(hl, x, G, G2, noise)
    out_c, l, gc = _train_grads(cl, x, G, G2, noise)
    assert f.shape == (B, D) and f.dtype == torch.float32
    if case["family"] == "dyvit":
        assert isinstance(out_h, tuple) and len(out_h) == len(out_c) == 4
        assert torch.equal(out_h[1], out_c[1])
    assert torch.equal(l, f.bfloat16().float())
    assert sorted(gh) == sorted(gc) and "norm.weight" in gh
    for n in gc:
        assert torch.equal(gh[n], gc[n]), (n, (gh[n] - gc[n]).abs().max().item())


# ---- 4. training with parts --------------------------------------------------------------------------------------------------------

def test_headless_trunk_torch_head_fused_adamw():
    """A torch nn.Linear head on the headless trunk, the trunk stepped by optim.FusedAdamW and, in a second run from the same start, by
    torch.optim.AdamW(fused=True): the loss goes down, and the trunk parameters agree bit for bit after every step."""
    from tokenreduction_amd.optim import FusedAdamW
    case = GOLDEN_CASES["topk_micro"]
    x = make_images(case["batch"], 224, case["xseed"]).cuda()
    y = grad_labels(case).cuda()
    runs = {}
    for kind in ("torch", "hip"):
        m = _headless(case)
        m.viz_mode = False
        m.train()
        torch.manual_seed(3)
        head = torch.nn.Linear(case["embed_dim"], case["num_classes"]).cuda()
        kw = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
        opt = torch.optim.AdamW(m.parameters(), fused=True, **kw) if kind == "torch" else FusedAdamW(list(m.parameters()), model=m, **kw)
        hopt = torch.optim.AdamW(head.parameters(), lr=2e-3)
        losses, trace = [], []
        for _ in range(6):
            loss = torch.nn.functional.cross_entropy(head(m(x)), y)
            opt.zero_grad(set_to_none=True)
            hopt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            hopt.step()
            losses.append(loss.item())
            trace.append([p.detach().clone() for p in m.parameters()])
        runs[kind] = (losses, trace)
    print(f"\nlosses: {runs['hip'][0]}")
    assert runs["hip"][0][-1] < runs["hip"][0][0]
    assert runs["hip"][0] == runs["torch"][0]
    for step, (a, b) in enumerate(zip(runs["torch"][1], runs["hip"][1])):
        for pa, pb in zip(a, b):
            assert torch.equal(pa, pb), step


def test_headless_flat_grad_reducer_world1_gives_plain_backward_bits():
    import torch.distributed as dist
    from tokenreduction_amd.dp import FlatGradReducer
    case = GOLDEN_CASES["topk_micro"]
    m = _headless(case)
    m.viz_mode = False
    m.train()
    x = make_images(case["batch"], 224, case["xseed"]).cuda()
    G = torch.randn(case["batch"], case["embed_dim"], generator=torch.Generator().manual_seed(2)).cuda()
    m(x).backward(G)
    want = {n: p.grad.clone() for n, p in m.named_parameters()}
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        red = FlatGradReducer(bucket_bytes=512 * 1024).attach(m)
        m.zero_grad(set_to_none=True)
        m(x).backward(G)
        torch.cuda.synchronize()
        assert len(red.launched) >= 2 and red.launched[-1][1] == m._train_state().flat.numel()
        for n, p in m.named_parameters():
            assert torch.equal(p.grad, want[n]), n
    finally:
        m._grad_reducer = None
        dist.destroy_process_group()


def test_headless_second_train_forward_before_backward_raises():
    case = GOLDEN_CASES["topk_micro"]
    m = _headless(case)
    m.viz_mode = False
    m.train()
    x = make_images(case["batch"], 224, case["xseed"]).cuda()
    f1 = m(x)
    m(x)
    with pytest.raises(RuntimeError, match="overwritten"):
        f1.backward(torch.ones_like(f1))


# ---- 5. classifier <-> headless -----------------------------------------------------------------------------------------------------

def test_classifier_headless_switches_match_fresh_models():
    case = GOLDEN_CASES["topk_micro"]
    B, D = case["batch"], case["embed_dim"]
    m = _headless(case)
    m.viz_mode = False
    x = make_images(B, 224, case["xseed"]).cuda()
    f0 = m(x)
    assert f0.shape == (B, D) and torch.equal(m(x), f0)                  # the second call replays a captured graph
    torch.manual_seed(4)
    m.reset_classifier(1000)
    l = m(x)
    assert l.shape == (B, 1000) and torch.equal(m(x), l)
    fresh, _, _ = build_model(dict(case, num_classes=1000))
    fresh.viz_mode = False
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(fresh(x), l)
    m.reset_classifier(0)
    f1 = m(x)
    assert f1.shape == (B, D) and torch.equal(f1, f0) and torch.equal(m(x), f0)
    fresh0 = _headless(case)
    fresh0.viz_mode = False
    assert torch.equal(fresh0(x), f0)
