"""Output taps of the eval forward (model.forward_taps / forward_async(cls_blocks=..., final_tokens=...)), GPU tier.

A CLS tap is the CLS row of viz_data["Features"][blk] and final_tokens is the parent teacher's Features[last] -> ops.layernorm_f32, both
bit for bit: the taps add the pending residuals in the order the next norm does, so every comparison with this package's own outputs is
equality.  One micro fixture per family (tests/_params.py), batch 3."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _launches
from tests._params import GOLDEN_CASES, make_images
from tests.test_hip_model import build_model, case_params

pytestmark = pytest.mark.gpu

FAMILIES = ["deit_micro", "topk_micro", "evit_micro", "tome_micro", "dyvit_micro", "sit_micro", "dpcknn_micro", "ats_micro", "kmedoids_micro",
            "sinkhorn_micro", "patchmerger_micro", "heuristic_micro_l2"]
PRECISIONS = ["bf16", "bf16x3", "fp32"]
B = 3
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _model(name):
    """The family's micro model, viz_mode off, with the recorded density noise where the family draws some (DPC-KNN)."""
    model, _, _ = build_model(GOLDEN_CASES[name])
    model.viz_mode = False
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    noise = {int(k.split("_")[1]): torch.from_numpy(g[k]) for k in g.files if k.startswith("noise_")}
    if noise:
        model.density_noise = noise
    return model


def _prepared(name, precision="bf16"):
    model = _model(name)
    model.precision, model.use_graph, model.viz_mode = precision, True, False
    return model


def _images(name, batch=B):
    return make_images(batch, 224, GOLDEN_CASES[name]["xseed"]).cuda()


def _viz(model, x):
    """(logits, Features) of a viz_mode forward: the parent commit's way to the rows."""
    model.viz_mode = True
    try:
        logits, viz = model(x)
    finally:
        model.viz_mode = False
    return logits, viz["Features"]


def _norm_f32(model, rows):
    """ops.layernorm_f32 with the model's final norm: the second half of the parent teacher's forward."""
    from tokenreduction_amd import ops
    return ops.layernorm_f32(rows, model.norm.weight.detach().float().contiguous(), model.norm.bias.detach().float().contiguous(),
                             float(model.norm.eps))


def _teacher_restated(model, x):
    """VisionTransformerTeacher.forward of the parent commit on a dense model: Features[last] through ops.layernorm_f32."""
    logits, feats = _viz(model, x)
    last = feats[model.depth - 1]
    n, D = last.shape[1], last.shape[2]
    return logits, _norm_f32(model, torch.from_numpy(last).cuda().view(-1, D)).view(x.shape[0], n, D)


def _same(a, b):
    (la, ta), (lb, tb) = a, b
    assert torch.equal(la, lb) and ta["blocks"] == tb["blocks"]
    for key in ("cls", "final_tokens"):
        assert (ta[key] is None) == (tb[key] is None), key
        if ta[key] is not None:
            assert torch.equal(ta[key], tb[key]), key


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", FAMILIES)
def test_cls_taps_are_the_cls_rows_of_viz_features(name, precision):
    model, x = _prepared(name, precision), _images(name)
    _, feats = _viz(model, x)
    blocks = sorted(feats)                                   # every block viz_mode records for this family
    assert blocks and blocks[-1] == model.depth - 1
    plain = model(x)
    logits, taps = model.forward_taps(x, cls_blocks=blocks)
    torch.cuda.synchronize()
    model.check_status()
    assert taps["blocks"] == tuple(blocks) and taps["final_tokens"] is None
    assert taps["cls"].shape == (B, len(blocks), model.embed_dim) and taps["cls"].dtype == torch.float32
    got = taps["cls"].cpu().numpy()
    for col, blk in enumerate(blocks):
        np.testing.assert_array_equal(got[:, col], feats[blk][:, 0], err_msg=f"block {blk}")
    assert torch.equal(logits, plain)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["deit_micro", "topk_micro"])
def test_final_tokens_are_the_parent_teacher_computation(name, precision):
    """Dense (the teacher's own shape) and behind three reductions (N_last < N0)."""
    model, x = _prepared(name, precision), _images(name)
    _, want = _teacher_restated(model, x)
    plain = model(x)
    logits, taps = model.forward_taps(x, cls_blocks=(), final_tokens=True)
    assert taps["cls"] is None and taps["blocks"] == ()
    assert taps["final_tokens"].shape == want.shape and torch.equal(taps["final_tokens"], want)
    assert torch.equal(logits, plain)
    # both kinds in one forward
    logits2, both = model.forward_taps(x, cls_blocks=(model.depth - 1,), final_tokens=True)
    assert torch.equal(both["final_tokens"], want) and torch.equal(logits2, plain)
    assert torch.equal(both["cls"][:, 0], model.forward_taps(x, cls_blocks=(model.depth - 1,))[1]["cls"][:, 0])


@pytest.mark.parametrize("training", [False, True])
def test_teacher_outputs_did_not_move(training):
    """VisionTransformerTeacher now takes norm(x) from the final_tokens tap: both outputs equal the parent's computation, restated on a
    dense model with the same weights (the module flag does not matter: the teacher is the inference executor in any mode)."""
    import tokenreduction_amd as tra
    case = GOLDEN_CASES["deit_micro"]
    _, params = case_params(case)
    teacher = tra.VisionTransformerTeacher(patch_size=16, embed_dim=case["embed_dim"], depth=case["depth"], num_heads=case["num_heads"],
                                           mlp_ratio=4, qkv_bias=True, num_classes=case["num_classes"])
    teacher.load_state_dict(params, strict=True)
    teacher = teacher.cuda().train(training)
    x = _images("deit_micro")
    want_logits, want_tokens = _teacher_restated(_prepared("deit_micro"), x)
    with torch.no_grad():
        logits, tokens = teacher(x)
        again = teacher(x)                                   # the replay
    assert teacher.training == training
    assert tokens.shape == (B, 196, case["embed_dim"])
    assert torch.equal(logits, want_logits) and torch.equal(tokens, want_tokens[:, 1:])
    assert torch.equal(again[0], logits) and torch.equal(again[1], tokens)
    labels = _launch_labels(teacher, lambda: teacher(x))
    assert labels.count("tr_final_tokens") == 1 and "tr_residual_snapshot" not in labels


@pytest.mark.parametrize("name", FAMILIES)
def test_last_block_tap_against_the_reference_in_fp32(name):
    """The fixture's final_tokens are the reference's own Features[last][:, :8] (tests/golden/gen_golden.py) at the case's batch size; 2e-4
    absolute is the bound tests/test_hip_fp32.py holds the same rows of viz_mode to.

    ATS: the fp32 executor's sampled ids are valid samples of the reference's cdf but not always the reference's ids (a 1-ulp difference
    in the cdf moves a sample to the neighbouring token: tests/test_hip_fp32.py::_check_ats_fp32, which for that reason holds ATS to 2e-4
    only where every id equals the reference's).  The same condition here: with other ids the reference's rows belong to another token set
    (ats_micro, measured: max|tap - reference| = 1.33e-01 with ids that differ) and what is held instead is the tap's equality with
    viz_mode's row, bit for bit."""
    case = GOLDEN_CASES[name]
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = _prepared(name, "fp32")
    x = _images(name, case["batch"])
    np.random.seed(case["xseed"])
    _, taps = model.forward_taps(x, cls_blocks=(model.depth - 1,))
    got, want = taps["cls"][:, 0].cpu().numpy(), g["final_tokens"][:, 0]
    d = float(np.abs(got - want).max())
    print(f"\n[{name}] fp32 CLS tap of the last block: max|tap - reference| = {d:.2e}")
    assert got.shape == want.shape
    if case["family"] == "ats":
        model.viz_mode = True
        try:
            _, viz = model(x)
        finally:
            model.viz_mode = False
        kept = {int(k.split("_")[1]): g[k] for k in g.files if k.startswith("kept_")}
        same = all(viz["Kept_Tokens"][blk].shape == ids.shape and bool((viz["Kept_Tokens"][blk] == ids).all()) for blk, ids in kept.items())
        print(f"[{name}] sampled ids identical to the reference's: {same}")
        np.testing.assert_array_equal(got, viz["Features"][model.depth - 1][:, 0])
        if not same:
            return
    assert d < 2e-4, d


def _launch_labels(model, fn):
    """Launch labels of fn() as plain launches, after a warm-up call."""
    graph, model.use_graph = model.use_graph, False
    try:
        fn()
        torch.cuda.synchronize()
        return _launches.labels(fn)
    finally:
        model.use_graph = graph


def test_launches_taps_ride_on_the_fast_path():
    model, x = _prepared("deit_micro"), _images("deit_micro")
    depth = model.depth
    base = _launch_labels(model, lambda: model(x))
    assert base.count("attention_kernel<cls>") == 1 and "tr_residual_snapshot" not in base
    model.viz_mode = True
    viz = _launch_labels(model, lambda: model(x))
    model.viz_mode = False
    assert viz.count("tr_residual_snapshot") == depth and "attention_kernel<cls>" not in viz      # what the taps avoid
    # CLS taps: the CLS-tail attention still runs, no snapshot, and apart from the tap launches nothing changed
    cls = _launch_labels(model, lambda: model.forward_taps(x, cls_blocks=range(depth)))
    assert cls.count("attention_kernel<cls>") == 1 and "tr_residual_snapshot" not in cls and cls.count("tr_cls_tap") == depth
    assert [lab for lab in cls if lab != "tr_cls_tap"] == base
    # final_tokens: exactly one launch of its own, the last block at full width, still no snapshot and lazy norms as before
    fin = _launch_labels(model, lambda: model.forward_taps(x, cls_blocks=(), final_tokens=True))
    assert fin.count("tr_final_tokens") == 1 and "tr_residual_snapshot" not in fin and "attention_kernel<cls>" not in fin
    assert fin.count("attention_kernel") == depth and len(fin) == len(base) + 1
    assert [lab for lab in fin if lab != "tr_final_tokens"][:-7] == base[:-7]       # everything in front of the last block's attention
    # no tap requested: the launches of model(x)
    assert _launch_labels(model, lambda: model.forward_taps(x, cls_blocks=())) == base


@pytest.mark.parametrize("name", ["deit_micro", "topk_micro", "sit_micro"])
def test_graph_replay_plain_launches_and_both_async_slots_agree(name):
    model, x = _prepared(name), _images(name)
    blocks = (0, model.depth - 1)
    first = model.forward_taps(x, cls_blocks=blocks, final_tokens=True)            # eager warm-up + capture + replay
    ws = model._last_ws
    assert any(key[-1] == (blocks, True) for key in ws["graphs"])
    _same(model.forward_taps(x, cls_blocks=blocks, final_tokens=True), first)      # replay
    model.use_graph = False
    _same(model.forward_taps(x, cls_blocks=blocks, final_tokens=True), first)      # plain launches
    model.use_graph = True
    handles = [model.forward_async(x, cls_blocks=blocks, final_tokens=True) for _ in range(4)]      # slots 1, 2, 1, 2
    for h in handles:
        _same(h.result(), first)
    torch.cuda.synchronize()
    model.check_status()
    assert model.forward_async(x).result().shape == first[0].shape                   # without keywords: the logits alone, as before
    assert torch.equal(model.forward_async(x).result(), first[0])


def test_a_second_batch_size_and_a_changed_tap_set_recapture():
    model = _prepared("topk_micro")
    x3, x2 = _images("topk_micro"), _images("topk_micro", 2)
    feats3, feats2 = _viz(model, x3)[1], _viz(model, x2)[1]

    def check(x, feats, blocks):
        logits, taps = model.forward_taps(x, cls_blocks=blocks)
        got = taps["cls"].cpu().numpy()
        assert taps["blocks"] == tuple(sorted(blocks)) and got.shape[1] == len(blocks)
        for col, blk in enumerate(sorted(blocks)):
            np.testing.assert_array_equal(got[:, col], feats[blk][:, 0])
        assert torch.equal(logits, model(x))
    check(x3, feats3, (1, 3))
    check(x3, feats3, (1, 3))
    check(x3, feats3, (3, 2, 1))                 # another tap set on the same workspace: its own graph, columns in ascending order
    assert {key[-1] for key in model._last_ws["graphs"]} >= {((1, 3), False), ((1, 2, 3), False)}
    check(x2, feats2, (1, 3))                    # another batch size: a new workspace
    check(x3, feats3, (3,))
    check(x3, feats3, (1, 3))


@pytest.mark.parametrize("name", ["deit_micro", "topk_micro"])
def test_pixel_input_equals_float_input(name):
    from tokenreduction_amd import pixels
    model = _prepared(name)
    u8 = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(8))
    mean, std = pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD
    xf = (((u8.float() / 255) - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]).cuda()
    blocks = (0, model.depth - 1)
    want = model.forward_taps(xf, cls_blocks=blocks, final_tokens=True)
    model.set_pixel_input(mean, std)
    try:
        _same(model.forward_taps(u8.cuda(), cls_blocks=blocks, final_tokens=True), want)
        _same(model.forward_taps(u8.cuda().contiguous(memory_format=torch.channels_last), cls_blocks=blocks, final_tokens=True), want)
        _same(model.forward_async(u8.cuda(), cls_blocks=blocks, final_tokens=True).result(), want)
    finally:
        model.set_pixel_input(None)


def test_refusals():
    from tokenreduction_amd import _lib
    import ctypes as C
    model, x = _prepared("deit_micro"), _images("deit_micro")
    for blocks in ((model.depth,), (-1,), (0, 12)):
        with pytest.raises(ValueError, match="outside 0"):
            model.forward_taps(x, cls_blocks=blocks)
        with pytest.raises(ValueError, match="outside 0"):
            model.forward_async(x, cls_blocks=blocks)
    with pytest.raises(ValueError, match="outside 0"):
        model.forward_taps(x)                            # the default blocks (3, 6, 9, 11) of a 12-block model on a 3-block one
    model.viz_mode = True
    try:
        with pytest.raises(RuntimeError, match="viz_mode"):
            model.forward_taps(x, cls_blocks=(0,))
        with pytest.raises(RuntimeError, match="viz_mode"):
            model.forward_async(x, final_tokens=True)
    finally:
        model.viz_mode = False
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            model.forward_taps(x, cls_blocks=(0,))
        with pytest.raises(RuntimeError, match="eval"):
            model.forward_async(x, cls_blocks=(0,))
    finally:
        model.eval()
    ats = _prepared("ats_micro")
    ats.dynamic_width = True
    try:
        with pytest.raises(RuntimeError, match="dynamic_width"):
            ats.forward_async(_images("ats_micro"), cls_blocks=(0,))
    finally:
        ats.dynamic_width = False
    # the C entry point: taps together with features_out, a bit at or above depth, blocks without a buffer
    model(x)
    pk, ws = model._packed, model._last_ws
    lib = _lib.load()
    out = torch.empty(B, model._out_width, device="cuda")
    buf = torch.empty(B * model.depth * 197 * model.embed_dim, device="cuda")

    def call(taps, feat=None):
        return lib.tr_vit_forward_taps(C.byref(pk["cfg"]), C.byref(pk["W"]), x.data_ptr(), out.data_ptr(), ws["buf"].data_ptr(), ws["nbytes"],
                                       None, None, None, None, feat, None, B, torch.cuda.current_stream().cuda_stream,
                                       None if taps is None else C.byref(taps))
    assert call(_lib.TrVitTaps(1, buf.data_ptr(), None), feat=buf.data_ptr()) == -5
    assert call(_lib.TrVitTaps(0, None, buf.data_ptr()), feat=buf.data_ptr()) == -5
    assert call(_lib.TrVitTaps(1 << model.depth, buf.data_ptr(), None)) == -5
    assert call(_lib.TrVitTaps(1, None, None)) == -5
    assert call(None) == -3
    assert call(_lib.TrVitTaps(0, None, None), feat=buf.data_ptr()) == 0           # no tap asked for: tr_vit_forward, features_out included
    torch.cuda.synchronize()
