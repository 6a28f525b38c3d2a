"""Multi-level dense feature maps at model level (model.forward_dense(blocks=...) / forward_async(dense=dict(blocks=...)) /
get_intermediate_layers), GPU tier.  The micro fixtures and helpers of tests/test_decisions_gpu.py: batch 3, the twelve families in bf16, topk /
tome / sit also in bf16x3 and fp32; one DeiT-S-width case.  Every comparison is bitwise: a level's map equals the numpy restatement
(tests/_dense_levels_ref.py) applied to viz_mode's Features of that block (norm=True: to their fp32 final norm) and to the decisions
forward_decisions returns, for the same model and input; the forward keeps its launches, its graph and its bits."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import _dense_levels_ref as lref
from tests import _dense_ref as ref
from tests._params import GOLDEN_CASES, make_images
from tests.test_decisions_gpu import B, FAMILIES, _images, _launch_labels, _prepared, _viz
from tests.test_hip_model import build_model

pytestmark = pytest.mark.gpu

CASES = [(n, "bf16") for n in FAMILIES] + [(n, p) for n in ("topk_micro", "tome_micro", "sit_micro") for p in ("bf16x3", "fp32")]
NEW = ["tr_dense_index_levels", "tr_dense_gather_levels"]
FILL = -7.5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextlib.contextmanager
def _plain_launches(model):
    """Plain launches for the tests that make many different requests in a row: a workspace that sees GRAPH_MISS_LIMIT new graph keys in a row
    stops capturing, and the micro models are shared with the other test modules.  (Replay has a test of its own below.)"""
    graph, model.use_graph = model.use_graph, False
    try:
        yield model
    finally:
        model.use_graph = graph


def _all_features(model, x):
    """viz_mode's residual stream after EVERY block of one forward, as device tensors [B, N_blk, D] (viz_data["Features"] names only the
    blocks the reference records; the executor writes them all)."""
    _viz(model, x)
    ws, tokens, D, n = model._last_ws, model._last_tokens, model.embed_dim, x.shape[0]
    feats, off = [], 0
    for t in tokens:
        feats.append(ws["feat"][off: off + n * t * D].view(n, t, D).clone())
        off += n * t * D
    return feats


@functools.lru_cache(maxsize=None)
def _reference(name, precision):
    """Computed once per model and precision, shared by the tests, left unchanged: the plain logits, viz_mode's rows of every block, the
    final norm of those rows, the host-side decisions and the restated index of every block."""
    from tokenreduction_amd import ops
    model, x = _prepared(name, precision), _images(name)
    with _plain_launches(model):
        plain = model(x)
        feats = _all_features(model, x)
        _, dec = model.forward_decisions(x)
    g, b = model.norm.weight.detach().float().contiguous(), model.norm.bias.detach().float().contiguous()
    normed = [ops.final_tokens_f32(f, g, b, float(model.norm.eps)).view_as(f) for f in feats]
    host = {key: {blk: t.cpu().numpy() for blk, t in dec[key].items()} for key in ("kept", "assign")}
    P0 = model.patch_embed.num_patches
    index = lref.dense_index_levels(host, model._decision_stages(), B, P0, list(range(model.depth)), rows=[f.shape[1] for f in feats])
    torch.cuda.synchronize()
    return plain, [f.cpu().numpy() for f in feats], [f.cpu().numpy() for f in normed], index


def _check_levels(model, out, blocks, rows, index, fmt="NCHW", bf16=False):
    h, w = model.patch_embed.grid_size
    P0, D = h * w, model.embed_dim
    assert out["blocks"] == tuple(blocks) and out["grid"] == (h, w) and len(out["features"]) == len(out["index"]) == len(blocks)
    assert out["cls"].shape == (B, len(blocks), D) and out["cls"].dtype == torch.float32
    for l, blk in enumerate(blocks):
        assert out["index"][l].shape == (B, P0) and out["index"][l].dtype == torch.int32
        np.testing.assert_array_equal(out["index"][l].cpu().numpy(), index[blk], err_msg=f"index of block {blk}")
        feat = out["features"][l]
        assert feat.shape == ((B, D, h, w) if fmt == "NCHW" else (B, h, w, D)) and feat.dtype == (torch.bfloat16 if bf16 else torch.float32)
        want = ref.dense_gather(rows[blk], index[blk], fmt, "bf16" if bf16 else "fp32", FILL)
        got = feat.view(torch.int16).cpu().numpy().view(np.uint16) if bf16 else feat.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got.reshape(want.shape), want if bf16 else want.view(np.uint32), err_msg=f"map of block {blk}")
        np.testing.assert_array_equal(out["cls"][:, l].cpu().numpy().view(np.uint32), rows[blk][:, 0].view(np.uint32), err_msg=f"cls of block {blk}")


@pytest.mark.parametrize("name,precision", CASES)
def test_every_block_unnormed_is_the_restatement_on_viz_modes_features(name, precision):
    plain, feats, _, index = _reference(name, precision)
    model, x = _prepared(name, precision), _images(name)
    blocks = tuple(range(model.depth))
    with _plain_launches(model):
        logits, out = model.forward_dense(x, blocks=blocks, norm=False, fill=FILL)
        logits_t, taps = model.forward_taps(x, cls_blocks=blocks)
        _, other = model.forward_dense(x, blocks=blocks, norm=False, output_fmt="NHWC", dtype=torch.bfloat16, fill=FILL)
    torch.cuda.synchronize()
    model.check_status()
    assert torch.equal(logits, plain) and torch.equal(logits_t, plain)
    _check_levels(model, out, blocks, feats, index)
    assert torch.equal(out["cls"].view(torch.int32), taps["cls"].view(torch.int32))
    family, stages = GOLDEN_CASES[name]["family"], model._decision_stages()
    first = stages[0][0] if stages else model.depth
    assert all((index[blk] == np.arange(1, index.shape[2] + 1)).all() for blk in range(first))       # in front of every stage: the identity
    if family in ("topk", "evit", "dyvit", "ats"):
        assert (index[-1] == -1).any() and all(((index[blk] < 0) | ~(index[blk - 1] < 0)).all() for blk in range(1, model.depth))
    # the other layout and the other dtype of the same forward
    _check_levels(model, other, blocks, feats, index, "NHWC", True)


@pytest.mark.parametrize("name,precision", CASES)
def test_every_block_normed_and_the_last_level_is_todays_map(name, precision):
    plain, _, normed, index = _reference(name, precision)
    model, x = _prepared(name, precision), _images(name)
    blocks = tuple(range(model.depth))
    with _plain_launches(model):
        logits, out = model.forward_dense(x, blocks=blocks, fill=FILL)              # norm=True is the default
        logits_1, single = model.forward_dense(x, fill=FILL)
        _, neg = model.forward_dense(x, blocks=(-1,), fill=FILL)                     # negative entries count from the end
    assert torch.equal(logits, plain)
    _check_levels(model, out, blocks, normed, index)
    assert torch.equal(logits_1, plain) and torch.equal(single["index"], out["index"][-1])
    assert torch.equal(single["features"].view(torch.int32), out["features"][-1].view(torch.int32))
    assert neg["blocks"] == (model.depth - 1,) and torch.equal(neg["features"][0].view(torch.int32), single["features"].view(torch.int32))
    model.check_status()


def _without(labels, extra):
    """labels with one occurrence of each entry of `extra` taken out, searched from the front in order."""
    out, want = [], list(extra)
    for lab in labels:
        if want and lab == want[0]:
            want.pop(0)
        else:
            out.append(lab)
    assert not want, (want, labels)
    return out


@pytest.mark.parametrize("name", FAMILIES)
def test_last_block_untapped_keeps_the_cls_tail_and_the_launch_count(name):
    plain, feats, normed, index = _reference(name, "bf16")
    model, x = _prepared(name), _images(name)
    blocks = (0, model.depth - 2)
    for norm, rows, tap in ((False, feats, "tr_cls_tap"), (True, normed, "tr_final_tokens")):
        with _plain_launches(model):
            logits, out = model.forward_dense(x, blocks=blocks, norm=norm, fill=FILL)
        assert torch.equal(logits, plain)
        _check_levels(model, out, blocks, rows, index)               # the same levels as in the every-block call: both equal the restatement
        base = _launch_labels(model, lambda: model(x))
        got = _launch_labels(model, lambda: model.forward_dense(x, blocks=blocks, norm=norm))
        n_dec = 1 if model._decision_stages() else 0
        # L taps inside the forward, the decisions, the two new launches behind it -- and nothing else changes, the CLS tail included
        assert len(got) == len(base) + len(blocks) + n_dec + 2
        assert got[-2:] == NEW and _without(got[:-2], [tap] * len(blocks) + ["tr_stage_decisions"] * n_dec) == base
        assert ("attention_kernel<cls>" in got) == ("attention_kernel<cls>" in base)
    if GOLDEN_CASES[name]["family"] in ("deit", "sit", "dpcknn"):
        assert "attention_kernel<cls>" in base                       # (these reduce nothing inside the last block: the tail runs)


@pytest.mark.parametrize("name", FAMILIES)
def test_launch_accounting_with_the_last_block_tapped_and_the_old_calls_unchanged(name):
    model, x = _prepared(name), _images(name)
    base = _launch_labels(model, lambda: model(x))
    taps = _launch_labels(model, lambda: model.forward_taps(x, cls_blocks=(0, model.depth - 1)))
    dec = _launch_labels(model, lambda: model.forward_decisions(x))
    dense = _launch_labels(model, lambda: model.forward_dense(x))
    full = _launch_labels(model, lambda: model.forward_taps(x, cls_blocks=(), final_tokens=True))      # the last block at full width
    blocks = tuple(range(model.depth))
    n_dec = 1 if model._decision_stages() else 0
    got = _launch_labels(model, lambda: model.forward_dense(x, blocks=blocks, norm=False))
    assert len(got) == len(full) - 1 + len(blocks) + n_dec + 2
    assert got[-2:] == NEW and _without(got[:-2], ["tr_cls_tap"] * len(blocks) + ["tr_stage_decisions"] * n_dec) == _without(full, ["tr_final_tokens"])
    assert "attention_kernel<cls>" not in got
    # the calls that were there before issue what they issued, before and after a level call
    assert _launch_labels(model, lambda: model(x)) == base and _launch_labels(model, lambda: model.forward_taps(x, cls_blocks=(0, model.depth - 1))) == taps
    assert _launch_labels(model, lambda: model.forward_decisions(x)) == dec and _launch_labels(model, lambda: model.forward_dense(x)) == dense
    assert not (set(NEW) | {"tr_final_tokens"}) & set(base) and not set(NEW) & set(taps + dec + dense)
    assert dense[-2:] == ["tr_dense_index", "tr_dense_gather"] and dec == base + ["tr_stage_decisions"] * n_dec


@functools.lru_cache(maxsize=None)
def _small():
    model, _, _ = build_model(GOLDEN_CASES["topk_small_kr07"])
    model.viz_mode = False
    return model


def test_deit_s_width_through_forward_dense_and_both_async_slots():
    """Under the `concurrent` hint (the side streams) the norm2 runs inside the fused Mlp and both residuals are pending at the tap."""
    from tokenreduction_amd import ops
    case = GOLDEN_CASES["topk_small_kr07"]
    model = _small()
    x = make_images(2, 224, case["xseed"]).cuda()
    blocks = (2, 3, 5, 8, 11)
    plain = model(x)
    feats = _all_features(model, x)
    g, b = model.norm.weight.detach().float().contiguous(), model.norm.bias.detach().float().contiguous()
    normed = [ops.final_tokens_f32(f, g, b, float(model.norm.eps)).view_as(f).cpu().numpy() for f in feats]
    feats = [f.cpu().numpy() for f in feats]
    _, dec = model.forward_decisions(x)
    host = {key: {blk: t.cpu().numpy() for blk, t in dec[key].items()} for key in ("kept", "assign")}
    index = lref.dense_index_levels(host, model._decision_stages(), 2, 196, list(range(12)), rows=[f.shape[1] for f in feats])
    h, w = model.patch_embed.grid_size

    def check(res, rows):
        logits, out = res
        assert torch.equal(logits, plain) and out["blocks"] == blocks
        for l, blk in enumerate(blocks):
            np.testing.assert_array_equal(out["index"][l].cpu().numpy(), index[blk])
            want = ref.dense_gather(rows[blk], index[blk], "NCHW", "fp32", 0.0)
            np.testing.assert_array_equal(out["features"][l].cpu().numpy().reshape(want.shape).view(np.uint32), want.view(np.uint32),
                                          err_msg=f"block {blk}")
            np.testing.assert_array_equal(out["cls"][:, l].cpu().numpy().view(np.uint32), rows[blk][:, 0].view(np.uint32))
    for norm, rows in ((False, feats), (True, normed)):
        check(model.forward_dense(x, blocks=blocks, norm=norm), rows)
        handles = [model.forward_async(x, dense=dict(blocks=blocks, norm=norm)) for _ in range(2)]      # slots 1 and 2
        for hd in handles:
            check(hd.result(), rows)
    torch.cuda.synchronize()
    model.check_status()
    assert torch.equal(model.forward_async(x).result(), plain)


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro", "sit_micro", "ats_micro", "dpcknn_micro"])
def test_graph_replay_plain_launches_and_both_async_slots_agree(name):
    model, x = _prepared(name), _images(name)
    blocks = (1, 3)

    def same(a, b):
        assert torch.equal(a[0], b[0]) and a[1]["blocks"] == b[1]["blocks"] and torch.equal(a[1]["cls"].view(torch.int32), b[1]["cls"].view(torch.int32))
        for l in range(len(blocks)):
            assert torch.equal(a[1]["index"][l], b[1]["index"][l])
            assert torch.equal(a[1]["features"][l].view(torch.int32), b[1]["features"][l].view(torch.int32))
    first = model.forward_dense(x, blocks=blocks, norm=False)        # eager warm-up + capture + replay
    key = ("dense", "NCHW", torch.float32, 0.0, blocks, False)
    assert sum(key in k for k in model._last_ws["graphs"]) == 1
    same(model.forward_dense(x, blocks=blocks, norm=False), first)   # replay
    other = model.forward_dense(x, blocks=blocks, norm=True)         # norm is part of the key: another graph, other maps
    assert sum(("dense", "NCHW", torch.float32, 0.0, blocks, True) in k for k in model._last_ws["graphs"]) == 1
    assert not torch.equal(other[1]["features"][0], first[1]["features"][0])
    same(model.forward_dense(x, blocks=(3, 1), norm=False), first)   # the same request in another order: the same key
    same(model.forward_dense(x, blocks=blocks, norm=False), first)
    model.use_graph = False
    same(model.forward_dense(x, blocks=blocks, norm=False), first)   # plain launches
    model.use_graph = True
    for hd in [model.forward_async(x, dense=dict(blocks=blocks, norm=False)) for _ in range(4)]:       # slots 1, 2, 1, 2
        same(hd.result(), first)
    torch.cuda.synchronize()
    model.check_status()
    assert torch.equal(model(x), first[0]) and torch.equal(model.forward_dense(x)[0], first[0])


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro"])
def test_pixel_input_equals_float_input(name):
    from tokenreduction_amd import pixels
    model = _prepared(name)
    u8 = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(8))
    mean, std = pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD
    xf = (((u8.float() / 255) - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]).cuda()
    want = model.forward_dense(xf, blocks=(0, 2, 3))
    model.set_pixel_input(mean, std)
    try:
        for got in (model.forward_dense(u8.cuda(), blocks=(0, 2, 3)), model.forward_async(u8.cuda(), dense=dict(blocks=(0, 2, 3))).result()):
            assert torch.equal(got[0], want[0]) and torch.equal(got[1]["cls"].view(torch.int32), want[1]["cls"].view(torch.int32))
            for l in range(3):
                assert torch.equal(got[1]["index"][l], want[1]["index"][l])
                assert torch.equal(got[1]["features"][l].view(torch.int32), want[1]["features"][l].view(torch.int32))
    finally:
        model.set_pixel_input(None)


@pytest.mark.parametrize("name", ["topk_micro", "dpcknn_micro"])
def test_get_intermediate_layers_is_timms_shape_over_forward_dense(name):
    model, x = _prepared(name), _images(name)
    h, w = model.patch_embed.grid_size
    D, depth = model.embed_dim, model.depth
    model.use_graph = False                                          # (many requests in a row: see _plain_launches; _prepared switches it on again)
    for n, blocks in ((2, (depth - 2, depth - 1)), ((1, 3), (1, 3)), ((-1, 0), (0, depth - 1)), (1, (depth - 1,))):
        for norm in (False, True):
            _, nchw = model.forward_dense(x, blocks=blocks, norm=norm, fill=1.5)
            _, nhwc = model.forward_dense(x, blocks=blocks, norm=norm, output_fmt="NHWC", fill=1.5)
            flat = model.get_intermediate_layers(x, n, norm=norm, fill=1.5)
            grid = model.get_intermediate_layers(x, n, reshape=True, norm=norm, fill=1.5)
            both = model.get_intermediate_layers(x, n, reshape=True, return_class_token=True, norm=norm, fill=1.5)
            assert isinstance(flat, tuple) and isinstance(grid, tuple) and len(flat) == len(grid) == len(both) == len(blocks)
            for l in range(len(blocks)):
                assert flat[l].shape == (B, h * w, D) and torch.equal(flat[l].view(torch.int32), nhwc["features"][l].reshape(B, h * w, D).view(torch.int32))
                assert grid[l].shape == (B, D, h, w) and torch.equal(grid[l].view(torch.int32), nchw["features"][l].view(torch.int32))
                tok, cls = both[l]
                assert torch.equal(tok, grid[l]) and cls.shape == (B, D) and torch.equal(cls.view(torch.int32), nchw["cls"][:, l].view(torch.int32))
    half = model.get_intermediate_layers(x, 1, dtype=torch.bfloat16)
    assert half[0].dtype == torch.bfloat16 and half[0].shape == (B, h * w, D)
    with pytest.raises(ValueError, match="blocks"):
        model.get_intermediate_layers(x, 0)
    with pytest.raises(ValueError, match="blocks"):
        model.get_intermediate_layers(x, depth + 1)


def test_refusals():
    model, x = _prepared("topk_micro"), _images("topk_micro")
    before = model(x)
    model.use_graph = False                                          # (_prepared switches it on again)
    calls = (lambda t: model.forward_dense(t, blocks=(1, 2)), lambda t: model.forward_async(t, dense=dict(blocks=(1, 2))),
             lambda t: model.get_intermediate_layers(t, 2))
    model.viz_mode = True
    try:
        for call in calls:
            with pytest.raises(RuntimeError, match="viz_mode"):
                call(x)
    finally:
        model.viz_mode = False
    model.train()
    try:
        for call in calls:
            with pytest.raises(RuntimeError, match="eval"):
                call(x)
    finally:
        model.eval()
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(x.cpu())
    ats = _prepared("ats_micro")
    ats.dynamic_width = True
    try:
        with pytest.raises(RuntimeError, match="dynamic_width"):
            ats.forward_dense(_images("ats_micro"), blocks=(1,))
        with pytest.raises(RuntimeError, match="dynamic_width"):
            ats.forward_async(_images("ats_micro"), dense=dict(blocks=(1,)))
    finally:
        ats.dynamic_width = False
    for bad in ((4,), (-5,), (0, 7), (1, 1), (1, -3), ()):
        with pytest.raises(ValueError, match="blocks"):
            model.forward_dense(x, blocks=bad)
        with pytest.raises(ValueError, match="blocks"):
            model.forward_async(x, dense=dict(blocks=bad))
    with pytest.raises(ValueError, match="output_fmt"):
        model.forward_dense(x, blocks=(1,), output_fmt="CHWN")
    with pytest.raises(ValueError, match="dtype"):
        model.forward_dense(x, blocks=(1,), dtype=torch.float16)
    with pytest.raises(ValueError, match="does not combine"):
        model.forward_async(x, decisions=True, dense=dict(blocks=(1,)))
    assert torch.equal(model(x), before) and torch.equal(model.forward_dense(x)[0], before)      # and nothing of that stuck
    assert torch.equal(model.forward_dense(x, blocks=(1, 2))[0], before)
