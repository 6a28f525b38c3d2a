"""Decision taps at model level (model.forward_decisions / forward_async(decisions=True)), GPU tier: the records they give equal the
records of a viz_mode forward of the same model and input; the op's output equals the numpy restatement of that same forward's raw slabs; the
forward keeps its launches, its graph and its bits.  The micro fixtures of tests/test_taps_gpu.py (batch 3, 224 x 224) plus three at
384 x 384 (577 tokens: lists longer than one workgroup pass)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _decisions_ref as ref
from tests import _launches
from tests._params import GOLDEN_CASES, make_images
from tests.test_hip_model import build_model

pytestmark = pytest.mark.gpu

FAMILIES = ["deit_micro", "topk_micro", "evit_micro", "tome_micro", "dyvit_micro", "sit_micro", "dpcknn_micro", "ats_micro", "kmedoids_micro",
            "sinkhorn_micro", "patchmerger_micro", "heuristic_micro_l2"]
LARGE = ["topk_micro_384", "ats_micro_384", "sit_micro_384_kr07"]
CASES = [(n, "bf16") for n in FAMILIES + LARGE] + [(n, p) for n in ("topk_micro", "tome_micro", "sit_micro") for p in ("bf16x3", "fp32")]
B = 3
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _model(name):
    """The family's micro model, viz_mode off, with the recorded density noise where the family draws some (DPC-KNN) and the batch is the
    fixture's."""
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


@functools.lru_cache(maxsize=None)
def _images(name, batch=B):
    case = GOLDEN_CASES[name]
    return make_images(batch, case.get("img_size", 224), case["xseed"]).cuda()


def _viz(model, x):
    model.viz_mode = True
    try:
        return model(x)
    finally:
        model.viz_mode = False


def _model_name(name):
    return GOLDEN_CASES[name]["family"] + "_micro"


def _same_dec(a, b):
    assert a["stages"] == b["stages"]
    for key in ("kept", "kept_count", "assign"):
        assert sorted(a[key]) == sorted(b[key]), key
        for blk in a[key]:
            assert a[key][blk].dtype == torch.int32 and torch.equal(a[key][blk], b[key][blk]), (key, blk)


def _same(a, b):
    assert torch.equal(a[0], b[0])
    _same_dec(a[-1], b[-1])


@pytest.mark.parametrize("name,precision", CASES)
def test_records_equal_the_records_of_a_viz_mode_forward(name, precision):
    from tokenreduction_amd import harness
    model, x = _prepared(name, precision), _images(name)
    _, viz = _viz(model, x)
    plain = model(x)
    logits, dec = model.forward_decisions(x)
    torch.cuda.synchronize()
    model.check_status()
    assert torch.equal(logits, plain)
    locs = model.get_reduction_count()
    assert set(dec["stages"]) == set(locs)
    host = harness.decisions_to_host(dec)
    n_keys = 0
    for i in range(x.shape[0]):
        got, want = harness.decision_records(_model_name(name), locs, host, i), harness.image_records(_model_name(name), locs, viz, i)
        assert list(got) == list(want) == [f"Stage-{loc}" for loc in locs]
        for stage in want:
            assert sorted(got[stage]) == sorted(want[stage]), stage
            for key in want[stage]:
                np.testing.assert_array_equal(got[stage][key], want[stage][key], err_msg=f"image {i} {stage} {key}")
                n_keys += 1
    assert n_keys == 0 if name == "deit_micro" else n_keys >= x.shape[0] * len(locs)


@pytest.mark.parametrize("name", FAMILIES + LARGE)
def test_op_output_is_the_restatement_of_the_same_forwards_raw_slabs(name):
    """Does not lean on viz_mode and the fast path choosing the same tokens: slabs and decisions come from one forward."""
    model, x = _prepared(name), _images(name)
    _, dec = model.forward_decisions(x)
    torch.cuda.synchronize()
    ws = model._last_ws
    stages = model._decision_stages()
    if not stages:
        assert name in ("deit_micro", "heuristic_micro_l2") and ws["dec"]["n"] == 0
        return
    soft = ws["dec"]["soft"]
    want = ref.stage_decisions(ws["kept"].cpu().numpy(), ws["compl"].cpu().numpy(), None if soft is None else soft.cpu().numpy(), stages,
                               x.shape[0], model.patch_embed.num_patches + 1)
    assert dec["stages"] == want["stages"] and len(stages) == 3
    for key in ("kept", "kept_count", "assign"):
        assert sorted(dec[key]) == sorted(want[key]), key
        for blk in want[key]:
            np.testing.assert_array_equal(dec[key][blk].cpu().numpy(), want[key][blk], err_msg=f"{key}[{blk}]")
            assert want[key][blk].min() >= -1                       # nothing out of range in a real forward


def _launch_labels(model, fn):
    """Launch labels of fn() as plain launches, after a warm-up call."""
    graph, model.use_graph = model.use_graph, False
    try:
        fn()
        torch.cuda.synchronize()
        return _launches.labels(fn)
    finally:
        model.use_graph = graph


@pytest.mark.parametrize("name", FAMILIES)
def test_launches_one_more_than_the_plain_forward(name):
    model, x = _prepared(name), _images(name)
    base = _launch_labels(model, lambda: model(x))
    assert "tr_stage_decisions" not in base and "tr_residual_snapshot" not in base
    dec = _launch_labels(model, lambda: model.forward_decisions(x))
    extra = 0 if name in ("deit_micro", "heuristic_micro_l2") else 1
    assert dec.count("tr_stage_decisions") == extra and len(dec) == len(base) + extra
    assert [lab for lab in dec if lab != "tr_stage_decisions"] == base
    if extra:
        assert dec[-1] == "tr_stage_decisions"                                     # behind the executor's launches
    assert _launch_labels(model, lambda: model(x)) == base                         # and a plain forward is plain again


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro", "sit_micro", "ats_micro", "dpcknn_micro"])
def test_graph_replay_plain_launches_and_both_async_slots_agree(name):
    model, x = _prepared(name), _images(name)
    first = model.forward_decisions(x)                              # eager warm-up + capture + replay
    ws = model._last_ws
    assert any(key[-1] is True for key in ws["graphs"])
    _same(model.forward_decisions(x), first)                        # replay
    model.use_graph = False
    _same(model.forward_decisions(x), first)                        # plain launches
    model.use_graph = True
    handles = [model.forward_async(x, decisions=True) for _ in range(4)]      # slots 1, 2, 1, 2
    for h in handles:
        _same(h.result(), first)
    torch.cuda.synchronize()
    model.check_status()
    assert torch.equal(model.forward_async(x).result(), first[0])   # without the keyword: the logits alone, as before
    assert torch.equal(model(x), first[0])


def test_a_second_batch_size_and_a_toggled_flag_recapture():
    model = _prepared("topk_micro")
    x3, x2 = _images("topk_micro"), _images("topk_micro", 2)
    model.use_graph = False
    want3, want2 = model.forward_decisions(x3), model.forward_decisions(x2)
    model.use_graph = True
    for _ in range(2):
        _same(model.forward_decisions(x3), want3)
        assert torch.equal(model(x3), want3[0])                    # the plain graph of the same workspace, not the one with the tap
        keys = list(model._last_ws["graphs"])
        assert sum(key[-1] is True for key in keys) == 1 and len(keys) == 2
        _same(model.forward_decisions(x2), want2)                  # another batch size: a new workspace, a new capture
        assert torch.equal(model(x2), want2[0])
    assert want2[1]["kept"][1].shape[0] == 2 and want3[1]["kept"][1].shape[0] == 3


@pytest.mark.parametrize("name", ["topk_micro", "sit_micro"])
def test_decisions_together_with_output_taps(name):
    model, x = _prepared(name), _images(name)
    solo_dec = model.forward_decisions(x)
    solo_taps = model.forward_taps(x, cls_blocks=(1, 3))
    for both in (model.forward_decisions(x, cls_blocks=(1, 3)), model.forward_async(x, cls_blocks=(1, 3), decisions=True).result()):
        logits, taps, dec = both
        assert torch.equal(logits, solo_dec[0]) and torch.equal(logits, solo_taps[0])
        assert taps["blocks"] == (1, 3) and torch.equal(taps["cls"], solo_taps[1]["cls"])
        _same_dec(dec, solo_dec[1])


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro"])
def test_pixel_input_equals_float_input(name):
    from tokenreduction_amd import pixels
    model = _prepared(name)
    u8 = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(8))
    mean, std = pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD
    xf = (((u8.float() / 255) - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]).cuda()
    want = model.forward_decisions(xf)
    model.set_pixel_input(mean, std)
    try:
        _same(model.forward_decisions(u8.cuda()), want)
        _same(model.forward_async(u8.cuda(), decisions=True).result(), want)
    finally:
        model.set_pixel_input(None)


def test_refusals():
    model, x = _prepared("topk_micro"), _images("topk_micro")
    model.viz_mode = True
    try:
        with pytest.raises(RuntimeError, match="viz_mode"):
            model.forward_decisions(x)
        with pytest.raises(RuntimeError, match="viz_mode"):
            model.forward_async(x, decisions=True)
    finally:
        model.viz_mode = False
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            model.forward_decisions(x)
        with pytest.raises(RuntimeError, match="eval"):
            model.forward_async(x, decisions=True)
    finally:
        model.eval()
    for call in (model.forward_decisions, lambda t: model.forward_async(t, decisions=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(x.cpu())
    ats = _prepared("ats_micro")
    ats.dynamic_width = True
    try:
        with pytest.raises(RuntimeError, match="dynamic_width"):
            ats.forward_decisions(_images("ats_micro"))
        with pytest.raises(RuntimeError, match="dynamic_width"):
            ats.forward_async(_images("ats_micro"), decisions=True)
    finally:
        ats.dynamic_width = False
    assert torch.equal(model.forward_decisions(x)[0], model(x))    # and nothing of that stuck
