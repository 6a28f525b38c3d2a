"""Dense feature maps at model level (model.forward_dense / forward_async(dense=...)), GPU tier.  The micro fixtures and helpers of
tests/test_decisions_gpu.py: batch 3, the twelve families in bf16, topk / tome / sit also in bf16x3 and fp32, three fixtures at 384 x 384.
The map and its index equal, bit for bit, the numpy restatement (tests/_dense_ref.py) applied to what forward_decisions(final_tokens=True)
returns for the same model and input; a tracer model (every block's output projections zeroed, so the embedded patches travel unchanged)
checks which patch a row stands for without either implementation; the forward keeps its launches, its graph and its bits."""
import numpy as np
import pytest
import torch

from tests import _dense_ref as ref
from tests import _launches
from tests._params import GOLDEN_CASES, case_params
from tests.test_decisions_gpu import B, CASES, FAMILIES, _images, _launch_labels, _prepared, _viz
from tests.test_hip_model import build_model

pytestmark = pytest.mark.gpu

NEW = ["tr_dense_index", "tr_dense_gather"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _host(dec):
    return {key: {blk: t.cpu().numpy() for blk, t in dec[key].items()} for key in ("kept", "assign")}


def _same(a, b):
    assert torch.equal(a[0], b[0]) and a[1]["grid"] == b[1]["grid"]
    assert torch.equal(a[1]["index"], b[1]["index"])
    assert a[1]["features"].dtype == b[1]["features"].dtype and a[1]["features"].shape == b[1]["features"].shape
    bits = torch.int16 if a[1]["features"].dtype == torch.bfloat16 else torch.int32
    assert torch.equal(a[1]["features"].view(bits), b[1]["features"].view(bits))


@pytest.mark.parametrize("name,precision", CASES)
def test_map_and_index_are_the_restatement_of_the_same_models_decisions(name, precision):
    model, x = _prepared(name, precision), _images(name)
    plain = model(x)
    logits_t, taps, dec = model.forward_decisions(x, final_tokens=True)
    logits, dense = model.forward_dense(x, fill=-7.5)
    torch.cuda.synchronize()
    model.check_status()
    assert torch.equal(logits, plain) and torch.equal(logits_t, plain)
    h, w = model.patch_embed.grid_size
    P0, D, n_last = h * w, model.embed_dim, taps["final_tokens"].shape[1]
    assert dense["grid"] == (h, w) and dense["features"].shape == (B, D, h, w) and dense["features"].dtype == torch.float32
    assert dense["index"].shape == (B, P0) and dense["index"].dtype == torch.int32
    stages = model._decision_stages()
    index = ref.dense_index(_host(dec), stages, B, P0, n_last)
    np.testing.assert_array_equal(dense["index"].cpu().numpy(), index)
    tokens = taps["final_tokens"].cpu().numpy()
    want = ref.dense_gather(tokens, index, "NCHW", "fp32", -7.5)
    np.testing.assert_array_equal(dense["features"].cpu().numpy().reshape(B, D, P0).view(np.uint32), want.view(np.uint32))
    family = GOLDEN_CASES[name]["family"]
    if family in ("deit", "heuristic"):
        assert not stages and (index == np.arange(1, P0 + 1)).all()
    elif family in ("topk", "evit", "dyvit", "ats"):
        lost = dense["index"] < 0
        assert lost.any() and (dense["features"].reshape(B, D, P0).permute(0, 2, 1)[lost] == -7.5).all()
    else:
        assert (index >= 1).all()
    if family == "ats":                                          # what the ATS index rests on: valid ids first, sorted, padding at the end
        raw, N0 = model._last_ws["kept"].cpu().numpy(), P0 + 1
        for blk, _, _, k in stages:
            assert ref.ats_valid_first(raw[blk * B * N0: blk * B * N0 + B * k].reshape(B, k))
    # the other layout and the other dtype of the same forward
    _, nhwc = model.forward_dense(x, output_fmt="NHWC", fill=-7.5)
    assert nhwc["features"].shape == (B, h, w, D) and torch.equal(nhwc["index"], dense["index"])
    assert torch.equal(nhwc["features"].permute(0, 3, 1, 2).view(torch.int32), dense["features"].view(torch.int32))
    for fmt, f32 in (("NCHW", dense), ("NHWC", nhwc)):
        logits_b, half = model.forward_dense(x, output_fmt=fmt, dtype=torch.bfloat16, fill=-7.5)
        assert torch.equal(logits_b, plain) and half["features"].dtype == torch.bfloat16
        assert torch.equal(half["features"].view(torch.int16), f32["features"].to(torch.bfloat16).view(torch.int16))
    np.testing.assert_array_equal(half["features"].view(torch.int16).cpu().numpy().view(np.uint16), ref.dense_gather(tokens, index, "NHWC", "bf16", -7.5)
                                  .reshape(B, h, w, D))


# ---- tracer: which patch does a row stand for? ---------------------------------------------------------------------------------------
def _zero_block_outputs(named):
    """Zero every block's attn.proj and mlp.fc2 (weight and bias): the residual stream passes the blocks unchanged."""
    with torch.no_grad():
        for key, t in named:
            if key.startswith("blocks.") and (".attn.proj." in key or ".mlp.fc2." in key):
                t.zero_()


def _rigged(name, precision):
    model, _, _ = build_model(GOLDEN_CASES[name])                # a model of its own: the shared fixtures keep their weights
    _zero_block_outputs(model.named_parameters())
    model.weights_changed()
    model.precision, model.viz_mode = precision, False
    deit, _, _ = build_model(GOLDEN_CASES["deit_micro"])
    own = model.state_dict()
    deit.load_state_dict({k: own[k] for k in deit.state_dict()}, strict=True)
    deit.weights_changed()
    deit.precision = precision
    return model, deit


@pytest.mark.parametrize("name", ["topk_micro", "evit_micro", "dyvit_micro", "ats_micro"])
def test_tracer_a_kept_row_is_its_patch(name):
    model, deit = _rigged(name, "bf16")
    x = _images(name)
    x0 = _viz(deit, x)[1]["Features"][0]                         # the embedded tokens [B, N0, D]: nothing is added to them afterwards
    _, dense = model.forward_dense(x)
    feats = _viz(model, x)[1]["Features"][model.depth - 1]
    index = dense["index"].cpu().numpy()
    assert feats.shape[1] == model._last_tokens[-1] and (index >= 1).any() and (index == -1).any()
    for b in range(B):
        p = np.nonzero(index[b] >= 0)[0]
        np.testing.assert_array_equal(feats[b, index[b, p]].view(np.uint32), x0[b, p + 1].view(np.uint32))


def test_tracer_a_merged_row_is_the_mean_of_its_patches():
    """ToMe in fp32 on the tracer model: the row index[b, p] names is the size-weighted running mean of the patches that share it, so it
    equals their fp64 mean up to fp32 rounding.  The bound comes from the CPU oracle (oracle.tome_forward, fp32) on the same rigged weights:
    its own largest deviation from the fp64 mean of ITS members, times 4 for another summation order.  Measured on the tome_micro fixture:
    oracle 8.94e-08 (bound 3.58e-07), the model 1.19e-07 (|x0| <= 2.55)."""
    import oracle
    case = GOLDEN_CASES["tome_micro"]
    model, deit = _rigged("tome_micro", "fp32")
    x = _images("tome_micro")
    stages = model._decision_stages()
    P0 = model.patch_embed.num_patches

    def deviation(x0, rows, index):
        worst = 0.0
        assert (index >= 1).all()
        for b in range(B):
            for r in range(1, rows.shape[1]):
                members = np.nonzero(index[b] == r)[0]
                assert len(members) >= 1
                mean = x0[b, members + 1].astype(np.float64).mean(axis=0)
                worst = max(worst, float(np.abs(rows[b, r].astype(np.float64) - mean).max()))
        return worst

    cfg, params = case_params(case)
    params = {k: v.clone() for k, v in params.items()}
    _zero_block_outputs(params.items())
    _, oviz = oracle.tome_forward(params, x.cpu(), cfg, "fp32", return_viz=True)
    ox0 = oracle.embed_tokens(oracle.patch_embed(x.cpu(), params["patch_embed.proj.weight"], params["patch_embed.proj.bias"], cfg.patch_size, "fp32"),
                              params["cls_token"], params["pos_embed"]).numpy()
    orows = oviz["Final_Tokens"].numpy()
    oindex = ref.dense_index({"kept": {}, "assign": oviz["Assignment_Maps"]}, stages, B, P0, orows.shape[1])
    bound = 4 * deviation(ox0, orows, oindex)

    x0 = _viz(deit, x)[1]["Features"][0]
    _, dense = model.forward_dense(x)
    feats = _viz(model, x)[1]["Features"][model.depth - 1]
    got = deviation(x0, feats, dense["index"].cpu().numpy())
    print(f"tome tracer: oracle deviation {bound / 4:.3e}, bound {bound:.3e}, model {got:.3e}")
    assert 0 < bound < 1e-4 and got <= bound


@pytest.mark.parametrize("name", FAMILIES)
def test_launches_are_those_of_the_decision_forward_plus_the_two_new_ones(name):
    model, x = _prepared(name), _images(name)
    base = _launch_labels(model, lambda: model(x))
    assert not set(NEW) & set(base)
    dec = _launch_labels(model, lambda: model.forward_decisions(x, final_tokens=True))
    dense = _launch_labels(model, lambda: model.forward_dense(x))
    assert dense == dec + NEW                                                      # behind everything else, in this order
    assert _launch_labels(model, lambda: model.forward_dense(x, output_fmt="NHWC", dtype=torch.bfloat16)) == dense
    assert _launch_labels(model, lambda: model(x)) == base                         # and a plain forward is plain again
    assert _launch_labels(model, lambda: model.forward_decisions(x, final_tokens=True)) == dec


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro", "sit_micro", "ats_micro", "dpcknn_micro"])
def test_graph_replay_plain_launches_and_both_async_slots_agree(name):
    model, x = _prepared(name), _images(name)
    first = model.forward_dense(x)                                  # eager warm-up + capture + replay
    ws = model._last_ws
    key = ("dense", "NCHW", torch.float32, 0.0)
    assert sum(key in k for k in ws["graphs"]) == 1
    _same(model.forward_dense(x), first)                            # replay
    model.use_graph = False
    _same(model.forward_dense(x), first)                            # plain launches
    model.use_graph = True
    handles = [model.forward_async(x, dense={}) for _ in range(4)]  # slots 1, 2, 1, 2
    for h in handles:
        _same(h.result(), first)
    other = model.forward_async(x, dense=dict(output_fmt="NHWC", dtype=torch.bfloat16, fill=2.0)).result()
    assert torch.equal(other[1]["features"].permute(0, 3, 1, 2).view(torch.int16),
                       torch.where((first[1]["index"] < 0).view(B, 1, *first[1]["grid"]), 2.0, first[1]["features"]).to(torch.bfloat16).view(torch.int16))
    torch.cuda.synchronize()
    model.check_status()
    assert torch.equal(model.forward_async(x).result(), first[0])   # without the keyword: the logits alone, as before
    assert torch.equal(model(x), first[0])


def test_a_second_batch_size_and_another_request_recapture():
    model = _prepared("topk_micro")
    x3, x2 = _images("topk_micro"), _images("topk_micro", 2)
    model.use_graph = False
    want3, want2, want3f = model.forward_dense(x3), model.forward_dense(x2), model.forward_dense(x3, fill=1.5)
    model.use_graph = True
    dense_keys = lambda: [k for k in model._last_ws["graphs"] if any(isinstance(e, tuple) and e[:1] == ("dense",) for e in k)]
    for _ in range(2):
        _same(model.forward_dense(x3), want3)
        assert torch.equal(model(x3), want3[0])                    # the plain graph of the same workspace, not the dense one
        _same(model.forward_dense(x3, fill=1.5), want3f)           # another fill: another key, the right result
        _same(model.forward_dense(x3), want3)
        assert len(dense_keys()) == 2
        _same(model.forward_dense(x2), want2)                      # another batch size: a new workspace, a new capture
        assert len(dense_keys()) == 1 and torch.equal(model(x2), want2[0])
    lost = want3[1]["index"] < 0
    assert lost.any() and not torch.equal(want3[1]["features"], want3f[1]["features"])
    assert (want3f[1]["features"].reshape(3, model.embed_dim, -1).permute(0, 2, 1)[lost] == 1.5).all()
    assert want2[1]["index"].shape[0] == 2 and torch.equal(want2[1]["index"], want3[1]["index"][:2])
    model.check_status()


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro"])
def test_pixel_input_equals_float_input(name):
    from tokenreduction_amd import pixels
    model = _prepared(name)
    u8 = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(8))
    mean, std = pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD
    xf = (((u8.float() / 255) - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]).cuda()
    want = model.forward_dense(xf)
    model.set_pixel_input(mean, std)
    try:
        _same(model.forward_dense(u8.cuda()), want)
        _same(model.forward_async(u8.cuda(), dense={}).result(), want)
    finally:
        model.set_pixel_input(None)


def test_alongside_a_headless_average_pooled_deit3_backbone():
    """num_classes=0, global_pool='avg', LayerScale and no_embed_class together, in every precision: the logits (here the pooled features) are
    those of model(x) and the map is the restatement of the same forward's decisions and final tokens."""
    import types
    import tokenreduction_amd as tra
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[1, 2], viz_mode=False)
    torch.manual_seed(5)
    model = tra.TopKVisionTransformer(patch_size=16, embed_dim=128, depth=3, num_heads=2, mlp_ratio=4, qkv_bias=True, num_classes=0,
                                      global_pool="avg", init_values=0.1, no_embed_class=True, args=args).cuda().eval()
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(6)).cuda()
    for precision in ("bf16", "bf16x3", "fp32"):
        model.precision = precision
        plain = model(x)
        _, taps, dec = model.forward_decisions(x, final_tokens=True)
        logits, dense = model.forward_dense(x, output_fmt="NHWC")
        assert plain.shape == (2, 128) and torch.equal(logits, plain)
        index = ref.dense_index(_host(dec), model._decision_stages(), 2, 196, taps["final_tokens"].shape[1])
        np.testing.assert_array_equal(dense["index"].cpu().numpy(), index)
        want = ref.dense_gather(taps["final_tokens"].cpu().numpy(), index, "NHWC", "fp32", 0.0)
        np.testing.assert_array_equal(dense["features"].cpu().numpy().reshape(2, 196, 128).view(np.uint32), want.view(np.uint32))
        assert (index == -1).any() and (index >= 1).any()
    model.check_status()


def test_refusals():
    model, x = _prepared("topk_micro"), _images("topk_micro")
    before = model(x)
    calls = (model.forward_dense, lambda t: model.forward_async(t, dense={}))
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
            ats.forward_dense(_images("ats_micro"))
        with pytest.raises(RuntimeError, match="dynamic_width"):
            ats.forward_async(_images("ats_micro"), dense={})
    finally:
        ats.dynamic_width = False
    with pytest.raises(ValueError, match="output_fmt"):
        model.forward_dense(x, output_fmt="CHWN")
    with pytest.raises(ValueError, match="output_fmt"):
        model.forward_async(x, dense=dict(output_fmt="nchw"))
    with pytest.raises(ValueError, match="dtype"):
        model.forward_dense(x, dtype=torch.float16)
    with pytest.raises(ValueError, match="does not combine"):
        model.forward_async(x, decisions=True, dense={})
    assert torch.equal(model(x), before) and torch.equal(model.forward_dense(x)[0], before)      # and nothing of that stuck
