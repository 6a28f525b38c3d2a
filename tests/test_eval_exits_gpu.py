"""The four ways out of the eval forward give the same bits: a hipGraph replay, plain launches (use_graph = False), plain launches after
the workspace gave the replay up (GRAPH_MISS_LIMIT inputs at new addresses, one RuntimeWarning), and forward_async on a side stream with
its own workspace.  With a classifier whose rows are padded (5 -> 8: the padded logits columns are cut off on the way out) and headless
(num_classes = 0: the CLS features), for micro Top-K and for micro DPC-KNN with given density noise (one static noise buffer per
workspace slot)."""
import types
import warnings

import pytest
import torch

import tokenreduction_amd as tra
from tests._headless_params import drop_head
from tests._params import GOLDEN_CASES, case_params, make_images

pytestmark = pytest.mark.gpu

B = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _model(family, num_classes):
    case = dict(GOLDEN_CASES[f"{family}_micro"], num_classes=num_classes, batch=B)
    args = types.SimpleNamespace(keep_rate=list(case["keep_rate"]), reduction_loc=list(case["reduction_loc"]), viz_mode=False, k_neighbors=5,
                                 equal_weight=False)
    cls = {"topk": tra.TopKVisionTransformer, "dpcknn": tra.DPCKNNVisionTransformer}[family]
    m = cls(patch_size=16, embed_dim=case["embed_dim"], depth=case["depth"], num_heads=case["num_heads"], mlp_ratio=4, qkv_bias=True,
            num_classes=num_classes, args=args)
    _, params = case_params(case)
    m.load_state_dict(params if num_classes else drop_head(params), strict=True)
    m = m.cuda().eval()
    if family == "dpcknn":
        g = torch.Generator().manual_seed(7)
        m.density_noise = {blk: torch.rand(B, p_in, generator=g) for blk, _, p_in in m._stage_shapes()}
    return m


@pytest.mark.parametrize("num_classes", [5, 0])
@pytest.mark.parametrize("family", ["topk", "dpcknn"])
def test_every_eval_exit_gives_the_same_bits(family, num_classes):
    model = _model(family, num_classes)
    assert model.precision == "bf16" and model.use_graph
    x = make_images(B, 224, 41).cuda()
    outs, tokens = {}, {}

    model(x)
    outs["replay"] = model(x).clone()                               # the second call replays the graph the first one captured
    ws = model._last_ws
    assert len(ws["graphs"]) == 1 and ws["graph_misses"] == 0 and not ws.get("graph_off")
    tokens["replay"] = list(model._last_tokens)

    model._ws = {}                                                   # drop workspaces and graphs
    model.use_graph = False
    outs["plain"] = model(x).clone()
    assert not model._last_ws.get("graphs")
    tokens["plain"] = list(model._last_tokens)
    model.use_graph = True

    model._ws = {}
    keep = []                                                        # hold the copies so the allocator cannot hand an address out twice
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(model.GRAPH_MISS_LIMIT + 2):
            keep.append(x.clone())
            outs["gave_up"] = model(keep[-1]).clone()
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning) and "hipGraph replay is off" in str(w.message)]) == 1
    assert model._last_ws.get("graph_off") and not model._last_ws["graphs"]
    tokens["gave_up"] = list(model._last_tokens)

    model._ws = {}
    outs["async"] = model.forward_async(x).result().clone()
    assert model._last_ws is model._ws[(B, 1)]                       # the side stream's own workspace slot
    tokens["async"] = list(model._last_tokens)
    torch.cuda.synchronize()
    model.check_status()

    want = outs["replay"]
    assert want.shape == (B, num_classes if num_classes else model.embed_dim) and want.is_contiguous() and torch.isfinite(want).all()
    for how, got in outs.items():
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), how
        assert tokens[how] == tokens["replay"], how
    if family == "dpcknn":
        bufs = model._noise_bufs                                                    # one static buffer per workspace slot
        assert set(bufs) == {0, 1} and model._noise_buf is bufs[0] and bufs[0].data_ptr() != bufs[1].data_ptr()
