"""CLS tail of the eval forward (tr_set_cls_tail / ops.set_cls_tail): in the last block the attention computes the CLS query only and proj,
norm2, fc1, fc2 run on the B CLS rows -- the only rows the final norm and the head read.  Per-row work of the same kernels, so every
comparison here is torch.equal, tail on against tail off, in the same process.  A captured graph keeps the form it was captured with: the
helpers drop the model's workspaces (and their graphs) whenever they flip the switch."""
import os
import types

import numpy as np
import pytest
import torch

from tests._hires_params import HIRES_CASES
from tests._launches import forward_launches
from tests._params import GOLDEN_CASES, make_images
from tests.test_hip_model import build_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(autouse=True)
def _tail_back_on():
    from tokenreduction_amd import ops
    yield
    ops.set_cls_tail(True)


def _set(model, on):
    from tokenreduction_amd import ops
    ops.set_cls_tail(on)
    model._ws = {}                       # workspaces and their captured graphs: the next forward enqueues (and captures) in the new form


def _off_on(model, x, fn=None):
    """(tail off, tail on) results of fn(model, x) -- model(x) by default."""
    fn = fn or (lambda m, v: m(v))
    outs = []
    for on in (False, True):
        _set(model, on)
        out = fn(model, x)
        torch.cuda.synchronize()
        model.check_status()
        outs.append(out.clone() if torch.is_tensor(out) else out)
    return outs


def _prepare(name, case):
    model, _, _ = build_model(case)
    model.viz_mode = False
    path = os.path.join(os.path.dirname(__file__), "golden", name + ".npz")
    if os.path.exists(path):
        g = np.load(path)
        noise = {int(k.split("_")[1]): torch.from_numpy(g[k]) for k in g.files if k.startswith("noise_")}
        if noise:
            model.density_noise = noise
    return model


def _small(name, keep_rate, loc, **kw):
    import tokenreduction_amd as tra
    args = types.SimpleNamespace(keep_rate=list(keep_rate), reduction_loc=list(loc), dyvit_distill=False, k_neighbors=5, equal_weight=False,
                                 cluster_iters=3, sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None,
                                 viz_mode=False)
    torch.manual_seed(0)
    return tra.create_model(name, pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0, args=args, **kw).cuda().eval()


EVAL_CASES = {n: c for n, c in GOLDEN_CASES.items() if not c.get("train_only")}
# beyond 224 tokens in the last block (online-softmax attention): dense, with key masks, and after three pre-block reductions
LONG_CASES = {n: HIRES_CASES[n] for n in ("deit_micro_448", "heuristic_micro_448", "dyvit_micro_448", "sit_micro_448")}


@pytest.mark.parametrize("name", list(EVAL_CASES) + list(LONG_CASES))
def test_every_family_gives_the_same_logits(name):
    """Every family at its micro fixture config, the DeiT-S and DeiT-B configs, 384 x 384 and 448 x 448 inputs (bf16; the fp32 and bf16x3
    executors always run the full-width block).  In-block families whose last block reduces take the full-width path either way."""
    case = EVAL_CASES.get(name) or LONG_CASES[name]
    model = _prepare(name, case)
    x = make_images(case["batch"], case.get("img_size", 224), case["xseed"]).cuda()

    def run(m, v):
        np.random.seed(case["xseed"])          # K-Medoids equal_weight draws its first medoids from numpy's global generator
        return m(v)
    off, on = _off_on(model, x, run)
    assert torch.isfinite(off).all()
    assert torch.equal(off, on)


@pytest.mark.parametrize("factory,keep_rate,loc", [("topk_small_patch16_224", [0.7], [3, 6, 9]),            # the headline
                                                   ("deit_small_patch16_224_local", [1.0], []),             # dense DeiT-S
                                                   ("evit_small_patch16_224", [0.5], [3, 6, 9]),
                                                   ("tome_small_patch16_224", [0.7], [3, 6, 9])])           # log-size key bias in the last block
def test_batch_256_gives_the_same_logits(factory, keep_rate, loc):
    model = _small(factory, keep_rate, loc)
    x = make_images(256, 224, 5).cuda()
    off, on = _off_on(model, x)
    assert off.shape == (256, 1000) and torch.isfinite(off).all()
    assert torch.equal(off, on)
    # ... and with two forwards in flight (whole-block fused Mlp launches in the full-width form)
    off2, on2 = _off_on(model, x, lambda m, v: m.forward_async(v).result())
    assert torch.equal(off2, off) and torch.equal(on2, off)


def test_deit_base_batch_64():
    model = _small("deit_base_patch16_224_local", [1.0], [])
    x = make_images(64, 224, 6).cuda()
    off, on = _off_on(model, x)
    assert torch.isfinite(off).all() and torch.equal(off, on)


@pytest.mark.parametrize("name", ["topk_micro", "deit_small", "deit_micro_448"])
def test_headless_model(name):
    case = EVAL_CASES.get(name) or LONG_CASES[name]
    model = _prepare(name, case)
    model.reset_classifier(0)
    x = make_images(case["batch"], case.get("img_size", 224), 7).cuda()
    off, on = _off_on(model, x)
    assert off.shape == (case["batch"], case["embed_dim"]) and torch.isfinite(off).all()
    assert torch.equal(off, on)


@pytest.mark.parametrize("name", ["deit_micro", "topk_small_kr07"])
def test_pixel_input(name):
    case = EVAL_CASES[name]
    model = _prepare(name, case)
    model.set_pixel_input()
    u8 = torch.randint(0, 256, (case["batch"], 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(8)).cuda()
    off, on = _off_on(model, u8)
    assert torch.isfinite(off).all() and torch.equal(off, on)


@pytest.mark.parametrize("name", ["deit_micro", "topk_small_kr07", "sit_micro", "deit_micro_448"])
def test_forward_async_and_model_call_both_honour_the_switch(name):
    case = EVAL_CASES.get(name) or LONG_CASES[name]
    model = _prepare(name, case)
    x = make_images(case["batch"], case.get("img_size", 224), 9).cuda()
    off, on = _off_on(model, x)
    a_off, a_on = _off_on(model, x, lambda m, v: m.forward_async(v).result())
    assert torch.equal(off, on) and torch.equal(a_off, off) and torch.equal(a_on, off)


def _launch_labels(model, x):
    """Launch labels of one plain-launch forward."""
    return [label for label, _, _ in forward_launches(model, x)]


def test_the_switch_changes_the_launches_and_only_where_the_predicate_holds():
    """The comparisons above would also pass if the switch did nothing: the executor's launch labels show the CLS-only attention exactly
    where the last block is plain and no Features are asked for."""
    case = EVAL_CASES["deit_micro"]
    model = _prepare("deit_micro", case)
    x = make_images(case["batch"], 224, 3).cuda()
    _set(model, True)
    on = _launch_labels(model, x)
    _set(model, False)
    off = _launch_labels(model, x)
    assert on.count("attention_kernel<cls>") == 1 and on.count("attention_kernel") == case["depth"] - 1
    assert off.count("attention_kernel<cls>") == 0 and off.count("attention_kernel") == case["depth"]
    assert len(on) == len(off)                        # launch for launch: attention, proj, norm2, fc1, fc2 in their short forms
    _set(model, True)
    model.viz_mode = True                             # Features wants every row of the last block
    assert "attention_kernel<cls>" not in _launch_labels(model, x)
    model.viz_mode = False
    model.precision = "fp32"                          # the validation executors keep the full-width block
    _set(model, True)
    assert not any("<cls>" in lab for lab in _launch_labels(model, x))
    # a last block that reduces inside the block
    tk = _prepare("topk_micro", EVAL_CASES["topk_micro"])
    _set(tk, True)
    assert not any("<cls>" in lab for lab in _launch_labels(tk, make_images(3, 224, 4).cuda()))


@pytest.mark.parametrize("name", ["deit_micro", "topk_micro", "dpcknn_micro", "sit_micro", "topk_small_kr07"])
def test_viz_mode_returns_the_same_features_and_kept_indices(name):
    """viz_mode's `Features` needs every row of the last block: the predicate turns the tail off, whatever the switch says."""
    case = EVAL_CASES[name]
    model = _prepare(name, case)
    model.viz_mode = True
    x = make_images(case["batch"], 224, case["xseed"]).cuda()
    (l_off, v_off), (l_on, v_on) = _off_on(model, x, lambda m, v: m(v))
    assert torch.equal(l_off, l_on)
    assert sorted(v_off) == sorted(v_on)
    for key in v_off:
        assert sorted(v_off[key]) == sorted(v_on[key]), key
        for blk in v_off[key]:
            np.testing.assert_array_equal(np.asarray(v_off[key][blk]), np.asarray(v_on[key][blk]), err_msg=f"{key}[{blk}]")
    model.viz_mode = False
    _set(model, True)
    assert torch.equal(model(x), l_off)


@pytest.mark.parametrize("factory,keep_rate,loc", [("tome_small_patch16_224", [196 - 16 * (i + 1) for i in range(12)], list(range(12))),
                                                   ("topk_small_patch16_224", [0.7], [3, 6, 11]),
                                                   ("evit_small_patch16_224", [0.7], [3, 6, 11])])
def test_a_last_block_that_reduces_keeps_the_full_width_path(factory, keep_rate, loc):
    model = _small(factory, keep_rate, loc)
    x = make_images(8, 224, 11).cuda()
    _set(model, True)
    assert not any("<cls>" in lab for lab in _launch_labels(model, x))
    off, on = _off_on(model, x)
    assert torch.isfinite(off).all() and torch.equal(off, on)


@pytest.mark.parametrize("factory,keep_rate,loc,batch", [("topk_small_patch16_224", [0.7], [3, 6, 9], 256),
                                                         ("deit_small_patch16_224_local", [1.0], [], 64)])
def test_race_screen(factory, keep_rate, loc, batch):
    """100 back-to-back forwards with no host synchronisation in between, each equal to the first (which equals the full-width forward):
    one at a time, then two in flight.  The tail's buffers (compact rows in the shared scratch, both residual buffers) are reused by the
    next forward's first blocks: a difference is a race or a read of a row the tail no longer writes."""
    model = _small(factory, keep_rate, loc)
    x = make_images(batch, 224, 12).cuda()
    _set(model, False)
    want = model(x).clone()
    _set(model, True)
    outs = [model(x) for _ in range(100)]
    torch.cuda.synchronize()
    assert all(torch.equal(o, want) for o in outs)
    handles = []
    outs = []
    for k in range(100):
        handles.append(model.forward_async(x))
        if len(handles) > 2:
            outs.append(handles.pop(0).result())
    outs += [h.result() for h in handles]
    torch.cuda.synchronize()
    model.check_status()
    assert len(outs) == 100 and all(torch.equal(o, want) for o in outs)


@pytest.mark.parametrize("N,H,masked", [(197, 6, False), (68, 6, False), (138, 2, True), (17, 1, False), (224, 3, True), (225, 2, False),
                                        (785, 2, True), (577, 12, False)])
def test_attention_cls_equals_row_0_of_the_full_attention(N, H, masked):
    from tokenreduction_amd import ops
    B = 5
    g = torch.Generator().manual_seed(N + H)
    qkv = (1.5 * torch.randn(B * N, 3 * H * 64, generator=g)).bfloat16().cuda()
    size = None
    if masked:                                    # log-size bias with some keys masked out (never the CLS key)
        size = (1.0 + torch.randint(0, 4, (B, N), generator=g)).float()
        size[:, 3::5] = 0.0
        size = size.cuda()
    full, _ = ops.attention(qkv, B, N, H, size=size)
    got = ops.attention_cls(qkv, B, N, H, size=size)
    assert torch.equal(got.view(torch.int16), full.view(B, N, H * 64)[:, 0].contiguous().view(torch.int16))


@pytest.mark.parametrize("N", [1, 16, 17, 32, 33, 98, 177, 224, 225, 256, 257, 1025])
def test_attention_cls_equals_row_0_at_the_block_edges(N):
    """The first query block alone at the 16- and 32-query block edges and both sides of the 224-token dispatch, with and without a key
    bias, on the shifted and masked inputs of tests/_attn_fwd_ref.py as well (a masked key 25 above every real one).  98 and 177: the
    CLS instantiations for 4 and 6 key blocks, which no other N of this file reaches."""
    from tokenreduction_amd import ops
    from tests import _attn_fwd_ref as R
    B, H = R.shape_of(N)
    cases = [(kind, bias) for kind in ("gaussian", "shift_neg") for bias in (False, True)] + ([("masked_dominant", True)] if N >= 2 else [])
    for kind, bias in cases:
        qkv, size = R.build(kind, B, N, H, bias)
        qkv, size = qkv.cuda(), None if size is None else size.cuda()
        full, _ = ops.attention(qkv, B, N, H, size=size)
        got = ops.attention_cls(qkv, B, N, H, size=size)
        assert torch.equal(got.view(torch.int16), full.view(B, N, H * 64)[:, 0].contiguous().view(torch.int16)), (kind, bias)
