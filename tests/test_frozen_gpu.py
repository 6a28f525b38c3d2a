"""GPU: frozen parameters (requires_grad False) in the HIP backward -- tr_vit_backward leaves the gradient work of a NULL unit out and stops
at the lowest block that owns a gradient (csrc/tr_train.hip, training.TrainState.grads_struct).

Every model-level test compares a masked run with the all-trainable run of the same build on the same inputs and the same draws
(the seeds are set before every forward: Gumbel, DPC-KNN density noise, DropPath and dropout masks are device draws).  What is still
computed must be the same BITS: a frozen norm runs ln_bwd_kernel without its parameter partials, which does not touch the row arithmetic;
at D = 128 every Linear gradient is its own wgrad_kernel launch, so leaving one out changes nothing for the others.  At D = 192 a block's
four layers are one grouped producer/consumer launch whose split sizes are planned per group: qkv and proj alone may get another split,
an fp32 re-association (REASSOC_BOUND below)."""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import _launches
from tests._params import GOLDEN_CASES, dyvit_train_loss, grad_labels, make_images
from tests.test_hip_model import build_model

pytestmark = pytest.mark.gpu

TR_ERR_NULL = -3
LN_FROZEN = "ln_bwd_kernel<no_params>"
WGRAD = ("wgrad_kernel", "wgrad_pc_kernel")
DGRAD = ("gemm_bf16_pc<EPI_BF16>", "gemm_bf16_pc<EPI_DGELU>")
ATTN = ("attention_bwd_kernel", "attention_bwd_kernel<policy>", "attention_bwd_long", "attention_bwd_long<policy>")

# qkv / proj gradients of the two-layer group (attn-only) against the same layers inside the four-layer group, D = 192: per-parameter
# relative L2.  Measured on MI355X at the shapes of test_attn_only_at_the_grouped_width (profiles/frozen_lab.md): largest value per case
# 9.70e-08 (topk), 9.57e-08 (evit), 9.78e-08 (tome), 8.07e-08 (sit_tiny); 7 to 11 of the 16 parameters differ at all -- plan_group picks
# other split sizes for two layers than for four, an fp32 re-association.  The bound is ten times the largest measured value.  It may
# never exceed 1e-4: one bf16 rounding of an operand is 4e-3 and a dropped 64-token slab at least 1/13 of the sum, so anything above
# that is a bug and not a re-association.
REASSOC_BOUND = 10 * 9.78e-08
assert REASSOC_BOUND <= 1e-4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---------------------------------------------------------------------------------------------------------------- library level
def _ln_bwd(lib, dy, x, gamma, g_in, g_out, gb_out, idx, K, n_in, n_out, g_fused, dgamma, dbeta, ws, M, D, add=False):
    p = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    nws = 0 if ws is None else ws.numel()
    if add:
        return lib.tr_layernorm_bwd_scatter_add(p(dy), p(x), p(gamma), p(g_in), p(g_out), p(idx), K, n_out, p(dgamma), p(dbeta), 0, p(ws), nws, M, D,
                                                1e-6, s)
    return lib.tr_layernorm_bwd(p(dy), p(x), D, p(gamma), p(g_in), D, p(g_out), D, p(gb_out), p(idx), K, n_in, n_out, p(g_fused), p(dgamma),
                                p(dbeta), 0, p(ws), nws, M, D, 1e-6, s)


def _ln_pair(M, D, with_gin, with_gb, idx=None, K=0, n_in=0, n_out=0, fused=False, add=False, seed=0):
    """The same LayerNorm backward with d_gamma / d_beta buffers and without: outputs of both, the frozen call's launch record and its
    (sentinel-filled) workspace."""
    from tokenreduction_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(1000 * D + 10 * M + seed)
    dy = torch.randn(M, D, generator=g).to(torch.bfloat16).cuda()
    x = (torch.randn(M, D, generator=g) * 2 + 0.3).cuda()
    gamma = (1 + 0.2 * torch.randn(D, generator=g)).cuda()
    g_in = torch.randn(M, D, generator=g).cuda() if with_gin else None
    rows = M if idx is None else (M // n_in) * n_out
    nws = lib.tr_layernorm_bwd_workspace_floats(M, D)
    outs = []
    for frozen in (False, True):
        g_out = torch.zeros(rows, D, device="cuda")
        gb_out = torch.zeros(rows, D, dtype=torch.bfloat16, device="cuda") if with_gb and not add else None
        g_fused = torch.zeros(M // n_in, D, device="cuda") if fused else None
        ws = torch.full((nws,), 12345.0, device="cuda")
        dgamma, dbeta = (None, None) if frozen else (torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"))
        rc = []
        recs = _launches.record(lambda: rc.append(_ln_bwd(lib, dy, x, gamma, g_in, g_out, gb_out, idx, K, n_in, n_out, g_fused, dgamma, dbeta,
                                                          ws, M, D, add)))
        assert rc == [0], _lib.load().tr_last_error()
        outs.append(dict(g=g_out, gb=gb_out, fused=g_fused, ws=ws, labels=[r[0] for r in recs], dgamma=dgamma))
    return outs


def _assert_ln_pair(full, frozen):
    assert torch.equal(frozen["g"], full["g"])
    assert (frozen["gb"] is None) == (full["gb"] is None) and (frozen["gb"] is None or torch.equal(frozen["gb"], full["gb"]))
    assert frozen["fused"] is None or torch.equal(frozen["fused"], full["fused"])
    assert bool((frozen["ws"] == 12345.0).all()), "the frozen LayerNorm backward wrote into the workspace"
    assert frozen["labels"] == [LN_FROZEN], frozen["labels"]               # one launch, the new label, no reduce behind it
    assert full["labels"][0] == "ln_bwd_kernel" and LN_FROZEN not in full["labels"] and bool(full["dgamma"].abs().sum() > 0)


@pytest.mark.parametrize("D", [64, 192, 1024])
@pytest.mark.parametrize("M", [1, 5, 197 * 2])
def test_layernorm_bwd_without_parameter_gradients_writes_the_same_bits(M, D):
    for with_gin in (False, True):
        for with_gb in (False, True):
            _assert_ln_pair(*_ln_pair(M, D, with_gin, with_gb))


@pytest.mark.parametrize("D", [64, 192, 1024])
def test_layernorm_bwd_scatter_forms_without_parameter_gradients(D):
    B, K, n_out = 5, 3, 9
    idx = torch.tensor([[0, 3, 7], [1, 2, 4], [7, 6, 5], [2, 0, 1], [4, 7, 3]], dtype=torch.int32).cuda()          # distinct ids in [0, n_out - 1)
    _assert_ln_pair(*_ln_pair(B * (K + 1), D, True, True, idx=idx, K=K, n_in=K + 1, n_out=n_out))
    _assert_ln_pair(*_ln_pair(B * (K + 2), D, True, True, idx=idx, K=K, n_in=K + 2, n_out=n_out, fused=True))
    # scatter-add, repeated ids (at most two rows per destination: a two-term float sum does not depend on the order of the atomics)
    rep = torch.tensor([[2, 2, 5], [0, 1, 0], [7, 3, 3], [4, 4, 6], [1, 5, 1]], dtype=torch.int32).cuda()
    _assert_ln_pair(*_ln_pair(B * (K + 1), D, True, False, idx=rep, K=K, n_in=K + 1, n_out=n_out, add=True))


def test_layernorm_bwd_half_null_pair_is_an_error():
    from tokenreduction_amd import _lib
    lib = _lib.load()
    M, D = 5, 64
    dy = torch.zeros(M, D, dtype=torch.bfloat16, device="cuda")
    x, gamma, g_out, one = torch.randn(M, D).cuda(), torch.ones(D).cuda(), torch.zeros(M, D).cuda(), torch.zeros(D).cuda()
    ws = torch.zeros(lib.tr_layernorm_bwd_workspace_floats(M, D), device="cuda")
    for dgamma, dbeta in ((one, None), (None, one)):
        rc = []
        recs = _launches.record(lambda: rc.append(_ln_bwd(lib, dy, x, gamma, None, g_out, None, None, 0, 0, 0, None, dgamma, dbeta, ws, M, D)))
        assert rc == [TR_ERR_NULL] and recs == []


# ------------------------------------------------------------------------------------------------------------------ model level
def _case(name, wide=False):
    case = dict(GOLDEN_CASES[name])
    if wide:           # the *_tiny width: tr_wgrad_pc_fits holds, a block's four Linear gradients are one grouped launch
        case.update(embed_dim=192, num_heads=3)
    return case


def _model(case):
    model, _, _ = build_model(case)
    model.viz_mode = False
    return model.train()


def _step(case, model, record=False):
    """One forward + loss + backward on the case's own batch with every draw fixed.  (loss, {name: grad clone or None}, launch record of
    the backward)."""
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    x = make_images(case["batch"], case.get("img_size", 224), case["xseed"]).cuda()
    out = model(x)
    y = grad_labels(case).cuda()
    loss = dyvit_train_loss(out, y, case) if case["family"] == "dyvit" else torch.nn.functional.cross_entropy(out, y)
    recs = _launches.record(loss.backward) if record else loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: None if p.grad is None else p.grad.clone() for n, p in model.named_parameters()}, recs


@functools.lru_cache(maxsize=None)
def _all_trainable(name, wide=False):
    """The reference of every comparison: the all-trainable step of the case, computed once per module run and left unchanged."""
    case = _case(name, wide)
    return _step(case, _model(case), record=True)


def _attn_only(model):
    from tokenreduction_amd import finetune
    finetune.freeze_attn_only(model)


def _trunk(model):          # head + blocks >= 2 trainable
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith(("head.", "blocks.2.", "blocks.3."))


def _head_only(model):
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("head.")


def _assert_same(model, loss, grads, ref, loose=()):
    ref_loss, ref_grads, _ = ref
    assert torch.equal(loss, ref_loss)
    worst = {}
    for n, p in model.named_parameters():
        if not p.requires_grad:
            assert grads[n] is None, f"{n} is frozen but holds a gradient"
        elif n.endswith(loose):
            worst[n] = float((grads[n].double() - ref_grads[n].double()).norm() / ref_grads[n].double().norm().clamp_min(1e-30))
        else:
            assert grads[n] is not None and torch.equal(grads[n], ref_grads[n]), n
    if loose:
        print(f"\nrelative L2 of the regrouped gradients vs all-trainable: max {max(worst.values()):.3e} "
              f"({sum(v > 0 for v in worst.values())} of {len(worst)} differ)")
        bad = {n: v for n, v in worst.items() if not v <= REASSOC_BOUND}
        assert not bad, bad


MICRO = ["deit_micro", "topk_micro", "evit_micro", "tome_micro", "dpcknn_micro", "ats_micro", "kmedoids_micro", "heuristic_micro_l2",
         "dyvit_micro_train", "sit_micro", "patchmerger_micro", "sinkhorn_micro", "topk_micro_droppath", "topk_micro_dropout"]


@pytest.mark.parametrize("name", MICRO)
def test_attn_only_gradients_are_the_all_trainable_bits(name):
    case = _case(name)
    model = _model(case)
    _attn_only(model)
    loss, grads, _ = _step(case, model)
    assert sum(g is not None for g in grads.values()) == 4 * case["depth"] + 3
    _assert_same(model, loss, grads, _all_trainable(name))


@pytest.mark.parametrize("name", ["topk_micro", "evit_micro", "tome_micro", "sit_tiny"])
def test_attn_only_at_the_grouped_width(name):
    """D = 192: the block's group shrinks from four layers to two; only qkv and proj may differ, by an fp32 re-association."""
    wide = name != "sit_tiny"
    case = _case(name, wide)
    model = _model(case)
    _attn_only(model)
    loss, grads, recs = _step(case, model, record=True)
    assert any(r[0] == "wgrad_pc_kernel" for r in recs)
    _assert_same(model, loss, grads, _all_trainable(name, wide), loose=("attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias"))


def test_attn_only_launch_record():
    case = _case("deit_micro")
    model = _model(case)
    _attn_only(model)
    loss, grads, recs = _step(case, model, record=True)
    labels = [r[0] for r in recs]
    B, D, depth, M = case["batch"], case["embed_dim"], case["depth"], case["batch"] * 197
    want = depth * (2.0 * M * 3 * D * D + 2.0 * M * D * D) + 2.0 * B * model._classes_padded * D          # qkv, proj and head
    assert sum(r[1] for r in recs if r[0] in WGRAD) == want
    assert labels.count(LN_FROZEN) == 2 * depth + 1 and "ln_bwd_kernel" not in labels
    assert "tr_embed_bwd" in labels                      # pos_embed is trainable: the walk goes all the way down
    full = [r[0] for r in _all_trainable("deit_micro")[2]]
    assert full.count("ln_bwd_kernel") == 2 * depth + 1 and LN_FROZEN not in full
    assert sum(r[1] for r in _all_trainable("deit_micro")[2] if r[0] in WGRAD) > 2 * want          # fc1, fc2 and the patch product are gone


@pytest.mark.parametrize("name", ["topk_micro", "evit_micro", "tome_micro", "ats_micro", "kmedoids_micro"])
def test_frozen_trunk_stops_after_block_two(name):
    case = _case(name)
    model = _model(case)
    _trunk(model)
    loss, grads, recs = _step(case, model, record=True)
    _assert_same(model, loss, grads, _all_trainable(name))
    labels = [r[0] for r in recs]
    assert sum(labels.count(a) for a in ATTN) == 2
    assert labels.count("gemm_bf16_pc<EPI_DGELU>") == 2 and labels.count("gemm_bf16_pc<EPI_BF16>") == 6
    assert labels.count("ln_bwd_kernel") == 4 and labels.count(LN_FROZEN) == 1          # two blocks' norms; the frozen final norm
    assert "tr_embed_bwd" not in labels
    # nothing after block 2's parameter gradients: norm1's is the last of them, its reduce the last launch
    assert labels[-1] in ("tr_layernorm_bwd (deferred reduce)", "tr_layernorm_bwd (reduce)"), labels[-4:]


def test_stop_block_skips_what_only_feeds_the_blocks_below():
    """Only blocks.1.attn.proj (+ the head) trains: block 1 is walked up to its attention backward, its qkv data gradient and norm1 do not run."""
    case = _case("deit_micro")
    model = _model(case)
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith(("head.", "blocks.1.attn.proj."))
    loss, grads, recs = _step(case, model, record=True)
    _assert_same(model, loss, grads, _all_trainable("deit_micro"))
    labels = [r[0] for r in recs]
    assert sum(labels.count(a) for a in ATTN) == 2 and labels.count("gemm_bf16_pc<EPI_BF16>") == 3 + 2
    assert labels.count(LN_FROZEN) == 1 + 2 + 1 and "ln_bwd_kernel" not in labels
    assert labels[-1] in ("tr_linear_bwd_params (reduce)", "tr_linear_bwd_params"), labels[-4:]


def test_head_only_runs_the_classifier_step_alone():
    case = _case("topk_micro")
    model = _model(case)
    _head_only(model)
    loss, grads, recs = _step(case, model, record=True)
    _assert_same(model, loss, grads, _all_trainable("topk_micro"))
    labels = [r[0] for r in recs]
    assert not [a for a in labels if a in ATTN or a in DGRAD or a.startswith("ln_bwd_kernel")], labels
    assert sum(a in WGRAD for a in labels) == 1 and "colsum_kernel" in labels and len(labels) <= 6, labels


def test_frozen_trunk_under_the_gradient_reducer():
    """As test_gradient_reducer_on_rccl_world1: the backward in per-bucket block ranges (the ranges below the stop block launch nothing,
    their all-zero slices are reduced along), equal to the single-call masked backward bit for bit."""
    import torch.distributed as dist
    from tokenreduction_amd.dp import FlatGradReducer
    case = _case("evit_micro")
    model = _model(case)
    _trunk(model)
    loss, want, _ = _step(case, model)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29573")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        red = FlatGradReducer(bucket_bytes=512 * 1024).attach(model)
        red.broadcast_parameters(model)
        model.zero_grad(set_to_none=True)
        loss2, got, _ = _step(case, model)
        assert len(red.launched) >= 3 and red.launched[-1][1] == model._train_state().flat.numel()
        assert torch.equal(loss2, loss)
        for n in want:
            assert (got[n] is None) == (want[n] is None) and (want[n] is None or torch.equal(got[n], want[n])), n
    finally:
        model._grad_reducer = None
        dist.destroy_process_group()


def test_accumulation_leaves_the_frozen_slices_alone():
    case = _case("topk_micro")
    model = _model(case)
    _attn_only(model)
    _, g1, _ = _step(case, model)
    _, g2, _ = _step(case, model)              # second micro-step: the gradients add up
    st = model._train_state()
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad.data_ptr() == st.views[n].data_ptr()
            assert torch.allclose(g2[n], 2 * g1[n], rtol=1e-5, atol=1e-7), n
        elif n != "cls_token":                 # (cls_token shares its unit with the trainable pos_embed: computed and discarded)
            assert not bool(st.views[n].any()), f"the slice of {n} (frozen, NULL unit) was written"


@pytest.mark.parametrize("masked_first", [True, False])
def test_toggling_requires_grad_takes_effect_on_the_next_backward(masked_first):
    case = _case("evit_micro")
    model = _model(case)
    order = [_trunk, None] if masked_first else [None, _trunk]
    for mask in order:
        for p in model.parameters():
            p.requires_grad_(True)
        if mask is not None:
            mask(model)
        model.zero_grad(set_to_none=True)
        loss, grads, _ = _step(case, model)
        _assert_same(model, loss, grads, _all_trainable("evit_micro"))


def test_a_mixed_unit_is_computed_and_its_frozen_half_discarded():
    case = _case("topk_micro")
    model = _model(case)
    dict(model.named_parameters())["blocks.1.mlp.fc1.bias"].requires_grad = False
    loss, grads, _ = _step(case, model)
    assert grads["blocks.1.mlp.fc1.bias"] is None and grads["blocks.1.mlp.fc1.weight"] is not None
    _assert_same(model, loss, grads, _all_trainable("topk_micro"))


def test_fused_adamw_steps_the_trainable_parameters_only():
    from tokenreduction_amd import finetune
    from tokenreduction_amd.optim import FusedAdamW
    case = _case("topk_micro")
    model = _model(case)
    _attn_only(model)
    opt = FusedAdamW(finetune.get_parameter_groups(model, 1e-2, 0.05, 1.0, 0), model=model)
    x = make_images(case["batch"], 224, case["xseed"]).cuda()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    logits0 = model.eval()(x).clone()
    model.train()
    _step(case, model)
    opt.step()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n]) != p.requires_grad, n          # frozen: the same bits; trainable: moved
    assert not torch.equal(model.eval()(x), logits0)                             # the next eval forward sees the new weights


def test_a_null_stage_the_walk_reaches_is_a_clean_error():
    """tr_vit_backward by hand on a DyViT micro model: the predictor of block 2 has a NULL gradient pointer while block 0 still takes a
    gradient -> TR_ERR_NULL with a message, before anything is launched."""
    from tokenreduction_amd import _lib
    lib = _lib.load()
    case = _case("dyvit_micro_train")
    model = _model(case)
    x = make_images(case["batch"], 224, case["xseed"]).cuda()
    model(x)
    st, pk = model._train_state(), model._pack(need_transposed=True)
    G, _ = st.grads_struct(model)
    assert G.stage[2].w2
    G.stage[2].w2 = None
    WT = st.transposed(model, pk)
    dl = torch.zeros(case["batch"], model._out_width, device="cuda")
    rc = []
    recs = _launches.record(lambda: rc.append(lib.tr_vit_backward(
        C.byref(pk["cfg"]), C.byref(pk["W"]), C.byref(WT), C.byref(G), dl.data_ptr(), None, None, None, st.tape.data_ptr(), st.tape.numel(),
        st.bws.data_ptr(), st.bws.numel(), 0, model.depth - 1, 0, case["batch"], torch.cuda.current_stream().cuda_stream, None, 0.0)))
    assert rc == [TR_ERR_NULL] and recs == []
    assert b"stage of block 2" in lib.tr_last_error()
