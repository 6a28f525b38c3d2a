"""GPU, model level: models built with img_size=(H, W), H != W, through every public entry a square model runs.

Cases (tests/_rect_params.py): embed_dim 384, depth 3, 6 heads, 16 classes, reduction_loc [1, 2], at (64, 96) and its transpose (96, 64)
-- a 4 x 6 and a 6 x 4 grid, 24 patches, every stage still reducing -- plus one embed_dim 128 model (the three-launch embedding).  The
reference is the subclassed oracle (num_patches = gh * gw), itself pinned on the reference's vectors at these sizes
(tests/test_rect_config.py); every case also has the reference's own recorded vectors (tests/golden/gen_golden_rect.py).

Wherever a square test of the suite states the check, that test's own function runs here on the rectangular case -- same code, same
tolerances: `_rect` puts the case into tests._params.GOLDEN_CASES for the duration of one test and swaps the int-only helpers
(make_images, make_params, case_config, case_params) of the modules involved for their pair forms."""
import contextlib

import numpy as np
import pytest
import torch

import oracle
from tests import _launches, _params
from tests import _rect_params as R

pytestmark = pytest.mark.gpu

NAMES = list(R.RECT_CASES)
SIZE_IDS = [f"{h}x{w}" for h, w in R.SIZES]


def _names(*families):
    return [R.case_name(f, s) for f in families for s in R.SIZES]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextlib.contextmanager
def _rect(monkeypatch, name):
    from tests import (_input_grad_ref, test_decisions_gpu, test_dense_gpu, test_dense_levels_gpu, test_dense_train_gpu,
                       test_dense_train_levels_gpu, test_hip_fp32, test_hip_model, test_hip_split, test_hip_train, test_input_grad_gpu)
    monkeypatch.setitem(_params.GOLDEN_CASES, name, R.RECT_CASES[name])
    with R.patched(_params, _input_grad_ref, test_decisions_gpu, test_dense_gpu, test_dense_levels_gpu, test_dense_train_gpu,
                   test_dense_train_levels_gpu, test_hip_fp32, test_hip_model, test_hip_split, test_hip_train, test_input_grad_gpu):
        yield R.RECT_CASES[name]


def _eval_model(name, precision="bf16"):
    model, params, cfg = R.build_model(R.RECT_CASES[name])
    model.viz_mode, model.precision = False, precision
    case = R.RECT_CASES[name]
    return model, params, cfg, R.make_images(case["batch"], case["img_size"], case["xseed"]).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- eval ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NAMES if R.RECT_CASES[n]["family"] != "tome"])
def test_eval_bf16_parity(golden_dir, name, monkeypatch):
    """tests/test_hip_model.test_model_parity on the rectangular case: executor == per-op sequence bit for bit, every decision exact on the
    device's own scores against the oracle, teacher-forced logits within FORCED_TOL of the subclassed oracle, the family's checks against
    the reference's vectors.  (The embed_dim 128 case takes the three-launch embedding.)  That function's free-running bounds depend on
    the width and the keep ratios of a case; the ones that hold here are stated in test_eval_bf16_free_running_bounds."""
    from tests import test_hip_model
    with _rect(monkeypatch, name):
        test_hip_model.test_model_parity(golden_dir, name)


# Free-running bounds of the rectangular cases, stated here and not inherited from a branch of test_model_parity: the values that function
# applies to the same family's MICRO case (embed_dim 128 at 224 x 224) -- relative L2 of the logits against the oracle with the HIP
# rounding points and against the reference's fp32 vectors below 0.05 (DyViT 0.35, its coarse regression bound at every size), kept-set
# overlap at least 0.60 at every stage and 0.95 at the first.  The rectangular models are wider (384) but three blocks deep on 24 patches;
# measured on an MI355X: 0.5e-2 ... 2.2e-2 and overlaps 0.86 ... 1.0 (profiles/rect_input_lab.md), so the micro values hold with room.
FREE_TOL = {"deit": 0.05, "topk": 0.05, "evit": 0.05, "tome": 0.05, "dyvit": 0.35}
OVERLAP_FLOOR, OVERLAP_FIRST = 0.60, 0.95


@pytest.mark.parametrize("name", _names("deit", "topk", "evit", "dyvit") + [R.case_name("topk", R.SIZES[0], 128)])
def test_eval_bf16_free_running_bounds(golden_dir, name):
    import os
    from tests.test_hip_model import _overlap
    case = R.RECT_CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    model, params, cfg = R.build_model(case)
    x = R.make_images(case["batch"], case["img_size"], case["xseed"])
    logits, viz = model(x.cuda())
    logits = logits.cpu()
    lb, vb = oracle.forward(params, x, cfg, precision="bf16", return_viz=True)
    ref = torch.from_numpy(g["logits"])
    rel_bf, rel_ref = ((logits - lb).norm() / lb.norm()).item(), ((logits - ref).norm() / ref.norm()).item()
    kept_keys = sorted((k for k in g.files if k.startswith("kept_")), key=lambda k: int(k.split("_")[1]))
    ov_bf = [_overlap(viz["Kept_Tokens"][b], vb["Kept_Tokens"][b]) for b in sorted(vb.get("Kept_Tokens", {}))]
    ov_ref = [_overlap(viz["Kept_Tokens"][int(k.split("_")[1])], g[k]) for k in kept_keys]
    print(f"\n[{name}] free-running relative L2 vs oracle_bf16 {rel_bf:.3e}, vs reference {rel_ref:.3e}; overlap {ov_bf} / {ov_ref}")
    tol = FREE_TOL[case["family"]]
    assert rel_bf < tol and rel_ref < tol, (rel_bf, rel_ref)
    assert (case["family"] == "deit") == (not ov_bf) and len(ov_bf) == len(ov_ref)
    assert all(o >= OVERLAP_FLOOR for o in ov_bf + ov_ref), (ov_bf, ov_ref)
    assert all(o[0] >= OVERLAP_FIRST for o in (ov_bf, ov_ref) if o), (ov_bf, ov_ref)


@pytest.mark.parametrize("name", _names("tome"))
def test_eval_bf16_parity_tome(golden_dir, name):
    """test_hip_model._tome_parity with the token count of the grid (it is written for 197): the oracle's matching on the device's own keys
    is the device's matching bit for bit, the token counts follow the schedule, teacher-forced logits within FORCED_TOL, free-running
    logits at FREE_TOL (that function's micro-case bound) and first-stage assignment agreement at its bounds."""
    import os
    from tests._stepwise import Trace, forward_stepwise
    from tests.test_hip_model import FORCED_TOL, _agree
    case = R.RECT_CASES[name]
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    model, params, cfg = R.build_model(case)
    x = R.make_images(case["batch"], case["img_size"], case["xseed"])
    logits, viz = model(x.cuda())
    logits = logits.cpu()
    trace = Trace(keep=True)
    l2, info = forward_stepwise(model, x.cuda(), trace)
    assert torch.equal(l2.cpu(), logits)
    B, n_in, forced = x.shape[0], cfg.num_patches + 1, {}
    sched = oracle.tome_schedule(cfg)
    for blk in range(cfg.depth):
        r = oracle.tome_block_r(sched.get(blk, 0), n_in)
        if r > 0:
            unm, src, dst = info["tome"][blk]
            forced[blk] = (unm.cpu().long(), src.cpu().long(), dst.cpu().long())
            k = trace.tensors[f"qkv_{blk}"].float().cpu().reshape(B, n_in, 3, cfg.num_heads, 64)[:, :, 1].permute(0, 2, 1, 3)
            for got, want in zip(forced[blk], oracle.tome_match(k.mean(1), r)):
                np.testing.assert_array_equal(got.numpy(), want.numpy())
            a = oracle.tome_assignment(*forced[blk], n_in).numpy()
            np.testing.assert_array_equal(viz["Assignment_Maps"][blk], a)
            assert viz["Assignment_Maps"][blk].shape == g[f"assign_{blk}"].shape
        n_in -= r
        assert model._last_tokens[blk] == n_in
    assert sorted(forced) == case["reduction_loc"] and n_in < cfg.num_patches + 1
    lb, vb = oracle.tome_forward(params, x, cfg, precision="bf16", return_viz=True)
    ref = torch.from_numpy(g["logits"])
    rel_bf, rel_ref = ((logits - lb).norm() / lb.norm()).item(), ((logits - ref).norm() / ref.norm()).item()
    lf = oracle.tome_forward(params, x, cfg, precision="bf16", forced=forced)
    rel_forced = ((logits - lf).norm() / lf.norm()).item()
    first = min(forced)
    ag_bf, ag_ref = _agree(viz["Assignment_Maps"][first], vb["Assignment_Maps"][first]), _agree(viz["Assignment_Maps"][first], g[f"assign_{first}"])
    print(f"\n[{name}] relative L2: teacher-forced {rel_forced:.3e}, vs oracle_bf16 {rel_bf:.3e}, vs reference {rel_ref:.3e}; "
          f"first-stage agreement {ag_bf:.3f} / {ag_ref:.3f}")
    assert rel_forced < FORCED_TOL, rel_forced
    assert rel_bf < FREE_TOL["tome"] and rel_ref < FREE_TOL["tome"], (rel_bf, rel_ref)
    assert ag_bf >= 0.90 and ag_ref >= 0.80, (ag_bf, ag_ref)


@pytest.mark.parametrize("name", _names("deit", "topk", "tome"))
def test_eval_fp32_matches_the_reference(golden_dir, name, monkeypatch):
    from tests import test_hip_fp32
    with _rect(monkeypatch, name):
        test_hip_fp32.test_model_fp32_matches_reference_golden(golden_dir, name)


@pytest.mark.parametrize("name", _names("deit", "topk", "tome"))
def test_eval_bf16x3_matches_the_reference(golden_dir, name, monkeypatch):
    from tests import test_hip_split
    with _rect(monkeypatch, name):
        test_hip_split.test_model_bf16x3_free_running_against_reference_golden(golden_dir, name)


def test_which_embedding_runs():
    """embed_dim 384: one patch_embed_kernel with the FLOPs of gh * gw patches; embed_dim 128: the three launches, no patch_embed_kernel."""
    model, _, _, x = _eval_model(R.case_name("topk", R.SIZES[0]))
    recs = _launches.forward_launches(model, x)
    pe = [r for r in recs if r[0] == "patch_embed_kernel"]
    assert len(pe) == 1 and pe[0][1] == 2.0 * x.shape[0] * 24 * 384 * 768
    small, _, _, xs = _eval_model(R.case_name("topk", R.SIZES[0], 128))
    labels = [r[0] for r in _launches.forward_launches(small, xs)]
    assert "patch_embed_kernel" not in labels and labels


@pytest.mark.parametrize("name", _names("topk", "tome", "dpcknn") + [R.case_name("topk", R.SIZES[0], 128)])
def test_graph_replay_and_forward_async_give_the_plain_forward_bits(name):
    model, _, _, x = _eval_model(name)
    if R.RECT_CASES[name]["family"] == "dpcknn":
        model.density_noise = {blk: torch.zeros(x.shape[0], P) for blk, _, P in model._stage_shapes()}
    model.use_graph = False
    plain = model(x).clone()
    model.use_graph = True
    for _ in range(3):                       # the capture, then replays
        assert torch.equal(_bits(model(x)), _bits(plain))
    a, b = model.forward_async(x), model.forward_async(x)
    assert torch.equal(_bits(a.result()), _bits(plain)) and torch.equal(_bits(b.result()), _bits(plain))
    model.check_status()


def test_uint8_input_in_eval_equals_the_normalized_image():
    from tokenreduction_amd import pixels
    model, _, _, _ = _eval_model(R.case_name("topk", R.SIZES[0]))
    H, W = R.SIZES[0]
    u8 = torch.randint(0, 256, (2, 3, H, W), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    mean, std = torch.tensor(pixels.IMAGENET_DEFAULT_MEAN), torch.tensor(pixels.IMAGENET_DEFAULT_STD)
    want = model((((u8.float() / 255) - mean[:, None, None]) / std[:, None, None]).cuda()).clone()
    model.set_pixel_input()
    d = u8.cuda()
    assert torch.equal(_bits(model(d)), _bits(want))
    assert torch.equal(_bits(model(d.contiguous(memory_format=torch.channels_last))), _bits(want))


# ---- dense ---------------------------------------------------------------------------------------------------------------------------
def _noise_for_three_images(name):
    """tests/test_decisions_gpu runs three images through its (cached) model; the fixtures here record DPC-KNN's density draws for two."""
    from tests import test_decisions_gpu
    model = test_decisions_gpu._model(name)
    if R.RECT_CASES[name]["family"] == "dpcknn":
        g = torch.Generator().manual_seed(R.RECT_CASES[name]["xseed"])
        model.density_noise = {blk: torch.rand(test_decisions_gpu.B, P, generator=g) for blk, _, P in model._stage_shapes()}
    return model


@pytest.mark.parametrize("name", _names("deit", "topk", "tome", "dpcknn"))
def test_dense_map_and_index_match_the_restatement(name, monkeypatch):
    """tests/test_dense_gpu's check: [B, D, gh, gw] / [B, gh, gw, D], index [B, gh*gw] and features equal tests/_dense_ref.py applied to the
    device's decisions, both layouts and dtypes."""
    from tests import test_dense_gpu
    with _rect(monkeypatch, name):
        _noise_for_three_images(name)
        test_dense_gpu.test_map_and_index_are_the_restatement_of_the_same_models_decisions(name, "bf16")


@pytest.mark.parametrize("name", _names("deit", "topk", "tome", "dpcknn"))
def test_dense_levels_match_the_restatement(name, monkeypatch):
    """tests/test_dense_levels_gpu's checks of forward_dense(blocks=every block), normed and unnormed, against tests/_dense_levels_ref.py."""
    from tests import test_dense_levels_gpu
    with _rect(monkeypatch, name):
        _noise_for_three_images(name)
        test_dense_levels_gpu.test_every_block_normed_and_the_last_level_is_todays_map(name, "bf16")
        test_dense_levels_gpu.test_every_block_unnormed_is_the_restatement_on_viz_modes_features(name, "bf16")


@pytest.mark.parametrize("name", _names("deit", "topk", "tome", "dpcknn"))
def test_get_intermediate_layers_on_a_rectangular_grid(name, monkeypatch):
    """tests/test_dense_levels_gpu.test_get_intermediate_layers_is_timms_shape_over_forward_dense with block sets of a depth-3 model:
    reshape=True gives [B, D, gh, gw], the flat form [B, gh*gw, D], both the bits of forward_dense's levels."""
    from tests import test_decisions_gpu
    with _rect(monkeypatch, name):
        model, x = _noise_for_three_images(name), test_decisions_gpu._images(name)
        model.precision, model.viz_mode, model.use_graph = "bf16", False, False
        (h, w), D, B = model.patch_embed.grid_size, model.embed_dim, x.shape[0]
        assert h != w
        for n, blocks in ((2, (1, 2)), ((0, 2), (0, 2)), ((-1, 0), (0, 2)), (1, (2,))):
            for norm in (False, True):
                _, nchw = model.forward_dense(x, blocks=blocks, norm=norm, fill=1.5)
                _, nhwc = model.forward_dense(x, blocks=blocks, norm=norm, output_fmt="NHWC", fill=1.5)
                flat = model.get_intermediate_layers(x, n, norm=norm, fill=1.5)
                grid = model.get_intermediate_layers(x, n, reshape=True, norm=norm, fill=1.5)
                both = model.get_intermediate_layers(x, n, reshape=True, return_class_token=True, norm=norm, fill=1.5)
                assert len(flat) == len(grid) == len(both) == len(blocks)
                for l in range(len(blocks)):
                    assert nhwc["features"][l].shape == (B, h, w, D)
                    assert flat[l].shape == (B, h * w, D) and torch.equal(_bits(flat[l]), _bits(nhwc["features"][l].reshape(B, h * w, D)))
                    assert grid[l].shape == (B, D, h, w) and torch.equal(_bits(grid[l]), _bits(nchw["features"][l]))
                    tok, cls = both[l]
                    assert torch.equal(tok, grid[l]) and cls.shape == (B, D) and torch.equal(_bits(cls), _bits(nchw["cls"][:, l]))


@pytest.mark.parametrize("size", R.SIZES, ids=SIZE_IDS)
def test_deit_map_is_the_final_normed_patch_rows_on_gh_by_gw(size):
    """No stage: the map is the final-normed patch rows reshaped (gh, gw) bit for bit -- and not (gw, gh): patch p sits at
    (p // gw, p % gw)."""
    model, _, _, x = _eval_model(R.case_name("deit", size))
    gh, gw = size[0] // 16, size[1] // 16
    B, D = x.shape[0], model.embed_dim
    _, taps = model.forward_taps(x, cls_blocks=(), final_tokens=True)
    rows = taps["final_tokens"][:, 1:].clone()                                  # [B, P, D]
    _, nchw = model.forward_dense(x)
    _, nhwc = model.forward_dense(x, output_fmt="NHWC")
    assert nchw["grid"] == (gh, gw) and nchw["features"].shape == (B, D, gh, gw) and nhwc["features"].shape == (B, gh, gw, D)
    assert torch.equal(nchw["index"].cpu(), torch.arange(1, gh * gw + 1, dtype=torch.int32).expand(B, -1))
    assert torch.equal(_bits(nhwc["features"]), _bits(rows.view(B, gh, gw, D)))
    assert torch.equal(_bits(nchw["features"]), _bits(rows.view(B, gh, gw, D).permute(0, 3, 1, 2)))
    assert not torch.equal(_bits(nchw["features"].permute(0, 1, 3, 2)), _bits(rows.view(B, gw, gh, D).permute(0, 3, 2, 1)))
    p = gw + 1                                                                   # patch (1, 1)
    assert torch.equal(nchw["features"][:, :, 1, 1], rows[:, p]) and torch.equal(nhwc["features"][:, p // gw, p % gw], rows[:, p])
    grid = model.get_intermediate_layers(x, 1, reshape=True, norm=True)
    assert grid[0].shape == (B, D, gh, gw) and torch.equal(_bits(grid[0]), _bits(nchw["features"]))
    a = model.forward_async(x, dense={})
    assert torch.equal(_bits(a.result()[1]["features"]), _bits(nchw["features"]))


# ---- training ------------------------------------------------------------------------------------------------------------------------
TRAIN = _names("deit", "topk", "tome", "sit")


@pytest.mark.parametrize("name", TRAIN)
def test_gradients_match_the_oracle_on_the_device_decisions(golden_dir, name, monkeypatch):
    """tests/test_hip_train's parity: torch.autograd over the subclassed oracle, bf16 rounding points, the device's decisions, grad_tol."""
    from tests import test_hip_train
    with _rect(monkeypatch, name):
        test_hip_train.test_gradients_match_the_oracle_on_the_device_decisions(golden_dir, name)


@pytest.mark.parametrize("name", TRAIN)
def test_input_gradient_is_b_c_h_w_and_matches_the_oracle(golden_dir, name, monkeypatch):
    """tests/test_input_grad_gpu's parity (it asserts x.grad.shape == x.shape = [B, 3, H, W]) at its tolerance."""
    from tests import test_input_grad_gpu
    with _rect(monkeypatch, name):
        test_input_grad_gpu.test_input_gradient_matches_the_oracle_on_the_device_decisions(golden_dir, name)


def _train_run(model, batch, labels):
    model.zero_grad(set_to_none=True)
    loss = torch.nn.functional.cross_entropy(model(batch), labels)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("size", R.SIZES, ids=SIZE_IDS)
def test_uint8_and_augmented_training_input_equal_the_materialized_images(size):
    """Training on uint8 pixels (NCHW and channels_last) and on one DeviceAugment batch (erase + mixup / cutmix boxes drawn in H x W): loss
    and every gradient are the bits of the same images materialized as fp32 on the host side of the executor."""
    from tokenreduction_amd import augment, pixels
    name = R.case_name("topk", size)
    model, _, _ = R.build_model(R.RECT_CASES[name])
    model.viz_mode = False
    model.train()
    model.set_pixel_input()
    B, (H, W) = 4, size
    u8 = torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).cuda()
    labels = torch.tensor([1, 5, 9, 3]).cuda()
    mean, std = torch.tensor(pixels.IMAGENET_DEFAULT_MEAN).cuda(), torch.tensor(pixels.IMAGENET_DEFAULT_STD).cuda()
    want = _train_run(model, ((u8.float() / 255) - mean[:, None, None]) / std[:, None, None], labels)
    for img in (u8, u8.contiguous(memory_format=torch.channels_last)):
        got = _train_run(model, img, labels)
        assert torch.equal(got[0], want[0]) and all(torch.equal(got[1][n], want[1][n]) for n in want[1])
    from tests.test_device_augment import restate
    torch.manual_seed(3)
    np.random.seed(3)
    aug = augment.DeviceAugment(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, label_smoothing=0.1, num_classes=16, re_prob=1.0)
    batch, _ = aug(u8, labels)
    assert tuple(batch.shape) == (B, 3, H, W)
    rec = batch.host_table
    assert (rec["yh"] <= H).all() and (rec["xh"] <= W).all() and (rec["ey"] + rec["eh"] <= H).all() and (rec["ex"] + rec["ew"] <= W).all()
    assert bool(rec["erased"].any())
    flat = restate(u8, pixels.pixel_lut(pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD).cuda(), rec, batch.noise)
    assert tuple(flat.shape) == (B, 3, H, W) and torch.equal(_bits(batch.float()), _bits(flat))
    got, ref = _train_run(model, batch, labels), _train_run(model, flat, labels)
    assert torch.equal(got[0], ref[0]) and all(torch.equal(got[1][n], ref[1][n]) for n in ref[1])


@pytest.mark.parametrize("size", R.SIZES, ids=SIZE_IDS)
def test_forward_dense_train_two_levels(size):
    """forward_dense_train(blocks=(0, 2)) on Top-K: `out` is model(x)'s bits in train mode, the maps are [B, D, gh, gw], and the gradients of
    cross_entropy(out) + sum_l (features[l] * G_l).sum() -- every parameter's and x.grad -- match torch autograd over the block composition
    of the subclassed oracle (tests/_dense_train_levels_ref.py: bf16 rounding points, the device's decisions, the device's index) under
    tests/test_dense_train_gpu._check_grads' bounds: grad_tol of depth <= 4 on the whole vector, twice that on the worst parameter and on
    x.grad.  G_l is seeded N(0, 1) / (B * P0), as in tests/test_dense_train_levels_gpu.py."""
    from tests import _dense_train_levels_ref as lref
    from tests.test_dense_train_gpu import FILL, _check_grads, _grads, _head_loss
    from tests.test_hip_model import FORCED_TOL
    from tests.test_hip_train import _rel
    from tokenreduction_amd import training
    name = R.case_name("topk", size)
    case = R.RECT_CASES[name]
    model, params, cfg = R.build_model(case)
    model.viz_mode = False
    model.train()
    B, blocks, (gh, gw) = case["batch"], (0, 2), (size[0] // 16, size[1] // 16)
    P0 = gh * gw
    x = R.make_images(B, size, case["xseed"]).cuda()
    plain = model(x).detach().clone()
    x.requires_grad_(True)
    Gs = [torch.randn(B, 384, P0, generator=torch.Generator().manual_seed(case["xseed"] + 23 + l)) / (B * P0) for l in range(2)]
    model.zero_grad(set_to_none=True)
    out, dense = model.forward_dense_train(x, blocks=blocks, fill=FILL)
    assert torch.equal(_bits(out.detach()), _bits(plain))
    assert dense["blocks"] == blocks and dense["grid"] == (gh, gw)
    assert all(f.shape == (B, 384, gh, gw) and f.requires_grad for f in dense["features"])
    assert all(i.shape == (B, P0) and i.dtype == torch.int32 for i in dense["index"])
    assert torch.equal(dense["index"][0].cpu(), torch.arange(1, P0 + 1, dtype=torch.int32).expand(B, -1))
    assert bool((dense["index"][1] < 0).any())
    loss = sum((f.reshape(G.shape).float() * G.cuda()).sum() for f, G in zip(dense["features"], Gs)) + _head_loss(case, out, None)
    loss.backward()
    torch.cuda.synchronize()
    grads, dx = _grads(model), x.grad.detach().clone()
    assert dx.shape == (B, 3, *size)
    forced = {blk: d.cpu() for blk, d in training.train_decisions(model).items()}
    index = [i.cpu() for i in dense["index"]]
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    img = x.detach().cpu().clone().requires_grad_(True)
    with torch.enable_grad():
        hs = lref.streams_after_blocks(leaves, img, cfg, "bf16", forced, None)
        o_out = lref.logits_of(leaves, hs[-1], cfg, "bf16")
        o_loss = _head_loss(case, o_out, None)
        for l, b in enumerate(blocks):
            m = lref.level_map(lref.level_rows(hs[b], leaves, cfg, True), index[l], FILL)
            o_loss = o_loss + (m.permute(0, 2, 1) * Gs[l]).sum()
        names = list(leaves)
        gs = torch.autograd.grad(o_loss, [leaves[n] for n in names] + [img], allow_unused=True)
    o_grads = {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, gs[:-1])}
    assert _rel(out.detach().cpu(), o_out.detach()) < FORCED_TOL
    _check_grads(f"{name} blocks={blocks}", case, grads, dx, o_grads, gs[-1])


# ---- refusals, before any launch --------------------------------------------------------------------------------------------------------
def test_a_transposed_input_is_refused_before_any_launch():
    model, _, _, x = _eval_model(R.case_name("topk", R.SIZES[0]))
    model(x)
    bad = x.transpose(2, 3).contiguous()                           # [B, 3, 96, 64] into a (64, 96) model: the same number of elements
    for call in (lambda: model(bad), lambda: model.forward_dense(bad), lambda: model.forward_async(bad).result(),
                 lambda: model.train()(bad), lambda: model.train().forward_dense_train(bad)):
        raised = []

        def run():
            try:
                call()
            except ValueError as e:
                raised.append(str(e))
        assert _launches.record(run) == []
        assert len(raised) == 1 and "[B, C, H, W] = [B,3,64,96]" in raised[0] and "96, 64" in raised[0]
        model.eval()


def test_training_beyond_640_tokens_is_refused_with_the_token_count():
    """(400, 656): 25 x 41 = 1025 patches, an eval-only size."""
    import types
    import tokenreduction_amd as tra
    args = types.SimpleNamespace(keep_rate=[1.0], reduction_loc=[], viz_mode=False)
    model = tra.VisionTransformer(img_size=(400, 656), patch_size=16, embed_dim=384, depth=2, num_heads=6, mlp_ratio=4, qkv_bias=True,
                                  num_classes=16, args=args).cuda().train()
    x = torch.zeros(1, 3, 400, 656, device="cuda")
    raised = []

    def run():
        try:
            model(x)
        except NotImplementedError as e:
            raised.append(str(e))
    recs = _launches.record(run)
    assert len(raised) == 1 and "no training path" in raised[0] and "640 tokens" in raised[0] and "1026" in raised[0]
    assert "224x224" not in raised[0]
    assert not [r for r in recs if "patch_embed" in r[0] or "im2col" in r[0]]


def test_heuristic_is_refused_at_construction():
    import types
    import tokenreduction_amd as tra
    args = types.SimpleNamespace(keep_rate=[0.7], reduction_loc=[1, 2], viz_mode=False, heuristic_pattern="l2", not_contiguous=True, min_radius=None)
    with pytest.raises(ValueError, match="square grid"):
        tra.HeuristicVisionTransformer(img_size=(64, 96), patch_size=16, embed_dim=384, depth=3, num_heads=6, mlp_ratio=4, qkv_bias=True,
                                       num_classes=16, args=args)
