"""GPU tests, model level, at 448 x 448 and 512 x 512 inputs (785 and 1025 tokens incl. CLS): every factory family in the three eval
precisions, the full-size DeiT-S Top-K / ToMe forward at batch 64 (eager, captured graph, forward_async), and a 224 x 224 checkpoint
loaded into a 448 x 448 model and run through harness.validate with viz_mode."""
import types

import pytest
import torch

import tokenreduction_amd as tra

pytestmark = pytest.mark.gpu

TINY = sorted(n for n in tra.list_models() if "_tiny_" in n)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _args(**kw):
    a = dict(keep_rate=[0.9], reduction_loc=[3, 6, 9], dyvit_distill=False, k_neighbors=5, equal_weight=False, cluster_iters=3,
             sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None, viz_mode=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _images(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, S, S, generator=g)


@pytest.mark.parametrize("S", [448, 512])
@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "fp32"])
@pytest.mark.parametrize("name", TINY)
def test_every_family_runs_at_high_resolution(name, precision, S):
    """keep_rate 0.9: the clustering families keep 705 (448^2) / 921 (512^2) centres, beyond the 640 the kernels held before."""
    torch.manual_seed(0)
    m = tra.create_model(name, pretrained=False, num_classes=100, img_size=S, args=_args()).cuda().eval()
    m.precision = precision
    out = m(_images(2, S, S).cuda())
    logits = out[0] if isinstance(out, tuple) else out
    assert logits.shape == (2, 100)
    assert bool(torch.isfinite(logits).all())


@pytest.mark.parametrize("name", ["topk_small_patch16_224", "tome_small_patch16_224"])
def test_full_size_448_batch64(name):
    """DeiT-S width at 448 x 448, batch 64, bf16: finite logits; a captured graph's replay and forward_async equal the eager forward."""
    torch.manual_seed(0)
    args = _args(keep_rate=[0.7])
    m = tra.create_model(name, pretrained=False, num_classes=1000, img_size=448, args=args).cuda().eval()
    x = _images(64, 448, 1).cuda()
    ref = m(x).clone()
    assert ref.shape == (64, 1000) and bool(torch.isfinite(ref).all())
    assert torch.equal(m.forward_async(x).result(), ref)
    static_x = x.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(static_x)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        out = m(static_x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_224_checkpoint_into_448_model_validate_viz():
    """A 224 x 224 micro Top-K model's state dict loaded into a 448 x 448 model of the same family (pos_embed 14 x 14 -> 28 x 28,
    train.py:343-370), then harness.validate with viz_mode: every Stage-{loc} record holds patch indices of the 28 x 28 grid and one
    of the token counts of the model's schedule, fewer at each stage."""
    from tokenreduction_amd import finetune, harness
    kw = dict(patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4, qkv_bias=True, num_classes=16)
    torch.manual_seed(0)
    small = tra.TopKVisionTransformer(img_size=224, args=_args(keep_rate=[0.7], reduction_loc=[1, 2]), **kw)
    big = tra.TopKVisionTransformer(img_size=448, args=_args(keep_rate=[0.7], reduction_loc=[1, 2], viz_mode=True), **kw)
    finetune.load_finetune_checkpoint(big, {"model": small.state_dict()})
    assert big.pos_embed.shape == (1, 785, 128)
    big = big.cuda().eval()
    loader = [(_images(2, 448, 10 + i), torch.tensor([i, i + 1])) for i in range(2)]
    names = [f"img{i}" for i in range(4)]
    data = harness.validate(loader, big, "cuda", "topk_tiny_patch16_224", names, keep_rate=[0.7], reduction_loc=[1, 2])
    counts = {n - 1 for n in big._last_tokens}
    for nm in names:
        kept = [data[nm][f"Stage-{s}"]["Kept_Token"] for s in (1, 2)]
        lens = [len(k) for k in kept]
        assert all(n in counts for n in lens) and lens[0] > lens[1] > 0
        for k in kept:
            k = torch.as_tensor(k)
            assert int(k.min()) >= 0 and int(k.max()) < 784 and len(set(k.tolist())) == len(k)
    # the records are the model's own Top-K on its CLS attention, composed to patch ids of the 28 x 28 grid (validate.py:199-229):
    # the per-op launch sequence gives each stage's scores; the oracle's top-k on them must be the stage's selection
    import oracle
    from tests._stepwise import forward_stepwise
    for bi, (images, _) in enumerate(loader):
        _, info = forward_stepwise(big, images.cuda())
        prev = None
        for s in sorted(info["kept"]):
            idx = info["kept"][s].cpu().long()
            assert torch.equal(idx, oracle.cls_topk_select(info["scores"][s].cpu(), idx.shape[1]))
            for i in range(idx.shape[0]):
                cur = idx[i].tolist() if prev is None else [prev[i][v] for v in idx[i].tolist()]
                assert [int(v) for v in data[names[2 * bi + i]][f"Stage-{s}"]["Kept_Token"]] == cur
            prev = [idx[i].tolist() if prev is None else [prev[i][v] for v in idx[i].tolist()] for i in range(idx.shape[0])]
