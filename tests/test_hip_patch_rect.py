"""GPU, op level: the one-launch patch embedding (all three loaders) and PatchEmbed's data gradient on rectangular images [B, C, H, W],
H != W -- the tr_patch_embed_hw_bf16 / tr_patch_embed_u8_hw_bf16 / tr_patch_embed_dgrad_hw entries, which share their kernels with the
square entries.  Patches are row-major on the gh x gw grid: patch p = (p // gw, p % gw).

The embedding is held to the oracle and to the three-launch path at tests/test_hip_ops.test_patch_embed_fused's tolerances, and bit for
bit to the square launch where a rectangular image is a strip of a square one; the uint8 loaders bit for bit to the fp32 loader on the
normalized image (tests/test_pixel_input_gpu.py); the data gradient by the integer-exact scheme of tests/test_hip_patch_dgrad.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from tests import _launches
from tokenreduction_amd import pixels

pytestmark = pytest.mark.gpu

MEAN, STD = pixels.IMAGENET_DEFAULT_MEAN, pixels.IMAGENET_DEFAULT_STD


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _randn(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _embed_operands(B, H, W, D, Cc, seed):
    rng = np.random.default_rng(seed)
    P = (H // 16) * (W // 16)
    img = _randn(rng, B, Cc, H, W)
    w, b = _randn(rng, D, Cc, 16, 16, scale=0.02), _randn(rng, D, scale=0.02)
    cls, pos = _randn(rng, 1, 1, D, scale=0.02), _randn(rng, 1, P + 1, D, scale=0.02)
    return img, w, b, cls, pos


# (B, H, W, D, C)
EMBED_SHAPES = [(2, 64, 224, 384, 3),       # a strip of the square image
                (2, 240, 224, 384, 3),      # 210 patches: the 208-row chunk boundary falls mid patch row
                (2, 208, 256, 384, 3),      # exactly one full chunk, no zero rows
                (1, 16, 640, 384, 3),       # gh = 1
                (1, 640, 16, 384, 3),       # gw = 1: the row stride is one run
                (5, 32, 48, 384, 1),        # one channel, several images
                (2, 96, 240, 384, 4),       # four channels
                (1, 64, 96, 768, 3),        # two column slabs
                (2, 384, 640, 384, 3)]      # 960 patches, five chunks: the largest eval grid the 1024 cap allows at this aspect


@pytest.mark.parametrize("B,H,W,D,Cc", EMBED_SHAPES)
def test_patch_embed_rect(ops, B, H, W, D, Cc):
    """Against the oracle (bf16 operands) and against the three-launch path (same products; pos_embed joins the sum at another point)."""
    img, w, b, cls, pos = _embed_operands(B, H, W, D, Cc, 9000 + H + 3 * W + D + Cc)
    P = (H // 16) * (W // 16)
    want = oracle.embed_tokens(oracle.patch_embed(img, w, b, 16, precision="bf16"), cls, pos)
    w16 = w.reshape(D, -1).cuda().bfloat16()
    posd, clsd = pos.reshape(P + 1, D).cuda(), cls.reshape(-1).cuda()
    recs = _launches.record(lambda: ops.patch_embed(img.cuda(), w16, b.cuda(), clsd, posd))
    got = ops.patch_embed(img.cuda(), w16, b.cuda(), clsd, posd)
    assert got.shape == (B, P + 1, D)
    torch.testing.assert_close(got.cpu(), want, atol=1e-4, rtol=1e-5)
    cols = ops.im2col(img.cuda(), 16)
    x = torch.empty(B * (P + 1), D, device="cuda")
    ops.gemm(cols, w16, b.cuda(), ops.TR_EPI_PATCH_F32, out=x, aux=posd, aux_i=P)
    ops.cls_pos_rows(clsd, posd, x, B, P + 1, D)
    torch.testing.assert_close(got.view(B * (P + 1), D), x, atol=2e-6, rtol=1e-6)
    # one launch, with the work and the traffic of gh * gw patches
    assert [r[0] for r in recs] == ["patch_embed_kernel"]
    assert recs[0][1] == 2.0 * B * P * D * Cc * 256
    assert recs[0][2] == 4.0 * B * Cc * H * W + 4.0 * B * (P + 1) * D


def test_a_strip_of_a_square_image_gives_the_square_launch_bits(ops):
    """(2, 64, 224) is the top four patch rows of a 224 x 224 image: with position rows 0..56 shared, rows 0..56 of the square launch and
    of the rectangular launch are the same bits -- the K order and the kernel are the same."""
    B, D = 2, 384
    img, w, b, cls, pos = _embed_operands(B, 224, 224, D, 3, 77)
    w16 = w.reshape(D, -1).cuda().bfloat16()
    posd, clsd = pos.reshape(197, D).cuda(), cls.reshape(-1).cuda()
    square = ops.patch_embed(img.cuda(), w16, b.cuda(), clsd, posd)
    strip = ops.patch_embed(img[:, :, :64].contiguous().cuda(), w16, b.cuda(), clsd, posd[:57].contiguous())
    assert strip.shape == (B, 57, D)
    assert torch.equal(strip.view(torch.int32), square[:, :57].contiguous().view(torch.int32))


def test_hw_entry_with_a_square_image_gives_the_square_entry_bits(ops):
    from tokenreduction_amd import _lib
    lib = _lib.load()
    B, S, D = 2, 48, 384
    img, w, b, cls, pos = _embed_operands(B, S, S, D, 3, 78)
    w16 = w.reshape(D, -1).cuda().bfloat16()
    posd, clsd, imgd, bd = pos.reshape(10, D).cuda(), cls.reshape(-1).cuda(), img.cuda(), b.cuda()
    want = ops.patch_embed(imgd, w16, bd, clsd, posd)
    got = torch.empty_like(want)
    _lib.check(lib.tr_patch_embed_hw_bf16(imgd.data_ptr(), w16.data_ptr(), bd.data_ptr(), clsd.data_ptr(), posd.data_ptr(), got.data_ptr(), B, 3,
                                          S, S, 16, D, torch.cuda.current_stream().cuda_stream), "tr_patch_embed_hw_bf16")
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def _normalized(u8, Cc):
    return ((u8.float() / 255) - torch.tensor(MEAN[:Cc])[:, None, None]) / torch.tensor(STD[:Cc])[:, None, None]


@pytest.mark.parametrize("B,H,W", [(2, 240, 224), (1, 16, 640)])
def test_patch_embed_u8_rect_equals_the_fp32_launch_on_the_normalized_image(ops, B, H, W):
    D, P = 384, (H // 16) * (W // 16)
    g = torch.Generator().manual_seed(H + W)
    w = (0.02 * torch.randn(D, 768, generator=g)).bfloat16().cuda()
    b, cls = (0.02 * torch.randn(D, generator=g)).cuda(), (0.02 * torch.randn(D, generator=g)).cuda()
    pos = (0.02 * torch.randn(P + 1, D, generator=g)).cuda()
    u8 = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    want = ops.patch_embed(_normalized(u8, 3).cuda(), w, b, cls, pos)
    lut = pixels.pixel_lut(MEAN, STD).cuda()
    d = u8.cuda()
    for name, img in (("nchw", d), ("nhwc", d.contiguous(memory_format=torch.channels_last))):
        recs = _launches.record(lambda: ops.patch_embed_u8(img, lut, w, b, cls, pos))
        got = ops.patch_embed_u8(img, lut, w, b, cls, pos)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
        assert [r[0] for r in recs] == ["patch_embed_kernel"] and recs[0][2] == 1.0 * B * 3 * H * W + 4.0 * B * (P + 1) * D


# ---- data gradient: integers in [-4, 4], torch.equal, NaN prefill, guard words, CLS rows poisoned -------------------------------------------
def _dgrad_operands(B, H, W, Cc, D, seed):
    g = torch.Generator().manual_seed(seed)
    P = (H // 16) * (W // 16)
    wide = torch.full((B * (P + 1), D), 64.0)              # the CLS rows, which the kernel must never read: poison
    body = torch.randint(-4, 5, (B, P, D), generator=g).float()
    wide.view(B, P + 1, D)[:, 1:] = body
    wt = torch.randint(-4, 5, (Cc * 256, D), generator=g).float()
    return body, wide.bfloat16(), wt.bfloat16()


def _fold(body, wt, B, H, W, Cc):
    """torch: dcols [B, P, C*256] = dY . W (fp64, exact), column (c, iy, ix) of row (b, py, px) -> dx[b, c, 16 py + iy, 16 px + ix]."""
    gh, gw = H // 16, W // 16
    cols = body.double() @ wt.double().t()
    return cols.view(B, gh, gw, Cc, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(B, Cc, H, W).float()


def _dgrad_run(ops, dy, wt, B, H, W, Cc, call=None):
    n = B * Cc * H * W
    buf = torch.full((n + 256,), float("nan"), device="cuda")
    guard = torch.arange(256, dtype=torch.int32, device="cuda") + 0x7FC00123          # NaN payloads: any write shows
    buf[n:].view(torch.int32).copy_(guard)
    out = buf[:n].view(B, Cc, H, W)
    got = (call or (lambda o: ops.patch_embed_dgrad(dy.cuda(), wt.cuda(), B, Cc, H=H, W=W, out=o)))(out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(buf[n:].view(torch.int32), guard), "the guard behind dx was written"
    return got


# (B, H, W, C, D)
DGRAD_SHAPES = [(1, 48, 400, 3, 128),       # gw = 25: a partial second 16-patch block on every one of three rows
                (2, 80, 16, 3, 128),        # gw = 1
                (1, 16, 640, 3, 192),       # gh = 1
                (2, 64, 224, 3, 384),       # mid-size case
                (1, 32, 48, 3, 768),        # base width
                (5, 16, 32, 1, 192)]        # units span images; the last workgroup is partly empty


@pytest.mark.parametrize("B,H,W,Cc,D", DGRAD_SHAPES)
def test_dgrad_rect_is_exact_on_integers(ops, B, H, W, Cc, D):
    body, dy, wt = _dgrad_operands(B, H, W, Cc, D, seed=B * 1000 + H + 7 * W + D)
    want = _fold(body, wt.float(), B, H, W, Cc)
    got = _dgrad_run(ops, dy, wt, B, H, W, Cc)
    assert got.shape == (B, Cc, H, W)
    assert not bool(torch.isnan(got).any()), "an element of dx was never written"
    assert torch.equal(got.cpu(), want)
    assert torch.equal(_dgrad_run(ops, dy, wt, B, H, W, Cc), got)                      # the same bits run after run
    # HW = (H, W) is the same call
    assert torch.equal(_dgrad_run(ops, dy, wt, B, H, W, Cc, lambda o: ops.patch_embed_dgrad(dy.cuda(), wt.cuda(), B, Cc, (H, W), out=o)), got)


@pytest.mark.parametrize("B,S,Cc,D", [(2, 64, 3, 128), (1, 400, 3, 128), (5, 16, 1, 192)])
def test_dgrad_hw_entry_with_a_square_image_gives_the_square_entry_bits(ops, B, S, Cc, D):
    body, dy, wt = _dgrad_operands(B, S, S, Cc, D, seed=S + D)
    square = _dgrad_run(ops, dy, wt, B, S, S, Cc, lambda o: ops.patch_embed_dgrad(dy.cuda(), wt.cuda(), B, Cc, S, out=o))
    hw = _dgrad_run(ops, dy, wt, B, S, S, Cc)
    assert torch.equal(square.view(torch.int32), hw.view(torch.int32))
    assert torch.equal(hw.cpu(), _fold(body, wt.float(), B, S, S, Cc))


def test_dgrad_rect_launch_record(ops):
    B, H, W, Cc, D = 2, 48, 80, 3, 128
    _, dy, wt = _dgrad_operands(B, H, W, Cc, D, seed=1)
    dy, wt = dy.cuda(), wt.cuda()
    recs = _launches.record(lambda: ops.patch_embed_dgrad(dy, wt, B, Cc, H=H, W=W))
    P = (H // 16) * (W // 16)
    assert [r[0] for r in recs] == ["patch_embed_dgrad_kernel"]
    assert recs[0][1] == 2.0 * B * P * D * Cc * 256
    assert recs[0][2] == 4.0 * B * Cc * H * W + 2.0 * B * P * D + 2.0 * Cc * 256 * D


@pytest.mark.parametrize("Cc,H,W,patch,D", [(3, 64, 100, 16, 128), (2, 64, 96, 16, 128), (3, 64, 96, 16, 256), (3, 64, 96, 8, 128)])
def test_unsupported_rect_shape_is_an_error_not_a_launch(ops, Cc, H, W, patch, D):
    from tokenreduction_amd import _lib
    lib = _lib.load()
    assert lib.tr_patch_embed_dgrad_hw_supported(Cc, H, W, patch, D) == 0
    dy = torch.zeros(64, D, dtype=torch.bfloat16, device="cuda")
    wt = torch.zeros(Cc * patch * patch, D, dtype=torch.bfloat16, device="cuda")
    dx = torch.full((1, Cc, H, W), 7.0, device="cuda")
    rc = []
    recs = _launches.record(lambda: rc.append(lib.tr_patch_embed_dgrad_hw(dy.data_ptr(), D, wt.data_ptr(), dx.data_ptr(), 1, Cc, H, W, patch, D,
                                                                          torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert rc == [-1] and recs == []
    assert bool((dx == 7.0).all())
