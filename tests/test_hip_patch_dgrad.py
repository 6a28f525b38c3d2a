"""GPU: tr_patch_embed_dgrad (csrc/tr_patch.hip) -- PatchEmbed's data gradient folded back into the image -- bit for bit against torch.

Inputs are integers in [-4, 4] (exact in bf16): every product is an integer of magnitude <= 16 and every fp32 partial sum up to
K = D = 768 is an integer below 2^24, so the result is exact whatever the summation order and the comparison is torch.equal.  dY is in the
token-row layout of the executor's stream gradient, [B * (P + 1), D] with one CLS row per image that the kernel must never read: those
rows hold 64, so a wrong row map shows in the output.  dx is prefilled with NaN (an element the kernel does not write stays NaN: every
element is written exactly once, there is no memset) and followed by a 256-float guard that must keep its bits."""
import pytest
import torch

from tests import _launches

pytestmark = pytest.mark.gpu

TR_ERR_SHAPE = -1
LABEL = "patch_embed_dgrad_kernel"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _operands(B, HW, Cc, D, seed, ldy=None):
    g = torch.Generator().manual_seed(seed)
    P = (HW // 16) ** 2
    ldy = D if ldy is None else ldy
    wide = torch.full((B * (P + 1), ldy), 64.0)            # CLS rows and (ldy > D) the columns beside the operand: poison
    body = torch.randint(-4, 5, (B, P, D), generator=g).float()
    wide.view(B, P + 1, ldy)[:, 1:, :D] = body
    wt = torch.randint(-4, 5, (Cc * 256, D), generator=g).float()
    return body, wide.bfloat16(), wt.bfloat16()


def _fold(body, wt, B, HW, Cc):
    """torch: dcols [B, P, C*256] = dY . W (fp64, exact), column (c, iy, ix) of row (b, py, px) -> dx[b, c, 16 py + iy, 16 px + ix]."""
    gw = HW // 16
    cols = body.double() @ wt.double().t()
    return cols.view(B, gw, gw, Cc, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(B, Cc, HW, HW).float()


def _run(dy, wt, B, HW, Cc, D):
    from tokenreduction_amd import ops
    n = B * Cc * HW * HW
    buf = torch.full((n + 256,), float("nan"), device="cuda")
    guard = torch.arange(256, dtype=torch.int32, device="cuda") + 0x7FC00123          # NaN payloads: any write shows
    buf[n:].view(torch.int32).copy_(guard)
    out = buf[:n].view(B, Cc, HW, HW)
    view = dy.cuda()[:, :D] if dy.shape[1] != D else dy.cuda()
    got = ops.patch_embed_dgrad(view, wt.cuda(), B, Cc, HW, 16, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(buf[n:].view(torch.int32), guard), "the guard behind dx was written"
    return got


SHAPES = [(1, 16, 3, 128),          # M = 1
          (3, 48, 3, 128),          # M = 27: below and off every tile
          (2, 224, 3, 384),         # M = 392: the product width
          (2, 64, 1, 128),          # one channel: kcols = 256
          (1, 32, 3, 768),          # base width
          (2, 224, 3, 192),         # tiny width
          (1, 400, 3, 128),         # 25 patches per row: a second, partial 16-patch block per patch row (625 tokens)
          (5, 16, 1, 192)]          # five one-patch images: a workgroup's units span images, the last workgroup is partly empty


@pytest.mark.parametrize("B,HW,Cc,D", SHAPES)
def test_dgrad_is_exact_on_integers(B, HW, Cc, D):
    body, dy, wt = _operands(B, HW, Cc, D, seed=B * 1000 + HW + D)
    want = _fold(body, wt.float(), B, HW, Cc)
    got = _run(dy, wt, B, HW, Cc, D)
    assert not bool(torch.isnan(got).any()), "an element of dx was never written"
    assert torch.equal(got.cpu(), want)
    assert torch.equal(_run(dy, wt, B, HW, Cc, D), got)                      # the same bits run after run


def test_dgrad_reads_a_column_slice_of_a_wider_tensor():
    B, HW, Cc, D = 2, 48, 3, 128
    body, dy, wt = _operands(B, HW, Cc, D, seed=5, ldy=D + 64)
    assert torch.equal(_run(dy, wt, B, HW, Cc, D).cpu(), _fold(body, wt.float(), B, HW, Cc))


def test_dgrad_launch_record():
    from tokenreduction_amd import ops
    B, HW, Cc, D = 2, 64, 3, 128
    _, dy, wt = _operands(B, HW, Cc, D, seed=1)
    dy, wt = dy.cuda(), wt.cuda()
    recs = _launches.record(lambda: ops.patch_embed_dgrad(dy, wt, B, Cc, HW))
    assert [r[0] for r in recs] == [LABEL]
    P = (HW // 16) ** 2
    assert recs[0][1] == 2.0 * B * P * D * Cc * 256 and recs[0][2] >= 4.0 * B * Cc * HW * HW


@pytest.mark.parametrize("Cc,HW,patch,D", [(3, 224, 16, 256), (3, 224, 16, 64), (2, 224, 16, 128), (3, 232, 16, 128), (3, 224, 8, 128),
                                           (3, 224, 32, 384)])
def test_unsupported_shape_is_an_error_not_a_launch(Cc, HW, patch, D):
    from tokenreduction_amd import _lib, ops
    lib = _lib.load()
    assert lib.tr_patch_embed_dgrad_supported(Cc, HW, patch, D) == 0
    B, P = 1, (HW // patch) ** 2
    dy = torch.zeros(B * (P + 1), D, dtype=torch.bfloat16, device="cuda")
    wt = torch.zeros(Cc * patch * patch, D, dtype=torch.bfloat16, device="cuda")
    dx = torch.full((B, Cc, HW, HW), 7.0, device="cuda")
    rc = []
    recs = _launches.record(lambda: rc.append(lib.tr_patch_embed_dgrad(dy.data_ptr(), D, wt.data_ptr(), dx.data_ptr(), B, Cc, HW, patch, D,
                                                                       torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert rc == [TR_ERR_SHAPE] and recs == []
    assert bool((dx == 7.0).all())
    if HW % patch == 0:
        with pytest.raises(RuntimeError, match="tr_patch_embed_dgrad"):
            ops.patch_embed_dgrad(dy, wt, B, Cc, HW, patch)


def test_supported_shapes():
    from tokenreduction_amd import _lib
    lib = _lib.load()
    for D in (128, 192, 384, 768):
        for Cc in (1, 3):
            for HW in (16, 224, 384, 400):
                assert lib.tr_patch_embed_dgrad_supported(Cc, HW, 16, D) == 1
    null = lib.tr_patch_embed_dgrad(None, 128, None, None, 1, 3, 224, 16, 128, None)
    assert null == -3                                                        # TR_ERR_NULL
