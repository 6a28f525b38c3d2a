"""GPU, op level: tr_layerscale_fold and tr_layerscale_unfold_grad (csrc/tr_layerscale.hip) against numpy fp32 (tests/_layerscale_ref.py).

Fold: bitwise -- dst is the fp32 product gamma[d] * W[d,k] (one rounding), in bf16 mode rounded once more to nearest-even; dst_t is the exact
transpose of the bf16 copy; b_dst the fp32 product; with gamma == 1 the bf16 copy is tr_cast_pack_bf16's.
Unfold: dW / db bitwise in both accumulate modes (fl(gamma * x), fl(old + fl(gamma * x))); dgamma within the forward-error bound of an fp32
sum of cols + 1 products in ANY order, |got - want_fp64| <= (cols + 2) * 2^-24 * (sum_k |dW' W| + |db' b|), and the same bits on two launches.
Under `accumulate` dgamma takes one more addition: (cols + 3) * 2^-24 * (sum_k |dW' W| + |db' b| + |old|).
Every operand is a view at an odd multiple of 16 bytes inside one sentinel-filled arena; the bytes outside the views must keep the sentinel
(guard words around every buffer), and an output that is not passed costs no write anywhere."""
import numpy as np
import pytest
import torch

from tests import _launches
from tests._layerscale_ref import bf16_rne, dgamma_ref, fold_ref, unfold_ref

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (192, 192), (192, 768), (384, 1536), (128, 512)]
SPECIAL = [0.0, -0.0, -0.75, 1e-6, 1.0]          # the first gamma values of every item
SENTINEL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class Arena:
    """One device buffer of sentinel bytes; take() hands out views that start at ODD multiples of 16 bytes with at least 16 guard bytes
    between two of them; check() asserts that no byte outside the views changed."""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.off, self.taken = 0, []

    def take(self, shape, dtype, fill=None):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        start = (self.off + 16 + 15) // 16 * 16
        if (start // 16) % 2 == 0:
            start += 16
        assert start + n + 16 <= self.buf.numel()
        self.off = start + n
        self.taken.append((start, start + n))
        v = self.buf[start: start + n].view(dtype).view(shape)
        assert v.data_ptr() % 16 == 0 and ((v.data_ptr() - self.buf.data_ptr()) // 16) % 2 == 1
        if fill is not None:
            v.copy_(torch.as_tensor(fill).to(dtype).view(shape))
        return v

    def check(self):
        mask = torch.ones(self.buf.numel(), dtype=torch.bool)
        for a, b in self.taken:
            mask[a:b] = False
        assert bool((self.buf.cpu()[mask] == SENTINEL).all()), "a kernel wrote outside its operands"


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def _gamma(rng, rows):
    g = (rng.standard_normal(rows) * 0.5).astype(np.float32)
    g[:len(SPECIAL)] = SPECIAL
    return g


def _fold_items(shapes, seed, f32, variants):
    """[(numpy W, b, gamma, device item tuple)] in one arena; variants[i] = (with dst, with dst_t, with b_dst)."""
    rng = np.random.default_rng(seed)
    total = sum(r * c * 12 + r * 16 + 256 for r, c in shapes) + 4096
    arena = Arena(total)
    host, items = [], []
    for (r, c), (w_dst, w_t, w_b) in zip(shapes, variants):
        W, b, g = rng.standard_normal((r, c)).astype(np.float32), rng.standard_normal(r).astype(np.float32), _gamma(rng, r)
        dW, db, dg = arena.take((r, c), torch.float32, W), arena.take((r,), torch.float32, b), arena.take((r,), torch.float32, g)
        dst = arena.take((r, c), torch.float32 if f32 else torch.bfloat16) if w_dst else None
        dst_t = arena.take((c, r), torch.bfloat16) if w_t else None
        b_dst = arena.take((r,), torch.float32) if w_b else None
        host.append((W, b, g))
        items.append((dW, db, dg, dst, dst_t, b_dst))
    return arena, host, items


def _check_fold(arena, host, items, f32):
    from tokenreduction_amd import ops
    ops.layerscale_fold(items, dst_f32=f32)
    for (W, b, g), (_w, _b, _g, dst, dst_t, b_dst) in zip(host, items):
        prod, bf, fb = fold_ref(W, b, g)
        if dst is not None:
            want = prod.view(np.int32) if f32 else bf.view(np.int16)
            assert np.array_equal(_bits(dst), want)
        if dst_t is not None:
            assert np.array_equal(_bits(dst_t), np.ascontiguousarray(bf.T).view(np.int16))
        if b_dst is not None:
            assert np.array_equal(_bits(b_dst), fb.view(np.int32))
    arena.check()


@pytest.mark.parametrize("with_t", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_fold_one_item(shape, f32, with_t):
    arena, host, items = _fold_items([shape], 17 + shape[0] + shape[1], f32, [(True, with_t, True)])
    _check_fold(arena, host, items, f32)
    W, _b, g = host[0]
    assert np.signbit(fold_ref(W, _b, g)[0][1]).any()          # gamma -0.0: the sign of a zero product is the kernel's too (bitwise above)


@pytest.mark.parametrize("f32", [False, True])
def test_fold_seven_items_with_null_outputs(f32):
    shapes = SHAPES + [(64, 192), (128, 64)]
    variants = [(True, True, True), (True, False, True), (False, True, True), (True, True, False), (True, False, False), (False, True, False),
                (False, False, True)]
    arena, host, items = _fold_items(shapes, 5, f32, variants)
    _check_fold(arena, host, items, f32)


def test_fold_with_gamma_one_is_the_cast_pack():
    from tokenreduction_amd import ops
    for r, c in SHAPES[:3]:
        rng = np.random.default_rng(r + c)
        W = torch.from_numpy(rng.standard_normal((r, c)).astype(np.float32)).cuda()
        b, one = torch.zeros(r, device="cuda"), torch.ones(r, device="cuda")
        a, at = torch.zeros(r, c, dtype=torch.bfloat16, device="cuda"), torch.zeros(c, r, dtype=torch.bfloat16, device="cuda")
        k, kt = torch.zeros_like(a), torch.zeros_like(at)
        ops.layerscale_fold([(W, b, one, a, at, None)])
        ops.cast_pack([(W, k, kt)])
        assert torch.equal(a, k) and torch.equal(at, kt) and torch.equal(a.float(), W.to(torch.bfloat16).float())


def _unfold_items(shapes, seed, variants):
    rng = np.random.default_rng(seed)
    arena = Arena(sum(r * c * 12 + r * 32 + 512 for r, c in shapes) + 4096)
    host, items = [], []
    for (r, c), (w_dw, w_db, w_dg) in zip(shapes, variants):
        X, W = rng.standard_normal((r, c)).astype(np.float32), rng.standard_normal((r, c)).astype(np.float32)
        xb, b, g = rng.standard_normal(r).astype(np.float32), rng.standard_normal(r).astype(np.float32), _gamma(rng, r)
        old = (rng.standard_normal((r, c)).astype(np.float32), rng.standard_normal(r).astype(np.float32), rng.standard_normal(r).astype(np.float32))
        dev = [arena.take(t.shape, torch.float32, t) for t in (X, xb, W, b, g)]
        outs = [arena.take(t.shape, torch.float32, t) if w else None for t, w in zip(old, (w_dw, w_db, w_dg))]
        host.append((X, xb, W, b, g, old))
        items.append(tuple(dev) + tuple(outs))
    return arena, host, items


def _check_unfold(arena, host, items, accumulate):
    from tokenreduction_amd import ops
    inputs = [[t.clone() for t in it[:5]] for it in items]
    ops.layerscale_unfold_grad(items, accumulate=accumulate)
    first = [[None if t is None else t.clone() for t in it[5:]] for it in items]
    for (X, xb, W, b, g, old), it in zip(host, items):
        dw, db, dg = it[5:]
        want_dw, want_db = unfold_ref(X, xb, g, old[0] if accumulate else None, old[1] if accumulate else None)
        if dw is not None:
            assert np.array_equal(_bits(dw), want_dw.view(np.int32))
        if db is not None:
            assert np.array_equal(_bits(db), want_db.view(np.int32))
        if dg is not None:
            want, bound = dgamma_ref(X, xb, W, b)
            if accumulate:      # one more addition: (cols + 3) * 2^-24 * (sum |dW' W| + |db' b| + |old|)
                bound = (X.shape[1] + 3) * (bound / (X.shape[1] + 2) + 2.0 ** -24 * np.abs(old[2].astype(np.float64)))
                want = want + old[2].astype(np.float64)
            err = np.abs(dg.cpu().numpy().astype(np.float64) - want)
            print(f"dgamma {X.shape} accumulate={accumulate}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (err <= bound).all()
    for it, keep in zip(items, inputs):                  # the folded gradients and the parameters are only read
        assert all(torch.equal(a, b) for a, b in zip(it[:5], keep))
    arena.check()
    # a second launch from the same state: identical bits (no atomics, an order that depends on cols alone)
    for (_X, _xb, _W, _b, _g, old), it in zip(host, items):
        for t, o in zip(it[5:], old):
            if t is not None:
                t.copy_(torch.from_numpy(o))
    ops.layerscale_unfold_grad(items, accumulate=accumulate)
    for it, f in zip(items, first):
        assert all(a is None or np.array_equal(_bits(a), _bits(b)) for a, b in zip(it[5:], f))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_unfold_one_item(shape, accumulate):
    arena, host, items = _unfold_items([shape], 29 + shape[0] + shape[1], [(True, True, True)])
    _check_unfold(arena, host, items, accumulate)


@pytest.mark.parametrize("accumulate", [False, True])
def test_unfold_seven_items_with_null_outputs(accumulate):
    shapes = SHAPES + [(64, 192), (128, 64)]
    variants = [(True, True, True), (True, True, False), (False, False, True), (True, False, True), (False, True, False), (True, False, False),
                (False, True, True)]
    arena, host, items = _unfold_items(shapes, 9, variants)
    _check_unfold(arena, host, items, accumulate)


def test_one_launch_each_and_refusals():
    from tokenreduction_amd import ops
    arena, _host, items = _fold_items(SHAPES[:2], 3, False, [(True, True, True)] * 2)
    assert _launches.labels(lambda: ops.layerscale_fold(items)) == ["tr_layerscale_fold"]
    arena2, _h2, it2 = _unfold_items(SHAPES[:2], 4, [(True, True, True)] * 2)
    assert _launches.labels(lambda: ops.layerscale_unfold_grad(it2)) == ["tr_layerscale_unfold_grad"]
    bad = torch.zeros(65, 64, device="cuda")
    with pytest.raises(RuntimeError, match="tr_layerscale_fold"):
        ops.layerscale_fold([(bad, None, torch.zeros(65, device="cuda"), None, None, None)])
    assert bf16_rne(np.array([1.00390625], dtype=np.float32))[0] == 0x3F80          # a tie rounds to the even neighbour
