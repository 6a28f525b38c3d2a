"""GPU parity tests of the DyViT training kernels (csrc/tr_dyvit_train.hip) at the op boundary, through the C ABI.

The reference of every test is a plain PyTorch restatement in float64 of the reference lines the kernel names (tests/_dyvit_ref.py, pinned
on the oracle by tests/test_dyvit_train_ref.py), fed the same bf16-rounded operands, with torch.autograd for the gradients -- the scheme
of tests/test_hip_backward.py.  Where a kernel rounds an intermediate to bf16 by design the restatement rounds at the same point, so
what is left is summation order and one final rounding: bf16 outputs are held to ONE bf16 ulp per element (_dyvit_ref.bf16_ulp_excess),
fp32 outputs to fp32 accuracy, pass-through values and decisions bit for bit, per image row and never over a whole tensor.

Tolerances the kernels' design leaves open, with the measurement they come from (tools: `python -m tests.test_hip_dyvit_train_ops`
prints them on the CPU from the float64 reference alone):
  * d policy of tr_pool_policy_bwd: the kernel recomputes the GELU output from the saved pre-activation in fp32 and does not round it to
    bf16, while the forward pooled the bf16-rounded rows.  The float64 reference with and without that rounding differs, per image, by a
    relative L2 of at most DPOL_MEASURED over the cases below; the kernel is allowed 2 x that (plus its GELU fit, 2.6e-5 absolute, and
    fp32 order, both far below).
  * hard decisions of tr_dyvit_decide: bit exact on every row whose float64 margin |t0 - t1| exceeds 1e-5; the share of rows inside the
    margin is asserted <= 1 % (the float64 reference shows 0 such rows for the seeds below)."""
import pytest
import torch

import oracle
from tests import _dyvit_ref as R

pytestmark = pytest.mark.gpu

DPOL_MEASURED = 3.88e-3         # worst image of POOL_BWD_CASES: printed by `python -m tests.test_hip_dyvit_train_ops`
DPOL_BOUND = 2 * DPOL_MEASURED
# ... and against the same reference WITHOUT that rounding (the form the kernel documents) what is left is the kernel's GELU fit, |fit - erf
# form| <= 2.6e-5 absolute (csrc/tr_common.h), on terms h0 - glob of rms >= 0.5 (GELU of unit normals): 5.2e-5 relative, x 2 for fp32 order
# and the rounding of 1 / S = 1.1e-4; held at 2e-4
DPOL_UNROUNDED_BOUND = 2e-4
MARGIN = 1e-5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


POLICIES = ("ones", "keep07", "keep03", "one", "frac")


def make_policy(kind, B, N, g):
    """fp32 [B,N], entry 0 (CLS) = 1; at least one patch token kept per image (a 0/1 policy also drops one)."""
    P = N - 1
    if kind == "ones":
        pol = torch.ones(B, P)
    elif kind in ("keep07", "keep03"):
        pol = (torch.rand(B, P, generator=g) < (0.7 if kind == "keep07" else 0.3)).float()
        for b in range(B):
            if P >= 2:
                pol[b, (3 * b + 2) % P] = 0.0                          # ... and at least one dropped
            pol[b, (3 * b + 1) % P] = 1.0
    elif kind == "one":
        pol = torch.zeros(B, P)
        for b in range(B):
            pol[b, (5 * b + 2) % P] = 1.0
    else:
        pol = torch.rand(B, P, generator=g) * 0.9 + 0.05
    return torch.cat([torch.ones(B, 1), pol], dim=1).contiguous()


# ------------------------------------------------------------------------------------------------------------------- tr_pool_policy
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [2, 14, 197, 577])
@pytest.mark.parametrize("C", [192, 384, 768, 132])
def test_pool_policy(ops, B, N, C):
    """glob = sum_p h[p,c] pol[p] / sum_p pol[p] + eps into channels C/2.. of all N rows (C/2 = 96 and 66 leave idle lanes in the last
    64-channel group)."""
    g = _gen(1000 * B + 10 * N + C)
    Ch = C // 2
    h = torch.randn(B, N, C, generator=g).bfloat16()
    for kind in POLICIES:
        pol = make_policy(kind, B, N, g)
        want = R.pool_policy_ref(h.double(), pol.double())
        pol_dev = pol.clone()
        pol_dev[:, 0] = float("nan")                                   # entry 0 must not be read
        got = ops.pool_policy(h.clone().cuda().view(B * N, C), pol_dev.cuda(), B, N).view(B, N, C).cpu()
        assert torch.isfinite(got.float()).all(), f"{kind}: policy[:, 0] was read"
        assert torch.equal(_bits(got[:, :, :Ch]), _bits(h[:, :, :Ch])), f"{kind}: the local half changed"
        assert torch.equal(_bits(got[:, :, Ch:]), _bits(got[:, :1, Ch:].expand(-1, N, -1))), f"{kind}: rows differ in the global half"
        for b in range(B):
            ex = R.bf16_ulp_excess(got[b, 1, Ch:], want[b, 1, Ch:])
            assert ex <= 0, f"{kind}: image {b}: global half off by more than one bf16 ulp (excess {ex:.3e})"
        if B > 1:                                                       # an image does not depend on its neighbours
            for b in range(B):
                alone = ops.pool_policy(h[b].clone().cuda(), pol_dev[b:b + 1].contiguous().cuda(), 1, N).cpu()
                assert torch.equal(_bits(alone), _bits(got[b])), f"{kind}: image {b} depends on the rest of the batch"


# ------------------------------------------------------------------------------------------------------------------- tr_pool_policy_bwd
# (B, N, C, offset): offset = 1 puts dcat / pre0 / dh one bf16 element into a larger buffer (the element-wise kernel); C = 132 takes the
# element-wise kernel by its width (C/2 % 8 != 0); the others the 16-byte kernel with 256 / (C/16) = 21, 10, 5, 1 row slices
POOL_BWD_CASES = [(2, 197, 192, 0), (3, 197, 384, 0), (2, 14, 768, 0), (2, 14, 4096, 0), (2, 577, 384, 0), (2, 197, 768, 0),
                  (2, 197, 132, 0), (3, 14, 132, 0), (2, 197, 384, 1), (2, 14, 384, 1)]


def pool_bwd_inputs(B, N, C, kind):
    g = _gen(7 * B + 3 * N + C + len(kind))
    pre0 = torch.randn(B, N, C, generator=g).bfloat16()
    dcat = torch.randn(B, N, C, generator=g).bfloat16()                # row 0 (CLS) is non-zero on purpose: it must not be summed
    pol = make_policy(kind, B, N, g)
    prefill = torch.randn(B, N, generator=g)
    return pre0, dcat, pol, prefill


def _offset_view(t, off):
    """t's values as a contiguous view that starts `off` elements into a larger device buffer."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (2 * off) % 16
    return v


def _run_pool_bwd(ops, pre0, dcat, cat, pol, prefill, B, N, C, off):
    dp = prefill.clone().cuda()
    dh = _offset_view(torch.full((B * N, C), 3.0).bfloat16(), off)
    ops.pool_policy_bwd(_offset_view(dcat.view(B * N, C), off), _offset_view(pre0.view(B * N, C), off), cat.view(B * N, C).cuda(), pol.cuda(), dp, B, N,
                        dh=dh)
    return dh.view(B, N, C).cpu(), dp.cpu()


@pytest.mark.parametrize("kind", ["keep07", "frac"])
@pytest.mark.parametrize("B,N,C,off", POOL_BWD_CASES)
def test_pool_policy_bwd(ops, B, N, C, off, kind):
    """Both kernels of tr_pool_policy_bwd against autograd over cat = [h0[:, :, :C/2] | glob.expand], h0 = bf16(gelu_erf(pre0)), with the
    stored broadcast value in the d policy term as the kernel documents."""
    Ch = C // 2
    pre0, dcat, pol, prefill = pool_bwd_inputs(B, N, C, kind)
    want_dh, want_dp, cat = R.pool_policy_bwd_ref(dcat.double(), pre0.double(), pol.double())
    _, unr_dp, _ = R.pool_policy_bwd_ref(dcat.double(), pre0.double(), pol.double(), round_h0=False, stored_value=cat[:, 1:2, Ch:])
    cat = cat.bfloat16()                                                # exact: the reference's broadcast value is a bf16 number
    dh, dp = _run_pool_bwd(ops, pre0, dcat, cat, pol, prefill, B, N, C, off)
    assert float(dh[:, 0].float().abs().max()) == 0.0, "dh row 0 (CLS) is not zero"
    assert torch.equal(_bits(dh[:, 1:, :Ch]), _bits(dcat[:, 1:, :Ch])), "dh local half is not a bit copy of dcat"
    assert torch.equal(_bits(dp[:, 0]), _bits(prefill[:, 0])), "d policy entry 0 was written"
    got_dp = dp.double() - prefill.double()
    for b in range(B):
        ex = R.bf16_ulp_excess(dh[b, 1:, Ch:], want_dh[b, 1:, Ch:])               # tolerance per row (its own largest entry)
        assert ex <= 0, f"image {b}: dh global half off by more than one bf16 ulp (excess {ex:.3e})"
        r = R.rel_l2(got_dp[b, 1:], want_dp[b, 1:])
        print(f"pool_policy_bwd B={B} N={N} C={C} off={off} {kind}: image {b} d policy rel L2 {r:.3e} (bound {DPOL_BOUND:.1e})")
        assert r <= DPOL_BOUND, f"image {b}: d policy rel L2 {r:.3e} > {DPOL_BOUND:.1e}"
        ru = R.rel_l2(got_dp[b, 1:], unr_dp[b, 1:])
        print(f"    ... against the reference with the unrounded GELU output: {ru:.3e} (bound {DPOL_UNROUNDED_BOUND:.1e})")
        assert ru <= DPOL_UNROUNDED_BOUND, f"image {b}: d policy rel L2 {ru:.3e} > {DPOL_UNROUNDED_BOUND:.1e} against the unrounded-h0 reference"
        dropped = (pol[b, 1:] == 0).nonzero().flatten() + 1
        if kind == "keep07" and N > 2:
            assert len(dropped) > 0
            assert float(dh[b, dropped, Ch:].float().abs().max()) == 0.0, f"image {b}: a dropped row received a global-half gradient"
            assert float(got_dp[b, dropped].abs().min()) > 0.0, f"image {b}: a dropped row has no policy gradient"
    dh2, dp2 = _run_pool_bwd(ops, pre0, dcat, cat, pol, prefill, B, N, C, off)
    assert torch.equal(_bits(dh2), _bits(dh)) and torch.equal(_bits(dp2), _bits(dp)), "not bit-identical run to run"


@pytest.mark.parametrize("B,N,C", [(2, 197, 384), (3, 14, 384), (2, 577, 192)])
def test_pool_policy_bwd_kernels_agree(ops, B, N, C):
    """The 16-byte kernel (aligned operands) and the element-wise kernel (the same operands one element into a buffer) on the same inputs:
    equal up to summation order -- one bf16 ulp on dh, fp32 accuracy on d policy (sums of C/2 <= 192 products: 192 * 2^-24 = 1.1e-5)."""
    Ch = C // 2
    pre0, dcat, pol, prefill = pool_bwd_inputs(B, N, C, "keep07")
    cat = R.pool_policy_ref(R.rb(oracle.gelu_erf(pre0.double())), pol.double()).bfloat16()
    dh_v, dp_v = _run_pool_bwd(ops, pre0, dcat, cat, pol, prefill, B, N, C, 0)
    dh_e, dp_e = _run_pool_bwd(ops, pre0, dcat, cat, pol, prefill, B, N, C, 1)
    assert torch.equal(_bits(dh_v[:, :, :Ch]), _bits(dh_e[:, :, :Ch]))
    for b in range(B):
        ex = R.bf16_ulp_excess(dh_v[b, :, Ch:], dh_e[b, :, Ch:].double())
        assert ex <= 0, f"image {b}: the two kernels differ by more than one bf16 ulp on dh (excess {ex:.3e})"
        a, e = dp_v[b, 1:].double() - prefill[b, 1:].double(), dp_e[b, 1:].double() - prefill[b, 1:].double()
        assert float((a - e).abs().max()) <= 1.1e-5 * float(e.abs().max()), f"image {b}: d policy differs between the kernels"


# ------------------------------------------------------------------------------------------------------------------- tr_dyvit_decide
DECIDE_SHAPES = [(3, 2), (3, 197), (1, 577), (5, 197)]                 # B * N = 6, 591, 577, 985: never a multiple of the 16 rows of a workgroup


def decide_inputs(B, N, C, pad):
    g = _gen(100 * B + N + C + (1 if pad else 0))
    ldh = ((C + 63) // 64 * 64 if C % 64 else C + 64) if pad else C     # padded: the next multiple of 64 (a whole extra group when C is one)
    h2 = torch.full((B, N, ldh), float("nan")).bfloat16()
    h2[:, :, :C] = torch.randn(B, N, C, generator=g).bfloat16()
    w = torch.randn(2, C, generator=g) * (0.5 / C ** 0.5)
    b = torch.randn(2, generator=g) * 0.1
    gumbel = -torch.empty(B, N - 1, 2).exponential_(generator=g).log()
    prev = (torch.rand(B, N, generator=g) < 0.7).float()
    prev[:, 0] = 1.0
    return h2, ldh, w, b, gumbel, prev


SENTINEL = 7.25


def _decide(ops, h2, w, b, gumbel, prev, B, N, C):
    outs = tuple(torch.full((B, N), SENTINEL, device="cuda") for _ in range(4))
    ops.dyvit_decide(h2.view(B * N, -1).cuda(), w.cuda(), b.cuda(), gumbel.cuda(), prev.cuda(), B, N, C, outs=outs)
    return tuple(t.cpu() for t in outs)


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("B,N", DECIDE_SHAPES)
@pytest.mark.parametrize("C", [48, 96, 192, 20])
def test_dyvit_decide(ops, B, N, C, pad):
    """ysoft0 / sm0 to fp32 accuracy, the hard decision and the policy bit exact outside the float64 margin, CLS rows untouched.
    rtol 5e-6: the logits are 16 lanes x <= 12 fma + 4 shuffle adds in fp32 (random-walk error ~ 4 * 2^-24 of sum |h w| ~ 3, so ~7e-7
    absolute on t0 - t1, which is the RELATIVE error of both outputs), plus two expf and one logf at <= 2 ulp each (3 * 1.2e-7 * |arg|);
    5e-6 is that estimate x 5 and still 1/4 of the worst-case fp32 bound 16 * 2^-24 * sum |h w| * 2 = 2e-5."""
    h2, ldh, w, b, gumbel, prev = decide_inputs(B, N, C, pad)
    ref = R.decide_ref(h2[:, :, :C].double(), w.double(), b.double(), gumbel.double(), prev.double())
    policy, ysoft0, sm0, hard0 = _decide(ops, h2, w, b, gumbel, prev, B, N, C)
    assert torch.equal(policy[:, 0], torch.ones(B)), "CLS policy is not 1"
    for t, nm in ((ysoft0, "ysoft0"), (sm0, "sm0"), (hard0, "hard0")):
        assert torch.equal(_bits(t[:, 0]), _bits(torch.full((B,), SENTINEL))), f"{nm}: a CLS entry was written"
        assert torch.isfinite(t).all(), f"{nm}: not finite (padding columns read?)"
    for got, nm in ((ysoft0, "ysoft0"), (sm0, "sm0")):
        want = ref[nm]
        rel = ((got[:, 1:].double() - want).abs() / want.abs().clamp_min(1e-30)).max()
        print(f"decide B={B} N={N} C={C} ldh={ldh}: {nm} max relative error {float(rel):.3e}")
        assert float(rel) <= 5e-6, f"{nm}: max relative error {float(rel):.3e}"
    sure = ref["margin"] > MARGIN
    share = 1.0 - float(sure.double().mean())
    assert share <= 0.01, f"{share:.3%} of the rows are inside the margin"
    assert torch.equal(hard0[:, 1:][sure].double(), ref["hard0"][sure]), "hard decision differs outside the margin"
    assert torch.equal(policy[:, 1:][sure].double(), (ref["hard0"] * prev[:, 1:].double())[sure]), "policy_out differs outside the margin"
    assert 0 < float(ref["hard0"].mean()) < 1 or N == 2, "degenerate case: one decision only"


def test_dyvit_decide_exact_tie_takes_the_first_index(ops):
    B, N, C = 2, 37, 48
    g = _gen(5)
    h2 = torch.randn(B, N, C, generator=g).bfloat16()
    pair = torch.randn(B, N - 1, 1, generator=g).expand(-1, -1, 2).contiguous()
    prev = torch.ones(B, N)
    policy, ysoft0, sm0, hard0 = _decide(ops, h2, torch.zeros(2, C), torch.full((2,), 0.3), pair, prev, B, N, C)
    assert torch.equal(hard0[:, 1:], torch.ones(B, N - 1)) and torch.equal(policy, torch.ones(B, N))
    assert torch.equal(ysoft0[:, 1:], torch.full((B, N - 1), 0.5)) and torch.equal(sm0[:, 1:], torch.full((B, N - 1), 0.5))


# ------------------------------------------------------------------------------------------------------------------- tr_dyvit_decide_bwd
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("B,N", [(3, 197), (1, 577), (5, 3), (1, 17)])          # B * N % 16 = 15, 1, 15, 1: the last workgroup is ragged
@pytest.mark.parametrize("C", [48, 96, 20])
def test_dyvit_decide_bwd(ops, B, N, C, pad):
    """Straight-through gradient against autograd over log_softmax -> + gumbel -> softmax -> hard - y_soft.detach() + y_soft -> * prev,
    with hard0 / ysoft0 / sm0 taken from the reference forward.  dW3 / db3: fp32 sums over <= 600 rows in a fixed order, held to 1e-5 of
    the largest entry (sqrt(600) * 2^-24 = 1.5e-6 expected, 600 * 2^-24 = 3.6e-5 worst case)."""
    h2, ldh, w, b, gumbel, prev = decide_inputs(B, N, C, pad)
    g = _gen(B + N + C)
    dkeep = torch.randn(B, N, generator=g)
    prefill = torch.randn(B, N, generator=g)
    want_dh2, want_dprev, want_dw, want_db, fwd = R.decide_bwd_ref(dkeep.double(), h2[:, :, :C].double(), w.double(), b.double(), gumbel.double(),
                                                                   prev.double())
    cls = lambda t: torch.cat([torch.full((B, 1), SENTINEL, dtype=torch.float64), t], dim=1).float().contiguous().cuda()
    hard0, ysoft0, sm0 = cls(fwd["hard0"]), cls(fwd["ysoft0"].detach()), cls(fwd["sm0"].detach())

    def run(accumulate, dw0=None, db0=None):
        dprev = prefill.clone().cuda()
        dw = None if dw0 is None else dw0.clone().cuda()
        db = None if db0 is None else db0.clone().cuda()
        dh2, dw, db = ops.dyvit_decide_bwd(dkeep.cuda(), prev.cuda(), hard0, ysoft0, sm0, h2.view(B * N, ldh).cuda(), w.cuda(), dprev, B, N, C,
                                           dw=dw, db=db, accumulate=accumulate)
        return dh2.view(B, N, ldh).cpu(), dprev.cpu(), dw.cpu(), db.cpu()

    dh2, dprev, dw, db = run(False)
    assert float(dh2[:, 0].float().abs().max()) == 0.0, "CLS rows of dh2 are not zero"
    if ldh > C:
        assert torch.equal(_bits(dh2[:, :, C:]), torch.zeros(B, N, ldh - C, dtype=torch.int16)), "padding columns of dh2 are not zero"
    for bb in range(B):
        ex = R.bf16_ulp_excess(dh2[bb, 1:, :C], want_dh2[bb, 1:])                  # tolerance per row (its own largest entry)
        assert ex <= 0, f"image {bb}: dh2 off by more than one bf16 ulp (excess {ex:.3e})"
    assert torch.equal(_bits(dprev[:, 0]), _bits(prefill[:, 0])), "d prev of a CLS entry was written"
    want = (prefill[:, 1:] + (dkeep[:, 1:] * fwd["hard0"].float()))                 # one fp32 product, one fp32 add
    assert torch.equal(dprev[:, 1:], want), "d prev is not prefill + d keep * hard"
    assert torch.allclose(want_dprev[:, 1:], (dkeep[:, 1:].double() * fwd["hard0"])), "reference d prev"
    tw, tb = 1e-5 * float(want_dw.abs().max()), 1e-5 * float(want_db.abs().max())
    assert float((dw.double() - want_dw).abs().max()) <= tw, f"dW3 max error {float((dw.double() - want_dw).abs().max()):.3e} > {tw:.3e}"
    assert float((db.double() - want_db).abs().max()) <= tb, f"db3 max error {float((db.double() - want_db).abs().max()):.3e} > {tb:.3e}"
    again = run(False)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip((dh2, dprev, dw, db), again)), "not bit-identical run to run"
    dw0, db0 = torch.randn(2, C, generator=g), torch.randn(2, generator=g)
    _, _, dwa, dba = run(True, dw0, db0)
    assert float((dwa.double() - dw0.double() - want_dw).abs().max()) <= tw + 2.0 ** -23 * float(dw0.abs().max())
    assert float((dba.double() - db0.double() - want_db).abs().max()) <= tb + 2.0 ** -23 * float(db0.abs().max())


def test_dyvit_decide_bwd_refuses_a_short_workspace(ops):
    from tokenreduction_amd import _lib
    B, N, C = 2, 50, 48
    h2, ldh, w, b, gumbel, prev = decide_inputs(B, N, C, False)
    z = torch.zeros(B, N, device="cuda")
    need = _lib.load().tr_dyvit_decide_bwd_workspace_floats(B, N, C)
    assert need == ((B * N + 15) // 16 + 1) * (2 * C + 4)
    short = torch.empty(need - 1, device="cuda")
    with pytest.raises(RuntimeError, match=r"code -1"):
        ops.dyvit_decide_bwd(z, prev.cuda(), z, z, z, h2.view(B * N, ldh).cuda(), w.cuda(), z.clone(), B, N, C, ws=short)


# ------------------------------------------------------------------------------------------------------------------- policy-gradient glue
@pytest.mark.parametrize("B,H,N", [(1, 3, 255), (1, 2, 256), (1, 6, 257), (3, 6, 197), (2, 12, 577), (4, 1, 64)])
def test_head_sum_adds_the_heads_in_index_order(ops, B, H, N):
    g = _gen(B + H + N)
    part = torch.randn(B, H, N, generator=g)
    prefill = torch.randn(B, N, generator=g)
    acc = torch.zeros(B, N)
    for h in range(H):
        acc = acc + part[:, h]
    got = ops.head_sum(part.cuda(), prefill.clone().cuda()).cpu()
    assert torch.equal(got, prefill + acc)


@pytest.mark.parametrize("B,N", [(1, 255), (1, 256), (1, 257), (3, 197), (2, 577), (128, 2)])
def test_add_patch_rows(ops, B, N):
    g = _gen(B + N)
    dst = torch.randn(B, N, generator=g)
    src = torch.randn(B, N - 1, generator=g)
    got = ops.add_patch_rows(dst.clone().cuda(), src.cuda()).cpu()
    assert torch.equal(_bits(got[:, 0]), _bits(dst[:, 0])), "column 0 was written"
    assert torch.equal(got[:, 1:], dst[:, 1:] + src)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 577])
def test_fill_f32(ops, n):
    t = torch.full((n + 5,), SENTINEL, device="cuda")
    ops.fill_f32(t, -1.5, n)
    assert torch.equal(t[:n].cpu(), torch.full((n,), -1.5)) and torch.equal(t[n:].cpu(), torch.full((5,), SENTINEL))


# ------------------------------------------------------------------------------------------------------------------- the predictor stage, chained
CHAIN_B, CHAIN_N = 4, 197
CHAIN_KEYS = ("in_conv.0.weight", "in_conv.0.bias", "in_conv.1.weight", "in_conv.1.bias", "out_conv.0.weight", "out_conv.0.bias",
              "out_conv.2.weight", "out_conv.2.bias", "out_conv.4.weight", "out_conv.4.bias")
# relative L2, each tensor against its own norm, between the gradients of the bf16-precision oracle and of the fp32-precision oracle on the
# inputs of test_predictor_stage_chain (the intrinsic cost of the rounding points): the worst parameter of either stage, and the worst of
# the two stream gradients.  Printed by `python -m tests.test_hip_dyvit_train_ops` (CPU).  The kernel path is allowed 2 x that.
CHAIN_MEASURED = {192: {"param": 8.52e-3, "stream": 7.03e-3}, 384: {"param": 8.41e-3, "stream": 8.01e-3}}


def chain_inputs(D):
    from tests._params import case_config, make_stage_params
    case = dict(family="dyvit", embed_dim=D, depth=2, num_heads=D // 64, num_classes=8, keep_rate=[0.7], reduction_loc=[0, 1], wseed=200 + D)
    params = make_stage_params(case_config(case), case)
    g = _gen(300 + D)
    B, N = CHAIN_B, CHAIN_N
    xs = [torch.randn(B, N, D, generator=g) + 0.3, torch.randn(B, N, D, generator=g) * 1.5 - 0.2]      # the stream entering each stage
    gum = [-torch.empty(B, N - 1, 2).exponential_(generator=g).log() for _ in range(2)]
    dpred = [torch.randn(B, N - 1, generator=g) for _ in range(2)]                                    # d out_pred_prob of each stage
    return params, xs, gum, dpred


def chain_oracle_grads(params, xs, gum, dpred, precision, forced=None):
    """torch.autograd over oracle.dyvit_predictor_logprob and the straight-through step of oracle.dyvit_train_forward, two stages chained
    through prev_decision.  -> ({parameter: gradient}, [d x of stage 0, of stage 1] (CLS rows zero), [hard decisions])."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    xl = [x.detach().clone().requires_grad_(True) for x in xs]
    B, P = xs[0].shape[0], xs[0].shape[1] - 1
    prev = torch.ones(B, P, 1)
    loss, hards = 0.0, []
    for j in range(2):
        score = oracle.dyvit_predictor_logprob(xl[j][:, 1:], prev, leaves, j, precision)
        y_soft = torch.softmax(score + gum[j], dim=-1)
        hard0 = (torch.argmax(y_soft, dim=-1) == 0).to(y_soft.dtype) if forced is None else forced[j].to(y_soft.dtype)
        y0 = (hard0 - y_soft[..., 0].detach() + y_soft[..., 0]).unsqueeze(-1)          # straight-through
        prev = y0 * prev
        loss = loss + (prev[..., 0] * dpred[j]).sum()
        hards.append(hard0.detach())
    loss.backward()
    return {k: v.grad for k, v in leaves.items()}, [x.grad for x in xl], hards


def _pad2(w, rows, cols):
    out = torch.zeros(rows, cols)
    out[:w.shape[0], :w.shape[1]] = w
    return out


@pytest.mark.parametrize("D", [192, 384])
def test_predictor_stage_chain(ops, D):
    """The predictor stage at the op boundary, chained exactly as tr_vit_forward_train and tr_vit_backward chain the ops: LayerNorm (eps
    1e-5) -> gemm_gelu_keep -> pool_policy -> two gemm_gelu_keep -> decide; then add_patch_rows -> decide_bwd -> gelu_bwd ->
    linear_bwd_params -> gemm_dgelu -> linear_bwd_params -> gemm -> pool_policy_bwd -> gelu_bwd -> linear_bwd_params -> gemm ->
    layernorm_bwd.  Two stages, so that d prev of the second reaches the first; D = 192 runs with the hidden layers zero-padded to
    128 / 64 columns as the models pack them.  Reference: autograd over the bf16-precision oracle with the DEVICE's hard decisions forced.
    Every parameter of in_conv.* / out_conv.* and both stream gradients are held by relative L2 against their OWN norm.
    Bound: 2 x the same quantity between the bf16- and the fp32-precision oracle (CHAIN_MEASURED; D = 192: worst parameter 8.52e-3 -> bound
    1.70e-2, stream 7.03e-3 -> 1.41e-2; D = 384: worst parameter 8.41e-3 -> 1.68e-2, stream 8.01e-3 -> 1.60e-2) -- the kernel path's extra bf16 roundings of the dY operands are of that size."""
    B, N = CHAIN_B, CHAIN_N
    M, Hr, Cq = B * N, D // 2, D // 4
    Hh, Q = (Hr + 63) // 64 * 64, (Cq + 63) // 64 * 64
    params, xs, gum, dpred = chain_inputs(D)
    dev = lambda t: t.contiguous().cuda()
    zeros_d = torch.zeros(D, device="cuda")
    W, tape = [], []
    prev = torch.ones(B, N, device="cuda")
    for j in range(2):                                                                  # ---- forward
        pre = f"score_predictor.{j}."
        w0, w1, w2 = params[pre + "in_conv.1.weight"], _pad2(params[pre + "out_conv.0.weight"], Hh, D), _pad2(params[pre + "out_conv.2.weight"], Q, Hh)
        w = dict(ln_g=dev(params[pre + "in_conv.0.weight"]), ln_b=dev(params[pre + "in_conv.0.bias"]),
                 w0=dev(w0.bfloat16()), b0=dev(params[pre + "in_conv.1.bias"]), w0t=dev(w0.t().bfloat16()),
                 w1=dev(w1.bfloat16()), b1=dev(_pad2(params[pre + "out_conv.0.bias"][None], 1, Hh)[0]), w1t=dev(w1.t().bfloat16()),
                 w2=dev(w2.bfloat16()), b2=dev(_pad2(params[pre + "out_conv.2.bias"][None], 1, Q)[0]), w2t=dev(w2.t().bfloat16()),
                 w3=dev(params[pre + "out_conv.4.weight"]), b3=dev(params[pre + "out_conv.4.bias"]))
        x0 = torch.empty(M, D, device="cuda")
        pu = ops.layernorm_to(dev(xs[j]).view(M, D), x0, w["ln_g"], w["ln_b"], 1e-5)
        pre0, cat = ops.gemm_gelu_keep(pu, w["w0"], w["b0"])
        ops.pool_policy(cat, prev, B, N)
        pre1, h1 = ops.gemm_gelu_keep(cat, w["w1"], w["b1"])
        pre2, h2 = ops.gemm_gelu_keep(h1, w["w2"], w["b2"])
        pol, ysoft, sm, hard = ops.dyvit_decide(h2, w["w3"], w["b3"], dev(gum[j]), prev, B, N, Cq)
        if Hh > Hr:
            assert float(h1[:, Hr:].float().abs().max()) == 0.0 and float(h2[:, Cq:].float().abs().max()) == 0.0, "padded columns are not zero"
        W.append(w)
        tape.append(dict(x0=x0, pu=pu, pre0=pre0, cat=cat, pre1=pre1, h1=h1, pre2=pre2, h2=h2, prev=prev, ysoft=ysoft, sm=sm, hard=hard))
        prev = pol
    got, got_dx = {}, [None, None]
    dpol = torch.zeros(B, N, device="cuda")
    for j in (1, 0):                                                                    # ---- backward, last stage first
        w, t = W[j], tape[j]
        pre = f"score_predictor.{j}."
        ops.add_patch_rows(dpol, dev(dpred[j]))
        dprev = torch.zeros(B, N, device="cuda")
        d2, got[pre + "out_conv.4.weight"], got[pre + "out_conv.4.bias"] = ops.dyvit_decide_bwd(dpol, t["prev"], t["hard"], t["ysoft"], t["sm"], t["h2"],
                                                                                                w["w3"], dprev, B, N, Cq)
        ops.gelu_bwd(t["pre2"], d2)
        got[pre + "out_conv.2.weight"], got[pre + "out_conv.2.bias"] = ops.linear_bwd_params(d2[:, :Cq], t["h1"][:, :Hr])
        d1 = ops.gemm_dgelu(d2, w["w2t"], t["pre1"])
        got[pre + "out_conv.0.weight"], got[pre + "out_conv.0.bias"] = ops.linear_bwd_params(d1[:, :Hr], t["cat"])
        dxn = ops.gemm(d1, w["w1t"], zeros_d, ops.TR_EPI_BF16)
        d0 = ops.pool_policy_bwd(dxn, t["pre0"], t["cat"], t["prev"], dprev, B, N)
        ops.gelu_bwd(t["pre0"], d0)
        got[pre + "in_conv.1.weight"], got[pre + "in_conv.1.bias"] = ops.linear_bwd_params(d0, t["pu"])
        dxn = ops.gemm(d0, w["w0t"], zeros_d, ops.TR_EPI_BF16)
        got_dx[j], _, got[pre + "in_conv.0.weight"], got[pre + "in_conv.0.bias"] = ops.layernorm_bwd(dxn, t["x0"], w["ln_g"], 1e-5)
        dpol = dprev                                                                    # what is left belongs to the previous stage's decision
    forced = [t["hard"][:, 1:].cpu() for t in tape]
    want, want_dx, _ = chain_oracle_grads(params, xs, gum, dpred, "bf16", forced)
    assert 0.05 < float(forced[0].mean()) < 0.95 and 0.05 < float(forced[1].mean()) < 0.95, "degenerate decisions"
    bound_p, bound_s = 2 * CHAIN_MEASURED[D]["param"], 2 * CHAIN_MEASURED[D]["stream"]
    failures = []
    for j in range(2):
        r = R.rel_l2(got_dx[j].view(B, N, D)[:, 1:], want_dx[j][:, 1:])
        print(f"predictor chain D={D}: stage {j} d stream rel L2 {r:.3e} (bound {bound_s:.2e})")
        assert float(got_dx[j].view(B, N, D)[:, 0].abs().max()) == 0.0, "the CLS rows received a gradient"
        if r > bound_s:
            failures.append(f"stage {j} d stream {r:.3e} > {bound_s:.2e}")
        for k in CHAIN_KEYS:
            key = f"score_predictor.{j}.{k}"
            r = R.rel_l2(got[key], want[key])
            print(f"predictor chain D={D}: d {key} rel L2 {r:.3e} (bound {bound_p:.2e})")
            if r > bound_p:
                failures.append(f"d {key} {r:.3e} > {bound_p:.2e}")
    assert not failures, "; ".join(failures)


def _measure_chain():
    for D in (192, 384):
        params, xs, gum, dpred = chain_inputs(D)
        gb, xb, hard = chain_oracle_grads(params, xs, gum, dpred, "bf16")
        gf, xf, _ = chain_oracle_grads(params, xs, gum, dpred, "fp32", hard)
        per = {k: R.rel_l2(gb[k], gf[k]) for k in sorted(gb)}
        for k, v in per.items():
            print(f"chain D={D}: bf16 vs fp32 oracle, d {k}: {v:.3e}")
        st = [R.rel_l2(xb[j], xf[j]) for j in range(2)]
        print(f"chain D={D}: worst parameter {max(per.values()):.3e}, stream gradients {st[0]:.3e} {st[1]:.3e}; kept share {[float(h.mean()) for h in hard]}")


def _measure():
    """CPU, float64 reference only: the figures the open tolerances above are derived from."""
    worst = 0.0
    for B, N, C, off in POOL_BWD_CASES:
        for kind in ("keep07", "frac"):
            pre0, dcat, pol, _ = pool_bwd_inputs(B, N, C, kind)
            _, dp_r, _ = R.pool_policy_bwd_ref(dcat.double(), pre0.double(), pol.double(), round_h0=True)
            _, dp_u, _ = R.pool_policy_bwd_ref(dcat.double(), pre0.double(), pol.double(), round_h0=False)
            per = [R.rel_l2(dp_u[b, 1:], dp_r[b, 1:]) for b in range(B)]
            worst = max(worst, max(per))
            print(f"pool_policy_bwd B={B} N={N} C={C} {kind}: d policy, unrounded vs bf16-rounded h0, per image: {['%.2e' % p for p in per]}")
    print(f"DPOL_MEASURED (worst image) = {worst:.3e}")
    inside = total = 0
    for C in (48, 96, 192, 20):
        for B, N in DECIDE_SHAPES:
            for pad in (False, True):
                h2, ldh, w, b, gumbel, prev = decide_inputs(B, N, C, pad)
                m = R.decide_ref(h2[:, :, :C].double(), w.double(), b.double(), gumbel.double(), prev.double())["margin"]
                inside += int((m <= MARGIN).sum())
                total += m.numel()
    print(f"decide: {inside} of {total} rows inside the margin {MARGIN}")


if __name__ == "__main__":
    _measure()
    _measure_chain()
