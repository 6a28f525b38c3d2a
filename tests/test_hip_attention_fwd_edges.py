"""Forward attention (csrc/tr_attention.hip and its fp32 / bf16x3 twins), kernel by kernel and block edge by block edge, against the float64
reference of tests/_attn_fwd_ref.py: `out` per block of 16 queries, image and head within 1.5 x the measured rounding noise of the kernels'
own rounding points (MEASURED there; tests/test_attn_fwd_ref.py proves the reference and that a leaking padded key, a leaking masked key
and a dropped last key exceed that bound more than tenfold on the designed inputs); the CLS rows and column sums at the tolerances the
older tests hold; exactly zero weight on masked keys; `out` bitwise the same with and without a side output where the same kernel serves
both.  The token counts put every ceil(N/32) = 1..7 of the register-resident kernels in every flag combination, and the 128-query-group and
128-key-chunk edges of the online-softmax, column-sum and two-pass kernels.  Every line printed carries the worst block next to its bound."""
import pytest
import torch

from tests import _attn_fwd_ref as R

pytestmark = pytest.mark.gpu

NAN_BF16 = 0x7FA5          # a bf16 NaN no kernel produces: the sentinel of the guarded `out`


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _close(got, want, atol, rtol, what):
    """entry-wise |got - want| <= atol + rtol |want|; prints the worst entry's share of its tolerance before it asserts"""
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape and not bool(got.isnan().any()), what
    ratio = float(((got - want).abs() / (atol + rtol * want.abs())).max()) if want.numel() else 0.0
    print(f"{what}: worst entry at {ratio:.2f} of its tolerance (atol {atol:.0e}, rtol {rtol:.0e})")
    assert ratio <= 1.0, f"{what}: an entry is off by {ratio:.2f} x its tolerance"


def _side_tolerances(N):
    return ((1e-6, 2e-4), (2e-4, 2e-5)) if N <= 224 else ((2e-6, 2e-3), (5e-4, 2e-3))


def _check_side(cls, part, size, want_cls, want_colsum, B, N, H, what):
    (ca, cr), (sa, sr) = _side_tolerances(N)
    if cls is not None:
        _close(cls, want_cls, ca, cr, what + " CLS rows")
        if size is not None:
            assert bool((cls.cpu()[(size == 0)[:, None, :].expand(B, H, N)] == 0).all()), f"{what}: a masked key has CLS weight"
    if part is not None:
        assert not bool(part.isnan().any()), f"{what}: a column-sum partial was not written"
        _close(part.sum(dim=(1, 2)), want_colsum, sa, sr, what + " column sums")


def _plain_bias_colsum(ops, group, B, N, H, kinds):
    """plain, bias, column sums and both together at one token count: (kind, bias) -> the four launches"""
    for kind in kinds:
        for bias in ((True,) if kind == "masked_dominant" else (False, True)):
            qkv, size, want, want_cls, want_colsum = R.case(kind, B, N, H, bias)
            dq, ds = qkv.cuda(), None if size is None else size.cuda()
            what = f"{group} {kind}{' +bias' if bias else ''}"
            out, cls = ops.attention(dq, B, N, H, want_cls=True, size=ds)
            R.assert_blocks(out, want, B, N, H, R.MEASURED[group], what)
            _check_side(cls, None, size, want_cls, want_colsum, B, N, H, what)
            out1, none = ops.attention(dq, B, N, H, size=ds)
            assert none is None and torch.equal(out1, out), f"{what}: the CLS side output changes out"
            if bias and N > 608:
                with pytest.raises(Exception):                  # column sums with a key bias: K and V^T of a head must fit the LDS
                    ops.attention(dq, B, N, H, size=ds, colsum_part=torch.zeros(B, H, 4, N, device="cuda"))
                continue
            part = torch.full((B, H, 4, N), float("nan"), device="cuda")
            out2, cls2 = ops.attention(dq, B, N, H, want_cls=True, size=ds, colsum_part=part)
            two_pass = bias and N > 224
            if not bias:
                assert torch.equal(out2, out), f"{what}: the column sums change out"       # same kernel (N <= 224) / same first pass
            else:
                R.assert_blocks(out2, want, B, N, H, R.MEASURED["twopass" if two_pass else group], what + " +colsum")
            _check_side(cls2, part, size, want_cls, want_colsum, B, N, H, what + " +colsum")


@pytest.mark.parametrize("B,N,H", R.SHAPES["16q"])
def test_register_resident_kernel(ops, B, N, H):
    """attention16_kernel<NP, column sums, bias>: every NP in every flag combination, partially filled query and key blocks"""
    _plain_bias_colsum(ops, "16q", B, N, H, R.KINDS + (("masked_dominant",) if N >= 2 else ()))


@pytest.mark.parametrize("B,N,H", R.SHAPES["flash"])
def test_online_softmax_kernel(ops, B, N, H):
    """attention_flash_kernel, attention_colsum_kernel after it (column sums without a bias) and -- at the two-pass list's lengths --
    attention_long_kernel<true> (column sums with a bias); 609 tokens and beyond refuse the latter"""
    if N in R.NS_TWOPASS or N > 608:
        _plain_bias_colsum(ops, "flash", B, N, H, R.KINDS + ("masked_dominant",))
        return
    # the other lengths: without the two-pass launches
    for kind in R.KINDS + ("masked_dominant",):
        for bias in ((True,) if kind == "masked_dominant" else (False, True)):
            qkv, size, want, want_cls, want_colsum = R.case(kind, B, N, H, bias)
            dq, ds = qkv.cuda(), None if size is None else size.cuda()
            what = f"flash {kind}{' +bias' if bias else ''}"
            part = None if bias else torch.full((B, H, 4, N), float("nan"), device="cuda")
            out, cls = ops.attention(dq, B, N, H, want_cls=True, size=ds, colsum_part=part)
            R.assert_blocks(out, want, B, N, H, R.MEASURED["flash"], what)
            _check_side(cls, part, size, want_cls, want_colsum, B, N, H, what)
            out1, _ = ops.attention(dq, B, N, H, size=ds)
            assert torch.equal(out1, out), f"{what}: a side output changes out"


@pytest.mark.parametrize("B,N,H", R.SHAPES["policy32"] + R.SHAPES["policy_flash"])
def test_policy_attention(ops, B, N, H):
    """attention_kernel<NKB, false, true, true> (every NKB) and attention_flash_kernel<true>: DyViT's softmax_with_policy"""
    group = "policy32" if N <= 224 else "policy_flash"
    for kind in ("gaussian", "policy_dominant"):
        qkv, policy, want = R.policy_case(kind, B, N, H)
        got = ops.attention_policy(qkv.cuda(), policy.cuda(), B, N, H)
        R.assert_blocks(got, want, B, N, H, R.MEASURED[group], f"{group} {kind}")


@pytest.mark.parametrize("N", R.NS_TWIN)
def test_fp32_and_bf16x3_twins(ops, N):
    """attention_f32, its split-bf16 form and the fp32 policy form (256 tokens at the most) at the tolerances their own tests hold"""
    B, H = R.shape_of(N)
    for kind in ("gaussian", "shift_neg", "masked_dominant"):
        qkv, size, want, want_cls, _ = R.case(kind, B, N, H, kind == "masked_dominant")
        dq, ds = qkv.float().cuda(), None if size is None else size.cuda()
        for split, (atol, rtol) in ((False, (2e-5, 2e-5)), (True, (1e-4, 3e-5))):
            got, cls = ops.attention_f32(dq, B, N, H, want_cls=True, size=ds, split=split)
            _close(got, want, atol, rtol, f"{'bf16x3' if split else 'fp32'} {kind} N={N} out")
            if size is not None:
                assert bool((cls.cpu()[(size == 0)[:, None, :].expand(B, H, N)] == 0).all()), f"{kind}: a masked key has CLS weight"
    if N <= 256:
        for kind in ("gaussian", "shift_neg"):
            qkv, policy = R.build_policy("gaussian", B, N, H)
            if kind == "shift_neg":
                qkv = R._set63(qkv, B, N, H, 10.0, -10.0)
            want = R.attention(qkv, B, N, H, policy=policy)[0]
            got = ops.attention_policy(qkv.float().cuda(), policy.cuda(), B, N, H)
            _close(got, want, 2e-5, 2e-5, f"fp32 policy {kind} N={N} out")


# ------------------------------------------------------------------------------------------------------------------------------ guard rows
def _guarded_call(B, N, H, qkv, size, policy, want_cls, want_colsum):
    """tr_attention_bf16 / tr_attention_policy_bf16 through the C ABI as ops.attention calls them, into buffers 32 rows (N floats) longer
    than needed and pre-filled with a sentinel -> (out [B*N, H*64], cls_rows | None, colsum_part | None) after the excess was found untouched
    and the inside wholly written"""
    from tokenreduction_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full(((B * N + 32) * H * 64,), NAN_BF16, dtype=torch.int16, device="cuda")
    cls = torch.full((B * H * N + N,), float("nan"), device="cuda") if want_cls else None
    part = torch.full((B * H * 4 * N + N,), float("nan"), device="cuda") if want_colsum else None
    if policy is not None:
        _lib.check(lib.tr_attention_policy_bf16(qkv.data_ptr(), out.data_ptr(), policy.data_ptr(), B, N, H, st), "tr_attention_policy_bf16")
    else:
        _lib.check(lib.tr_attention_bf16(qkv.data_ptr(), out.data_ptr(), None if cls is None else cls.data_ptr(),
                                         None if size is None else size.data_ptr(), None if part is None else part.data_ptr(), B, N, H, st),
                   "tr_attention_bf16")
    torch.cuda.synchronize()
    n = B * N * H * 64
    assert bool((out[n:] == NAN_BF16).all()), "out: rows past the last image were written"
    assert not bool((out[:n] == NAN_BF16).any()), "out: an element inside was not written"
    for buf, m, nm in ((cls, B * H * N, "cls_rows"), (part, B * H * 4 * N, "colsum_part")):
        if buf is not None:
            assert bool(buf[m:].isnan().all()), f"{nm}: floats past the end were written"
            assert not bool(buf[:m].isnan().any()), f"{nm}: a float inside was not written"
    return (out[:n].view(torch.bfloat16).view(B * N, H * 64), None if cls is None else cls[:B * H * N].view(B, H, N),
            None if part is None else part[:B * H * 4 * N].view(B, H, 4, N))


@pytest.mark.parametrize("kernel,N,bias,colsum", [("16q", 17, True, True), ("16q", 209, True, True), ("16q", 209, False, False),
                                                  ("flash", 225, False, True), ("flash", 257, False, True), ("flash", 257, True, False),
                                                  ("twopass", 257, True, True)])
def test_guard_rows(ops, kernel, N, bias, colsum):
    """a partially filled last query block must not write past the last image, nor the side outputs past their ends"""
    B, H = R.shape_of(N)
    qkv, size, want, want_cls, want_colsum = R.case("masked_dominant" if bias else "gaussian", B, N, H, bias)
    dq, ds = qkv.cuda(), None if size is None else size.cuda()
    out, cls, part = _guarded_call(B, N, H, dq, ds, None, True, colsum)
    R.assert_blocks(out, want, B, N, H, R.MEASURED[kernel], f"guarded {kernel}")
    _check_side(cls, part, size, want_cls, want_colsum, B, N, H, f"guarded {kernel}")
    ref, ref_cls = ops.attention(dq, B, N, H, want_cls=True, size=ds,
                                 colsum_part=torch.zeros(B, H, 4, N, device="cuda") if colsum else None)
    assert torch.equal(out, ref) and torch.equal(cls, ref_cls)


def test_guard_rows_policy(ops):
    B, N, H = 2, 33, 3
    qkv, policy, want = R.policy_case("policy_dominant", B, N, H)
    out, _, _ = _guarded_call(B, N, H, qkv.cuda(), None, policy.cuda(), False, False)
    R.assert_blocks(out, want, B, N, H, R.MEASURED["policy32"], "guarded policy32")
    assert torch.equal(out, ops.attention_policy(qkv.cuda(), policy.cuda(), B, N, H))
