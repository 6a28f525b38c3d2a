"""References for the ATS forward kernels (csrc/tr_ats.hip): inputs whose cdf is exact, the two nearest-entry searches, and the CPU
measurement the cdf bound for random inputs comes from.  Shared by tests/test_ats_ref.py (CPU) and tests/test_hip_ats_edges.py (GPU).

The sampled ids are an integer decision on fp32 roundings: which of two near-equidistant cdf entries a grid point takes.  torch.cdist (the
reference, ats.py:73) has two forms for it:
  direct   sqrt((s - c)^2)                       when both sides have <= 25 rows (P <= 25 cdf entries AND <= 25 grid points)
  matmul   sqrt(max(-2 s c + s^2 + c^2, 1e-30))  otherwise; its rounding decides among candidates closer than ~3e-4
To aim at such near-ties the cdf has to be the same on the device and in the oracle bit for bit, which it is not for arbitrary inputs (the
kernel sums sequentially in fp32, torch's CPU cumsum accumulates in double).  exact_case() removes that:
  * cls_rows holds integer-valued floats, every v head-row is one-hot with value 1.0 (|v| = 1 exactly in bf16 and fp32), and the integers
    of an image sum to 2^22.  Head sum, total and running sum are then exact in any order, fl(2^22 + 1e-6) = 2^22, the division is by a
    power of two: every cdf entry is a chosen multiple of 2^-22.
  * per grid point s that gets a pair, two entries round((s - d) / 2^-22) and round((s + d) / 2^-22) + j, d = 0.1 .. 0.45 of the grid
    spacing, j in [-8, 8]; the last entry is 2^22 (cdf 1.0) and surplus entries repeat it (zero significance, a plateau).

Case tables (P, K, seed).  SMALL takes the direct form; BOUNDARY and LONG the matmul form.  The seed of a case is the first one whose
inputs hold a decision that tells the two forms apart (`python -m tests._ats_ref scan`); tests/test_ats_ref.py asserts that they do.  A
pair needs three entries (two and the closing 1.0), so P = 1 (one candidate: no decision at all) and P = 2 are in SMALL for the kernel's
sake only.

cdf bound for random inputs: kernel_cdf() restates the kernel's documented arithmetic in numpy fp32 (heads summed in order, total + eps,
quotient, sequential running sum, +0.1 on masked entries) and is compared with oracle.ats_cdf(oracle.ats_scores(...)) over the GPU tests'
own shapes and seeds.  `python -m tests._ats_ref` prints the worst difference per length; MEASURED holds those figures as printed (lengths
N <= 70 share the worst of their sweep: single lengths there measure one or two roundings of a value near 1, which says nothing about the
next length).  The kernel is allowed 2 x that: its total is summed in 64 lanes and a tree, and |v|^2 is an fma chain.
"""
import numpy as np
import torch

import oracle

F32 = np.float32
UNIT = 2.0 ** -22
TOTAL = 1 << 22
DIRECT_MAX = 25            # torch.cdist's direct form: both row counts <= 25

# ---------------------------------------------------------------------------------------------------------------- the tests' shapes
EXACT_B = 4
# (P, K, seed): K = the sample count, oracle.ats_sample_steps(K) the grid
SMALL = [(1, 2, 0), (2, 2, 0), (2, 3, 0), (3, 2, 41), (5, 3, 16), (7, 3, 11), (9, 5, 1), (15, 8, 0), (17, 6, 7), (24, 25, 0), (25, 13, 0),
         (25, 20, 0), (25, 25, 0), (25, 26, 0)]
BOUNDARY = [(26, 3, 8), (26, 6, 0), (26, 13, 0), (25, 27, 0), (12, 27, 0)]
LONG = [(196, 98, 0), (576, 288, 0), (1024, 512, 0), (1024, 26, 0)]
MIN_SMALL_TOTAL, MIN_LONG_EACH = 20, 20

# random-input cases of the every-length test: N = 2 .. 70 with B = 2, then (N, H, K) -- K of 64, 65 and 66 give 63, 64 and 65 grid points
SWEEP_N = tuple(range(2, 71))
LARGE = [(130, 1, 64), (130, 6, 65), (130, 12, 66), (257, 16, 129), (513, 6, 300), (577, 12, 404), (785, 1, 400), (1025, 16, 513),
         (1025, 20, 700)]
RANDOM_B = 2

# worst |kernel_cdf - oracle cdf| per length over the inputs above, bf16 and fp32, with and without mask: `python -m tests._ats_ref`
MEASURED = {70: 4.172e-07, 130: 4.768e-07, 257: 4.768e-07, 513: 8.941e-07, 577: 5.96e-07, 785: 7.153e-07, 1025: 1.848e-06}
CDF_FACTOR = 2.0


def sweep_shape(N):
    """(H, K) of length N in the N = 2 .. 70 sweep"""
    return (1, 3, 6)[N % 3], max(2, (7 * (N - 1)) // 10 + 1)


def n_steps(K):
    return int(oracle.ats_sample_steps(K).numel())


def form_of(P, K):
    return "direct" if P <= DIRECT_MAX and n_steps(K) <= DIRECT_MAX else "matmul"


# ---------------------------------------------------------------------------------------------------------------- exact-cdf inputs
def _one_hot_qkv(rng, B, N, H):
    """qkv fp32 [B*N, 3*H*64]: q and k arbitrary (bf16-exact), every v head-row one-hot 1.0"""
    qkv = torch.from_numpy(rng.standard_normal((B, N, 3, H, 64)).astype(F32)).bfloat16().float()
    v = np.zeros((B, N, H, 64), F32)
    hot = rng.integers(0, 64, (B, N, H))
    np.put_along_axis(v, hot[..., None], 1.0, axis=-1)
    qkv[:, :, 2] = torch.from_numpy(v)
    return qkv.reshape(B * N, 3 * H * 64)


def from_units(units, H, rng):
    """units int64 [B,P], non-decreasing, last = 2^22: the cdf in units of 2^-22.  -> dict(cls_rows fp32 [B,H,N] of integer-valued floats
    (significance split across the heads; the CLS column, which nothing may read, is NaN), qkv fp32 [B*N, 3*H*64], cdf fp32 [B,P])."""
    units = np.asarray(units, np.int64)
    B, P = units.shape
    sig = np.diff(units, axis=1, prepend=0)
    assert (sig >= 0).all() and (units[:, -1] == TOTAL).all()
    left, parts = sig.copy(), []
    for _ in range(H - 1):
        take = rng.integers(0, left + 1)
        parts.append(take)
        left = left - take
    parts.append(left)
    cls = np.full((B, H, P + 1), np.nan, F32)
    cls[:, :, 1:] = np.stack(parts, axis=1).astype(F32)
    cdf = (units.astype(np.float64) * UNIT).astype(F32)
    # the round trip integer -> quotient -> fp32 running sum, in fp32 all the way
    quot = cls[:, :, 1:].sum(axis=1, dtype=F32) / F32(F32(TOTAL) + F32(1e-6))
    assert np.array_equal(np.cumsum(quot, axis=1, dtype=F32), cdf) and np.array_equal(cdf.astype(np.float64), units * UNIT)
    return dict(cls_rows=torch.from_numpy(cls), qkv=_one_hot_qkv(rng, B, P + 1, H), cdf=torch.from_numpy(cdf))


def exact_case(P, K, H, seed, B=EXACT_B):
    """Near-symmetric pairs of cdf entries around grid points of oracle.ats_sample_steps(K) (module docstring).  -> dict(cls_rows, qkv,
    cdf, steps fp32 [n_steps], mask fp32 ones [B,N]); a pure function of its arguments."""
    rng = np.random.default_rng([P, K, H, seed])
    steps = oracle.ats_sample_steps(K)
    s64 = steps.double().numpy()
    ns = len(s64)
    n_pairs = min(ns, (P - 1) // 2)
    units = np.full((B, P), TOTAL, np.int64)
    for b in range(B):
        at = np.sort(rng.permutation(ns)[:n_pairs])
        d = rng.uniform(0.1, 0.45, n_pairs) / K
        j = rng.integers(-8, 9, n_pairs)
        lo = np.rint((s64[at] - d) / UNIT).astype(np.int64)
        hi = np.rint((s64[at] + d) / UNIT).astype(np.int64) + j
        units[b, :2 * n_pairs] = np.stack([lo, hi], axis=1).reshape(-1)
    assert (np.diff(units, axis=1) >= 0).all() and (units[:, 0] > 0).all()
    case = from_units(units, H, rng)
    case.update(steps=steps, mask=torch.ones(B, P + 1))
    return case


def v_of(qkv, B, N, H):
    """v [B,H,N,64] of a token-major qkv [B*N, 3*H*64]"""
    return qkv.reshape(B, N, 3, H, 64)[:, :, 2].permute(0, 2, 1, 3)


def oracle_cdf(cls_rows, qkv, mask):
    B, H, N = cls_rows.shape
    return oracle.ats_cdf(oracle.ats_scores(cls_rows, v_of(qkv, B, N, H)), mask.bool())


# ---------------------------------------------------------------------------------------------------------------- the two searches
def _first_min(d):
    return np.argmin(d, axis=-1)                                           # numpy keeps the first minimum, like torch


def matmul_form_argmin(cdf, steps):
    """torch.cdist's matmul form in fp32, every operation rounded once: [-2s, s^2, 1] . [c, 1, c^2] summed in that order, clamp at 1e-30,
    sqrt; the first minimum wins.  cdf [B,P], steps [S] -> int64 [B,S]"""
    c, s = np.asarray(cdf, F32)[:, None, :], np.asarray(steps, F32)[None, :, None]
    r = (F32(-2.0) * s) * c
    r = r + s * s
    r = r + c * c
    assert r.dtype == F32
    return _first_min(np.sqrt(np.maximum(r, F32(1e-30))))


def direct_form_argmin(cdf, steps):
    """torch.cdist's direct form in fp32: x = s - c, sqrt(x * x), each rounded once; the first minimum wins."""
    c, s = np.asarray(cdf, F32)[:, None, :], np.asarray(steps, F32)[None, :, None]
    x = s - c
    d = np.sqrt(x * x)
    assert d.dtype == F32
    return _first_min(d)


def cdist_argmin(cdf, steps):
    """The oracle's own search (oracle.ats_ids_from_cdf, first two lines) -> int64 [B,S]"""
    cdf, steps = torch.as_tensor(cdf), torch.as_tensor(steps)
    return torch.argmin(torch.cdist(steps.unsqueeze(0).unsqueeze(2), cdf.unsqueeze(2)), dim=-1).numpy()


def telling_decisions(cdf, steps, P, K):
    """How many decisions of this input the form that does NOT apply at (P, K) gets wrong against torch.cdist."""
    other = matmul_form_argmin if form_of(P, K) == "direct" else direct_form_argmin
    return int((other(cdf, steps) != cdist_argmin(cdf, steps)).sum())


# ---------------------------------------------------------------------------------------------------------------- the kernel's cdf
def kernel_cdf(cls_rows, qkv, mask=None, eps=1e-6):
    """ats_sample_kernel's arithmetic in numpy fp32: |v|^2 summed in element order, sqrt, one product per (head, token); heads summed in
    order; the total summed in token order, + eps; the quotients; the running sum in token order; +0.1 on masked entries.  -> fp32 [B,P]"""
    cls = np.asarray(cls_rows, F32)
    B, H, N = cls.shape
    v = np.asarray(v_of(torch.as_tensor(qkv).float(), B, N, H), F32)[:, :, 1:]
    ss = np.zeros(v.shape[:-1], F32)
    for e in range(64):
        ss = ss + v[..., e] * v[..., e]
    part = cls[:, :, 1:] * np.sqrt(ss)
    sig = np.zeros((B, N - 1), F32)
    for h in range(H):
        sig = sig + part[:, h]
    total = np.cumsum(sig, axis=1, dtype=F32)[:, -1:] + F32(eps)
    cdf = np.cumsum(sig / total, axis=1, dtype=F32)
    if mask is not None:
        cdf = np.where(np.asarray(mask)[:, 1:] == 0, cdf + F32(0.1), cdf)
    assert cdf.dtype == F32
    return cdf


def random_case(N, H, seed, masked, f32, B=RANDOM_B):
    """Random probabilities and values, as an ATS block sees them.  masked: image 0 keeps a random number of leading patches, the last image
    keeps ONE patch; masked keys have exactly zero probability.  -> dict(cls_rows fp32 [B,H,N], qkv fp32 [B*N, 3*H*64] (bf16-exact unless
    f32), mask fp32 [B,N])"""
    rng = np.random.default_rng([N, H, seed, int(masked), int(f32)])
    qkv = torch.from_numpy(rng.standard_normal((B * N, 3 * H * 64)).astype(F32))
    if not f32:
        qkv = qkv.bfloat16().float()
    mask = torch.ones(B, N)
    if masked:
        for b in range(B - 1):
            mask[b, 1 + int(rng.integers(1, N)):] = 0
        mask[B - 1, 2:] = 0
    logits = torch.from_numpy((rng.standard_normal((B, H, N)) * 2.0).astype(F32))
    cls = torch.softmax(logits.masked_fill(mask[:, None, :] == 0, -1e30), dim=-1)
    return dict(cls_rows=cls, qkv=qkv, mask=mask)


def random_cases():
    """(N, H, K) of every random-input case"""
    return [(N, *sweep_shape(N)) for N in SWEEP_N] + LARGE


def length_key(N):
    return 70 if N <= 70 else N


def cdf_bound(N):
    return CDF_FACTOR * MEASURED[length_key(N)]


def measure(cases=None):
    """-> {length key: worst |kernel_cdf - oracle cdf|} over random_cases(), both precisions, with and without mask"""
    worst = {}
    for N, H, _ in (random_cases() if cases is None else cases):
        for f32 in (False, True):
            for masked in (False, True):
                c = random_case(N, H, 0, masked, f32)
                err = np.abs(kernel_cdf(c["cls_rows"], c["qkv"], c["mask"]).astype(np.float64)
                             - oracle_cdf(c["cls_rows"], c["qkv"], c["mask"]).double().numpy()).max()
                worst[length_key(N)] = max(worst.get(length_key(N), 0.0), float(err))
    return worst


# ---------------------------------------------------------------------------------------------------------------- command line
def _scan(n_seeds=200):
    """The first seed of every table case whose H = 1 and H = 3 inputs both hold a telling decision (at least MIN_LONG_EACH for LONG)"""
    for name, table in (("SMALL", SMALL), ("BOUNDARY", BOUNDARY), ("LONG", LONG)):
        out = []
        for P, K, _ in table:
            need = MIN_LONG_EACH if name == "LONG" else 1 if P >= 3 else 0
            for seed in range(n_seeds):
                got = [telling_decisions(c["cdf"].numpy(), c["steps"].numpy(), P, K) for c in (exact_case(P, K, H, seed) for H in (1, 3))]
                if min(got) >= need:
                    break
            else:
                seed, got = None, None
            out.append((P, K, seed))
            print(f"{name} (P, K) = ({P}, {K}) [{form_of(P, K)}, {n_steps(K)} grid points]: seed {seed}, telling decisions {got}")
        print(f"{name} = {out}")


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1 and sys.argv[1] == "scan":
        _scan()
    else:
        print("MEASURED =", {k: float(f"{v:.3e}") for k, v in sorted(measure().items())})
