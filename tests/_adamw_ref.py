"""Element-wise comparison of the one-launch AdamW step (csrc/tr_optim.hip, through ops.adamw_step and optim.FusedAdamW) with a plain
float64 AdamW, the inputs of tests/test_hip_adamw_edges.py, and the CPU measurement its parameter bound comes from.

`reference` is torch's documented AdamW (decoupled decay) in float64 with no fp32 rounding anywhere.  `emulated` is the same step with
fp32 roundings where the header comment of csrc/tr_optim.hip says the kernel rounds, in numpy (no fused multiply-add); it exists only to
measure what that rounding costs against `reference` and is never compared with the kernel.

Metrics (`errors`), per element, none exempt:
  * exp_avg', exp_avg_sq': |got - ref| in fp32 ulps of the reference value.  Each is ONE rounding of a double expression, so the kernel
    is allowed MOMENT_ULPS = 1 -- derived, not measured (0.5 for the rounding, the rest for the double expression's own form).
  * p': |got - ref| / (ulp32(p'_ref) + |u_ref| * 2^-23), u the update.  The update is a chain of fp32 operations, so its error scales
    with |u|; the final subtraction adds half an ulp of p'.  The bound is MARGIN x MEASURED, MEASURED the worst `emulated` element over
    the GPU tests' own inputs (`python -m tests._adamw_ref` prints it), MARGIN = 2: the device's sqrtf and division may be 1 ulp where
    numpy's are 0.5, and the kernel contracts three expressions that numpy does not.
  * where the reference is not finite, or beyond the fp32 range, the positions and signs of inf / NaN must coincide; a position that does
    not counts as an infinite error.
  * a degenerate element -- reference update exactly 0 -- must equal the decayed p, fp32(p - lr * wd * p), bit for bit.  An element whose
    reference exp_avg_sq' is finite but beyond the fp32 range (g = 1e21: (1 - beta2) g^2 = 1e39) is degenerate too: every fp32 optimizer
    stores inf there and its update is m / inf = 0.
"""
import collections
import functools

import numpy as np
import torch

F32_MAX = float(np.finfo(np.float32).max)
F32_OVER = F32_MAX * (1.0 + 2.0 ** -25)          # from here a double rounds to an fp32 infinity
MOMENT_ULPS = 1.0
MARGIN = 2.0
# Worst p' metric of `emulated` against `reference` over the inputs below, printed by `python -m tests._adamw_ref` (CPU) and rounded up
# in the third digit.  tests/test_adamw_ref.py fails if the measurement gives more than this now.
MEASURED = 2.14

EPS = 1e-8
# eight groups; the tile test uses GROUPS_USED (distinct lr, group 2 without decay, one group at index 7)
LRS = (1e-3, 7e-4, 3e-3, 5e-4, 2e-3, 1.5e-3, 9e-4, 2.5e-3)
WDS = (0.05, 0.01, 0.0, 0.02, 0.03, 0.1, 0.04, 0.07)
GROUPS_USED = (0, 2, 5, 7)

# ---------------------------------------------------------------------------------------------------------------- the tile test's items
# rows, cols, with dst, with dst_t, offsets of p / g / m / v in floats and of dst / dst_t in bf16 elements inside their buffers
Spec = collections.namedtuple("Spec", "rows cols dst dst_t po go mo vo do to", defaults=(True, True, 0, 0, 0, 0, 0, 0))
TILE_SPECS = [
    Spec(130, 1536), Spec(1536, 130), Spec(384, 1000), Spec(64, 64),        # 0-3   vector path, full and ragged row / column tiles
    Spec(65, 63), Spec(63, 65), Spec(1, 384), Spec(384, 1), Spec(1, 1),     # 4-8   cols % 4 != 0: scalar elements; rows % 4 != 0: scalar dst_t
    Spec(64, 384, True, False), Spec(384, 64, False, True),                 # 9-10  dst without dst_t and the reverse, vector path
    Spec(65, 63, True, False), Spec(63, 65, False, True),                   # 11-12 the same on the scalar paths
    Spec(64, 384, False, False),                                            # 13    neither copy (a bias, a norm weight)
    Spec(384, 64, po=1),                                                    # 14    p 4 bytes off: scalar elements
    Spec(64, 128, go=1), Spec(64, 128, mo=1), Spec(64, 128, vo=1),          # 15-17 g / m / v 4 bytes off, each alone
    Spec(64, 128, po=2, go=2, mo=2, vo=2),                                  # 18    all four 8 bytes off (16-byte alignment is what counts)
    Spec(64, 384, do=1),                                                    # 19    dst 2 bytes off: scalar elements and straight stores
    Spec(384, 384, to=1),                                                   # 20    dst_t 2 bytes off: scalar transposed stores
    Spec(64, 384, do=2), Spec(384, 64, to=2),                               # 21-22 dst / dst_t 4 bytes off (not 8-byte aligned), each alone
    Spec(1000, 384, do=2, to=2),                                            # 23    both, 16 x 6 tiles with a ragged last row tile
    Spec(65, 1000), Spec(1000, 65), Spec(130, 66),                          # 24-26 c + e < cols inside a 4-column group (66 = 64 + 2)
    Spec(1, 4099, True, False),                                             # 27    a vector over 65 column tiles, 3 columns in the last
    Spec(1, 1, False, False),                                               # 28    the last item: one tile, one element
]
TILE_STEPS = 3
TILE_BETAS = (0.9, 0.98)

# -------------------------------------------------------------------------------------------------------------- the item-table test's items
BIG = [(130, 200), (65, 300), (384, 64), (200, 130), (1, 4099), (70, 70)]
SMALL = [(1, 64), (1, 1), (64, 64)]


def table_shapes(n):
    """n = 1, n = 2, or the scale of a DeiT parameter list: six multi-tile items with runs of one-tile ones between them, a one-tile item
    last"""
    if n == 1:
        return [(65, 63)]
    if n == 2:
        return [(130, 66), (1, 1)]
    shapes = []
    for i in range(n - 1):
        shapes.append(BIG[(i // 25) % len(BIG)] if i % 25 == 3 else SMALL[i % 3])
    return shapes + [(1, 64)]


TABLE_NS = (1, 2, 150)
TABLE_STEPS = 2
TABLE_BETAS = (0.9, 0.999)

# ------------------------------------------------------------------------------------------------------------------- FusedAdamW's parameters
FUSED_SHAPES = [(), (7,), (1, 5, 7), (6, 3, 4, 4), (65, 63)] * 2          # parameter i in group i % 8
FUSED_STEPS = 3
FUSED_BETAS = (0.9, 0.999)

# ------------------------------------------------------------------------------------------------------------------------ value edges
EDGE_SHAPES = [(65, 67), (64, 128)]            # one ragged scalar-path item, one vector-path item
EDGE_GROUPS = (0, 2)                           # each item under wd = 0.05 and under wd = 0
EDGE_STEPS = (1, 2, 1000, 200000)
EDGE_BETAS = ((0.9, 0.999), (0.9, 0.98))
EDGE_KINDS = ("g0_m0_v0", "g0", "g+1e-30", "g-1e-30", "g1e-30_m0_v0", "g1e20", "g1e21", "g+inf", "g-inf", "p-0", "p_subnormal",
              "v_subnormal", "v_subnormal_g0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def draw_p(shape, seed):
    return (0.5 * torch.randn(_numel(shape), generator=_gen(seed))).reshape(shape)


def draw_g(shape, seed):
    """Gaussian times 10^-5U: magnitudes from 1e-5 to 1 inside every item, so that eps matters beside sqrt(v) in some elements and not in
    others"""
    g = _gen(seed)
    n = _numel(shape)
    return (torch.randn(n, generator=g) * 10.0 ** (-5.0 * torch.rand(n, generator=g))).reshape(shape)


def seed_of(test, item, step=0):
    return {"tile": 100000, "table": 200000, "fused": 300000, "edge": 400000}[test] + 1000 * step + item


def edge_positions(kind, numel):
    """three flat positions per kind: near the start, in the middle and near the end (the first and the last element among them)"""
    k = EDGE_KINDS.index(kind)
    return [k, numel // 2 + k, numel - 1 - k]


@functools.lru_cache(maxsize=None)
def edge_item(i):
    """-> p, g, m, v (fp32 tensors) of value-edge item i with the kinds of EDGE_KINDS planted among Gaussian values"""
    shape = EDGE_SHAPES[i]
    n = _numel(shape)
    p, g = draw_p(shape, seed_of("edge", i)).flatten(), draw_g(shape, seed_of("edge", i, 1)).flatten()
    m = 0.3 * draw_g(shape, seed_of("edge", i, 2)).flatten()
    v = (draw_g(shape, seed_of("edge", i, 3)).flatten() ** 2) * 0.5
    for kind in EDGE_KINDS:
        for pos in edge_positions(kind, n):
            if kind in ("g0_m0_v0", "g1e-30_m0_v0"):
                m[pos], v[pos] = 0.0, 0.0
            if kind in ("g0_m0_v0", "g0", "v_subnormal_g0"):
                g[pos] = 0.0
            if kind in ("g+1e-30", "g1e-30_m0_v0"):
                g[pos] = 1e-30
            if kind == "g-1e-30":
                g[pos] = -1e-30
            if kind == "g1e20":
                g[pos] = 1e20                    # g^2 is beyond fp32; (1 - beta2) g^2 = 1e37 (2e38 with beta2 = 0.98) is not
            if kind == "g1e21":
                g[pos] = 1e21                    # (1 - beta2) g^2 = 1e39: exp_avg_sq becomes inf and the update 0
            if kind == "g+inf":
                g[pos] = float("inf")
            if kind == "g-inf":
                g[pos] = float("-inf")
            if kind == "p-0":
                p[pos] = -0.0
            if kind == "p_subnormal":
                p[pos] = 1e-40
            if kind in ("v_subnormal", "v_subnormal_g0"):
                v[pos] = 1e-40
    return tuple(t.reshape(shape) for t in (p, g, m, v))


# ------------------------------------------------------------------------------------------------------------------------------ arithmetic
def reference(p, g, m, v, lr, wd, betas, eps, step, fault=None):
    """-> p', exp_avg', exp_avg_sq', update: torch.optim.AdamW's documented step in float64.  fault: tests/test_adamw_ref.py"""
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    beta1, beta2 = betas if fault != "swap_betas" else betas[::-1]
    with np.errstate(all="ignore"):
        if fault == "l2":
            g = g + wd * p
        else:
            p = p * (1.0 - lr * wd)
        m1 = beta1 * m + (1.0 - beta1) * g
        v1 = beta2 * v + (1.0 - beta2) * g * g
        bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
        if fault == "bc2_no_sqrt":
            den = np.sqrt(v1) / bc2 + eps
        elif fault == "eps_in_sqrt":
            den = np.sqrt(v1 / bc2 + eps)
        else:
            den = np.sqrt(v1 / bc2) + eps
        u = lr * (m1 / bc1) / den
        p1 = p - u
        if fault == "twice":
            p1 = p1 - u
    return p1, m1, v1, u


def decayed(p, lr, wd):
    """fp32(p - lr * wd * p), the parameter of an element whose update is exactly 0"""
    p64 = np.asarray(p, dtype=np.float64)
    return (p64 - (lr * wd) * p64).astype(np.float32) if wd != 0.0 else np.asarray(p, dtype=np.float32)


def emulated(p, g, m, v, lr, wd, betas, eps, step):
    """-> p', exp_avg', exp_avg_sq' (fp32): the step with the roundings of csrc/tr_optim.hip's header comment -- decay, exp_avg and
    exp_avg_sq in double and rounded on the store; the step size lr / bc1 and the sum with eps in double, rounded to float; the rest in
    float; bc1 and bc2_sqrt formed in double and rounded to float"""
    f32, f64 = np.float32, np.float64
    p, g, m, v = (np.asarray(t, dtype=f32) for t in (p, g, m, v))
    beta1, beta2 = betas
    bc1, bc2_sqrt = f32(1.0 - beta1 ** step), f32(np.sqrt(1.0 - beta2 ** step))
    with np.errstate(all="ignore"):
        p1 = decayed(p, lr, wd)
        m1 = (beta1 * m.astype(f64) + (1.0 - beta1) * g.astype(f64)).astype(f32)
        v1 = (beta2 * v.astype(f64) + ((1.0 - beta2) * g.astype(f64)) * g.astype(f64)).astype(f32)
        step_size = f32(lr / f64(bc1))
        den = ((np.sqrt(v1) / bc2_sqrt).astype(f64) + eps).astype(f32)
        p1 = p1 - (step_size * m1) / den
    assert p1.dtype == f32 and m1.dtype == f32 and v1.dtype == f32 and den.dtype == f32
    return p1, m1, v1


def ulp32(x):
    """spacing of fp32 at |x| (x float64): 2^-149 below the smallest normal, the last binade's from the fp32 maximum on"""
    _, e = np.frexp(np.abs(x))
    e = np.where(x == 0, -200, e)
    return np.ldexp(1.0, np.clip(e - 1, -126, 127) - 23)


def _special(got, ref):
    """positions where the reference is NaN, infinite or rounds to an fp32 infinity -> (mask of them, mask of those that `got` misses)"""
    nan = np.isnan(ref)
    inf = ~nan & (np.abs(ref) >= F32_OVER)
    miss = (nan & ~np.isnan(got)) | (inf & ~(np.isinf(got) & (np.sign(got) == np.sign(ref))))
    return nan | inf, miss


def errors(got_p, got_m, got_v, p_in, ref, lr, wd):
    """-> {"p": worst metric, "m": ..., "v": ...} of one item (see the module docstring); inf where a NaN / inf position or a degenerate
    element misses"""
    ref_p, ref_m, ref_v, u = ref
    got_p, got_m, got_v = (np.asarray(t, dtype=np.float32).astype(np.float64).reshape(ref_p.shape) for t in (got_p, got_m, got_v))
    res = {}
    with np.errstate(all="ignore"):
        for name, got, want in (("m", got_m, ref_m), ("v", got_v, ref_v)):
            spec, miss = _special(got, want)
            err = np.where(spec, np.where(miss, np.inf, 0.0), np.abs(got - want) / ulp32(want))
            res[name] = float(np.max(np.where(np.isnan(err), np.inf, err)))
        v_over = np.isfinite(ref_v) & (np.abs(ref_v) >= F32_OVER) & np.isfinite(ref_m)
        degenerate = (u == 0.0) | v_over
        spec, miss = _special(got_p, np.where(degenerate, 0.0, ref_p))
        want_deg = decayed(p_in, lr, wd).astype(np.float64).reshape(ref_p.shape)
        deg_err = np.where(got_p.astype(np.float32).view(np.int32) == want_deg.astype(np.float32).view(np.int32), 0.0, np.inf)
        err = np.abs(got_p - ref_p) / (ulp32(ref_p) + np.abs(u) * 2.0 ** -23)
        err = np.where(degenerate, deg_err, np.where(spec, np.where(miss, np.inf, 0.0), err))
        res["p"] = float(np.max(np.where(np.isnan(err), np.inf, err)))
    return res


def bound(name):
    return MARGIN * MEASURED if name == "p" else MOMENT_ULPS


def check(what, got_p, got_m, got_v, p_in, g, m, v, lr, wd, betas, step, worst=None):
    """One item of one step against `reference`: asserts the three bounds; `worst` (a dict) collects the largest metric seen"""
    ref = reference(p_in, g, m, v, lr, wd, betas, EPS, step)
    res = errors(got_p, got_m, got_v, p_in, ref, lr, wd)
    for k, e in res.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), e)
        assert e <= bound(k), f"{what}: {k}' metric {e:.3f} > {bound(k):.3f}"
    return res


# ------------------------------------------------------------------------------------------------------------------ the measurement (CPU)
def _np(t):
    return t.numpy() if torch.is_tensor(t) else t


def chained(test, shapes, groups, steps, betas):
    """yields (step, item, group, p, g, m, v) of a test that starts from zero moments and steps `steps` times with fresh gradients, the
    state carried through `emulated` (the GPU tests carry the kernel's own state: another draw of the same rounding noise)"""
    state = [(draw_p(s, seed_of(test, i)).numpy(), np.zeros(s, np.float32), np.zeros(s, np.float32)) for i, s in enumerate(shapes)]
    for step in range(1, steps + 1):
        for i, s in enumerate(shapes):
            p, m, v = state[i]
            g = draw_g(s, seed_of(test, i, step)).numpy()
            yield step, i, groups[i], p, g, m, v
            state[i] = emulated(p, g, m, v, LRS[groups[i]], WDS[groups[i]], betas, EPS, step)


def tile_groups():
    return [GROUPS_USED[i % 4] for i in range(len(TILE_SPECS))]


def all_cases():
    """yields (name, group, betas, step, p, g, m, v) of every item of every launch of tests/test_hip_adamw_edges.py"""
    shapes = [(s.rows, s.cols) for s in TILE_SPECS]
    for step, i, grp, p, g, m, v in chained("tile", shapes, tile_groups(), TILE_STEPS, TILE_BETAS):
        yield f"tile step {step} item {i}", grp, TILE_BETAS, step, p, g, m, v
    shapes = table_shapes(150)
    for step, i, grp, p, g, m, v in chained("table", shapes, [GROUPS_USED[i % 4] for i in range(150)], TABLE_STEPS, TABLE_BETAS):
        yield f"table step {step} item {i}", grp, TABLE_BETAS, step, p, g, m, v
    for step, i, grp, p, g, m, v in chained("fused", FUSED_SHAPES, [i % 8 for i in range(len(FUSED_SHAPES))], FUSED_STEPS, FUSED_BETAS):
        yield f"fused step {step} item {i}", grp, FUSED_BETAS, step, p, g, m, v
    yield from edge_cases()


def edge_cases():
    for betas in EDGE_BETAS:
        for step in EDGE_STEPS:
            for i in range(len(EDGE_SHAPES)):
                for grp in EDGE_GROUPS:
                    yield (f"edge step {step} betas {betas} item {i} group {grp}", grp, betas, step) + tuple(_np(t) for t in edge_item(i))


def measure(cases=None):
    """-> worst {"p", "m", "v"} metric of `emulated` against `reference` and the case each was found in"""
    worst, where = {"p": 0.0, "m": 0.0, "v": 0.0}, {}
    for name, grp, betas, step, p, g, m, v in (all_cases() if cases is None else cases):
        lr, wd = LRS[grp], WDS[grp]
        res = errors(*emulated(p, g, m, v, lr, wd, betas, EPS, step), p, reference(p, g, m, v, lr, wd, betas, EPS, step), lr, wd)
        for k, e in res.items():
            if e > worst[k]:
                worst[k], where[k] = e, name
    return worst, where


FAULTS = ("l2", "bc2_no_sqrt", "eps_in_sqrt", "swap_betas", "other_lr", "twice")


def fault_visible(fault, grp, betas, step):
    """A fault that changes nothing in a case cannot be seen there: coupled decay without decay, and bc2 against its square root once
    both are 1 to within fp32 (beta2^step = 1.7e-9 at step 1000 with beta2 = 0.98 and 0 at step 200000; 0.37 at step 1000 with 0.999)"""
    if fault == "l2":
        return WDS[grp] != 0.0
    if fault == "bc2_no_sqrt":
        return betas[1] ** step > 2.0 ** -20
    return True


def fault_ratio(fault, grp, betas, step, p, g, m, v):
    """-> the largest of the three metrics of the faulty float64 step against the sound one, each over its bound"""
    lr, wd = LRS[grp], WDS[grp]
    bad = reference(p, g, m, v, LRS[(grp + 1) % 8] if fault == "other_lr" else lr, wd, betas, EPS, step, fault=fault)
    with np.errstate(all="ignore"):
        res = errors(*(t.astype(np.float32) for t in bad[:3]), p, reference(p, g, m, v, lr, wd, betas, EPS, step), lr, wd)
    return max(res[k] / bound(k) for k in res)


def _measure():
    worst, where = measure()
    for k in ("p", "m", "v"):
        print(f"{k}': emulated against reference, worst element {worst[k]:.4f} in {where[k]}" +
              (f"; committed MEASURED {MEASURED}, bound {MARGIN} x = {MARGIN * MEASURED:.2f}" if k == "p" else f"; bound {MOMENT_ULPS} ulp"))


if __name__ == "__main__":
    _measure()
