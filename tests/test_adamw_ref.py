"""The float64 AdamW reference of tests/_adamw_ref.py, its metrics and its committed measurement (no GPU): the reference against an
unfused float64 torch.optim.AdamW, the committed rounding noise against what the measurement gives now, and six planted faults that the
bounds of tests/test_hip_adamw_edges.py must catch with a factor of ten to spare on that test's own inputs.  This proves the reference and
the bounds before the GPU test compares the kernel with them."""
import numpy as np
import pytest
import torch

from tests import _adamw_ref as R


@pytest.fixture(scope="module")
def cases():
    return list(R.all_cases())


def test_committed_measurement_holds(cases):
    worst, where = R.measure(cases)
    print(f"p': measured {worst['p']:.4f} in {where['p']}, committed {R.MEASURED}; m' {worst['m']:.4f} ulp, v' {worst['v']:.4f} ulp")
    assert worst["p"] <= R.MEASURED, f"the measurement gives {worst['p']:.4f}, more than the committed {R.MEASURED}"
    assert R.MEASURED <= 1.02 * worst["p"], f"the committed {R.MEASURED} is more than the rounded-up measurement {worst['p']:.4f}"
    # one rounding of a double expression: half an ulp, which is what the derived 1-ulp moment bound rests on
    assert worst["m"] <= 0.5 + 1e-6 and worst["v"] <= 0.5 + 1e-6
    assert R.MARGIN == 2.0 and R.MOMENT_ULPS == 1.0


@pytest.mark.parametrize("betas,wd,lr", [((0.9, 0.999), 0.05, 1e-3), ((0.9, 0.98), 0.0, 3e-3), ((0.8, 0.95), 0.3, 2e-2)])
def test_reference_is_torchs_unfused_float64_adamw(betas, wd, lr):
    """five steps from zero moments with fresh gradients; p, exp_avg and exp_avg_sq to 1e-12 relative, element by element.  Relative to the
    larger of the element and the terms it was summed from: torch forms exp_avg as a lerp, and where beta1 m and (1 - beta1) g cancel, the
    two forms' 1e-16 lies 1e4 times higher against the small result"""
    shape = (37, 29)
    p = torch.nn.Parameter(R.draw_p(shape, 1).double())
    opt = torch.optim.AdamW([p], lr=lr, betas=betas, eps=R.EPS, weight_decay=wd, foreach=False, fused=False)
    mine = (p.detach().numpy().copy(), np.zeros(shape), np.zeros(shape))
    for step in range(1, 6):
        g = R.draw_g(shape, 10 + step).double()
        p.grad = g.clone()
        opt.step()
        before = mine
        mine = R.reference(mine[0], g.numpy(), mine[1], mine[2], lr, wd, betas, R.EPS, step)
        scales = (np.maximum(np.abs(before[0]), np.abs(mine[3])), np.maximum(np.abs(before[1]), np.abs(g.numpy())), 0.0)
        for name, got, want, scale in zip(("p", "exp_avg", "exp_avg_sq"), mine, (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]), scales):
            want = want.numpy()
            assert got.dtype == np.float64 and want.dtype == np.float64
            rel = np.abs(got - want) / np.maximum(np.abs(want), scale)
            assert float(rel.max()) <= 1e-12, f"step {step}: {name} differs by {rel.max():.1e}"
        mine = mine[:3]


def test_update_is_what_reference_returns():
    p, g, m, v = (t.numpy() for t in R.edge_item(1))
    keep = np.isfinite(g)
    p1, m1, v1, u = R.reference(p, g, m, v, 1e-3, 0.0, (0.9, 0.999), R.EPS, 7)
    assert np.array_equal((p.astype(np.float64) - u)[keep], p1[keep]) and bool(np.isnan(p1[~keep]).all())


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_exceed_the_bounds_tenfold(fault, cases):
    """per launch of the GPU tests (one step of one test, or one step count and beta pair of the value-edge test): the worst element of
    the faulty float64 step lies at least ten bounds from the sound one, wherever the fault changes the arithmetic at all"""
    launches = {}
    for name, grp, betas, step, p, g, m, v in cases:
        key = name.split(" item ")[0]
        if R.fault_visible(fault, grp, betas, step):
            launches[key] = max(launches.get(key, 0.0), R.fault_ratio(fault, grp, betas, step, p, g, m, v))
    assert len(launches) >= R.TILE_STEPS + R.TABLE_STEPS + R.FUSED_STEPS + 4
    for key, ratio in launches.items():
        print(f"{fault} in {key}: {ratio:.3g} x the bound")
        assert ratio >= 10.0, (fault, key, ratio)


def test_special_positions_and_degenerate_elements_are_held():
    """`errors` on the value-edge items: the sound emulation passes; a finite value at an inf / NaN position, a NaN elsewhere, an update
    applied to a degenerate element and a decay left out of one are each an infinite error"""
    lr, wd, betas, step = R.LRS[0], R.WDS[0], (0.9, 0.999), 2
    p, g, m, v = (t.numpy() for t in R.edge_item(0))
    ref = R.reference(p, g, m, v, lr, wd, betas, R.EPS, step)
    good = R.emulated(p, g, m, v, lr, wd, betas, R.EPS, step)
    res = R.errors(*good, p, ref, lr, wd)
    assert res["p"] <= R.MEASURED and res["m"] <= 0.5 and res["v"] <= 0.5
    n = p.size
    pos = {k: R.edge_positions(k, n)[0] for k in R.EDGE_KINDS}
    assert np.isnan(good[0].flat[pos["g+inf"]]) and np.isinf(good[2].flat[pos["g1e21"]]) and np.isfinite(good[2].flat[pos["g1e20"]])
    assert good[0].flat[pos["g1e21"]] == R.decayed(p, lr, wd).flat[pos["g1e21"]] and ref[3].flat[pos["g0_m0_v0"]] == 0.0

    def broken(which, at, value):
        out = [t.copy() for t in good]
        out[which].flat[at] = value
        return R.errors(*out, p, ref, lr, wd)

    assert broken(0, pos["g+inf"], 1.0)["p"] == np.inf and broken(1, pos["g-inf"], np.inf)["m"] == np.inf
    assert broken(2, pos["g1e21"], R.F32_MAX)["v"] == np.inf and broken(0, 100, np.nan)["p"] == np.inf
    assert broken(0, pos["g0_m0_v0"], np.nextafter(good[0].flat[pos["g0_m0_v0"]], np.float32(9)))["p"] == np.inf
    assert broken(0, pos["g0_m0_v0"], p.flat[pos["g0_m0_v0"]])["p"] == np.inf          # the decay left out
    assert broken(0, pos["g1e21"], good[0].flat[pos["g1e21"]] - np.float32(1e-3))["p"] == np.inf


def test_inputs_reach_what_the_gpu_test_claims():
    specs = R.TILE_SPECS
    assert {s.rows for s in specs} | {s.cols for s in specs} >= {1, 63, 64, 65, 130, 384, 1000, 1536, 4099}
    assert all(s.rows * s.cols <= 1000 * 1000 for s in specs) and (specs[-1].rows, specs[-1].cols) == (1, 1)
    for field in ("po", "go", "mo", "vo"):          # each fp32 operand misaligned ALONE on an item the vector path would otherwise take
        assert any(getattr(s, field) == 1 and sum((s.po, s.go, s.mo, s.vo, s.do)) == 1 and s.cols % 4 == 0 for s in specs), field
    assert any(s.do == 1 for s in specs) and any(s.do == 2 for s in specs) and any(s.to == 1 for s in specs) and any(s.to == 2 for s in specs)
    scalar = [s for s in specs if s.cols % 4 or s.po or s.go or s.mo or s.vo or s.do]
    assert any(s.dst and not s.dst_t for s in scalar) and any(s.dst_t and not s.dst for s in scalar) and any(not s.dst and not s.dst_t for s in specs)
    groups = R.tile_groups()
    assert set(groups) == set(R.GROUPS_USED) and 7 in groups and len({R.LRS[g] for g in groups}) == 4 and len(set(R.LRS)) == 8
    assert [R.WDS[g] == 0.0 for g in R.GROUPS_USED].count(True) == 1
    big = R.table_shapes(150)
    tiles = [((r + 63) // 64) * ((c + 63) // 64) for r, c in big]
    assert len(big) == 150 and tiles[-1] == 1 and sum(t > 1 for t in tiles) >= 5 and sum(t == 1 for t in tiles) >= 140
    assert len(R.table_shapes(1)) == 1 and len(R.table_shapes(2)) == 2
    for i, shape in enumerate(R.EDGE_SHAPES):
        p, g, m, v = R.edge_item(i)
        assert int(torch.isinf(g).sum()) == 6 and int((g == 0).sum()) == 9 and int((v == 1e-40).sum()) == 6 and bool((v >= 0).all())
        assert int(((p == 0) & torch.signbit(p)).sum()) == 3 and int((p == 1e-40).sum()) == 3
        flat = [q for k in R.EDGE_KINDS for q in R.edge_positions(k, p.numel())]
        assert len(set(flat)) == len(flat) and 0 in flat and p.numel() - 1 in flat
