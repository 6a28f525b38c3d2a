"""CPU checks of the partial-sum reduces' order model (tests/_reduce_ref.py): it is a sum, and on the inputs of the GPU test the two block
layouts give different bits -- so a kernel that takes the wrong layout cannot pass there."""
import pytest
import torch

from tests import _reduce_ref as RR


@pytest.mark.parametrize("lanes", [RR.FLAT, RR.TALL])
@pytest.mark.parametrize("S,count", [(1, 5), (3, 8), (16, 7), (17, 64), (37, 1027), (63, 12), (64, 16), (65, 256), (200, 6), (512, 68)])
def test_order_model_is_the_sum(S, count, lanes):
    """Against float64: every element is a sum of at most S + 1 terms in some order, S additions, so |error| <= gamma_S sum |terms| with
    gamma_S = S u / (1 - S u) <= (S + 1) 2^-24 (Higham, any summation order).  S <= 2 leaves no order: equal to the sequential fp32 sum."""
    g = torch.Generator().manual_seed(100 * S + count + lanes)
    part, prior = torch.randn(S, count, generator=g), torch.randn(count, generator=g)
    for pf in (None, prior):
        got = RR.kernel_order_sum(part, pf, lanes)
        assert got.dtype == torch.float32 and got.shape == (count,)
        want = part.double().sum(0) + (0 if pf is None else pf.double())
        bound = (S + 1) * 2.0 ** -24 * (part.abs().sum(0) + (0 if pf is None else pf.abs())).double()
        assert bool(((got.double() - want).abs() <= bound).all())
    if S <= 2:
        seq = part[0] if S == 1 else part[0] + part[1]
        assert torch.equal(RR.kernel_order_sum(part, None, lanes), seq)


def test_lane_count_four_is_the_documented_order():
    """lanes = 4 written out: the order include/tokenreduction_hip.h documents for tr_reduce_partials_f32"""
    g = torch.Generator().manual_seed(7)
    p = torch.randn(37, 6, generator=g)
    lane = []
    for y in range(4):
        a = torch.zeros(6)
        a = a + ((p[y] + p[y + 4]) + (p[y + 8] + p[y + 12]))
        a = a + ((p[y + 16] + p[y + 20]) + (p[y + 24] + p[y + 28]))
        for s in range(y + 32, 37, 4):
            a = a + p[s]
        lane.append(a)
        t = torch.zeros(6)
        for s in range(y, 37, 4):
            t = t + p[s]
        lane.append(t)
    full, tail = ((lane[0] + lane[2]) + lane[4]) + lane[6], ((lane[1] + lane[3]) + lane[5]) + lane[7]
    assert torch.equal(RR.kernel_order_sum(p, None), torch.cat([full[:4], tail[4:]]))


@pytest.mark.parametrize("M,D", RR.LN_REDUCE_SHAPES)
def test_layouts_differ_on_the_layernorm_cases(M, D):
    """The GPU test's inputs (their fp32 restatement): at every S >= 64 the 64 x 4 and the 16 x 16 order differ in at least one element of
    d_gamma | d_beta.  Below 64 the call site takes the flat layout whatever D is."""
    S = RR.ln_grid(M)
    assert RR.layout_lanes(S, D) == (RR.TALL if S >= 64 else RR.FLAT)
    pg, pb = RR.ln_partials_model(M, D)
    assert pg.shape == (S, D) and pb.shape == (S, D)
    both = torch.cat([pg, pb], dim=1)
    differ = int((RR.kernel_order_sum(both, None, RR.FLAT) != RR.kernel_order_sum(both, None, RR.TALL)).sum())
    print(f"M={M} D={D} S={S}: {differ} of {2 * D} sums differ between the layouts")
    if S >= 64:
        assert differ >= 1
