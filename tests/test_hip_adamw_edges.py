"""GPU tests of the one-launch AdamW step (csrc/tr_optim.hip: adamw_pack_kernel) at the op boundary, through ops.adamw_step and
optim.FusedAdamW without a model: every tile, alignment and store path, the item table's search, and the value range.

Two oracles.  (a) torch.optim.AdamW(fused=True) on the GPU, on clones of the same tensors: p, exp_avg and exp_avg_sq compared as bits
(NaN against NaN by position).  (b) the float64 AdamW of tests/_adamw_ref.py, every element within that module's bounds: 1 fp32 ulp for
the moments, MARGIN x MEASURED on the parameter metric, inf / NaN by position, a zero update bit-exact (tests/test_adamw_ref.py proves
the reference and that the bounds catch six planted faults tenfold).  Every test prints its worst element's metrics beside the bounds.
The inputs (shapes, offsets, groups, seeds, planted values) live in tests/_adamw_ref.py, where the CPU measurement walks the same ones."""
import numpy as np
import pytest
import torch

from tests import _adamw_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
GUARD = 64                   # elements: 256 B of fp32, 128 B of bf16 -- a front guard keeps the alignment of what follows it


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd import ops as _ops
    return _ops


def _guarded(shape, dtype, off_elems):
    """A view `off_elems` elements behind the front guard of a sentinel-filled device buffer, with guard space behind it as well."""
    n = shape[0] * shape[1]
    buf = torch.full((GUARD + off_elems + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    view = buf[GUARD + off_elems:GUARD + off_elems + n].view(shape)
    assert view.data_ptr() % 16 == (off_elems * buf.element_size()) % 16
    return buf, view


def _guards_intact(buf, off_elems, n):
    b = buf.cpu()
    sent = torch.tensor(SENTINEL, dtype=buf.dtype)
    return bool((b[:GUARD + off_elems] == sent).all()) and bool((b[GUARD + off_elems + n:] == sent).all())


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same_bits(a, b):
    """bit equality; a NaN equals a NaN (its payload is nobody's contract), an infinity only the same infinity"""
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = a.isnan(), b.isnan()
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


class _Item:
    """p, g, exp_avg, exp_avg_sq and the two bf16 copies of one table entry, each a guarded view at its own offset"""

    def __init__(self, shape, group, dst=True, dst_t=True, po=0, go=0, mo=0, vo=0, do=0, to=0):
        self.shape, self.group, self.n = shape, group, shape[0] * shape[1]
        self.offs = dict(p=po, g=go, m=mo, v=vo, dst=do, dst_t=to)
        self.bufs, self.t = {}, {}
        for k in ("p", "g", "m", "v"):
            self.bufs[k], self.t[k] = _guarded(shape, torch.float32, self.offs[k])
        self.bufs["dst"], self.t["dst"] = _guarded(shape, torch.bfloat16, do) if dst else (None, None)
        self.bufs["dst_t"], self.t["dst_t"] = _guarded(shape[::-1], torch.bfloat16, to) if dst_t else (None, None)

    def set(self, **values):
        for k, val in values.items():
            self.t[k].copy_(val.reshape(self.shape))

    def entry(self):
        return tuple(self.t[k] for k in ("p", "g", "m", "v", "dst", "dst_t")) + (self.group,)

    def cpu(self):
        return {k: self.t[k].cpu() for k in ("p", "g", "m", "v")}

    def check_guards(self, what):
        for k, buf in self.bufs.items():
            if buf is not None:
                assert _guards_intact(buf, self.offs[k], self.n), f"{what}: elements around {k} were written"

    def check_copies(self, what):
        """dst = RNE bf16 of the new p, dst_t its transpose, both as bits"""
        want = self.t["p"].cpu().bfloat16()
        if self.t["dst"] is not None:
            assert _same_bits(self.t["dst"], want), f"{what}: dst is not the bf16 rounding of the new p"
        if self.t["dst_t"] is not None:
            assert _same_bits(self.t["dst_t"], want.t().contiguous()), f"{what}: dst_t is not the transposed bf16 rounding of the new p"


def _torch_opt(ps, groups, betas):
    """oracle (a): one nn.Parameter per item on clones, one parameter group per group index with its lr / weight decay"""
    params = [torch.nn.Parameter(p.detach().clone().cuda()) for p in ps]
    by = {}
    for prm, grp in zip(params, groups):
        by.setdefault(grp, []).append(prm)
    opt = torch.optim.AdamW([dict(params=v, lr=R.LRS[g], weight_decay=R.WDS[g]) for g, v in sorted(by.items())], betas=betas, eps=R.EPS, fused=True)
    return params, opt


def _check_against_both(what, got, before, g, prm, opt, group, betas, step, worst):
    """one item after one step: bits of oracle (a), bounds of oracle (b); `got` / `before` dicts of CPU tensors"""
    st = opt.state[prm]
    for k, want in (("p", prm), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
        assert _same_bits(got[k], want.detach().reshape(got[k].shape)), \
            f"{what}: {k} differs from torch's fused AdamW in {int((_bits(got[k]) != _bits(want.detach().reshape(got[k].shape))).sum())} elements"
    R.check(what, got["p"].numpy(), got["m"].numpy(), got["v"].numpy(), before["p"].numpy(), g.numpy(), before["m"].numpy(), before["v"].numpy(),
            R.LRS[group], R.WDS[group], betas, step, worst)


def _report(what, worst):
    print(f"{what}: worst element p' {worst.get('p', 0.0):.3f} (bound {R.bound('p'):.2f} = {R.MARGIN} x {R.MEASURED}), "
          f"exp_avg' {worst.get('m', 0.0):.3f} ulp, exp_avg_sq' {worst.get('v', 0.0):.3f} ulp (bound {R.bound('m'):.0f})")


def _run_from_zero(ops, test, items, betas, steps, zero_grads):
    """`steps` launches from zero moments with fresh gradients, every item checked after every step"""
    groups = [it.group for it in items]
    for i, it in enumerate(items):
        it.set(p=R.draw_p(it.shape, R.seed_of(test, i)).cuda(), m=torch.zeros(it.shape).cuda(), v=torch.zeros(it.shape).cuda())
    params, opt = _torch_opt([it.t["p"] for it in items], groups, betas)
    worst = {}
    for step in range(1, steps + 1):
        grads = [R.draw_g(it.shape, R.seed_of(test, i, step)) for i, it in enumerate(items)]
        for it, prm, g in zip(items, params, grads):
            it.set(g=g.cuda())
            prm.grad = g.clone().cuda()
        before = [it.cpu() for it in items]
        ops.adamw_step([it.entry() for it in items], R.LRS, R.WDS, betas, R.EPS, step, zero_grads=zero_grads)
        opt.step()
        for i, (it, prm, g, bef) in enumerate(zip(items, params, grads, before)):
            what = f"{test} step {step} item {i} {it.shape} group {it.group}"
            got = it.cpu()
            _check_against_both(what, got, bef, g, prm, opt, it.group, betas, step, worst)
            if zero_grads:
                assert torch.equal(_bits(got["g"]), torch.zeros(it.shape, dtype=torch.int32)), f"{what}: the gradient is not all +0.0"
            else:
                assert torch.equal(_bits(got["g"]), _bits(g)), f"{what}: the gradient changed"
            it.check_copies(what)
            it.check_guards(what)
    _report(f"{test} zero_grads={zero_grads} {len(items)} items", worst)


@pytest.mark.parametrize("zero_grads", [False, True])
def test_tiles_paths_and_alignment(ops, zero_grads):
    """All of _adamw_ref.TILE_SPECS in one launch, three consecutive steps, four groups {0, 2, 5, 7} with distinct lr (item i in group
    GROUPS_USED[i % 4]; group 2 has wd = 0, so decayed and undecayed items alternate inside the launch).  Which item reaches what:
      scalar elements by cols % 4 != 0: 4, 5, 7, 8, 11, 12, 26 (66 = 64 + 2: c + e < cols inside a 4-column group), 27 (4099), 28;
        by p / g / m / v 4 bytes off, each alone: 14, 15, 16, 17; all four 8 bytes off: 18; by dst 2 / 4 bytes off: 19, 21, 23;
      ragged last row tile: 0, 2 (vector path), 4, 24 (65 rows), 23 (1000 rows); ragged last column tile: 1, 2, 25 (vector), 4, 5, 26, 27;
      scalar transposed store by rows % 4 != 0: 4, 5, 6, 8, 12, 24 (vector elements, scalar dst_t); by dst_t 2 / 4 bytes off: 20, 22, 23;
      dst without dst_t: 9 (vector), 11, 27 (scalar); dst_t without dst: 10 (vector), 12 (scalar); neither: 13, 28;
      ZERO on the scalar path: every scalar item above, in the zero_grads case;
      groups beyond the second: 5 and 7; wd == 0 beside decayed items: group 2;
      (1, 4099): item 27, 65 column tiles, 3 columns in the last; (1, 1): items 8 and 28, 28 the table's last.
    After every step, per item: p, exp_avg, exp_avg_sq against both oracles; g bit-unchanged or all +0.0; dst / dst_t bitwise the
    (transposed) RNE bf16 of the new p; the guard elements before and after each of the six buffers untouched."""
    items = [_Item((s.rows, s.cols), grp, s.dst, s.dst_t, s.po, s.go, s.mo, s.vo, s.do, s.to) for s, grp in zip(R.TILE_SPECS, R.tile_groups())]
    _run_from_zero(ops, "tile", items, R.TILE_BETAS, R.TILE_STEPS, zero_grads)


@pytest.mark.parametrize("n", R.TABLE_NS)
def test_item_table(ops, n):
    """The binary search over `first`: one item, two items, and 150 items -- one-tile items (1, 64), (1, 1), (64, 64) in runs of 24
    between six multi-tile ones (up to 65 tiles), a one-tile item last.  Two steps; the bitwise match with torch's fused AdamW on every
    item after each shows a tile that was skipped, given to a neighbour or visited twice.  Every third item carries dst, every fifth
    dst_t."""
    shapes = R.table_shapes(n)
    items = [_Item(s, R.GROUPS_USED[i % 4], dst=i % 3 == 0, dst_t=i % 5 == 0) for i, s in enumerate(shapes)]
    _run_from_zero(ops, "table", items, R.TABLE_BETAS, R.TABLE_STEPS, zero_grads=False)


@pytest.mark.parametrize("betas", R.EDGE_BETAS)
@pytest.mark.parametrize("step", R.EDGE_STEPS)
def test_value_edges(ops, step, betas):
    """_adamw_ref.edge_item: a ragged scalar-path item (65, 67) and a vector-path item (64, 128), each under wd = 0.05 (group 0) and
    wd = 0 (group 2) in one launch, with these planted at three positions each (the first and the last element among them) among
    Gaussian values: g = 0 with zero moments; g = 0 with moments; g = +-1e-30 (g^2 underflows); g = 1e-30 with zero moments; g = 1e20 --
    g^2 is beyond fp32 but (1 - beta2) g^2 is 1e37 / 2e38, so exp_avg_sq stays finite; g = 1e21, added for what that case was meant to
    reach: exp_avg_sq becomes inf and the update exactly 0; g = +-inf (exp_avg inf, exp_avg_sq inf, p NaN); p = -0.0; p and v subnormal,
    v also with g = 0.  The moments are set in place (torch: after a priming step, state["step"].fill_(step - 1)).  At step 200000 both
    bias corrections round to 1.  Held to both oracles on every element, the bf16 copies included."""
    entries = [(i, grp) for i in range(len(R.EDGE_SHAPES)) for grp in R.EDGE_GROUPS]
    items = [_Item(R.EDGE_SHAPES[i], grp) for i, grp in entries]
    for it, (i, _) in zip(items, entries):
        p, g, m, v = R.edge_item(i)
        it.set(p=p.cuda(), g=g.cuda(), m=m.cuda(), v=v.cuda())
    params, opt = _torch_opt([it.t["p"] for it in items], [it.group for it in items], betas)
    for prm in params:
        prm.grad = torch.zeros_like(prm)
    opt.step()                                   # priming step: creates the state
    with torch.no_grad():
        for prm, it in zip(params, items):
            st = opt.state[prm]
            prm.copy_(it.t["p"])
            st["exp_avg"].copy_(it.t["m"])
            st["exp_avg_sq"].copy_(it.t["v"])
            st["step"].fill_(step - 1)
            prm.grad = it.t["g"].clone()
    before = [it.cpu() for it in items]
    ops.adamw_step([it.entry() for it in items], R.LRS, R.WDS, betas, R.EPS, step)
    opt.step()
    worst = {}
    for it, prm, bef, (i, _) in zip(items, params, before, entries):
        what = f"value edges step {step} betas {betas} item {it.shape} group {it.group}"
        got = it.cpu()
        assert float(opt.state[prm]["step"]) == step
        _check_against_both(what, got, bef, bef["g"], prm, opt, it.group, betas, step, worst)
        flat = got["p"].flatten()
        n = flat.numel()
        assert all(bool(flat[q].isnan()) for k in ("g+inf", "g-inf") for q in R.edge_positions(k, n)) and int(flat.isnan().sum()) == 6
        assert all(bool(got["v"].flatten()[q].isinf()) for q in R.edge_positions("g1e21", n)) and int(got["v"].isinf().sum()) == 9
        assert torch.equal(_bits(got["g"]), _bits(bef["g"])), f"{what}: the gradient changed"
        it.check_copies(what)
        it.check_guards(what)
    _report(f"value edges step {step} betas {betas}", worst)


def _fused_params():
    return [torch.nn.Parameter(R.draw_p(s, R.seed_of("fused", i)).cuda()) for i, s in enumerate(R.FUSED_SHAPES)]


def _fused_groups(params, n_groups=8):
    return [dict(params=[p for i, p in enumerate(params) if i % 8 == g], lr=R.LRS[g % 8], weight_decay=R.WDS[g % 8]) for g in range(n_groups)]


@pytest.mark.parametrize("zero_grads", [False, True])
def test_fused_adamw_without_a_model(zero_grads):
    """optim.FusedAdamW on bare parameters of shape (), (7,), (1, 5, 7), (6, 3, 4, 4), (65, 63), two of each over eight groups
    (parameter i in group i % 8), three steps against both oracles; zero_grads=True leaves every gradient at +0.0."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd.optim import FusedAdamW
    mine, theirs = _fused_params(), _fused_params()
    opt = FusedAdamW(_fused_groups(mine), betas=R.FUSED_BETAS, eps=R.EPS, zero_grads=zero_grads)
    ref = torch.optim.AdamW(_fused_groups(theirs), betas=R.FUSED_BETAS, eps=R.EPS, fused=True)
    worst = {}
    for step in range(1, R.FUSED_STEPS + 1):
        grads = [R.draw_g(s, R.seed_of("fused", i, step)) for i, s in enumerate(R.FUSED_SHAPES)]
        before = []
        for p, q, g in zip(mine, theirs, grads):
            p.grad, q.grad = g.clone().cuda(), g.clone().cuda()
            st = opt.state.get(p, {})
            before.append(dict(p=p.detach().cpu(), m=st["exp_avg"].cpu() if "exp_avg" in st else torch.zeros_like(g),
                               v=st["exp_avg_sq"].cpu() if "exp_avg_sq" in st else torch.zeros_like(g)))
        opt.step()
        ref.step()
        for i, (p, q, g, bef) in enumerate(zip(mine, theirs, grads, before)):
            what = f"FusedAdamW step {step} parameter {i} {tuple(p.shape)} group {i % 8}"
            got = dict(p=p.detach().cpu(), m=opt.state[p]["exp_avg"].cpu(), v=opt.state[p]["exp_avg_sq"].cpu())
            assert got["m"].shape == p.shape and opt.state[p]["step"] == step
            _check_against_both(what, got, bef, g, q, ref, i % 8, R.FUSED_BETAS, step, worst)
            if zero_grads:
                assert torch.equal(_bits(p.grad), torch.zeros(p.shape, dtype=torch.int32)), f"{what}: the gradient is not all +0.0"
            else:
                assert torch.equal(_bits(p.grad), _bits(g)), f"{what}: the gradient changed"
    _report(f"FusedAdamW zero_grads={zero_grads}", worst)


def test_fused_adamw_refuses_what_it_cannot_step():
    """a ninth parameter group raises; a parameter without a gradient in one step makes the NEXT step, where it has one again, raise the
    documented "step counts differ" error -- and neither refusal has touched a parameter"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tokenreduction_amd.optim import FusedAdamW
    params = _fused_params()
    for p in params:
        p.grad = torch.ones_like(p)
    nine = [dict(params=[p]) for p in params[:9]]
    start = [p.detach().clone() for p in params]
    with pytest.raises(NotImplementedError, match="at most 8 parameter groups"):
        FusedAdamW(nine).step()
    assert all(torch.equal(p.detach(), s) for p, s in zip(params, start))

    opt = FusedAdamW(_fused_groups(params), betas=R.FUSED_BETAS, eps=R.EPS)
    opt.step()
    params[4].grad = None                         # (65, 63) sits out one step
    opt.step()
    assert opt.state[params[4]]["step"] == 1 and opt.state[params[3]]["step"] == 2
    for p in params:
        p.grad = torch.ones_like(p)
    held = [p.detach().clone() for p in params]
    with pytest.raises(NotImplementedError, match="step counts differ"):
        opt.step()
    assert all(torch.equal(p.detach(), s) for p, s in zip(params, held))
    assert opt.state[params[4]]["step"] == 1 and opt.state[params[3]]["step"] == 2
