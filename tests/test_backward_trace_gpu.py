"""The backward executor (csrc/tr_train.hip) enqueues the launches it enqueued at the commit tests/golden/backward_trace.json was recorded
from -- the same kernels with the same shapes (label, FLOPs, bytes of every launch) in the same order -- and writes the same gradient bits:
every family, whole-model and block-range calls, the input gradient, accumulation, the frozen forms, the headless and the pooled head
(tests/_backward_trace.py).  Exact on both counts.  The workspace is NaN-filled before every recorded backward, so a lost memset changes
the bits.  A block-range backward must also give the bits of the single call.  The weight-gradient group's plan depends on the device's
compute-unit count, so the fixture names the device it was recorded on and the test asserts (does not skip) that this is one."""
import json
import os

import pytest
import torch

from tests import _backward_trace as bt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    with open(os.path.join(golden_dir, "backward_trace.json")) as f:
        return json.load(f)


def test_the_fixture_was_recorded_on_this_kind_of_device(fixture):
    want = {k: fixture["header"][k] for k in ("device", "compute_units")}
    assert bt.device_header() == want


def test_the_fixture_holds_every_case(fixture):
    assert sorted(fixture["cases"]) == sorted(bt.CASES)
    lost = [n for n, c in fixture["cases"].items() if c["hash"] is None]
    assert len(lost) <= 2 and not set(lost) & set(bt.MUST_HASH), lost
    assert fixture["header"]["zero_workspace"] == sorted(bt.ZERO_WS)
    assert len(bt.ZERO_WS) <= 2 and not set(bt.ZERO_WS) & set(bt.MUST_HASH)


@pytest.mark.parametrize("name", list(bt.CASES))
def test_same_launches_same_bits(fixture, name):
    want = fixture["cases"][name]
    launches, digest = bt.run_case(name)
    got = [list(rec) for rec in launches]
    exp = [fixture["records"][i] for i in want["launches"]]
    first = next((i for i, (g, e) in enumerate(zip(got, exp)) if g != e), min(len(got), len(exp)))
    assert got == exp, f"{len(got)} launches, recorded {len(exp)}; first difference at launch {first}: {got[first:first + 3]} != {exp[first:first + 3]}"
    if want["hash"] is not None:          # (null: the gradients did not reproduce at the recorded commit itself)
        assert digest == want["hash"]
    one = bt.single_call(name)
    if one is not None and fixture["cases"][one]["hash"] is not None:          # block ranges: the single call's bits
        assert digest == fixture["cases"][one]["hash"], f"not the bits of {one}"
