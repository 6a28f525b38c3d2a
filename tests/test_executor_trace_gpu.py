"""The forward executor (csrc/tr_vit.hip) enqueues the launches it enqueued at the commit tests/golden/executor_trace.json was recorded
from -- the same kernels with the same shapes (label, FLOPs, bytes of every launch) in the same order -- and writes the same bits:
every family, precision, eval and training form of tests/_executor_trace.py.  Exact on both counts.  The fused-Mlp schedule depends on
the device's compute-unit count, so the fixture names the device it was recorded on and the test asserts (does not skip) that this is one."""
import json
import os

import pytest
import torch

from tests import _executor_trace as et

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    with open(os.path.join(golden_dir, "executor_trace.json")) as f:
        return json.load(f)


def test_the_fixture_was_recorded_on_this_kind_of_device(fixture):
    want = {k: fixture["header"][k] for k in ("device", "compute_units")}
    assert et.device_header() == want


def test_the_fixture_holds_every_case(fixture):
    assert sorted(fixture["cases"]) == sorted(et.CASES)
    lost = [n for n, c in fixture["cases"].items() if c["hash"] is None]
    assert len(lost) <= 2 and not set(lost) & set(et.MUST_HASH), lost


@pytest.mark.parametrize("name", list(et.CASES))
def test_same_launches_same_bits(fixture, name):
    want = fixture["cases"][name]
    launches, digest = et.run_case(name)
    got = [list(rec) for rec in launches]
    exp = [fixture["records"][i] for i in want["launches"]]
    first = next((i for i, (g, e) in enumerate(zip(got, exp)) if g != e), min(len(got), len(exp)))
    assert got == exp, f"{len(got)} launches, recorded {len(exp)}; first difference at launch {first}: {got[first:first + 3]} != {exp[first:first + 3]}"
    if want["hash"] is not None:          # (null: the outputs did not reproduce at the recorded commit itself)
        assert digest == want["hash"]
