"""Pin the oracle against the reference's own vectors at 448 x 448 and 512 x 512 inputs (tests/golden/gen_golden_hires.py, case table
tests/_hires_params.py), with the checks and tolerances of test_oracle_golden.py.  CPU only."""
import pytest

from tests import _params, test_oracle_golden
from tests._hires_params import HIRES_CASES, ORACLE_NEAR_TIE


@pytest.mark.parametrize("name", [n for n in HIRES_CASES if n not in ORACLE_NEAR_TIE])
def test_oracle_matches_reference_at_high_resolution(golden_dir, name, monkeypatch):
    monkeypatch.setitem(_params.GOLDEN_CASES, name, HIRES_CASES[name])
    test_oracle_golden.test_model_matches_reference(golden_dir, name)
