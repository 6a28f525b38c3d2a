"""The executor against the reference's own vectors at 448 x 448 and 512 x 512 inputs (tests/golden/gen_golden_hires.py), in all three
precisions, with the checks and tolerances the 224 / 384 fixtures are held to:
  fp32    test_hip_fp32.py   -- Top-K / EViT / DyViT indices, complements, ToMe and cluster assignment maps exact; logits within 2e-4
  bf16x3  test_hip_split.py  -- the reference's token sets, logits within 1e-3, free-running
  bf16    test_hip_model.py  -- selections exact on the device's own scores, teacher-forced relative L2
Centre counts reach 921 (Sinkhorn, DPC-KNN, K-Medoids at keep_rate 0.9, 512 x 512)."""
import pytest

from tests import _params, test_hip_fp32, test_hip_model, test_hip_split
from tests._hires_params import BF16_PARITY_224_ONLY, BF16X3_NEAR_TIE, HIRES_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("name", list(HIRES_CASES))
def test_fp32_executor_matches_reference(golden_dir, name, monkeypatch):
    monkeypatch.setitem(_params.GOLDEN_CASES, name, HIRES_CASES[name])
    test_hip_fp32.test_model_fp32_matches_reference_golden(golden_dir, name)


@pytest.mark.parametrize("name", [n for n in HIRES_CASES if n not in BF16X3_NEAR_TIE])
def test_bf16x3_executor_matches_reference(golden_dir, name, monkeypatch):
    monkeypatch.setitem(_params.GOLDEN_CASES, name, HIRES_CASES[name])
    test_hip_split.test_model_bf16x3_free_running_against_reference_golden(golden_dir, name)


@pytest.mark.parametrize("name", [n for n in HIRES_CASES if n not in BF16_PARITY_224_ONLY])
def test_bf16_executor_parity(golden_dir, name, monkeypatch):
    monkeypatch.setitem(_params.GOLDEN_CASES, name, HIRES_CASES[name])
    test_hip_model.test_model_parity(golden_dir, name)
