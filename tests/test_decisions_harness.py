"""harness.validate(..., stage_records=True), GPU tier: the dictionary of a viz_mode run, key by key, from the decision taps of the fast-path
forward -- over a loader of three batches whose last one is short -- and validate's defaults untouched."""
import numpy as np
import pytest
import torch

from tests._params import GOLDEN_CASES, make_images
from tests.test_decisions_gpu import _model_name, _prepared

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _loader(name, n=8, bs=3):
    case = GOLDEN_CASES[name]
    imgs = make_images(n, 224, case["xseed"] + 5)
    target = torch.arange(n) % case["num_classes"]
    return [(imgs[i: i + bs], target[i: i + bs]) for i in range(0, n, bs)], [f"img_{i}.JPEG" for i in range(n)]


def _equal_dicts(got, want, path=""):
    assert type(got) is type(want) or (np.isscalar(got) and np.isscalar(want)), path
    if isinstance(want, dict):
        assert list(got) == list(want), path
        for key in want:
            _equal_dicts(got[key], want[key], f"{path}/{key}")
    elif isinstance(want, np.ndarray):
        assert got.shape == want.shape, path
        np.testing.assert_array_equal(got, want, err_msg=path)
    else:
        assert got == want, path


@pytest.mark.parametrize("name", ["topk_micro", "tome_micro", "ats_micro"])
def test_stage_records_equal_the_viz_mode_run(name):
    from tokenreduction_amd import harness
    model = _prepared(name)
    loader, names = _loader(name)
    assert [x.shape[0] for x, _ in loader] == [3, 3, 2]
    dev = torch.device("cuda")
    model.viz_mode = True
    try:
        want = harness.validate(loader, model, dev, _model_name(name), names, keep_rate=[0.7], reduction_loc=[1, 2, 3])
    finally:
        model.viz_mode = False
    got = harness.validate(loader, model, dev, _model_name(name), names, keep_rate=[0.7], reduction_loc=[1, 2, 3], stage_records=True)
    _equal_dicts(got, want)
    rec = got[names[-1]]
    assert sorted(rec) == ["Loss", "Predictions", "Stage-1", "Stage-2", "Stage-3", "Target"] and all(rec[f"Stage-{s}"] for s in (1, 2, 3))
    # stage_records under viz_mode changes nothing: viz_mode's own path
    model.viz_mode = True
    try:
        _equal_dicts(harness.validate(loader, model, dev, _model_name(name), names, keep_rate=[0.7], reduction_loc=[1, 2, 3], stage_records=True),
                     want)
    finally:
        model.viz_mode = False


def test_defaults_return_what_they_returned():
    """No stage record without viz_mode, and the per-image entries of a plain forward."""
    from tokenreduction_amd import harness
    model = _prepared("topk_micro")
    loader, names = _loader("topk_micro")
    dev = torch.device("cuda")
    data = harness.validate(loader, model, dev, "topk_micro", names)
    taps = harness.validate(loader, model, dev, "topk_micro", names, stage_records=True)
    assert list(data) == list(taps)
    for n in names:
        assert sorted(data[n]) == ["Loss", "Predictions", "Target"]
        assert data[n]["Loss"] == taps[n]["Loss"] and (data[n]["Predictions"] == taps[n]["Predictions"]).all()
    assert (data["Top1-Acc"], data["Top5-Acc"], data["Params"]) == (taps["Top1-Acc"], taps["Top5-Acc"], taps["Params"])
