"""Constructors against tests/golden/model_construction.json (recorded by tests/golden/gen_model_construction.py before the schedule
parsing of the nine families was folded into one function): parameter registration order and shapes, state_dict keys, the keep schedule,
the helper surface, the public attributes and the number of random draws of every registered factory, and the executor-state contract of
copy.deepcopy.  No GPU needed."""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn

import tokenreduction_amd as tra
from tests import _construction as con

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_construction.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        fixture = json.load(f)
    return fixture["entries"], fixture["mismatch"]


@pytest.mark.parametrize("size", ["tiny", "small", "base"])
def test_construction_matches_the_record(recorded, size):
    want, _ = recorded
    cases = [c for c in con.cases() if f"_{size}_" in c[1]]
    assert len(cases) == 46 and {k for k, _, _ in con.cases()} == set(want)
    for key, name, args in cases:
        got = json.loads(json.dumps(con.snapshot(name, args)))          # tuples -> lists, as the record went through JSON
        for field in want[key]:
            assert got[field] == want[key][field], (key, field)
        assert set(got) == set(want[key]), key


@pytest.mark.parametrize("which", sorted(con.MISMATCH_CASES))
def test_schedule_length_mismatch_message(recorded, which):
    assert con.mismatch_message(which) == recorded[1][which]


class _NoCopy:
    def __deepcopy__(self, memo):
        raise TypeError("cannot be deep-copied (stands in for torch.cuda.CUDAGraph)")


def test_deepcopy_resets_every_executor_attribute():
    """Whatever _reset_executor_state() assigns is left behind by a copy -- the attribute list is taken from the method's effect on a
    bare nn.Module, so a cache added to it later is covered without this test being edited."""
    probe = nn.Module()
    tra.VisionTransformer._reset_executor_state(probe)
    owned = set(vars(probe)) - set(vars(nn.Module()))
    assert {"_ws", "_packed", "_tstate", "_pack_slots", "_noise_bufs", "_pixel_luts", "_pipe_streams"} <= owned
    args = con._args([0.7], [1, 2])
    kw = dict(patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4, qkv_bias=True, num_classes=8, args=args)
    fresh, m = tra.DPCKNNVisionTransformer(**kw), tra.DPCKNNVisionTransformer(**kw)
    assert owned <= set(vars(fresh))                      # every one of them exists from construction
    fresh._reset_executor_state()
    m.set_pixel_input()
    m.precision = "fp32"
    for k in owned:
        setattr(m, k, _NoCopy())
    twin = copy.deepcopy(m)
    assert {k: vars(twin)[k] for k in owned} == {k: vars(fresh)[k] for k in owned}
    assert twin._noise_buf is None
    assert twin.pixel_input == m.pixel_input and twin.precision == "fp32" and twin._keep == m._keep      # settings survive
    assert all(isinstance(vars(m)[k], _NoCopy) for k in owned)                                            # the original is untouched
    for (n, a), (_, b) in zip(m.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr(), n
