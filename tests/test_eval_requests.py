"""Eval requests against tests/golden/eval_requests.json (recorded by tests/golden/gen_eval_requests.py before the request record replaced
the loose (taps, decisions, dense) positionals): what every public eval entry raises on a CPU image in eval mode, train mode, viz_mode and
under dynamic_width -- the full message of every refusal and which one wins -- and the record itself.  No GPU needed."""
import json
import os

import pytest
import torch

from tests import _eval_requests as req
from tokenreduction_amd.models import EvalRequest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_requests.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        fixture = json.load(f)
    assert fixture["model"] == req.MODEL
    return fixture["states"]


@pytest.fixture(scope="module")
def model():
    return req.make_model()


def test_the_record_covers_the_matrix(recorded):
    assert list(recorded) == [s[0] for s in req.STATES]
    for state, row in recorded.items():
        assert list(row) == [label for label, _ in req.CALLS], state
        assert all(kind != "returned" for kind, _ in row.values()), state        # on a CPU image every request ends in an exception


@pytest.mark.parametrize("state", req.STATES, ids=[s[0] for s in req.STATES])
def test_refusals_match_the_record(recorded, model, state):
    for label, call in req.CALLS:
        assert req.outcome(model, state, call) == recorded[state[0]][label], (state[0], label)


class _OnDevice:
    """Stands in for a device tensor where only the request is built: the constructor reads is_cuda and device."""
    is_cuda, device = True, torch.device("cuda", 0)


def _request(model, **kw):
    return model._eval_request(_OnDevice(), "test", **kw)


def test_request_record_is_hashable_and_compares_by_value(model):
    a = _request(model, cls_blocks=[6, 3, 3], final_tokens=True)
    b = _request(model, cls_blocks=(3, 6), final_tokens=1)
    assert isinstance(a, EvalRequest) and a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert a.cls_blocks == (3, 6) and a.final_tokens is True and a.taps == ((3, 6), True) and not a.wants_decisions
    assert a != _request(model, cls_blocks=(3, 6)) and a != _request(model, cls_blocks=(3, 6), final_tokens=True, decisions=True)
    dense = _request(model, dense={})
    assert dense == _request(model, dense=dict(output_fmt="NCHW", dtype=torch.float32, fill=0)) and hash(dense) == hash(_request(model, dense={}))
    assert dense != _request(model, dense=dict(dtype=torch.bfloat16)) and dense != _request(model, dense=dict(fill=1.0))
    levels = _request(model, dense=dict(blocks=(-1, 3), norm=1))
    assert levels == _request(model, dense=dict(blocks=[3, 11], norm=True)) and levels != _request(model, dense=dict(blocks=(3, 11), norm=False))
    assert len({EvalRequest(), dense, levels, a}) == 4 and EvalRequest() == EvalRequest()


def test_what_a_request_implies_is_derived(model):
    plain, dense, levels = EvalRequest(), _request(model, dense={}), _request(model, dense=dict(blocks=(3,)))
    assert plain.taps is None and not plain.wants_decisions and plain.graph_key() == (None,)
    # a dense map is the final_tokens tap placed by the decisions; levels are placed by the decisions and leave the output taps alone
    assert dense.cls_blocks is None and dense.final_tokens is False and dense.decisions is False
    assert dense.taps == ((), True) and dense.wants_decisions
    assert levels.taps is None and levels.wants_decisions
    assert _request(model, decisions=True).wants_decisions and _request(model, decisions=True).taps is None
    # the graph key's layout: (taps, [("dense", fmt, dtype, fill[, blocks, norm])], [True])
    assert _request(model, cls_blocks=(3, 6)).graph_key() == (((3, 6), False),)
    assert _request(model, decisions=True).graph_key() == (None, True)
    assert dense.graph_key() == (((), True), ("dense", "NCHW", torch.float32, 0.0), True)
    assert levels.graph_key() == (None, ("dense", "NCHW", torch.float32, 0.0, (3,), True), True)
