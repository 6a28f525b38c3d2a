"""Frozen parameters, host side (CPU): finetune.freeze_attn_only against the names the reference's --attn-only leaves trainable
(tests/golden/attn_only_names.json, recorded by tests/golden/gen_attn_only.py from train.py:372-392 on the reference's own models),
and the parameter groups built afterwards."""
import json
import os

import pytest

from tokenreduction_amd import finetune
from tests.test_finetune import case_args

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_only_names.json")
WANT = json.load(open(GOLDEN))


@pytest.mark.parametrize("factory", sorted(WANT))
def test_freeze_attn_only_matches_the_reference(factory):
    import tokenreduction_amd as tra
    model = tra.create_model(factory, pretrained=False, num_classes=10, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None,
                             img_size=224, args=case_args())
    names = finetune.freeze_attn_only(model)
    want = WANT[factory]
    assert len(want["trainable"]) == 51                     # 12 x (qkv w,b + proj w,b) + pos_embed + head.weight + head.bias
    assert names == want["trainable"]                       # membership and order
    assert [n for n, p in model.named_parameters() if not p.requires_grad] == want["frozen"]
    # the peculiarities are the contract
    named = dict(model.named_parameters())
    assert named["pos_embed"].requires_grad and not named["cls_token"].requires_grad
    assert not any(p.requires_grad for p in model.patch_embed.parameters())
    assert not any(p.requires_grad for n, p in named.items() if "norm" in n or ".mlp." in n)
    # get_parameter_groups afterwards holds exactly the trainable ones
    groups = finetune.get_parameter_groups(model, 1e-3, 0.05, with_names=True)
    held = [n for g in groups for n in g["params"]]
    assert sorted(held) == sorted(want["trainable"]) and len(held) == len(set(held))
    ps = [p for g in finetune.get_parameter_groups(model, 1e-3, 0.05) for p in g["params"]]
    assert all(p.requires_grad for p in ps) and len(ps) == 51
