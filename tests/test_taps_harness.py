"""harness.extract_cls_features (extract_cls_features.py:113-141) on the CPU: a stub model with forward_async's tap interface, checked
against the reference loop written out longhand -- np.vstack of viz_data["Features"][block][:, 0] per batch."""
import numpy as np
import torch

from tokenreduction_amd import harness

DEPTH, D = 12, 8


def _features(n):
    """Pre-baked 'stream after every block', [DEPTH, n, 3 tokens, D]: every (block, image) has its own values."""
    g = torch.Generator().manual_seed(11)
    return torch.randn(DEPTH, n, 3, D, generator=g)


class _Handle:
    def __init__(self, model, k, out):
        self.model, self.k, self.out = model, k, out

    def result(self):
        self.model.events.append(("result", self.k))
        return self.out


class _Stub(torch.nn.Module):
    """forward_async(x, cls_blocks=...) -> handle of (logits, taps) keyed by the first pixel of each image; logs launches and results."""

    def __init__(self, feats):
        super().__init__()
        self.feats, self.events, self.launched = feats, [], 0

    def forward_async(self, x, cls_blocks=None, final_tokens=False):
        assert not self.training and not final_tokens
        ids = x[:, 0, 0, 0].long()
        blocks = tuple(sorted(set(cls_blocks)))
        cls = torch.stack([self.feats[b][ids][:, 0] for b in blocks], dim=1)          # [B, n, D]
        k, self.launched = self.launched, self.launched + 1
        self.events.append(("launch", k))
        return _Handle(self, k, (torch.zeros(len(ids), 5), {"cls": cls, "blocks": blocks, "final_tokens": None}))

    def check_status(self):
        self.events.append(("status", None))


def _loader(n, bs):
    imgs = torch.zeros(n, 3, 2, 2)
    imgs[:, 0, 0, 0] = torch.arange(n).float()
    return [(imgs[i:i + bs], torch.zeros(len(imgs[i:i + bs]), dtype=torch.long)) for i in range(0, n, bs)]


def _longhand(feats, loader, keys):
    """extract_cls_features.py:113-132 on the pre-baked Features."""
    mats = {k: None for k in keys}
    for x, _ in loader:
        ids = x[:, 0, 0, 0].long()
        viz = {"Features": {b: feats[b][ids].numpy() for b in range(DEPTH)}}
        for key in list(mats.keys()):
            if mats[key] is None:
                mats[key] = viz["Features"][key][:, 0]
            else:
                mats[key] = np.vstack([mats[key], viz["Features"][key][:, 0]])
    return mats


def test_default_blocks_in_loader_order_with_a_partial_last_batch():
    feats, loader = _features(11), _loader(11, 4)                    # batches of 4, 4, 3
    model = _Stub(feats).train()
    got = harness.extract_cls_features(loader, model, torch.device("cpu"))
    want = _longhand(feats, loader, (3, 6, 9, 11))
    assert sorted(got) == [3, 6, 9, 11] and not model.training
    for b in want:
        assert got[b].shape == (11, D) and got[b].dtype == np.float32
        np.testing.assert_array_equal(got[b], want[b])


def test_block_selection_any_order_and_a_single_batch():
    feats, loader = _features(5), _loader(5, 8)
    got = harness.extract_cls_features(loader, _Stub(feats), torch.device("cpu"), blocks=(7, 0, 2))
    want = _longhand(feats, loader, (0, 2, 7))
    assert sorted(got) == [0, 2, 7]
    for b in want:
        np.testing.assert_array_equal(got[b], want[b])


def test_one_batch_of_lookahead_then_the_status_check():
    feats, loader = _features(9), _loader(9, 3)
    model = _Stub(feats)
    harness.extract_cls_features(loader, model, torch.device("cpu"), blocks=(1,))
    assert model.events == [("launch", 0), ("launch", 1), ("result", 0), ("launch", 2), ("result", 1), ("result", 2), ("status", None)]


def test_an_empty_loader_leaves_every_block_none_like_the_reference():
    model = _Stub(_features(1))
    assert harness.extract_cls_features([], model, torch.device("cpu"), blocks=(3, 6)) == {3: None, 6: None}
    assert model.events == [("status", None)]
