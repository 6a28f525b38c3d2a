"""Output taps against the paths they replace, both sides in one process on one box (profiles/taps_lab.md).

    python tools/taps_bench.py cls [--batch 256] [--steps 20] [--rounds 3]
        The CLS-feature dump of extract_cls_features.py:113-132 on dense DeiT-S: images/s through viz_mode (the parent's only way: every
        row of every block to the host, then [:, 0]) against model.forward_taps and against harness.extract_cls_features (taps with one
        batch of lookahead); the three results are compared bit for bit before anything is timed.
    python tools/taps_bench.py distill [--batch 128] [--steps 20] [--rounds 3]
        A DyViT-S distillation step (student forward + loss of losses.py:100-158 + backward + FusedAdamW) with the teacher on the parent's
        path (features_out of every block, read back, a separate fp32 LayerNorm) against the final_tokens tap; the teachers' outputs are
        compared bit for bit first.
The two sides alternate within a round, so a drift of the box shows as spread between rounds.  One JSON line per leg."""
import argparse
import functools
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = (3, 6, 9, 11)


def _args(**kw):
    base = dict(keep_rate=[0.7], reduction_loc=[3, 6, 9], viz_mode=False, dyvit_distill=False, k_neighbors=5, equal_weight=False, cluster_iters=3,
                sinkhorn_eps=1.0, heuristic_pattern="l2", not_contiguous=False, min_radius=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _create(name, args, **kw):
    import torch
    import tokenreduction_amd as tra
    torch.manual_seed(0)
    return tra.create_model(name, pretrained=False, num_classes=1000, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None, img_size=224,
                            args=args, **kw).cuda()


def _timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(sides, steps, rounds, warmup=2):
    """{name: [seconds per round]} with the sides taking turns inside every round."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(_timed(fn, steps))
    return out


def cls_dump(batch, steps, rounds):
    import numpy as np
    import torch
    from tokenreduction_amd import harness
    m = _create("deit_small_patch16_224_local_viz", _args(keep_rate=[1.0], reduction_loc=[])).eval()
    x = torch.randn(batch, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    loader = [(x, None)] * steps

    def viz():
        m.viz_mode = True
        try:
            _, v = m(x)
        finally:
            m.viz_mode = False
        return {k: v["Features"][k][:, 0] for k in BLOCKS}

    def taps():
        _, t = m.forward_taps(x, cls_blocks=BLOCKS)
        c = t["cls"].cpu().numpy()
        return {k: c[:, i] for i, k in enumerate(BLOCKS)}

    a, b = viz(), taps()
    c = harness.extract_cls_features(loader[:2], m, torch.device("cuda"), blocks=BLOCKS)
    same = all(np.array_equal(a[k], b[k]) and np.array_equal(np.vstack([a[k], a[k]]), c[k]) for k in BLOCKS)
    secs = _alternate({"viz_mode": viz, "forward_taps": taps}, steps, rounds)
    secs["extract_cls_features"] = [_timed(lambda: harness.extract_cls_features(loader, m, torch.device("cuda"), blocks=BLOCKS), 1)
                                    for _ in range(rounds)]
    ips = {k: [round(batch * steps / s, 1) for s in v] for k, v in secs.items()}
    print(json.dumps({"leg": "cls_dump", "model": "deit_small", "B": batch, "steps": steps, "blocks": BLOCKS, "bitwise_equal": bool(same),
                      "images_per_s": ips, "median_images_per_s": {k: statistics.median(v) for k, v in ips.items()}}), flush=True)
    assert same, "the CLS taps differ from viz_data['Features'][blk][:, 0]"


def distill(batch, steps, rounds):
    import torch
    import torch.nn.functional as F
    from tokenreduction_amd import finetune, ops
    from tokenreduction_amd.models import VisionTransformerTeacher
    from tokenreduction_amd.optim import FusedAdamW

    class ParentTeacher(VisionTransformerTeacher):
        """The teacher's forward as it was before the final_tokens tap: Features of every block, the last one through ops.layernorm_f32."""
        _always_features = True

        def forward(self, x):
            was_training, self.training = self.training, False
            try:
                logits = self._forward_eval(x, 0)
            finally:
                self.training = was_training
            B, N, D = x.shape[0], self._last_tokens[-1], self.embed_dim
            off = sum(B * n * D for n in self._last_tokens[:-1])
            feat = ops.layernorm_f32(self._last_ws["feat"][off: off + B * N * D].view(B * N, D), self.norm.weight.detach().float().contiguous(),
                                     self.norm.bias.detach().float().contiguous(), float(self.norm.eps)).view(B, N, D)
            return logits, feat[:, 1:]

    student = _create("dyvit_small_patch16_224", _args(dyvit_distill=True)).train()
    new = _create("dyvit_small_patch16_224_teacher", _args()).eval()
    old = ParentTeacher(patch_size=16, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4, qkv_bias=True, num_classes=1000,
                        norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6))
    old.load_state_dict(new.state_dict())
    old = old.cuda().eval()
    opt = FusedAdamW(finetune.get_parameter_groups(student, 1e-4, 0.05, 1.0, 0), model=student)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 1000, (batch,), generator=g).cuda()
    with torch.no_grad():
        (la, ta), (lb, tb) = old(x), new(x)
    same = bool(torch.equal(la, lb) and torch.equal(ta, tb))

    def step(teacher):
        pred, token_pred, mask, scores = student(x)                             # losses.py:100-158, mse_token, batchmean
        loss = F.cross_entropy(pred, y)
        loss = loss + 2.0 * sum(((s.mean(1) - r) ** 2).mean() for s, r in zip(scores, student.token_ratio)) / len(scores)
        with torch.no_grad():
            cls_t, token_t = teacher(x)
        loss = loss + 0.5 * F.kl_div(F.log_softmax(pred, -1), F.log_softmax(cls_t, -1), reduction="batchmean", log_target=True)
        keep = mask.reshape(-1) > 0.5
        loss = loss + 0.5 * (token_pred.reshape(-1, token_pred.shape[-1])[keep] - token_t.reshape(-1, token_t.shape[-1])[keep]).pow(2).mean()
        loss.backward()
        opt.step()
        opt.zero_grad()

    secs = _alternate({"teacher_features_out": lambda: step(old), "teacher_final_tokens_tap": lambda: step(new)}, steps, rounds)
    with torch.no_grad():
        tsecs = _alternate({"teacher_features_out": lambda: old(x), "teacher_final_tokens_tap": lambda: new(x)}, steps, rounds)
    ms = {k: [round(1e3 * s / steps, 3) for s in v] for k, v in secs.items()}
    tms = {k: [round(1e3 * s / steps, 3) for s in v] for k, v in tsecs.items()}
    print(json.dumps({"leg": "distill_step", "model": "dyvit_small kr 0.7", "B": batch, "steps": steps, "teacher_outputs_bitwise_equal": same,
                      "ms_per_step": ms, "median_ms_per_step": {k: statistics.median(v) for k, v in ms.items()},
                      "teacher_forward_ms": tms, "median_teacher_forward_ms": {k: statistics.median(v) for k, v in tms.items()}}), flush=True)
    assert same, "the teacher's outputs moved"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["cls", "distill"])
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    if a.leg == "cls":
        cls_dump(a.batch or 256, a.steps, a.rounds)
    else:
        distill(a.batch or 128, a.steps, a.rounds)
