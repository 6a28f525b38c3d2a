"""Host logic of the fine-tune recipe: which parameters train at which learning rate, and the LR schedule.

Mirrors, for models built by tokenreduction_amd.create_model (same parameter names and `get_new_module_names()` as the reference):

    optim.py:39-100      get_parameter_groups()   decay / no_decay backbone groups at `bone_lr_scale` x lr, frozen for `fix_steps`
                                                   epochs; new modules (head, pos_embed, patch_embed, the method's own layers) at
                                                   full lr; optional constant cls / pos tokens
    train.py:416-419     linear LR scaling         lr * total_batch_size / lr_batch_normalizer
    engine.py:35-37      frozen_lr()               groups whose `fix_step` has not been reached run at lr 0
    scheduler_factory.py:10-66 + timm==0.4.12 timm/scheduler/cosine_lr.py (not vendored by the reference; its published algorithm is
                         restated in CosineSchedule): linear warm-up, cosine to lr_min, counted in optimizer STEPS when
                         `sched_in_steps` (t_in_epochs=False) -- `step_update(num_updates)` -- or in epochs -- `step(epoch)`.

    train.py:372-392     freeze_attn_only()        --attn-only: attention layers, head and pos_embed train, everything else is frozen
    train.py:343-370     load_finetune_checkpoint() ingest of a DeiT-layout checkpoint: mismatching classifier dropped, position
                                                   embedding resized to the model's patch grid

Host-side bookkeeping only -- nothing here touches the GPU; the step it configures (forward, backward, the data-parallel gradient
mean) is the HIP training path (training.py, dp.py), driven by harness.train_one_epoch.
The parameter-group membership is pinned against lists recorded from the reference's own function
(tests/golden/param_groups.json, tests/golden/gen_param_groups.py); the cosine schedule has no reference run behind it (timm is
not installed here) and is checked against its closed form only.
"""
import math
from typing import Iterable, List, Optional, Sequence

import torch

NEW_MODULE_NAMES = ["head.weight", "head.bias", "head_dist.weight", "head_dist.bias", "pos_embed", "patch_embed"]   # optim.py:43


def scale_lr(lr: float, total_batch_size: int, lr_batch_normalizer: float) -> float:
    """train.py:416-419 (skipped by the reference under --unscale_lr)."""
    return lr * total_batch_size / lr_batch_normalizer


def get_parameter_groups(model, learning_rate, weight_decay=1e-5, bone_lr_scale=0.01, fix_steps=5, constant_cls=False,
                         constant_pos=False, skip_list=(), with_names=False):
    """optim.py:39-100.  Returns the optimizer's param-group dicts in first-seen order; `with_names=True` returns the same
    groups with parameter NAMES in `params` (what the reference prints)."""
    new_names = list(NEW_MODULE_NAMES)
    if hasattr(model, "get_new_module_names"):
        new_names.extend(model.get_new_module_names())
    groups = {}
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if ("cls_token" in name or "dist_token" in name) and constant_cls:
            continue
        if "pos_embed" in name and constant_pos:
            continue
        no_decay = len(param.shape) == 1 or name.endswith(".bias") or name in skip_list
        if any(name in s for s in new_names) or any(s in name for s in new_names):
            group, wd, scale, fix = ("new_param_no_decay", 0, 1.0, 0) if no_decay else ("new_param", weight_decay, 1.0, 0)
        else:
            group, wd, scale, fix = ("no_decay", 0.0, bone_lr_scale, fix_steps) if no_decay else ("decay", weight_decay, bone_lr_scale, fix_steps)
        if group not in groups:
            groups[group] = {"weight_decay": wd, "params": [], "lr": learning_rate * scale, "fix_step": fix}
        groups[group]["params"].append(name if with_names else param)
    return list(groups.values())


def freeze_attn_only(model) -> List[str]:
    """train.py:372-392 (--attn-only): only the attention layers (every name with `.attn.`: qkv and proj, weights and biases), the
    classifier and `pos_embed` keep requires_grad; everything else is frozen -- `cls_token`, `patch_embed`, every norm, the Mlps and
    the family's own modules included.  Returns the trainable names.  The HIP backward skips the frozen gradients (training.py)."""
    for name, p in model.named_parameters():
        p.requires_grad = ".attn." in name
    model.head.weight.requires_grad = True
    model.head.bias.requires_grad = True
    model.pos_embed.requires_grad = True
    for p in model.patch_embed.parameters():
        p.requires_grad = False
    return [name for name, p in model.named_parameters() if p.requires_grad]


def frozen_lr(param_groups: Iterable[dict], epoch: int) -> None:
    """engine.py:35-37: called before every step; a group is frozen (lr 0) until its `fix_step` epoch."""
    for g in param_groups:
        if epoch < g.get("fix_step", 0):
            g["lr"] = 0


class CosineSchedule:
    """timm 0.4.12 CosineLRScheduler as scheduler_factory.py:34-50 builds it (t_mul and decay_rate per cycle, cycle_limit,
    warm-up not a prefix).  `base_lrs` are the groups' initial lrs; with warm-up the groups start at `warmup_lr_init`."""

    def __init__(self, param_groups: Sequence[dict], t_initial: int, lr_min: float = 0.0, warmup_t: int = 0, warmup_lr_init: float = 0.0,
                 t_in_epochs: bool = True, t_mul: float = 1.0, decay_rate: float = 1.0, cycle_limit: int = 1):
        self.groups = list(param_groups)
        for g in self.groups:
            g.setdefault("initial_lr", g["lr"])
        self.base = [g["initial_lr"] for g in self.groups]
        self.t_initial, self.lr_min, self.warmup_t, self.warmup_lr_init = max(int(t_initial), 1), lr_min, warmup_t, warmup_lr_init
        self.t_in_epochs, self.t_mul, self.decay_rate, self.cycle_limit = t_in_epochs, t_mul, decay_rate, cycle_limit
        if warmup_t:
            self.warmup_steps = [(v - warmup_lr_init) / warmup_t for v in self.base]
            self._set([warmup_lr_init] * len(self.base))
        else:
            self.warmup_steps = [1.0] * len(self.base)

    @classmethod
    def from_args(cls, args, param_groups):
        """scheduler_factory.py:10-50 for args.sched == 'cosine' (no LR noise)."""
        in_epochs = not args.sched_in_steps
        per = 1 if in_epochs else args.num_steps_epoch
        return cls(param_groups, t_initial=args.epochs * per, lr_min=args.min_lr, warmup_t=args.warmup_epochs * per,
                   warmup_lr_init=args.warmup_lr, t_in_epochs=in_epochs, t_mul=getattr(args, "lr_cycle_mul", 1.0),
                   decay_rate=args.decay_rate, cycle_limit=getattr(args, "lr_cycle_limit", 1))

    def lr_at(self, t: int) -> List[float]:
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * s for s in self.warmup_steps]
        if self.t_mul != 1:
            i = math.floor(math.log(1 - t / self.t_initial * (1 - self.t_mul), self.t_mul))
            t_i = self.t_mul ** i * self.t_initial
            t_curr = t - (1 - self.t_mul ** i) / (1 - self.t_mul) * self.t_initial
        else:
            i = t // self.t_initial
            t_i = self.t_initial
            t_curr = t - self.t_initial * i
        gamma = self.decay_rate ** i
        lr_min = self.lr_min * gamma
        if self.cycle_limit == 0 or i < self.cycle_limit:
            return [lr_min + 0.5 * (v * gamma - lr_min) * (1 + math.cos(math.pi * t_curr / t_i)) for v in self.base]
        return [self.lr_min for _ in self.base]

    def _set(self, lrs):
        for g, v in zip(self.groups, lrs):
            g["lr"] = v

    def step(self, epoch: int) -> None:
        if self.t_in_epochs:
            self._set(self.lr_at(epoch))

    def step_update(self, num_updates: int) -> None:          # engine.py:110-111
        if not self.t_in_epochs:
            self._set(self.lr_at(num_updates))


def load_finetune_checkpoint(model, checkpoint, src_grid=None):
    """Ingest of a pre-trained checkpoint for fine-tuning (train.py:343-370): `checkpoint` is what torch.load returns for a
    DeiT-layout .pth ({"model": state_dict}) or the state dict itself.  A classifier whose shape does not fit the model is dropped,
    the position embedding is resized to the model's patch grid (class / distillation rows kept, the grid bicubically
    interpolated to the model's (gh, gw) -- 14 x 14 -> 24 x 24 for a 224 -> 384 fine-tune, 14 x 14 -> 24 x 40 for a 384 x 640 model; the
    checkpoint's grid is taken as square unless src_grid=(h, w) names it, and a length that is no square without src_grid raises), a model with global_pool='avg' takes a checkpoint's fc_norm.* as its
    norm.* when the checkpoint has no norm.* of its own (timm's layout of MAE fine-tuned weights), everything else is loaded non-strictly.
    A LayerScale model (init_values) takes a checkpoint's blocks.N.gamma_1 / gamma_2 (the DeiT-III repository's and older timm's names) as
    ls1.gamma / ls2.gamma unless the new names are there; a no_embed_class model's table has no class row, so all of it is the grid.  Returns load_state_dict's
    (missing_keys, unexpected_keys).  Host-side only: the executor re-packs its operand copies at the next forward (new addresses
    and values are detected by the packing key)."""
    import torch.nn.functional as F
    sd = dict(checkpoint["model"] if isinstance(checkpoint, dict) and "model" in checkpoint else checkpoint)
    own = model.state_dict()
    for k in ("head.weight", "head.bias", "head_dist.weight", "head_dist.bias"):
        if k in sd and k in own and sd[k].shape != own[k].shape:
            del sd[k]
    if getattr(model, "global_pool", "") == "avg":
        # an average-pooled timm checkpoint (MAE fine-tuning) keeps its final norm as fc_norm -- applied after the pool, like this model's norm
        for k in ("weight", "bias"):
            if f"fc_norm.{k}" in sd and f"norm.{k}" not in sd:
                sd[f"norm.{k}"] = sd.pop(f"fc_norm.{k}")
    if any(k.endswith(".ls1.gamma") for k in own):
        # a LayerScale model: the DeiT-III repository and older timm releases call the two vectors blocks.N.gamma_1 / gamma_2 -- taken as
        # ls1.gamma / ls2.gamma unless the checkpoint has the new names (sd is a copy: the caller's dict keeps its keys)
        for k in [k for k in sd if k.startswith("blocks.") and k.endswith((".gamma_1", ".gamma_2"))]:
            new = k[:-len("gamma_1")] + ("ls1.gamma" if k.endswith("1") else "ls2.gamma")
            v = sd.pop(k)
            if new not in sd:
                sd[new] = v
    pos = sd.get("pos_embed")
    gh, gw = model.patch_embed.grid_size
    if src_grid is not None:
        src_grid = tuple(int(v) for v in src_grid)
        if len(src_grid) != 2 or min(src_grid) <= 0:
            raise ValueError(f"src_grid: expected (h, w) of the checkpoint's position grid, got {src_grid}")
    if pos is not None and (pos.shape != model.pos_embed.shape or (src_grid is not None and src_grid != (gh, gw))):
        n_extra = model.pos_embed.shape[-2] - gh * gw
        n_src = pos.shape[-2] - n_extra
        if src_grid is None:
            side = int(round(n_src ** 0.5)) if n_src > 0 else 0
            if side <= 0 or side * side != n_src:
                raise ValueError(f"pos_embed: the checkpoint's table has {n_src} grid rows (of {pos.shape[-2]}), which is no square grid; "
                                 "name its grid with src_grid=(h, w)")
            src_grid = (side, side)
        elif src_grid[0] * src_grid[1] != n_src:
            raise ValueError(f"src_grid {src_grid} has {src_grid[0] * src_grid[1]} patches, the checkpoint's table {n_src} grid rows (of {pos.shape[-2]})")
        grid = pos[:, n_extra:].reshape(-1, src_grid[0], src_grid[1], pos.shape[-1]).permute(0, 3, 1, 2)
        grid = F.interpolate(grid, size=(gh, gw), mode="bicubic", align_corners=False)
        sd["pos_embed"] = torch.cat((pos[:, :n_extra], grid.permute(0, 2, 3, 1).flatten(1, 2)), dim=1)
    return model.load_state_dict(sd, strict=False)
