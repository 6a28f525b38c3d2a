"""Host-side mirror of the reference's model classes for the hot path.

Same constructor signature, attribute names, state-dict keys, helper methods and forward return
contract as
    models/deit_viz.py:75-212   VisionTransformer            (timm-0.4.12 ViT, the DeiT trunk)
    models/topk.py:102-212      TopKVisionTransformer
    models/evit.py:132-244      EfficientVisionTransformer
so a `train.py` / `validate.py`-style driver can swap `timm.models.create_model` for
`tokenreduction_amd.create_model` unchanged.  The nn.Modules below only HOLD parameters (so
load_state_dict / state_dict / optimizers see the reference's key names); `forward` never calls
them: it hands the image batch to the gfx950 executor (csrc/tr_vit.hip) through the C ABI.

There is no CPU path: forward() on a CPU tensor raises.  In train mode forward() runs the training executor
(activations kept on a tape) and `loss.backward()` runs the HIP backward executor (training.py) -- every family and
every factory width, 224 x 224 and 384 x 384; what the training path refuses (attn_drop_rate, the distillation token,
more than 640 tokens) raises there.  In eval mode every family runs at up to 1024 patch tokens + CLS (448 x 448 and 512 x 512
inputs) in all three precisions; more tokens raise.
img_size=(H, W), H and W multiples of 16, is a rectangular input [B, C, H, W]: a gh x gw = H/16 x W/16 grid of row-major patches, through
every entry a square model runs, with the same limits on the token count; Heuristic, whose distance grid is square, refuses it.
A headless model (num_classes=0 or reset_classifier(0): head = nn.Identity(), deit_viz.py:142,182) returns the fp32 final-normed CLS row
[B, embed_dim] wherever a classifier returns logits -- eval in all three precisions, viz_mode, forward_async, training and its backward.
global_pool='avg' (constructor, create_model, reset_classifier; timm's average-pooled head with fc_norm, the MAE fine-tuning layout): the
head -- or a headless model's output -- reads LayerNorm(weighted mean of the patch tokens after the last block) instead of the final-normed CLS
row; the weights are ToMe's token sizes and the ATS padding mask, ones elsewhere.  Eval in all three precisions, training and backward; DyViT
refuses it in train mode (its masked tokens stay in the stream).  '' and 'token' are the CLS row, the default.
init_values (timm's LayerScale: blocks[i].ls1 / ls2, gamma [D]) and no_embed_class (pos_embed [1, P, D]) are the two options of a DeiT-III
backbone: gamma reaches the executor folded into proj / fc2 (csrc/tr_layerscale.hip), its gradient is unfolded behind the backward (training.py);
every family, eval in all three precisions, training and backward.
Intermediate outputs of an eval forward: viz_mode (every row of every recorded block, on the host) or the output taps of forward_taps /
forward_async -- the CLS rows after chosen blocks and the final-normed tokens, fp32 device tensors written while the fast path runs.
The stages' decisions (which tokens each stage kept, which output every token went to) come the same two ways: viz_mode's viz_data, or
forward_decisions / forward_async(decisions=True) -- int32 device tensors in the form of validate.py's per-image records, one launch
(tr_stage_decisions) behind the fast-path forward.
forward_dense / forward_async(dense=...) put the final-normed rows of the last block back on the input's patch grid ([B, D, h, w] or
[B, h, w, D]) through those decisions: two more launches (tr_dense_index, tr_dense_gather), `fill` where no row stands for a patch.
forward_dense(blocks=...) / get_intermediate_layers do the same for chosen intermediate blocks: the executor writes every row of those
blocks while the fast path runs (tr_vit_forward_levels), each level is placed by the stages at or before its block, and one index launch and
one gather launch serve all levels (tr_dense_index_levels, tr_dense_gather_levels).
forward_dense_train is the last block's map of a TRAINING forward, a second output of the training autograd node: its gradient reaches the
backbone through tr_dense_scatter (the gather's adjoint) and tr_vit_backward_dense (training.py).  forward_dense_train(blocks=...) returns
the maps of chosen blocks, each a further output of that node (tr_vit_forward_train_levels, tr_dense_scatter_levels, tr_vit_backward_levels).
"""
from __future__ import annotations

import copy
import ctypes as C
import types
import warnings
from functools import partial
from typing import Callable, List, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, pixels
from .augment import AugmentedBatch
from .eval_request import DENSE_TRAIN_REFUSALS, REFUSALS, REFUSE_CPU, DenseOutput, EvalRequest, Levels


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class PatchEmbed(nn.Module):
    """Parameter holder with timm PatchEmbed's attribute surface (num_patches, grid_size, proj)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        self.img_size, self.patch_size = _pair(img_size), _pair(patch_size)
        self.grid_size = (self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)


class _Pending:
    """Handle of a forward enqueued by VisionTransformer.forward_async: result() makes the caller's CURRENT stream wait for it."""

    def __init__(self, out, event):
        self._out, self._event = out, event

    def result(self):
        if self._event is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(self._event)
            def keep(t):                                # (forward_taps / forward_decisions: dicts of tensors beside the logits)
                if torch.is_tensor(t):
                    t.record_stream(cur)
                elif isinstance(t, dict):
                    for u in t.values():
                        keep(u)
                elif isinstance(t, (tuple, list)):
                    for u in t:
                        keep(u)
            keep(self._out)
            self._event = None
        return self._out


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias=True, keep_rate=1.0):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.keep_rate = keep_rate
        self.init_n = 14 * 14   # topk.py:40 -- hard-coded in the reference, independent of img_size


class LayerScale(nn.Module):
    """timm's LayerScale (init_values; DeiT-III): the branch's output times a learnable per-channel `gamma` [D].  A parameter holder like
    every module here: the executor reads gamma folded into the Linear that ends the branch (VisionTransformer._pack)."""

    def __init__(self, dim, init_values=1e-5):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True, norm_layer=nn.LayerNorm, keep_rate=1.0, init_values=None):
        super().__init__()
        # registration order is timm's: norm1, attn, ls1, norm2, mlp, ls2 -- and without init_values nothing is registered for ls1 / ls2 (not
        # even an Identity): parameter order and state-dict keys of a plain block stay what they were
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads, qkv_bias, keep_rate)
        if init_values:
            self.ls1 = LayerScale(dim, init_values)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        if init_values:
            self.ls2 = LayerScale(dim, init_values)


def _init_vit_weights(m: nn.Module):
    """deit_viz.py:215-247 with name='' / jax_impl=False (what `self.apply(self._init_weights)` does)."""
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=0.02)
        if m.bias is not None:
            nn.init.zeros_(m.bias)
    elif isinstance(m, nn.LayerNorm):
        nn.init.zeros_(m.bias)
        nn.init.ones_(m.weight)


def _pad8(n):
    """Rows of a matrix whose row count the kernels pad with zeros: the classifier, the K outputs of a soft-assignment stage."""
    return (n + 7) // 8 * 8


def _pad64(n):
    """Widths the bf16 GEMMs reduce over (K-step 64): hidden layers of the reduction modules, leading dimensions of their transposed copies."""
    return (n + 63) // 64 * 64


class Op(NamedTuple):
    """One operand of the executor's weight structs (tr_vit_weights / tr_block_weights / tr_stage_weights): THE declaration the pack (W), the
    gradient pointers (G), the gradient slot sizes and the transposed dgrad operands (WT) are all derived from.  Trunk and block rows come in
    pairs, the two gradients one launch of the backward produces (a unit)."""
    field: str                          # member of the struct
    name: Optional[str] = None          # the parameter behind it, relative to the model / "blocks.i." / the stage's module; None: no parameter
    kind: str = "f32"                   # "f32": fp32 as it is | "w": matrix in the operand type | "wt": ... with a transposed bf16 copy made by
                                        # the packer | "grad": no operand, the field takes the parameter's gradient only | "f32_row0": fp32 table
                                        # of `rows` rows in a buffer of its own, born zeros: row 0 stays zero, the parameter is rows 1 ..
    rows: int = 0                       # the operand is a zero-padded copy with this many rows / columns (0: the value's own)
    cols: int = 0
    grad_rows: int = 0                  # rows of the gradient the kernels write: the parameter's slot in the flat buffer (0: the parameter's own)
    t_rows: Optional[int] = None        # stage rows: the dgrad operand is the transposed bf16 copy of the value padded to this many rows, its
                                        # leading dimension (0: the operand's rows; None: no such copy)
    value: Optional[Callable] = None    # value() -> fp32 tensor, for an operand that is not the parameter as it stands
    gamma: Optional[str] = None         # block rows: the LayerScale gamma folded into this Linear when the model has one
    grad: bool = True                   # the field of the gradient struct points at the parameter's slot


def _unit(field, path, kind="f32", gamma=None):
    """The two rows of a LayerNorm ("f32": <field>_g, <field>_b) or a Linear (<field>_w, <field>_b) at module `path`."""
    return Op(field + ("_g" if kind == "f32" else "_w"), path + ".weight", kind, gamma=gamma), Op(field + "_b", path + ".bias")


# tr_block_weights: the six units of a block, names relative to "blocks.i." (mlp_pk, the fragment-major Mlp buffer, derives from fc1 / fc2)
_BLOCK_UNITS = (_unit("ln1", "norm1"), _unit("qkv", "attn.qkv", "wt"), _unit("proj", "attn.proj", "wt", "ls1.gamma"),
                _unit("ln2", "norm2"), _unit("fc1", "mlp.fc1", "wt"), _unit("fc2", "mlp.fc2", "wt", "ls2.gamma"))


def _padded(t, rows=0, cols=0):
    """Detached fp32 copy of a vector [n] / matrix [r, c] with zeros appended up to `rows` (and `cols`); 0 keeps the size."""
    shape = (rows or t.shape[0],) + ((cols or t.shape[1],) if t.dim() > 1 else ())
    out = torch.zeros(shape, dtype=torch.float32, device=t.device)
    out[tuple(slice(n) for n in t.shape)] = t.detach()
    return out


def _expand_schedule(values, locs, expand, what):
    """The per-stage values of a (keep_rate, reduction_loc) pair: ONE value is expanded to a geometric schedule by the family's own rule
    `expand(value, stage index)`, a list is taken as given and must name one value per location (`what` = the two nouns of the reference's
    assertion message)."""
    values, locs = list(values), list(locs)
    if len(values) == 1:
        values = [expand(values[0], idx) for idx in range(len(locs))]
    assert len(values) == len(locs), f"Mismatch between the {what[0]} location ({locs}) and {what[1]} ({values})"
    return values


class _Packer:
    """The operand copies of one _pack() call: w16(t) / f32(t) return the device address the executor reads parameter t through.  A LIVE
    parameter storage (fp32, contiguous, on the device) is passed through as it is -- always current, never copied; everything else goes
    into a persistent slot of `model._pack_slots`, keyed (call index, kind), so the ORDER of the calls is the identity of a slot: a repack
    rewrites the same buffers in place and addresses, workspaces and captured graphs survive."""

    def __init__(self, model, dev, wdt, want_t):
        self.dev, self.wdt, self.want_t = dev, wdt, want_t
        self.slots = model._pack_slots
        self.own = {p.untyped_storage().data_ptr() for p in model.parameters()}      # storages that ARE parameters
        self.calls = 0
        self.fused = []                  # (fp32 source, bf16 slot, transposed bf16 slot or None): one tr_cast_pack_bf16 launch for all
        self.folds = []                  # (W, b, gamma, operand slot, transposed slot or None, bias slot): one tr_layerscale_fold launch for all
        self.keep_alive = []
        self.moved = False               # a slot was (re)allocated: addresses changed
        self.copied = False              # an operand copy the fused table does not cover (optim.FusedAdamW then leaves the refresh to _pack)

    def _live(self, t):
        return t.dtype == torch.float32 and t.is_contiguous() and t.device == self.dev and t.untyped_storage().data_ptr() in self.own

    def _slot(self, kind, shape, dtype):
        k = (self.calls, kind)
        t = self.slots.get(k)
        if t is None or t.shape != torch.Size(shape) or t.dtype != dtype or t.device != self.dev:
            t = self.slots[k] = torch.zeros(shape, dtype=dtype, device=self.dev)
            self.moved = True
        return t

    def buffer(self, kind, shape, dtype):
        """A persistent buffer that is no parameter copy (the fragment-major Mlp pack): counts as a call of its own."""
        self.calls += 1
        return self._slot(kind, shape, dtype)

    def w16(self, t, transposed=False):
        """Weight matrix in the executor's operand type.  transposed=True: returns (address, slot of its [cols, rows] bf16 copy or None --
        the copies exist once training asked for them, in bf16 only)."""
        self.calls += 1
        t = t.detach()
        ct = None
        if self.wdt == torch.float32:
            if self._live(t):
                self.keep_alive.append(t)
                ptr = t.data_ptr()
            else:
                c = self._slot("w", t.shape, torch.float32)
                c.copy_(t)
                ptr = c.data_ptr()
            return (ptr, None) if transposed else ptr
        c = self._slot("w", t.shape, torch.bfloat16)
        if transposed and self.want_t:
            ct = self._slot("t", (t.shape[1], t.shape[0]), torch.bfloat16)
        # the fused cast kernel moves 16-byte vectors: rows must be whole vectors and start on one
        if (t.dim() == 2 and self._live(t) and t.numel() >= 4096 and t.shape[1] % 4 == 0 and t.data_ptr() % 16 == 0
                and (ct is None or t.shape[0] % 4 == 0)):
            self.fused.append((t, c, ct))
        else:
            c.copy_(t)
            self.copied = True
            if ct is not None:
                ct.copy_(t.t())
        return (c.data_ptr(), ct) if transposed else c.data_ptr()

    def folded(self, w, b, gamma):
        """Weight and bias of the Linear that ends a LayerScale branch, as the executor reads them: (address of gamma[d] * w[d, k] in the operand
        type, slot of its transposed bf16 copy or None, address of gamma o b in fp32).  Always slots, written by tr_layerscale_fold."""
        self.calls += 1
        w, b, gamma = w.detach(), b.detach(), gamma.detach()
        if not (self._live(w) and self._live(b) and self._live(gamma)):
            raise NotImplementedError("LayerScale: proj / fc2 and gamma must be fp32, contiguous parameters on the model's device")
        c = self._slot("w", w.shape, self.wdt)
        ct = self._slot("t", (w.shape[1], w.shape[0]), torch.bfloat16) if self.want_t else None
        cb = self._slot("fb", b.shape, torch.float32)
        self.folds.append((w, b, gamma, c, ct, cb))
        return c.data_ptr(), ct, cb.data_ptr()

    def f32(self, t):
        self.calls += 1
        t = t.detach()
        if self._live(t):
            self.keep_alive.append(t)
            return t.data_ptr()
        c = self._slot("f", t.shape, torch.float32)
        c.copy_(t)
        return c.data_ptr()


def _pool_code(global_pool):
    """tr_vit_config.global_pool for timm's `global_pool` argument: '' and 'token' read the CLS row, 'avg' the average of the patch tokens."""
    if global_pool in ("", "token"):
        return _lib.TR_POOL_CLS
    if global_pool == "avg":
        return _lib.TR_POOL_AVG
    raise ValueError(f"global_pool must be '', 'token' (the CLS row) or 'avg' (the average of the patch tokens), got {global_pool!r}")


class VisionTransformer(nn.Module):
    """DeiT trunk, no reduction (deit_viz.py:75-212); also the base class of the reduction models."""

    _family = _lib.TR_FAMILY_DEIT
    _blocks_last = False
    GRAPH_CACHE = 8              # captured graphs kept per workspace (one per input buffer / output set)
    # consecutive forwards with a never-seen input address before a workspace stops capturing hipGraphs: one more than the cache holds, so
    # that a caller rotating up to GRAPH_CACHE static input buffers (prefetch ring, multi-crop eval) gets through its first pass
    GRAPH_MISS_LIMIT = GRAPH_CACHE + 1
    pipeline_depth = 2           # side streams (and workspaces) of forward_async
    dynamic_width = False        # ATS only (ATSVisionTransformer)
    _always_features = False     # the residual stream after every block is recorded outside viz_mode too (the teacher's former path: tools/taps_bench.py)

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, representation_size=None, distilled=False,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., embed_layer=None, norm_layer=None,
                 act_layer=None, weight_init='', args=None, global_pool='', init_values=None, no_embed_class=False):
        super().__init__()
        _pool_code(global_pool)
        if distilled:
            # the reference's forwards only ever concatenate cls_token -- deit_viz.py:186-189 adds the [1, P + 2, D] position
            # embedding of a distilled model to P + 1 tokens (a broadcast error at the first forward), and head_dist is only created by
            # reset_classifier (deit_viz.py:178-181): a distilled model cannot run in the reference either
            raise NotImplementedError("distilled (dist_token) models are not on the hot path: the reference's own forward fails for them "
                                      "(deit_viz.py:186-189 adds a [1, P + 2, D] position embedding to P + 1 tokens)")
        if representation_size:
            raise NotImplementedError("representation_size / pre_logits is not used by any registered factory")
        if not qkv_bias:
            raise NotImplementedError("every registered factory uses qkv_bias=True")
        if act_layer not in (None, nn.GELU):
            raise NotImplementedError("only nn.GELU (erf) is implemented in the fc1 epilogue")
        if embed_dim != 64 * num_heads:
            raise ValueError("head_dim must be 64 (192/3, 384/6, 768/12 in models_act.py)")
        self.num_classes = num_classes
        self.global_pool = global_pool   # '' / 'token': the head reads the CLS row; 'avg': LayerNorm(average of the patch tokens) (timm's fc_norm)
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens = 1
        self.depth = depth
        self.num_heads = num_heads
        self.drop_rate, self.attn_drop_rate, self.drop_path_rate = drop_rate, attn_drop_rate, drop_path_rate
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.dist_token = None
        # timm's no_embed_class (DeiT-III): the position table has the patch rows only; the class token is concatenated behind the addition
        # and gets no position
        self.no_embed_class = bool(no_embed_class)
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + (0 if self.no_embed_class else self.num_tokens), embed_dim))
        self.mlp_ratio, self.qkv_bias, self._norm_layer = mlp_ratio, qkv_bias, norm_layer
        self.init_values = init_values   # timm's LayerScale: blocks[i].ls1 / ls2 (gamma [D]) scale the two branches; None / 0: no such modules
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer, init_values=init_values) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.pre_logits = nn.Identity()
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        # registration order = parameter order = the positional keys of an optimizer state_dict.  The reference's topk / evit / tome /
        # dyvit / kmedoids classes delete the base class's `blocks` and build their own AFTER norm and head exist (topk.py:150-158):
        # their parameters run patch_embed, norm, head, blocks; the other families keep timm's order (deit_viz.py:113-119)
        if self._blocks_last:
            self._modules["blocks"] = self._modules.pop("blocks")
        self.viz_mode = getattr(args, 'viz_mode', False)
        self._keep = [0] * depth
        # "bf16" = the product path; "fp32" = validation path (reference arithmetic on the GPU, VALU); "bf16x3" = the fp32 executor
        # with its Linears and attention on the matrix cores as split-bf16 products (3 MFMAs per product, ~1e-5 relative per Linear)
        self.precision = "bf16"
        self.use_graph = True        # eval forward replays a captured hipGraph (False: plain launches)
        self._pixel_input = None     # set_pixel_input(): a setting, not executor state
        self._reset_executor_state()
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        self.apply(_init_vit_weights)

    # ---- executor state ---------------------------------------------------------------------------
    def _reset_executor_state(self):
        """Every attribute the executor owns (ctypes structs, GPU workspaces with captured hipGraphs, operand copies, the tape / flat
        gradient buffer, noise buffers, side streams), at its empty value: state of THIS object's executor, rebuilt on demand.  This is
        their one declaration -- __init__ starts from it and a copy does (__deepcopy__); settings (precision, use_graph, viz_mode,
        pixel_input, the keep schedule, ...) are not in here."""
        self._packed = None              # _pack(): dict(key, W, cfg, keep_alive, gen, tblocks, tpatch)
        self._ws = {}                    # _workspace(): {B or (B, slot): dict(buf, nbytes, kept, compl, soft, feat, graphs, ...)}
        self._last_ws = None             # workspace and per-block token counts of the last forward
        self._last_tokens = None
        self._pack_slots = {}            # persistent operand copies {(call index, kind): tensor} (_Packer)
        self._pack_table = None          # device-side item table of the fused cast launch (_run_fused_pack)
        self._pack_all_fused = False     # that table covers every bf16 operand (optim.FusedAdamW may then refresh them itself)
        self._ls_fold = None             # LayerScale: dict(sig, items, shapes, n, f32) -- the item table of tr_layerscale_fold (_run_layerscale_fold)
        self._grad_rows = None           # {parameter name: rows of its gradient slot} where the declaration pads them (_grad_slot_numel)
        self._stage_t = {}               # {(block, field): transposed bf16 dgrad operand of a reduction stage} (_pack_stages)
        self._pos_table = None           # no_embed_class: the executor's [(P + 1), D] position table (row 0 zeros), a _Packer slot
        self._mlp_pack_items = None      # ([(fc1_w, fc2_w, fc2_b, pack buffer)], D, Hd) of _refresh_mlp_pack
        self._mlp_pk_stale = False       # the fragment-major Mlp copies are older than the bf16 copies
        self._want_transposed = False    # training asked for the transposed copies (dgrad operands)
        self._weights_dirty = False      # weights_changed(): values changed behind autograd's version counters
        self._dirty_by_backward = False  # ... by this model's own backward (training.py), which optim.FusedAdamW may declare clean
        self._tstate = None              # training.TrainState
        self._grad_reducer = None        # dp.py: gradient reduction overlapped with the backward
        self._pipe_streams = {}          # forward_async: {device: [side streams]}
        self._pipe_next = 0
        self._pixel_luts = None          # {device: uint8 -> normalized fp32 table}
        self._noise_bufs = {}            # {workspace slot: static buffer of the per-stage random inputs} (DPC-KNN)
        self._noise_slot = 0             # the slot of the forward being enqueued
        self._gumbel_buf = None          # DyViT training: the Gumbel draws
        self._kmed_draws = None          # K-Medoids equal_weight: the first medoids of the last forward
        self._decision_tables = {}       # Heuristic: {device: {block: int32 kept-token table}} of forward_decisions

    @property
    def _noise_buf(self):
        """The noise buffer of workspace slot 0 (model(x) and the training forward)."""
        return self._noise_bufs.get(0)

    @_noise_buf.setter
    def _noise_buf(self, buf):
        self._noise_bufs[0] = buf

    def __deepcopy__(self, memo):
        """A copy (copy.deepcopy: ModelEma, torch's swa_utils) gets parameters, buffers and settings and starts with an empty executor:
        captured torch.cuda.CUDAGraph objects cannot be deep-copied at all, and a copied workspace would not belong to the copy's own
        packed weights."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new._reset_executor_state()
        owned = set(new.__dict__)
        for k, v in self.__dict__.items():
            if k not in owned:
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    # ---- reference helper surface -------------------------------------------------------------
    def _set_keep(self, loc, k, rule):
        """Token / cluster count of the reduction at block `loc`.  0 is this package's "no reduction here" marker, so a schedule that
        rounds down to zero tokens (int(0.3**5 * 196) = 0: the reference would go on with the CLS token alone) raises instead of being
        skipped silently."""
        k = int(k)
        if k < 1:
            raise ValueError(f"block {loc}: {rule} keeps {k} tokens -- schedules that leave no patch token / cluster are not built")
        self._keep[loc] = k

    def _init_weights(self, m):
        _init_vit_weights(m)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'cls_token', 'dist_token'}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=None):
        """timm's reset_classifier: a new head of `num_classes` outputs (0: headless); global_pool '' / 'token' (the CLS row) or 'avg' (the
        average of the patch tokens, normed after the pool) changes what the head reads, None keeps the current pooling."""
        if global_pool is not None:
            _pool_code(global_pool)
            self.global_pool = global_pool
        self.num_classes = num_classes
        dev = self.pos_embed.device
        self.head = (nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()).to(dev)
        self._packed = None
        self._tstate = None          # the flat gradient buffer is laid out for the old head
        self._grad_rows = None

    def _pool_mode(self):
        """tr_vit_config.global_pool of this model (ValueError for a value written into the attribute that is none of '', 'token', 'avg')."""
        return _pool_code(self.global_pool)

    @property
    def _classes_padded(self):
        """The classifier as the kernels see it: rows padded with zeros to a multiple of 8 (any --num_classes works: NABirds 555,
        NUS-WIDE 81, train.py:334); the padded logits columns are cut off again before anything is returned."""
        return _pad8(self.num_classes)

    @property
    def _out_width(self):
        """Columns of the executor's output buffer: the padded classifier, or -- headless (num_classes == 0, head = nn.Identity()) -- the
        final-normed CLS features [B, embed_dim] (deit_viz.py:142,182, :209-212)."""
        return self._classes_padded if self.num_classes > 0 else self.embed_dim

    @property
    def _out_cols(self):
        """Columns returned to the caller: the logits, or the CLS features of a headless model."""
        return self.num_classes if self.num_classes > 0 else self.embed_dim

    def get_new_module_names(self):
        return []

    def get_reduction_count(self):
        return getattr(self, "pruning_loc", [])

    # ---- packing: bf16 weight copies + the C structs ------------------------------------------------
    def _param_key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def sync_pipeline(self):
        """Makes the caller's current stream wait for every forward that forward_async has put on its side streams.  Called before the
        operand copies are rewritten (_pack) and when the model goes to train mode; call it yourself before you modify parameters in place
        while handles may be outstanding -- like any tensor used on another stream, the weights of a forward in flight must not change under it."""
        for dev, streams in self._pipe_streams.items():
            cur = torch.cuda.current_stream(dev)
            for st in streams:
                cur.wait_stream(st)

    def train(self, mode: bool = True):
        if mode:
            self.sync_pipeline()
        return super().train(mode)

    def weights_changed(self):
        """Tell the executor that parameter VALUES changed behind autograd's version counters.  Automatic after every backward pass (an
        optimizer step follows: torch's fused optimizers -- AdamW(fused=True) -- update the parameters without bumping `_version`, which
        round 2's packing cache keyed on: the bf16 operand copies went stale and training silently ran on the initial matrices).  Call it
        yourself after writing into `p.data` through an API that does not bump versions."""
        self._weights_dirty = True
        self._dirty_by_backward = False          # (training._VitTrainFn.backward sets it after its own call: optim.FusedAdamW may clear only that)

    def _pack(self, need_transposed=False):
        """bf16 (or fp32) operand copies of every parameter the executor reads + the C structs.  The copies live in PERSISTENT buffers:
        a repack after an optimizer step rewrites them in place -- one fused launch for all matrices (tr_cast_pack_bf16), transposed
        copies for the data-gradient GEMMs included once training asked for them -- so addresses, workspaces and captured graphs survive.
        Which parameter goes into which member, in which type and padding, is read off the operand rows (Op: _trunk_units, _BLOCK_UNITS and
        the families' _stage_operands); a slot's identity is the index of its packer call, so the rows' order must not depend on values."""
        if self.precision not in ("bf16", "fp32", "bf16x3"):
            raise ValueError("precision must be 'bf16', 'bf16x3' or 'fp32'")
        self._pre_pack()
        if need_transposed:
            self._want_transposed = True
        want_t = self._want_transposed and self.precision == "bf16"
        key = (self.precision, want_t, self._pool_mode()) + self._param_key()
        if self._packed is not None and self._packed["key"] == key and not self._weights_dirty:
            return self._packed
        self.sync_pipeline()        # the operand copies are rewritten in place: no forward_async forward may still be reading them
        dev = self.pos_embed.device
        if dev.type != "cuda":
            raise RuntimeError(f"model is on {dev}: tokenreduction_amd runs on MI355X only (no CPU path); call .cuda()")
        headless = not isinstance(self.head, nn.Linear)
        if headless != (self.num_classes <= 0):
            raise RuntimeError(f"num_classes = {self.num_classes} but head is {type(self.head).__name__}: use reset_classifier() to change the head")
        wdt = torch.bfloat16 if self.precision == "bf16" else torch.float32
        pk = _Packer(self, dev, wdt, want_t)
        W = _lib.TrVitWeights()
        D = self.embed_dim
        Hd = self.blocks[0].mlp.fc1.out_features
        lib = _lib.load()
        mlp_pk_bytes = int(lib.tr_mlp_pack_bytes(D, Hd)) if lib.tr_mlp_fused_supported(D, Hd) else 0
        mlp_items = []
        named = dict(self.named_parameters())
        self._pos_table = None
        tpatch = None
        for u in self._trunk_units():
            t = self._pack_unit(pk, W, named, "", u)
            if u[0].field == "patch_w":      # (its transposed copy: the input gradient's operand, training.py)
                tpatch = t
        tblocks = []
        for i in range(self.depth):
            b = W.blocks[i]
            ts = [self._pack_unit(pk, b, named, f"blocks.{i}.", u) for u in _BLOCK_UNITS]
            tblocks.append(tuple(t for (a, _), t in zip(_BLOCK_UNITS, ts) if a.kind == "wt"))
            if wdt == torch.bfloat16 and mlp_pk_bytes:
                # the fragment-major copy of the two Mlp matrices the fused eval Mlp kernel streams (csrc/tr_mlp_fused.hip), refreshed below /
                # by _refresh_mlp_pack() whenever the bf16 copies were rewritten
                pkb = pk.buffer("p", (mlp_pk_bytes,), torch.uint8)
                b.mlp_pk = pkb.data_ptr()
                mlp_items.append((b.fc1_w, b.fc2_w, b.fc2_b, pkb))
        stages = self._pack_stages(W, pk, named)
        # may an optimizer that rewrites the fused table's copies itself declare the operands fresh?  Only if that table is all there is:
        # no copied operand, and no reduction stage whose dgrad operand is made here, at every repack
        self._pack_all_fused = not pk.copied and wdt == torch.bfloat16 and not self._stages_transposed(stages)
        if pk.fused:
            self._run_fused_pack(pk.fused, dev)
        if pk.folds:                 # before the fragment-major Mlp copies, which derive from the folded fc2 operand
            self._run_layerscale_fold(pk.folds, dev, wdt == torch.float32)
        else:
            self._ls_fold = None
        self._mlp_pack_items = (mlp_items, D, Hd)
        if self.training:
            # a repack from the training forward (every step of a non-fused optimizer, every accumulation micro-step): the train executor
            # never reads the fragment-major Mlp copies -- 12 launches and ~56 MB per step for nothing; the next eval forward refreshes them
            self._mlp_pk_stale = bool(mlp_items)
        else:
            self._refresh_mlp_pack(dev)
        cfg = _lib.TrVitConfig()
        cfg.family = self._family
        self._cfg_geometry(cfg)
        cfg.embed_dim, cfg.depth, cfg.num_heads = D, self.depth, self.num_heads
        cfg.mlp_hidden = self.blocks[0].mlp.fc1.out_features
        cfg.num_classes = self._classes_padded
        cfg.ln_eps = float(self.norm.eps)
        cfg.precision = {"bf16": _lib.TR_PREC_BF16, "fp32": _lib.TR_PREC_FP32, "bf16x3": _lib.TR_PREC_BF16X3}[self.precision]
        cfg.knn_k = int(getattr(self, "k_neighbors", 0))
        cfg.cluster_iters = int(getattr(self, "sinkhorn_iters", 0))
        cfg.sinkhorn_eps = float(getattr(self, "sinkhorn_eps", 0.0))
        cfg.global_pool = self._pool_mode()
        for i in range(self.depth):
            cfg.keep[i] = int(self._keep[i])
        old = self._packed
        gen = 1 if old is None else old.get("gen", 0) + 1
        self._packed = dict(key=key, W=W, cfg=cfg, keep_alive=pk.keep_alive, gen=gen, tblocks=tblocks if want_t else None,
                            tpatch=tpatch)
        self._weights_dirty = False
        # workspaces and captured graphs hold the operand addresses: they survive a repack unless a buffer had to be (re)allocated or the
        # configuration changed (first pack, precision switch, new head, new keep schedule)
        # ... or a LIVE pointer moved: biases, LayerNorm parameters, pos_embed / cls_token (and every weight in fp32 mode) are read through
        # the parameter's own storage, so `p.data = ...`, load_state_dict(assign=True) or an optimizer that flattens its parameters puts
        # a new address into W while every slot stays where it was -- a captured graph would keep reading the old (possibly freed) memory
        if pk.moved or old is None or bytes(old["cfg"]) != bytes(cfg) or bytes(old["W"]) != bytes(W):
            self._ws = {}
        return self._packed

    def _cfg_geometry(self, cfg):
        """The image side of tr_vit_config: img_size (the height) and img_width, the two 16-bit halves of what was one int -- a square
        image keeps img_width = 0, the bytes the int wrote -- then patch and in_chans."""
        (H, W), patch = self.patch_embed.img_size, self.patch_embed.patch_size
        if patch[0] != patch[1]:
            raise ValueError(f"patch_size {patch}: the executor takes square patches")
        if not (0 < H < 32768 and 0 < W < 32768):
            raise ValueError(f"img_size {(H, W)}: a side is outside 1 ... 32767")
        cfg.img_size, cfg.img_width, cfg.patch = H, (0 if W == H else W), patch[0]
        cfg.in_chans = self.patch_embed.proj.in_channels
        return cfg

    def _refresh_mlp_pack(self, dev=None):
        """Rewrite the fragment-major Mlp copies from the (current) bf16 operand copies: one small launch per block, in place -- after every
        _pack() refresh and, on the first eval forward after an optim.FusedAdamW step (which rewrites the bf16 copies itself and marks these
        stale), from forward()."""
        items, D, Hd = self._mlp_pack_items or ([], 0, 0)
        self._mlp_pk_stale = False
        if not items:
            return
        lib = _lib.load()
        dev = dev or items[0][3].device
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream().cuda_stream
            for w1, w2, b2, pkb in items:
                _lib.check(lib.tr_mlp_pack_bf16(w1, w2, b2, pkb.data_ptr(), D, Hd, st), "tr_mlp_pack_bf16")

    def _run_fused_pack(self, fused, dev):
        """All large matrices through ONE tr_cast_pack_bf16 launch; the item table lives on the device and is rebuilt only when an
        address changed."""
        tab = self._pack_table
        sig = tuple((t.data_ptr(), c.data_ptr(), 0 if ct is None else ct.data_ptr(), t.shape[0], t.shape[1]) for t, c, ct in fused)
        if tab is None or tab["sig"] != sig:
            items = np.zeros(len(fused), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("dst_t", "<u8"), ("rows", "<i4"), ("cols", "<i4")]))
            first = np.zeros(len(fused) + 1, dtype=np.int32)
            for n, (sp, dp, tp_, r, c) in enumerate(sig):
                items[n] = (sp, dp, tp_, r, c)
                first[n + 1] = first[n] + ((r + 63) // 64) * ((c + 63) // 64)
            tab = self._pack_table = dict(sig=sig, items=torch.from_numpy(items.view(np.uint8).copy()).to(dev),
                                          first=torch.from_numpy(first).to(dev), n=len(fused), tiles=int(first[-1]))
        with torch.cuda.device(dev):
            _lib.check(_lib.load().tr_cast_pack_bf16(tab["items"].data_ptr(), tab["first"].data_ptr(), tab["n"], tab["tiles"],
                                                     torch.cuda.current_stream().cuda_stream), "tr_cast_pack_bf16")

    def _run_layerscale_fold(self, folds, dev, f32):
        """Every folded operand of the model (2 * depth matrices, their transposed copies and biases) through ONE tr_layerscale_fold launch;
        like the cast table, the item table lives on the device and is rebuilt only when an address changed."""
        from . import ops
        tab = self._ls_fold
        sig = (f32,) + tuple((w.data_ptr(), b.data_ptr(), g.data_ptr(), c.data_ptr(), 0 if ct is None else ct.data_ptr(), cb.data_ptr(),
                              w.shape[0], w.shape[1]) for w, b, g, c, ct, cb in folds)
        if tab is None or tab["sig"] != sig:
            tab = self._ls_fold = dict(ops.layerscale_table(sig[1:], ops.LS_FOLD_ITEM, dev), sig=sig, f32=f32, dev=dev)
        self._launch_layerscale_fold()

    def _launch_layerscale_fold(self):
        tab = self._ls_fold
        with torch.cuda.device(tab["dev"]):
            _lib.check(_lib.load().tr_layerscale_fold(tab["items"].data_ptr(), tab["shapes"], tab["n"], 1 if tab["f32"] else 0,
                                                      torch.cuda.current_stream().cuda_stream), "tr_layerscale_fold")

    def _refresh_derived_operands(self):
        """The operand copies no optimizer table covers, rewritten in place from the current parameters: the LayerScale-folded proj / fc2
        operands (one tr_layerscale_fold launch) and the [(P + 1), D] position table of a no_embed_class model.  optim.FusedAdamW calls this
        behind its step, before it declares the operands fresh; a plain model has neither and launches nothing."""
        if self._ls_fold is not None:
            self._launch_layerscale_fold()
        if self._pos_table is not None:
            self._pos_table[1:].copy_(self.pos_embed.detach()[0])

    # ---- the operand declaration: rows (Op) -> W, G, WT and the gradient slot sizes -------------------------------
    def _trunk_units(self):
        """tr_vit_weights: the trunk's units.  The classifier's rows are padded to a multiple of 8; a no_embed_class model's position operand
        and gradient are [(P + 1), D] tables (row 0: zeros / scratch); a headless model has no classifier unit."""
        P, cpad = self.patch_embed.num_patches, self._classes_padded
        pad = cpad if cpad != self.num_classes else 0
        pos = dict(kind="f32_row0", rows=P + 1, grad_rows=P + 1) if self.no_embed_class else {}
        units = [(Op("patch_w", "patch_embed.proj.weight", "wt"), Op("patch_b", "patch_embed.proj.bias")),
                 (Op("cls_token", "cls_token"), Op("pos_embed", "pos_embed", **pos)),
                 (Op("norm_g", "norm.weight"), Op("norm_b", "norm.bias"))]
        if isinstance(self.head, nn.Linear):
            units.append((Op("head_w", "head.weight", "w", rows=pad, grad_rows=cpad), Op("head_b", "head.bias", rows=pad, grad_rows=cpad)))
        return units

    def _stage_operands(self, j, loc):
        """(name prefix of the stage's module, rows, scalar members) of tr_stage_weights for reduction stage j at block loc: what a family
        with operands of its own declares.  A scalar may be a callable, read when the operands are packed."""
        return "", (), {}

    def _stages(self):
        """{block: _stage_operands} of every reduction stage."""
        return {loc: self._stage_operands(j, loc) for j, loc in enumerate(self.get_reduction_count())}

    def _operand_rows(self, blocks=True):
        """Every row of the declaration as (struct, parameter name or None, row); struct: "trunk", ("blocks", i) or ("stage", block)."""
        for u in self._trunk_units():
            for r in u:
                yield "trunk", r.name, r
        for i in range(self.depth if blocks else 0):
            for u in _BLOCK_UNITS:
                for r in u:
                    yield ("blocks", i), f"blocks.{i}.{r.name}", r
        for loc, (pre, rows, _) in self._stages().items():
            for r in rows:
                yield ("stage", loc), r.name and pre + r.name, r

    def _stages_transposed(self, stages=None):
        """A reduction stage has a dgrad operand of its own (_pack_stages makes them: not something an optimizer's table refreshes)."""
        return any(r.t_rows is not None for _, rows, _ in (stages or self._stages()).values() for r in rows)

    def _pack_row(self, pk, row, src):
        """One operand through the packer: (address, slot of the packer's transposed copy or None)."""
        if row.kind == "f32_row0":
            # no_embed_class: the executor adds a [(P + 1), D] table to [cls; patches]: row 0 zeros (cls + 0 = cls), rows 1 .. P the parameter.  A slot of its
            # own (born zeros), rewritten here and by _refresh_derived_operands
            self._pos_table = pk.buffer("pe", (row.rows, src.shape[-1]), torch.float32)
            self._pos_table[1:].copy_(src.detach()[0])
            return self._pos_table.data_ptr(), None
        if src.dim() > 2:               # the convolution's weight as [D, C*p*p]; cls_token / pos_embed as rows of D
            src = src.reshape(-1, src.shape[-1]) if row.kind == "f32" else src.reshape(src.shape[0], -1)
        if row.rows or row.cols:
            src = _padded(src, row.rows, row.cols)
        if row.kind == "f32":
            return pk.f32(src), None
        return pk.w16(src, True) if row.kind == "wt" else (pk.w16(src), None)

    def _pack_unit(self, pk, S, named, pre, unit):
        """The two operands of a trunk / block unit into struct S; returns the slot of the matrix's transposed copy (or None).  LayerScale: proj and
        fc2 reach the executor with gamma folded in (csrc/tr_layerscale.hip)."""
        a, b = unit
        if a.gamma and pre + a.gamma in named:
            wa, t, wb = pk.folded(named[pre + a.name], named[pre + b.name], named[pre + a.gamma])
        else:
            (wa, t), (wb, _) = self._pack_row(pk, a, named[pre + a.name]), self._pack_row(pk, b, named[pre + b.name])
        setattr(S, a.field, wa)
        setattr(S, b.field, wb)
        return t

    def _pack_stages(self, W, pk, named=None):
        """The reduction stages' operands and scalar members (W.stage[block]) from the families' rows -- and, once training asked for transposed
        copies, the stages' dgrad operands from the same values (self._stage_t: training.TrainState.transposed points WT at them and keeps
        them alive).  Returns the stages' declaration it went through."""
        named = named or dict(self.named_parameters())
        self._stage_t = {}
        stages = self._stages()
        for loc, (pre, rows, scalars) in stages.items():
            st = W.stage[loc]
            for k, v in scalars.items():
                setattr(st, k, v() if callable(v) else v)
            for row in rows:
                if row.kind == "grad":
                    continue
                src = row.value() if row.value else named[pre + row.name]
                setattr(st, row.field, self._pack_row(pk, row, src)[0])
                if row.t_rows is not None and pk.want_t:
                    self._stage_t[loc, row.field] = _padded(src, row.t_rows or row.rows, row.cols).t().to(torch.bfloat16).contiguous()
        return stages

    def _grad_slot_numel(self, name, p):
        """fp32 elements reserved for parameter `name` in the flat gradient buffer (>= p.numel(): the rows its declaration pads the gradient to)."""
        if self._grad_rows is None:
            self._grad_rows = {n: r.grad_rows for _, n, r in self._operand_rows(blocks=False) if r.grad_rows}
        rows = self._grad_rows.get(name)
        return rows * (p.shape[-1] if p.dim() > 1 else 1) if rows else p.numel()

    def _noise_ptr(self, B, dev):
        """Device pointer of the per-stage random inputs (DPC-KNN density noise), None for deterministic families."""
        return None

    def _pre_pack(self):
        """Parameter maintenance the reference does inside forward() (Sinkhorn re-normalises its centres in place)."""

    def _per_forward_config(self, cfg):
        """Host-side random draws of a forward that the executor takes as inputs (K-Medoids equal_weight)."""

    def _soft_elems(self, B):
        """fp32 elements of the soft-assignment output (SiT), 0 for families without one."""
        return 0

    def _workspace(self, B, dev, slot=0):
        """The executor's buffers for batch size B.  slot > 0: a further, independent set (its own workspace, outputs and captured graphs) for
        a forward that is in flight beside another one (forward_async)."""
        wkey = B if slot == 0 else (B, slot)
        ws = self._ws.get(wkey)
        if ws is None:
            pk = self._packed
            nbytes = _lib.load().tr_vit_workspace_bytes(C.byref(pk["cfg"]), B)
            if nbytes == 0:
                raise RuntimeError("tr_vit_workspace_bytes rejected the model configuration (dims must be multiples of 64, "
                                   "classes of 4, head_dim 64)")
            P = self.patch_embed.num_patches
            ws = dict(buf=torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes=nbytes,
                      kept=torch.empty(self.depth * B * (P + 1), dtype=torch.int32, device=dev),
                      compl=torch.empty(self.depth * B * (P + 1), dtype=torch.int32, device=dev), soft=None)
            if self.viz_mode and self._soft_elems(B):
                ws["soft"] = torch.empty(self._soft_elems(B), dtype=torch.float32, device=dev)
            # keep one batch size resident (all of its slots)
            self._ws = {k: v for k, v in self._ws.items() if (k[0] if isinstance(k, tuple) else k) == B}
            self._ws[wkey] = ws
        return ws

    # ---- raw uint8 pixels (pixels.py) ---------------------------------------------------------------
    @property
    def pixel_input(self):
        """None, or the (mean, std) with which uint8 inputs are normalized on the device (set_pixel_input)."""
        return self._pixel_input

    def set_pixel_input(self, mean=pixels.IMAGENET_DEFAULT_MEAN, std=pixels.IMAGENET_DEFAULT_STD):
        """Opt-in: a uint8 input [B, C, H, W] -- contiguous (NCHW) or torch.channels_last (NHWC), read in place -- is taken as raw pixels and
        normalized inside the kernels that read the image, bitwise as if the fp32 tensor of torchvision's ToTensor() + Normalize(mean, std)
        had been passed.  Float inputs are unaffected.  set_pixel_input(None) turns it off (a uint8 tensor is then cast to fp32 as before).
        mean and std have in_chans entries.  Not a buffer: state_dict() stays the reference's; copy.deepcopy keeps the setting."""
        new = None if mean is None else pixels.check_mean_std(mean, std, self.patch_embed.proj.in_channels)
        if new != self.pixel_input:
            self.sync_pipeline()          # the old table may still be read by forwards in flight on forward_async's side streams
            self._pixel_luts = None
        self._pixel_input = new
        return self

    def _executor_input(self, x: torch.Tensor):
        """(image tensor, TR_INPUT_* format, LUT pointer or None) of the executor for input x."""
        if self.pixel_input is None or x.dtype != torch.uint8:
            return x.detach().to(torch.float32).contiguous(), _lib.TR_INPUT_F32, None
        x, fmt = pixels.as_executor_input(x, self.patch_embed.proj.in_channels)
        luts = self._pixel_luts
        if luts is None:
            luts = self._pixel_luts = {}
        if x.device not in luts:                       # one table per device, built at its first uint8 forward
            luts[x.device] = pixels.pixel_lut(*self.pixel_input).to(x.device)
        return x, fmt, luts[x.device].data_ptr()

    # ---- training state (flat gradient buffer, tape, workspaces): training.py -----------------------
    def _train_state(self):
        st = self._tstate
        if st is None or st.flat.device != self.pos_embed.device or len(st.order) != len(list(self.parameters())):
            from . import training
            st = self._tstate = training.TrainState(self)
        return st

    # ---- forward ------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor):
        if isinstance(x, AugmentedBatch) and not (self.training and self.pixel_input is not None):
            x = x.float()         # eval, the teacher, pixel input off: the augmented fp32 image, then the float path
        if self.training:
            # engine.py:50-51 `output = model(samples)` in train mode: logits with the HIP backward behind them (training.py)
            from . import training
            return training.train_forward(self, x)
        return self._forward_eval(x, 0)

    def _eval_request(self, x, what, cls_blocks=None, final_tokens=False, decisions=False, dense=None, dynamic_width_ok=False):
        """The EvalRequest of the public entry `what` -- every entry builds its request here -- or the refusal: eval_request.REFUSALS' checks
        of the request's feature, the first that applies wins.  dense: forward_dense's keywords (any subset), which stand alone."""
        feature = "dense" if dense is not None else "decisions" if decisions else "taps"
        applies = {"train": self.training, "viz_mode": self.viz_mode, "dynamic_width": self.dynamic_width and not dynamic_width_ok,
                   "cpu": not x.is_cuda}
        for check, message in REFUSALS[feature].items():
            if check != "args":
                if applies[check]:
                    raise RuntimeError(message.format(what=what, device=x.device))
            elif dense is not None:
                request = EvalRequest(None, False, False, *self._dense_arguments(**dict(dense)))
            else:
                blocks = None
                if cls_blocks is not None or final_tokens:
                    blocks = tuple(sorted({int(b) for b in (cls_blocks or ())}))
                    if blocks and not (0 <= blocks[0] and blocks[-1] < self.depth):
                        raise ValueError(f"cls_blocks {blocks} names a block outside 0 ... {self.depth - 1}")
                request = EvalRequest(blocks, bool(final_tokens), bool(decisions))
        return request

    def forward_taps(self, x: torch.Tensor, cls_blocks=(3, 6, 9, 11), final_tokens=False):
        """Eval forward with output taps: (logits, {"cls", "blocks", "final_tokens"}).  taps["cls"] is fp32 [B, n, D]: the CLS row of the
        residual stream after each block of `cls_blocks` (ascending, listed in taps["blocks"]) -- bit for bit what viz_mode's
        viz_data["Features"][blk][:, 0] holds (extract_cls_features.py:113-132), None for an empty set.  final_tokens=True adds
        taps["final_tokens"], fp32 [B, N_last, D]: the final norm of every row after the last block in fp32 arithmetic (norm(x) of the DyViT
        teacher, dyvit.py:325-334).  The taps stay on the device and the forward stays on the fast path: hipGraph replay, lazy norms and --
        unless final_tokens asks for every row of the last block -- the CLS tail; the logits are those of model(x).  Refuses train mode,
        viz_mode and a block index outside 0 ... depth-1."""
        if isinstance(x, AugmentedBatch):
            x = x.float()
        return self._forward_eval(x, 0, self._eval_request(x, "forward_taps", tuple(cls_blocks or ()), final_tokens, dynamic_width_ok=True))

    def forward_decisions(self, x: torch.Tensor, cls_blocks=None, final_tokens=False):
        """Eval forward with decision taps: (logits, dec), dec = {"stages": (blk, ...), "kept": {blk: int32 [B, W]}, "kept_count": {blk: int32
        [B]}, "assign": {blk: int32 [B, P_in]}} -- per reduction stage what validate.py stores in an image's `Stage-{loc}` record: the kept
        tokens as ABSOLUTE patch indices of the input grid (-1 behind a row's kept_count valid entries) and the stage-relative assignment map;
        a family has one, the other or both (harness.decision_records turns a row into the record).  Device tensors, written by one launch
        (tr_stage_decisions) behind the forward, which stays on the fast path; the logits are those of model(x).  With cls_blocks /
        final_tokens the output taps of forward_taps ride along: (logits, taps, dec).  Refuses train mode, viz_mode, dynamic_width."""
        if isinstance(x, AugmentedBatch):
            x = x.float()
        return self._forward_eval(x, 0, self._eval_request(x, "forward_decisions", cls_blocks, final_tokens, decisions=True))

    _DENSE_FORMATS = ("NCHW", "NHWC")

    def _dense_arguments(self, output_fmt="NCHW", dtype=torch.float32, fill=0.0, blocks=None, norm=True):
        """(DenseOutput, Levels or None) of forward_dense's keywords: the blocks ascending and counted from the front."""
        if output_fmt not in self._DENSE_FORMATS:
            raise ValueError(f"output_fmt must be one of {self._DENSE_FORMATS}, got {output_fmt!r}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        if self.patch_embed.num_patches > 1024 or self.embed_dim % 4 or self.embed_dim > 1024:
            raise ValueError(f"dense feature maps take at most 1024 patches and a width that is a multiple of 4 up to 1024 "
                             f"({self.patch_embed.num_patches} patches, width {self.embed_dim})")
        out = DenseOutput(output_fmt, dtype, float(fill))
        if blocks is None:
            return out, None
        if isinstance(blocks, (int, np.integer)):
            blocks = (blocks,)
        asked = [int(b) for b in blocks]
        if not asked:
            raise ValueError("blocks is empty: name at least one block (blocks=None is the last block's map)")
        if any(not -self.depth <= b < self.depth for b in asked):
            raise ValueError(f"blocks {tuple(asked)} names a block outside {-self.depth} ... {self.depth - 1}")
        levels = sorted(b % self.depth for b in asked)
        if len(set(levels)) != len(levels):
            raise ValueError(f"blocks {tuple(asked)} names a block twice")
        return out, Levels(tuple(levels), bool(norm))

    def forward_dense(self, x: torch.Tensor, blocks=None, norm=True, output_fmt="NCHW", dtype=torch.float32, fill=0.0):
        """Eval forward with a dense feature map: (logits, {"features", "index", "grid": (h, w)}).  `features` is the final norm of the last
        block's rows (the final_tokens tap, fp32 arithmetic) put back on the input's patch grid: [B, D, h, w] for output_fmt "NCHW", [B, h, w,
        D] for "NHWC", fp32 or bf16 (dtype; round to nearest even of the fp32 value).  `index` int32 [B, h * w] names, per grid patch, the row of
        the reduced stream (1 ... N_last-1) that stands for it -- the stages' decisions composed on the device (tr_dense_index): an
        assignment map sends a patch to the row it was merged into (ToMe, DPC-KNN, K-Medoids; the hard argmax map for the soft families), a
        kept list to its position in the list.  A patch no row stands for has index -1 and `fill` in every channel: the patches a pruning
        family dropped, and the patches EViT put into its fused token (the fused token is not followed; it is nobody's row).  DeiT and
        Heuristic keep every row: the index is the identity.  The forward is that of forward_decisions(final_tokens=True) with two more
        launches (tr_dense_index, tr_dense_gather) in the same stream and the same captured graph; the request is part of the graph key and
        the logits are those of model(x).  The map and the index are static buffers per workspace slot, allocated on the first dense call
        (at 512 x 512 inputs, DeiT-B width and batch 256 the fp32 map is about 0.8 GB per slot) and cloned out like the taps.  The taps and
        decision records themselves are not returned: ask forward_decisions for them.
        blocks=(...) asks for the maps of chosen blocks instead (ints in [-depth, depth), negative ones count from the end, no duplicates;
        results in ascending block order): (logits, {"features": [L maps], "index": [L int32 [B, h * w]], "blocks", "grid", "cls": fp32 [B, L,
        D]}).  Level l is the stream after block blocks[l] -- every row, with the residuals pending there, bit for bit the rows of viz_mode's
        Features[blocks[l]] -- through the model's final norm (norm=True) or as it stands (norm=False), put on the grid by the decisions of
        the stages at or before that block: a block in front of every stage has the identity as its index.  `cls` is row 0 of each level.
        The forward stays on the fast path (tr_vit_forward_levels: one launch per level where its CLS tap would run; the CLS tail stays unless
        the last block is asked for), followed by tr_stage_decisions and ONE tr_dense_index_levels and ONE tr_dense_gather_levels for all
        levels; blocks and norm are part of the graph key.  blocks=None is the call described first, unchanged.
        A soft-weighted un-merge and following EViT's fused token are not built; in train mode the same maps, each with a gradient, are
        forward_dense_train's.  Refuses train mode, viz_mode, dynamic_width and a block out of range."""
        if isinstance(x, AugmentedBatch):
            x = x.float()
        dense = dict(output_fmt=output_fmt, dtype=dtype, fill=fill, blocks=blocks, norm=norm)
        return self._forward_eval(x, 0, self._eval_request(x, "forward_dense", dense=dense))

    def forward_dense_train(self, x: torch.Tensor, blocks=None, norm=True, output_fmt="NCHW", dtype=torch.float32, fill=0.0):
        """Training forward with a dense feature map that carries a gradient: (out, {"features", "index", "grid"}).  `out` is what model(x)
        returns in train mode (the logits, or the CLS features of a headless model), bit for bit; the dictionary has the shapes, layouts,
        dtypes and index / fill semantics of eval's forward_dense (the last block's final-normed rows, single level).  `features` is the
        second output of the SAME autograd node as `out`: any loss on it, on `out`, or on both drives loss.backward() into the parameters
        through the HIP backward -- tr_dense_scatter (the gather's adjoint) takes the map's gradient back to the token rows, and
        tr_vit_backward_dense adds the final norm's backward of every row to the stream gradient.  Gradient accumulation, frozen units, a
        gradient reducer's block ranges, DropPath and dropout, uint8 and augmented inputs, x.grad and the one-tape guard behave as for
        model(x).  `index` carries no gradient; a patch without a row shows `fill` and receives none.  The buffers (rows, stream, decision
        slabs, index, map) are one set per model, like the tape; the map and the index are cloned out.
        blocks=(...) asks for the maps of chosen blocks (validated as in forward_dense: ints in [-depth, depth), no duplicates, not empty;
        results in ascending block order): (out, {"features": [L maps], "index": [L int32 [B, h * w]], "blocks", "grid", "cls": fp32 [B, L,
        D]}).  Level l is the stream after block blocks[l]: every row with the residual pending there -- the training forward's own branch,
        DropPath-scaled and dropout-masked, summed in fp32 -- through the model's final norm in fp32 arithmetic (norm=True) or as it stands
        (norm=False), placed on the grid by the decisions of the stages at or before that block.  Every map is a further output of the same
        autograd node: a loss on any subset of the maps and / or `out` drives ONE loss.backward() -- one tr_dense_scatter_levels launch for
        the maps that have a gradient, then tr_vit_backward_levels, which injects each level's gradient into the stream gradient in front of
        its block (norm=True: the final norm's backward over the level's rows, which also adds to norm.weight.grad / norm.bias.grad;
        norm=False: one add launch).  A map without a gradient costs no scatter work and no injection; with no map gradient at all the
        backward is model(x)'s.  `index` and `cls` carry no gradient (`cls` is a detached copy of row 0 of each level).  Memory, one set per
        model and (B, L, norm) beside the tape: with norm=True a level costs two fp32 slabs of B * N0 * D (the summed stream and its norm),
        with norm=False one (the gather's operand; the backward needs nothing more); plus per level one token-gradient slab (bf16 / fp32),
        the index and the map.  blocks=None is the call described first, unchanged.
        Refuses eval mode (use forward_dense), viz_mode, a CPU input, dynamic_width, a precision other than bf16, DyViT and a block out of
        range.  A gradient through `cls`, a differentiable eval forward, a soft-weighted un-merge and following EViT's fused token are not
        built."""
        applies = {"eval": not self.training, "viz_mode": self.viz_mode, "cpu": not x.is_cuda, "dynamic_width": self.dynamic_width,
                   "precision": self.precision != "bf16", "dyvit": self._family == _lib.TR_FAMILY_DYVIT}
        dense = levels = None
        for check, message in DENSE_TRAIN_REFUSALS.items():
            if check == "args":
                dense, levels = self._dense_arguments(output_fmt=output_fmt, dtype=dtype, fill=fill, blocks=blocks, norm=norm)
            elif applies[check]:
                exc = NotImplementedError if check in ("precision", "dyvit") else RuntimeError
                raise exc(message.format(what="forward_dense_train", device=x.device))
        if isinstance(x, AugmentedBatch) and self.pixel_input is None:
            x = x.float()         # pixel input off: the augmented fp32 image, then the float path (as forward does)
        from . import training
        return training.train_forward(self, x, dense, levels)

    def get_intermediate_layers(self, x: torch.Tensor, n=1, reshape=False, return_class_token=False, norm=False, dtype=torch.float32, fill=0.0):
        """timm's VisionTransformer.get_intermediate_layers on the fast path: the patch tokens after the last `n` blocks (int n) or after the
        blocks `n` names (a sequence; negative entries count from the end), in ascending block order -- a tuple of [B, h * w, D] tensors, of
        [B, D, h, w] with reshape=True; norm=True applies the model's final norm; with return_class_token a tuple of (tokens, cls [B, D])
        pairs.  A thin wrapper over forward_dense(blocks=...), with its refusals.  Unlike a dense ViT, a reduced stream has no row for every
        patch: a patch whose row was pruned (or went into EViT's fused token) shows `fill` in every channel, and the patches merged into one
        row all show that row."""
        blocks = tuple(range(self.depth - int(n), self.depth)) if isinstance(n, (int, np.integer)) else tuple(n)
        if isinstance(n, (int, np.integer)) and not 1 <= int(n) <= self.depth:
            raise ValueError(f"n = {n}: the model has {self.depth} blocks")
        _, out = self.forward_dense(x, blocks=blocks, norm=norm, output_fmt="NCHW" if reshape else "NHWC", dtype=dtype, fill=fill)
        B, D = x.shape[0], self.embed_dim
        feats = out["features"] if reshape else [f.view(B, -1, D) for f in out["features"]]
        if return_class_token:
            return tuple((f, out["cls"][:, l]) for l, f in enumerate(feats))
        return tuple(feats)

    def forward_async(self, x: torch.Tensor, cls_blocks=None, final_tokens=False, decisions=False, dense=None):
        """Eval forward that may run BESIDE the previous one: the call enqueues the forward on one of `pipeline_depth` (default 2) side streams
        -- each with its own workspace and captured hipGraph -- behind everything already enqueued on the caller's current stream, and
        returns a handle at once; `handle.result()` makes the caller's current stream wait for that forward and returns what `model(x)`
        would.  Forwards on different side streams are independent launches sequences, so the device fills the tail of one forward's launches
        (partial last rounds of the persistent GEMM-class kernels, the short launches of the last stage) with the other's: the headline
        forward runs 2.65 -> 2.44 ms per batch of 256 with two in flight (tools/lab/two_stream_full.py).  A data loop uses it with one batch
        of lookahead (harness.evaluate_multiclass does): launch batch k + 1, then consume batch k.  Same kernels, same bits as `model(x)`.
        Train mode, viz_mode and ATS's dynamic width run synchronously (the handle is already complete).
        cls_blocks / final_tokens: the output taps of forward_taps -- the result is then what forward_taps returns.  With taps, train mode,
        viz_mode and dynamic_width are refused instead of run synchronously.  decisions=True: the decision taps of forward_decisions, with
        the same refusals -- the result is what forward_decisions returns.  dense=dict(output_fmt=..., dtype=..., fill=..., blocks=...,
        norm=...) (any subset; {} for the defaults): the dense feature map(s) of forward_dense, with its refusals -- the result is what
        forward_dense returns; it does not combine with the other keywords."""
        if isinstance(x, AugmentedBatch):
            x = x.float()
        asked = decisions or cls_blocks is not None or final_tokens
        if dense is not None and asked:
            raise ValueError("forward_async: dense= does not combine with cls_blocks / final_tokens / decisions")
        if dense is not None or asked:
            what = "forward_async" + ("(dense=...)" if dense is not None else "(decisions=True)" if decisions else "")
            request = self._eval_request(x, what, cls_blocks, final_tokens, decisions, dense)
        elif self.training or self.viz_mode or self.dynamic_width or not x.is_cuda:
            return _Pending(self(x), None)
        else:
            request = EvalRequest()
        depth = max(1, int(self.pipeline_depth))
        st = self._pipe_streams
        key = x.device
        if key not in st or len(st[key]) != depth:
            st[key] = [torch.cuda.Stream(device=x.device) for _ in range(depth)]
        slot = self._pipe_next % depth
        self._pipe_next = slot + 1
        side = st[key][slot]
        cur = torch.cuda.current_stream(x.device)
        self._pack()                                   # (re)pack on the caller's stream, where the optimizer / loader wrote
        if self._mlp_pk_stale:
            self._refresh_mlp_pack(x.device)
        side.wait_stream(cur)                          # inputs and weights are ready where the forward runs
        with torch.cuda.stream(side):
            out = self._forward_eval(x, slot + 1, request)
            done = torch.cuda.Event()
            done.record(side)
        x.record_stream(side)
        return _Pending(out, done)

    def _forward_eval(self, x: torch.Tensor, slot: int, request: EvalRequest = EvalRequest()):
        """One eval forward on workspace slot `slot`: the request's static buffers, then the executor call and the request's launches behind
        it -- as one hipGraph replay where the workspace allows, plain launches otherwise -- then the request's result."""
        if not x.is_cuda:
            raise RuntimeError(REFUSE_CPU.format(device=x.device))
        pk = self._pack()
        if self._mlp_pk_stale:
            self._refresh_mlp_pack(x.device)
        cfg = pk["cfg"]
        B, Cc, Hh, Ww = x.shape
        if (Cc, Hh, Ww) != (cfg.in_chans, *cfg.image_hw):
            raise ValueError(f"expected [B, C, H, W] = [B,{cfg.in_chans},{cfg.image_hw[0]},{cfg.image_hw[1]}], got {tuple(x.shape)}")
        image = self._executor_input(x)
        x = image[0]
        ws = self._workspace(B, x.device, slot)
        out = self._request_buffers(ws, request, B, x.device)
        self._noise_slot = slot                      # (a static buffer per workspace slot: two forwards in flight must not share one)
        noise_ptr = self._noise_ptr(B, x.device)
        self._kmed_draws = None
        self._per_forward_config(cfg)
        cfg.concurrent = 1 if slot > 0 else 0        # forward_async: other forwards run beside this one (a scheduling hint, same bits)

        def launch(logits):
            tokens = self._launch_executor(pk, ws, out, image, noise_ptr, logits, B)
            self._launch_outputs(ws, request, out, tokens, B)
            return list(tokens)

        with torch.cuda.device(x.device):
            res = None
            if (self.use_graph and not ws.get("graph_off") and not torch.cuda.is_current_stream_capturing()
                    and not self.dynamic_width):      # (ATS dynamic width: the executor reads a token count back mid-forward)
                key = (x.data_ptr(), x.dtype, *image[1:], out.features is not None, ws.get("soft") is not None, noise_ptr, self._kmed_draws,
                       self._out_width) + request.graph_key()
                res = self._replay(ws, key, launch, B, x.device)
            logits, tokens = res if res is not None else self._plain_launch(launch, B, x.device)
        cfg.concurrent = 0                           # (the packed configuration is compared byte-wise on a repack: leave no per-call state in it)
        self._last_tokens = list(tokens)
        self._last_ws = ws
        return self._eval_result(ws, request, out, logits, list(tokens), B)

    def _request_buffers(self, ws, req, B, dev):
        """The outputs of a request beside the logits -- static per workspace slot like every other output, allocated by the first request that
        asks for them -- and the executor's structs over them: features (viz_data["Features"]: the stream after every block, upper bound depth
        * B * N0 * D fp32), soft, taps (a TrVitTaps or None: the CLS taps [B, n, D] with room for every block, the final tokens [B, N0, D]),
        dec (the decision plan or None), and for a dense request maps = ws["levels"][L] (per level count; 0: the single map of the
        final_tokens tap): the level slabs [L, B * N0 * D] fp32, the indices [L, B, P0] and one map buffer per output dtype (either layout is
        L * B * P0 * D elements), of which feat is the request's; levels is the TrVitLevels over the slabs (zeroed: no level taps)."""
        D, P0 = self.embed_dim, self.patch_embed.num_patches
        empty = lambda n, dtype=torch.float32: torch.empty(n, dtype=dtype, device=dev)
        if self.viz_mode and self._soft_elems(B) and ws.get("soft") is None:      # viz_mode switched on after the first call
            ws["soft"] = empty(self._soft_elems(B))
        out = types.SimpleNamespace(features=None, soft=ws.get("soft"), taps=None, dec=None, maps=None, feat=None, levels=_lib.TrVitLevels())
        if (self.viz_mode or self._always_features) and req.taps is None:
            if ws.get("feat") is None:
                ws["feat"] = empty(self.depth * B * (P0 + 1) * D)
            out.features = ws["feat"]
        if req.taps is not None:
            blocks, final = req.taps
            if blocks and ws.get("tap_cls") is None:
                ws["tap_cls"] = empty(B * self.depth * D)
            if final and ws.get("tap_final") is None:
                ws["tap_final"] = empty(B * (P0 + 1) * D)
            out.taps = _lib.TrVitTaps(sum(1 << b for b in blocks), ws["tap_cls"].data_ptr() if blocks else None,
                                      ws["tap_final"].data_ptr() if final else None)
        if req.wants_decisions:
            out.dec = self._decision_plan(ws, B, dev)
            if out.dec["soft"] is not None:
                out.soft = out.dec["soft"]             # (a buffer of its own: ws["soft"] stays viz_mode's)
        if req.dense is not None:
            L = len(req.levels.blocks) if req.levels is not None else 0
            out.maps = ws.setdefault("levels", {}).get(L)
            if out.maps is None:
                out.maps = ws["levels"][L] = dict(tokens=empty(L * B * (P0 + 1) * D) if L else None, index=empty(max(L, 1) * B * P0, torch.int32),
                                                  feat={})
            out.feat = out.maps["feat"].get(req.dense.dtype)
            if out.feat is None:
                out.feat = out.maps["feat"][req.dense.dtype] = empty(max(L, 1) * B * P0 * D, req.dense.dtype)
            if L:
                out.levels = _lib.TrVitLevels(sum(1 << b for b in req.levels.blocks), int(req.levels.norm), out.maps["tokens"].data_ptr(),
                                              out.maps["tokens"].numel())
        return out

    def _launch_executor(self, pk, ws, out, image, noise_ptr, logits, B):
        """The eval path's one executor call -> the token count after every block.  tr_vit_forward_levels is the superset entry point: a float
        image is TR_INPUT_F32 without a LUT, no output taps a NULL tr_vit_taps, no level taps a zeroed tr_vit_levels."""
        x, fmt, lut = image
        tokens = (C.c_int * self.depth)()
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = _lib.load().tr_vit_forward_levels(C.byref(pk["cfg"]), C.byref(pk["W"]), x.data_ptr(), fmt, lut, logits.data_ptr(), ws["buf"].data_ptr(),
                                               ws["nbytes"], ws["kept"].data_ptr(), ws["compl"].data_ptr(), ptr(out.soft), noise_ptr,
                                               ptr(out.features), tokens, B, torch.cuda.current_stream().cuda_stream,
                                               None if out.taps is None else C.byref(out.taps), C.byref(out.levels))
        _lib.check(rc, "tr_vit_forward")
        return tokens

    def _launch_outputs(self, ws, req, out, tokens, B):
        """The request's launches behind the executor, in the forward's stream (and its graph): the raw decision slabs -> record form
        (tr_stage_decisions), then for a dense request the decisions composed into one row per grid patch and the un-reduce -- of the
        final_tokens tap, or of every level at once (the _levels forms: every level's prefix of the decisions)."""
        lib, dec, stream = _lib.load(), out.dec, torch.cuda.current_stream().cuda_stream
        D, P0 = self.embed_dim, self.patch_embed.num_patches
        if dec is not None and dec["n"]:
            rc = lib.tr_stage_decisions(ws["kept"].data_ptr(), ws["compl"].data_ptr(), ws["kept"].numel(), dec["soft_ptr"], dec["soft_elems"],
                                        dec["table"], dec["n"], B, P0 + 1, dec["kept_ptr"], dec["kept_elems"], dec["count_ptr"],
                                        dec["assign_ptr"], dec["assign_elems"], stream)
            _lib.check(rc, "tr_stage_decisions")
        if req.dense is None:
            return
        records = (dec["kept_ptr"], dec["kept_elems"], dec["assign_ptr"], dec["assign_elems"], dec["table"], dec["n"], B, P0)
        layout = (_lib.TR_LAYOUT_NCHW if req.dense.fmt == "NCHW" else _lib.TR_LAYOUT_NHWC, int(req.dense.dtype == torch.bfloat16), req.dense.fill)
        index, feat = out.maps["index"].data_ptr(), out.feat.data_ptr()
        if req.levels is None:
            n_last = tokens[self.depth - 1]
            _lib.check(lib.tr_dense_index(*records, n_last, index, stream), "tr_dense_index")
            _lib.check(lib.tr_dense_gather(ws["tap_final"].data_ptr(), index, feat, *layout, B, P0, n_last, D, stream), "tr_dense_gather")
        else:
            L = len(req.levels.blocks)
            blocks, rows = (C.c_int32 * L)(*req.levels.blocks), (C.c_int32 * L)(*[tokens[b] for b in req.levels.blocks])
            _lib.check(lib.tr_dense_index_levels(*records, blocks, rows, L, index, stream), "tr_dense_index_levels")
            _lib.check(lib.tr_dense_gather_levels(out.maps["tokens"].data_ptr(), B * (P0 + 1) * D, rows, L, index, feat, *layout, B, P0, D, stream),
                       "tr_dense_gather_levels")

    def _eval_result(self, ws, req, out, logits, tokens, B):
        """What the request's entry returns, one section per output kind.  Every output is cloned out of its static buffer in stream order, the
        way a replay's logits are: the next forward on this slot overwrites them."""
        D, dec = self.embed_dim, out.dec
        if req.dense is not None:
            if dec["static"] is None and not dec["checked"]:
                self._decision_result(dec, B, tokens)           # (the stage table against the executor's token counts, once per workspace)
            (h, w), levels = self.patch_embed.grid_size, req.levels
            n = len(levels.blocks) if levels is not None else 1
            feat = out.feat.clone().view((n, B, D, h, w) if req.dense.fmt == "NCHW" else (n, B, h, w, D))
            index = out.maps["index"].clone().view(n, B, h * w)
            if levels is None:
                return logits, {"features": feat[0], "index": index[0], "grid": (h, w)}
            # row 0 of every level's [B, N_l, D] rows: a strided copy out of the static slabs
            slabs = out.maps["tokens"].view(n, -1)
            cls = torch.stack([slabs[l, :B * tokens[b] * D].view(B, tokens[b], D)[:, 0] for l, b in enumerate(levels.blocks)], dim=1)
            return logits, {"features": list(feat), "index": list(index), "blocks": levels.blocks, "grid": (h, w), "cls": cls}
        result = (logits,)
        if req.taps is not None:
            blocks, final = req.taps
            result += ({"cls": ws["tap_cls"][:B * len(blocks) * D].view(B, len(blocks), D).clone() if blocks else None, "blocks": blocks,
                        "final_tokens": ws["tap_final"][:B * tokens[-1] * D].view(B, tokens[-1], D).clone() if final else None},)
        if dec is not None:
            result += (self._decision_result(dec, B, tokens),)
        if len(result) > 1:
            return result
        if self.viz_mode:
            viz = self._viz_data(ws, B, tokens)
            viz["Features"] = self._features(ws, B, tokens)
            return logits, viz
        return logits

    def _plain_launch(self, launch, B, dev):
        """The forward as plain launches into a fresh output buffer: (logits without the padded classifier columns, tokens per block)."""
        logits = torch.empty(B, self._out_width, dtype=torch.float32, device=dev)
        tokens = launch(logits)
        if self._out_width != self._out_cols:
            logits = logits[:, :self._out_cols].contiguous()
        return logits, tokens

    def _replay(self, ws, key, launch, B, dev):
        """The forward as ONE hipGraph replay: (logits, tokens), or None when this workspace has gone back to plain launches.
        The forward is a fixed sequence of ~90-130 dependent launches with no host decision in between: it is captured once per batch size /
        input buffer / output set (`key`; the workspace and every output are static buffers) and kept in ws["graphs"], at most GRAPH_CACHE
        per workspace, oldest out first.  Re-packing the weights or a new batch size drops the workspace and its graphs with it.
        A capture bakes the input ADDRESS in.  Callers whose batches arrive at a new address every time (a dtype / layout conversion, a
        loader without a static buffer, K-Medoids --equal_weight with its per-forward draws) would re-capture on every call -- slower
        than not using a graph at all: after GRAPH_MISS_LIMIT misses in a row the workspace goes back to plain launches (at batch 256
        within 0.5 % of the replay; bench.py ms_per_step_plain_launches)."""
        graphs = ws.setdefault("graphs", {})
        ent = graphs.get(key)
        if ent is not None:
            ws["graph_misses"] = 0
        else:
            ws["graph_misses"] = ws.get("graph_misses", 0) + 1
            if graphs and ws["graph_misses"] >= self.GRAPH_MISS_LIMIT:
                ws["graph_off"] = True
                graphs.clear()
                warnings.warn(f"{type(self).__name__}: {self.GRAPH_MISS_LIMIT} forwards in a row came with a new input address (or new "
                              "per-forward draws); hipGraph replay is off for this batch size -- keep the input in one static "
                              "buffer to get it back (model.use_graph = False silences this)", RuntimeWarning, stacklevel=4)
                return None
            out = torch.empty(B, self._out_width, dtype=torch.float32, device=dev)
            if not ws.get("warm"):
                launch(out)                                   # eager once per workspace: first touch, lazy module load
                ws["warm"] = True
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                toks = launch(out)
            if len(graphs) >= self.GRAPH_CACHE:
                graphs.pop(next(iter(graphs)))
            ent = graphs[key] = (g, out, toks)
        g, out, toks = ent
        g.replay()
        return out[:, :self._out_cols].clone(), toks

    def check_status(self):
        """Status check of the eval forwards since the last call (tr_vit_forward_status): waits for the stream and raises RuntimeError if
        the device recorded a failure that no launch status can show -- the fused Mlp's stream-K hand-over poll running out (the logits
        of that forward are invalid).  The forward itself never synchronises; call this where the logits are consumed
        (harness.evaluate_multiclass / validate and bench.py do)."""
        if self._packed is None:
            return
        for wkey, ws in list(self._ws.items()):
            if "buf" not in ws:
                continue
            B = wkey[0] if isinstance(wkey, tuple) else wkey
            with torch.cuda.device(ws["buf"].device):
                torch.cuda.synchronize()                   # every stream a forward may have run on (forward_async's side streams)
                _lib.check(_lib.load().tr_vit_forward_status(C.byref(self._packed["cfg"]), ws["buf"].data_ptr(), ws["nbytes"], B,
                                                             torch.cuda.current_stream().cuda_stream), "tr_vit_forward_status")

    def _viz_data(self, ws, B, tokens):
        return {}

    # ---- decision taps (forward_decisions): the stage table of tr_stage_decisions and its static output buffers ---------------------
    def _decision_stages(self):
        """[(blk, TR_DECISION_* kind, n_in, k)] of the stages that decide on the device, in block order (n_in: tokens entering the stage, CLS
        included; k as tr_stage_decisions reads it).  The shapes are static: the executor's token counts are checked against them."""
        return []

    def _static_decisions(self, B, dev):
        """Decisions that do not depend on the image (Heuristic): the dec dictionary, or None."""
        return None

    def _decision_plan(self, ws, B, dev):
        """ws["dec"]: the stage table, where every stage's rows lie in the outputs, and the static buffers -- kept / assign (int32, the
        stages' [B, W] / [B, P_in] blocks back to back), count [S, B], and for the soft families a soft-assignment buffer of its own."""
        dec = ws.get("dec")
        if dec is not None:
            return dec
        stages = self._decision_stages()
        if len(stages) > _lib.TR_MAX_DECISION_STAGES:
            raise ValueError(f"{len(stages)} reduction stages: the decision taps take at most {_lib.TR_MAX_DECISION_STAGES}")
        from . import ops
        table, layout, kept_n, assign_n, soft_n = ops.decision_table(stages, B)
        if soft_n != self._soft_elems(B):
            raise RuntimeError(f"the soft stages hold {soft_n} elements, the executor writes {self._soft_elems(B)}")
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev) if n else None
        dec = ws["dec"] = dict(table=table, n=len(stages), layout=layout, kept=i32(kept_n), assign=i32(assign_n), count=i32(max(1, len(stages) * B)),
                               soft=torch.empty(soft_n, dtype=torch.float32, device=dev) if soft_n else None,
                               static=self._static_decisions(B, dev), checked=False)
        ptr = lambda t: None if t is None else t.data_ptr()
        size = lambda t: 0 if t is None else t.numel()
        # the buffers as tr_stage_decisions and the dense index launches take them: address and element count, NULL and 0 where a family has none
        for name in ("soft", "kept", "assign"):
            dec[name + "_ptr"], dec[name + "_elems"] = ptr(dec[name]), size(dec[name])
        dec["count_ptr"] = dec["count"].data_ptr()
        return dec

    def _decision_result(self, dec, B, tokens):
        """The dec dictionary of forward_decisions: views of ONE clone per static buffer (the next forward on this slot overwrites them)."""
        if dec["static"] is not None:
            return dec["static"]
        if not dec["checked"]:
            n0 = self.patch_embed.num_patches + 1
            for blk, n_in, *_ in dec["layout"]:
                if n_in != (tokens[blk - 1] if blk else n0):
                    raise RuntimeError(f"block {blk}: the stage table expects {n_in} tokens, the executor had {tokens[blk - 1] if blk else n0}")
            dec["checked"] = True
        kept = None if dec["kept"] is None else dec["kept"].clone()
        assign = None if dec["assign"] is None else dec["assign"].clone()
        count = dec["count"].clone() if dec["n"] else None
        out = {"stages": tuple(lay[0] for lay in dec["layout"]), "kept": {}, "kept_count": {}, "assign": {}}
        for i, (blk, n_in, W, koff, A, aoff) in enumerate(dec["layout"]):
            if W:
                out["kept"][blk] = kept[koff: koff + B * W].view(B, W)
                out["kept_count"][blk] = count[i * B: (i + 1) * B]
            if A:
                out["assign"][blk] = assign[aoff: aoff + B * A].view(B, A)
        return out

    _features_every_block = True

    def _feature_blocks(self, tokens):
        """Blocks whose output the reference records in viz_data["Features"]: every block (deit_viz.py:199, sit.py:130), or --
        families that reduce inside a block -- the blocks that reduced plus the last one (topk.py:195-200 and alike)."""
        if self._features_every_block:
            return list(range(self.depth))
        n_in, out = self.patch_embed.num_patches + 1, {self.depth - 1}
        for blk, n in enumerate(tokens):
            k = self._keep[blk]
            if self._family in (_lib.TR_FAMILY_TOPK, _lib.TR_FAMILY_EVIT):
                reduced = k > 0 and k != n_in - 1                      # topk.py:57: left_tokens == N-1 returns idx None
            elif self._family == _lib.TR_FAMILY_TOME:
                reduced = min(k, (n_in - 1) // 2) > 0
            else:
                reduced = k > 0
            if reduced:
                out.add(blk)
            n_in = n
        return sorted(out)

    def _features(self, ws, B, tokens):
        D = self.embed_dim
        want = set(self._feature_blocks(tokens))
        feats, off = {}, 0
        for blk in range(self.depth):
            n = B * tokens[blk] * D
            if blk in want:
                feats[blk] = ws["feat"][off: off + n].reshape(B, tokens[blk], D).cpu().numpy()
            off += n
        return feats

    def _stage_slab(self, arr, blk, B, n):
        """[B, n] int64: the first B * n entries of block `blk`'s slab in a per-stage index output (ws["kept"], ws["compl"])."""
        base = blk * B * (self.patch_embed.num_patches + 1)
        return arr[base: base + B * n].reshape(B, n).astype(np.int64)

    def _stage_indices(self, ws, B, tokens):
        """Per reduction block: (blk, N_in, K) from the static per-stage shapes."""
        P = self.patch_embed.num_patches
        out = []
        n_in = P + 1
        for i in range(self.depth):
            K = self._keep[i]
            if K and K != n_in - 1:
                out.append((i, n_in, K))
            n_in = tokens[i]
        return out


class _TopKBase(VisionTransformer):
    """Shared ctor logic of topk.py:108-171 / evit.py:138-201."""
    _blocks_last = True

    _features_every_block = False

    def __init__(self, *a, args=None, dyvit_distillation=False, **kw):
        super().__init__(*a, args=args, **kw)
        pruning_loc = list(args.reduction_loc)
        token_ratio = _expand_schedule(args.keep_rate, pruning_loc, lambda r, idx: r ** (idx + 1), ("pruning", "token ratios"))   # topk.py:141-142
        self.num_patches = self.patch_embed.num_patches
        self.deit_distillation = False
        self.pruning_loc = pruning_loc
        self.token_ratio = token_ratio
        for r, loc in zip(token_ratio, pruning_loc):
            assert 0 < r <= 1, "keep_rate must > 0 and <= 1, got {0}".format(r)   # topk.py:39
            self.blocks[loc].attn.keep_rate = r
            if r < 1:
                self._set_keep(loc, int(r * 196), f"int({r:.4g} * 196) (topk.py:56, 196 hard-coded)")
            else:
                self._keep[loc] = 0
        self._check_static_shapes()

    def _check_static_shapes(self):
        n = self.num_patches + 1
        for i in range(self.depth):
            K = self._keep[i]
            if K and K != n - 1:
                if not 1 <= K < n - 1:
                    raise ValueError(f"block {i}: cannot keep {K} of {n - 1} patch tokens")
                n = self._tokens_after(K)

    def get_reduction_count(self):
        return self.pruning_loc

    def _decision_stages(self):
        kind = _lib.TR_DECISION_EVIT if self._family == _lib.TR_FAMILY_EVIT else _lib.TR_DECISION_PRUNE
        out, n = [], self.num_patches + 1
        for blk in range(self.depth):
            K = self._keep[blk]
            if K and K != n - 1:                                        # (topk.py:57: left_tokens == N-1 reduces nothing)
                out.append((blk, kind, n, K))
                n = self._tokens_after(K)
        return out


class TopKVisionTransformer(_TopKBase):
    """models/topk.py:102-212."""
    _family = _lib.TR_FAMILY_TOPK

    def _tokens_after(self, K):
        return K + 1

    def _viz_data(self, ws, B, tokens):
        kept = ws["kept"].cpu().numpy()
        decisions = {blk: self._stage_slab(kept, blk, B, K) for blk, n_in, K in self._stage_indices(ws, B, tokens)}
        return {"Kept_Tokens": decisions, "Features": {}}


class EfficientVisionTransformer(_TopKBase):
    """models/evit.py:132-244."""
    _family = _lib.TR_FAMILY_EVIT

    def _tokens_after(self, K):
        return K + 2

    def _viz_data(self, ws, B, tokens):
        kept = ws["kept"].cpu().numpy()
        compl = ws["compl"].cpu().numpy()
        decisions, fusion = {}, {}
        for blk, n_in, K in self._stage_indices(ws, B, tokens):
            decisions[blk] = np.concatenate([self._stage_slab(kept, blk, B, K), -np.ones((B, 1), dtype=np.int64)], axis=1)   # evit.py:123
            fusion[blk] = self._stage_slab(compl, blk, B, n_in - 1 - K)
        return {"Kept_Tokens": decisions, "Fusion_Assign": fusion, "Features": {}}


class ToMeVisionTransformer(VisionTransformer):
    """models/tome.py:107-223: bipartite soft matching + size-weighted merge between attention and MLP, proportional attention."""
    _blocks_last = True
    _family = _lib.TR_FAMILY_TOME

    _features_every_block = False

    def __init__(self, *a, args=None, **kw):
        super().__init__(*a, args=args, **kw)
        pruning_loc = list(args.reduction_loc)
        P0 = self.patch_embed.num_patches
        token_ratio = _expand_schedule(args.keep_rate, pruning_loc, lambda r, idx: int(P0 * r ** (idx + 1)), ("pruning", "token ratios"))   # tome.py:145-146
        # explicit values are ABSOLUTE patch-token counts; the CLI delivers floats, which crash the reference's slicing
        #  -- cast to int here
        token_ratio = [int(t) for t in token_ratio]
        prev = P0
        for t, loc in zip(token_ratio, pruning_loc):                                                        # tome.py:152-155
            self._keep[loc] = prev - t
            self.blocks[loc].r = prev - t
            prev = t
        if any(k < 0 for k in self._keep):
            raise ValueError(f"ToMe token counts must be non-increasing, got {token_ratio}")
        self.num_patches = P0
        self.deit_distillation = False
        self.pruning_loc = pruning_loc
        self.token_ratio = token_ratio
        self.prop_attn = True

    def get_reduction_count(self):
        return self.pruning_loc

    def _decision_stages(self):
        out, n = [], self.patch_embed.num_patches + 1
        for blk in range(self.depth):
            r = min(self._keep[blk], (n - 1) // 2)
            if r > 0 and blk in self.pruning_loc:
                out.append((blk, _lib.TR_DECISION_TOME, n, r))
            n -= max(r, 0)
        return out

    def _viz_data(self, ws, B, tokens):
        """Assignment_Maps[blk] (tome.py:91-99): for every input patch token, the index of its output token minus 1 -- derived
        from the device's (unm, src, dst) instead of pushing a B*N*N identity through the merge like the reference does."""
        N0 = self.patch_embed.num_patches + 1
        slab = ws["kept"].cpu().numpy()
        maps = {}
        n_in = N0
        for blk in range(self.depth):
            r = min(self._keep[blk], (n_in - 1) // 2)
            if r > 0 and blk in self.pruning_loc:
                na, nb = (n_in + 1) // 2, n_in // 2
                base = blk * B * N0
                unm = slab[base: base + B * (na - r)].reshape(B, na - r).astype(np.int64)
                src = slab[base + B * (na - r): base + B * na].reshape(B, r).astype(np.int64)
                dst = slab[base + B * na: base + B * (na + r)].reshape(B, r).astype(np.int64)
                pos_a = np.zeros((B, na), dtype=np.int64)
                np.put_along_axis(pos_a, unm, np.broadcast_to(np.arange(na - r), (B, na - r)), axis=1)
                np.put_along_axis(pos_a, src, (na - r) + dst, axis=1)
                out = np.empty((B, n_in), dtype=np.int64)
                out[:, 0::2] = pos_a
                out[:, 1::2] = (na - r) + np.arange(nb)
                maps[blk] = (out - 1)[:, 1:]
            n_in = tokens[blk]
        return {"Assignment_Maps": maps, "Features": {}}


def _pad_rows(w, rows):
    return _padded(w, rows)


def _pad_cols(w, cols):
    return _padded(w, 0, cols)


def _pad_vec(b, n):
    return _padded(b, n)


def _ln_default(dim):
    return nn.LayerNorm(dim)          # eps 1e-5: the reduction modules use nn.LayerNorm's default (dyvit.py:97, sit.py:30)


class PredictorLG(nn.Module):
    """Parameter holder with the reference's module tree (dyvit.py:90-110); evaluated by the HIP executor."""

    def __init__(self, embed_dim=384, eps=1e-6):
        super().__init__()
        self.in_conv = nn.Sequential(_ln_default(embed_dim), nn.Linear(embed_dim, embed_dim), nn.GELU())
        self.out_conv = nn.Sequential(nn.Linear(embed_dim, embed_dim // 2), nn.GELU(), nn.Linear(embed_dim // 2, embed_dim // 4),
                                      nn.GELU(), nn.Linear(embed_dim // 4, 2), nn.LogSoftmax(dim=-1))
        self.eps = eps


class DynamicVisionTransformer(VisionTransformer):
    """models/dyvit.py:122-263.  Eval: per pruning block, PredictorLG scores the patch tokens, the best int(P0*ratio) are gathered
    (argsort order) BEFORE the block runs.  Training (dyvit.py:221-229): no token is removed; a straight-through Gumbel-softmax
    sample of the scores becomes the keep policy every later block attends under, and forward returns
    (logits, out_pred_prob) or, with dyvit_distillation, (logits, features, prev_decision, out_pred_prob) (dyvit.py:257-261)."""
    _blocks_last = True
    _family = _lib.TR_FAMILY_DYVIT

    _features_every_block = False

    def __init__(self, *a, args=None, dyvit_distillation=False, **kw):
        distilled = kw.pop("distilled", False)
        super().__init__(*a, args=args, **kw)
        assert (dyvit_distillation & distilled) is False, "Cannot have both DeiT Distillation token and DyViT Distillation scheme"
        if distilled:
            raise NotImplementedError("the distillation token is not built")
        pruning_loc = list(args.reduction_loc)
        token_ratio = _expand_schedule(args.keep_rate, pruning_loc, lambda r, idx: r ** (idx + 1), ("pruning", "token ratios"))   # dyvit.py:175-176
        self.num_patches = self.patch_embed.num_patches
        self.score_predictor = nn.ModuleList([PredictorLG(self.embed_dim) for _ in range(len(pruning_loc))])
        for m in self.score_predictor.modules():
            _init_vit_weights(m)
        for ratio, loc in zip(token_ratio, pruning_loc):
            self._set_keep(loc, int(self.num_patches * ratio), f"int({self.num_patches} * {ratio:.4g}) (dyvit.py:232)")
        self.deit_distillation = False
        self.dyvit_distillation = dyvit_distillation
        self.pruning_loc = pruning_loc
        self.token_ratio = token_ratio

    def get_new_module_names(self):
        return ["score_predictor"]

    # ---- training (dyvit.py:221-229, 257-261) ------------------------------------------------------------------
    gumbel_noise = None      # tests: {stage: tensor [B,P,2]} = the reference's -log(Exp(1)) draws; None = drawn on the device

    def _gumbel_ptr(self, B, dev):
        P, n_st = self.num_patches, len(self.pruning_loc)
        buf = self._gumbel_buf
        if buf is None or buf.numel() != n_st * B * P * 2 or buf.device != dev:
            buf = self._gumbel_buf = torch.empty(n_st * B * P * 2, dtype=torch.float32, device=dev)
        if self.gumbel_noise is not None:
            buf.copy_(torch.cat([self.gumbel_noise[j].to(device=dev, dtype=torch.float32).reshape(-1) for j in range(n_st)]))
        else:
            buf.exponential_().log_().neg_()          # F.gumbel_softmax: -empty_like(logits).exponential_().log()
        return buf.data_ptr()

    def get_reduction_count(self):
        return self.pruning_loc

    def _hidden_pad(self):
        """The predictor's hidden widths D/2 and D/4 as the kernels see them, padded with zero weights: K % 64 for the bf16 GEMMs
        (DeiT-T: 96 -> 128); the training path's GEMMs reduce over the D/4 rows too."""
        return _pad64(self.embed_dim // 2), _pad64(self.embed_dim // 4)

    def _stage_operands(self, j, loc):
        hh, qq = self._hidden_pad()      # (w0 .. w2 have a backward: transposed copies of the operands as padded)
        rows = (Op("ln_g", "in_conv.0.weight"), Op("ln_b", "in_conv.0.bias"),
                Op("w0", "in_conv.1.weight", "w", t_rows=0), Op("b0", "in_conv.1.bias"),
                Op("w1", "out_conv.0.weight", "w", rows=hh, t_rows=0), Op("b1", "out_conv.0.bias", rows=hh),
                Op("w2", "out_conv.2.weight", "w", rows=qq, cols=hh, t_rows=0), Op("b2", "out_conv.2.bias", rows=qq),
                Op("w3", "out_conv.4.weight"), Op("b3", "out_conv.4.bias"))
        return f"score_predictor.{j}.", rows, dict(h_pad=hh, reserved_=qq)

    def _viz_data(self, ws, B, tokens):
        kept = ws["kept"].cpu().numpy()
        return {"Kept_Tokens": {blk: self._stage_slab(kept, blk, B, self._keep[blk]) for blk in self.pruning_loc}, "Features": {}}

    def _decision_stages(self):
        out, n = [], self.patch_embed.num_patches + 1
        for blk in sorted(self.pruning_loc):
            out.append((blk, _lib.TR_DECISION_PRUNE, n, self._keep[blk]))
            n = self._keep[blk] + 1
        return out


class _ClusterBase(VisionTransformer):
    """Shared part of the five families that replace the patch tokens by cluster_count[j] tokens BEFORE block cluster_loc[j] through a
    module cluster_layers[j] -- SiT, DPC-KNN, Sinkhorn, K-Medoids, PatchMerger: one schedule rule (sit.py:80-81, dpcknn.py:214-215,
    sinkhorn.py:128-129, patchmerger.py:78-79) and one constructor order; a family adds its own settings in _cluster_settings and its
    module in _make_cluster_layer."""

    def __init__(self, *a, args=None, **kw):
        super().__init__(*a, args=args, **kw)
        P0 = self.patch_embed.num_patches
        self.cluster_loc = list(args.reduction_loc)
        self.cluster_count = [int(c) for c in _expand_schedule(args.keep_rate, self.cluster_loc, lambda r, idx: int(P0 * r ** (idx + 1)),
                                                               ("cluster", "cluster centers"))]
        self._cluster_settings(args)
        self.cluster_layers = nn.ModuleList([self._make_cluster_layer(c) for c in self.cluster_count])
        for m in self.cluster_layers.modules():
            _init_vit_weights(m)
        for c, loc in zip(self.cluster_count, self.cluster_loc):
            self._set_keep(loc, c, "the cluster schedule")

    def _cluster_settings(self, args):
        """The family's own constructor arguments (read before its modules are built)."""

    def _make_cluster_layer(self, count):
        raise NotImplementedError

    def get_new_module_names(self):
        return ["cluster_layers"]

    def get_reduction_count(self):
        return self.cluster_loc

    def _stage_shapes(self):
        """[(blk, K, P_in)] per clustering stage, in block order."""
        out, p_in = [], self.patch_embed.num_patches
        for K, loc in sorted(zip(self.cluster_count, self.cluster_loc), key=lambda t: t[1]):
            out.append((loc, K, p_in))
            p_in = K
        return out

    _decision_kind = _lib.TR_DECISION_CENTRES

    def _decision_stages(self):
        return [(blk, self._decision_kind, P + 1, K) for blk, K, P in self._stage_shapes()]

    def _viz_data(self, ws, B, tokens):
        """Hard clusterings (DPC-KNN, K-Medoids): the centre tokens and every input token's cluster."""
        kept, assign = ws["kept"].cpu().numpy(), ws["compl"].cpu().numpy()
        decisions, assignments = {}, {}
        for blk, K, P in self._stage_shapes():
            decisions[blk] = self._stage_slab(kept, blk, B, K)
            assignments[blk] = self._stage_slab(assign, blk, B, P)
        return {"Kept_Tokens": decisions, "Assignment_Maps": assignments, "Center_Feats": {}, "Features": {}}


class TokenSlimmingModule(nn.Module):
    """Parameter holder (sit.py:25-34)."""

    def __init__(self, embed_dim, cluster_centers, ratio=0.5):
        super().__init__()
        hidden_dim = int(embed_dim * ratio)
        self.weight = nn.Sequential(_ln_default(embed_dim), nn.Linear(embed_dim, hidden_dim), nn.GELU(),
                                    nn.Linear(hidden_dim, cluster_centers))
        self.scale = nn.Parameter(torch.ones(1, 1, 1))


class SelfSlimmedVisionTransformer(_ClusterBase):
    """models/sit.py:43-150: a TokenSlimmingModule softly assigns the patch tokens to K outputs before each block in
    reduction_loc."""
    _family = _lib.TR_FAMILY_SIT
    _center_feats = False            # viz_data carries an (empty) "Center_Feats" entry (sinkhorn.py / patchmerger.py)
    _decision_kind = _lib.TR_DECISION_SOFT

    def _make_cluster_layer(self, count):
        return TokenSlimmingModule(self.embed_dim, count)

    def _stage_operands(self, j, loc):
        m = self.cluster_layers[j]
        n_pad, ld = self._soft_pad(self.cluster_count[j])
        hh = _pad64(m.weight[1].out_features)     # hidden width padded with zero weights (DeiT-T: 96 -> 128)
        rows = (Op("ln_g", "weight.0.weight"), Op("ln_b", "weight.0.bias"),
                Op("w0", "weight.1.weight", "w", rows=hh, t_rows=0), Op("b0", "weight.1.bias", rows=hh),
                # the last Linear's rows are padded to a multiple of 8 by the weight-gradient kernel too (rows >= K receive zeros)
                Op("w1", "weight.3.weight", "w", rows=n_pad, cols=hh, grad_rows=n_pad, t_rows=ld), Op("b1", "weight.3.bias", rows=n_pad, grad_rows=n_pad),
                Op("b2", "scale", "grad"))       # the operand is the scalar member; d scale (sit.py:34), fp32[1], lands in b2
        return f"cluster_layers.{j}.", rows, dict(scale=lambda: float(m.scale.detach().reshape(-1)[0]), n_pad=n_pad, h_pad=hh)

    def _soft_pad(self, K):
        """(rows, leading dimension of the transposed copy) of a soft-assignment matrix with K outputs, as the kernels pad them."""
        return _pad8(K), _pad64(K)

    def _soft_elems(self, B):
        return sum(B * K * P for _, K, P in self._stage_shapes())

    def _viz_data(self, ws, B, tokens):
        soft = ws["soft"].cpu().numpy()
        assignments, hard = {}, {}
        off = 0
        for blk, K, P in self._stage_shapes():
            a = soft[off: off + B * K * P].reshape(B, K, P)
            off += B * K * P
            assignments[blk] = a
            hard[blk] = np.argmax(a, axis=-2).astype(np.int64)                       # sit.py:122
        out = {"Assignment_Maps": hard, "Soft_Assignment_Maps": assignments, "Features": {}}
        if self._center_feats:
            out["Center_Feats"] = {}
        return out


class CTM(nn.Module):
    """Parameter holder (dpcknn.py:143-151)."""

    def __init__(self, embed_dim, cluster_num, k=5, equal_weight=False):
        super().__init__()
        self.cluster_num, self.equal_weight, self.k = cluster_num, equal_weight, k
        if not self.equal_weight:
            self.score = nn.Linear(embed_dim, 1)


class DPCKNNVisionTransformer(_ClusterBase):
    """models/dpcknn.py:175-290: before each block in reduction_loc the patch tokens are clustered by DPC-KNN and every cluster
    is replaced by the exp(score)-weighted mean of its tokens.

    The reference adds `torch.rand * 1e-6` to the densities (dpcknn.py:71-72).  Here the draws come from torch.rand on the
    device each forward, or from `self.density_noise = {blk: tensor[B,P_in]}` when set (tests feed the reference's draws)."""
    _family = _lib.TR_FAMILY_DPCKNN

    def _cluster_settings(self, args):
        self.k_neighbors = int(args.k_neighbors)
        self.equal_weight = bool(args.equal_weight)
        self.density_noise = None

    def _make_cluster_layer(self, count):
        return CTM(self.embed_dim, count, self.k_neighbors, self.equal_weight)

    def _stage_operands(self, j, loc):
        if self.equal_weight:            # (no score layer: CTM registers none)
            return "", (), {}
        return f"cluster_layers.{j}.", (Op("w3", "score.weight"), Op("b3", "score.bias")), {}

    def _noise_ptr(self, B, dev):
        shapes = self._stage_shapes()
        n = sum(B * P for _, _, P in shapes)
        buf = self._noise_bufs.get(self._noise_slot)                                 # forward_async: one buffer per forward in flight
        if buf is None or buf.numel() != n or buf.device != dev:
            # static: a captured forward reads this address
            buf = self._noise_bufs[self._noise_slot] = torch.empty(n, dtype=torch.float32, device=dev)
        if self.density_noise is not None:
            parts = [self.density_noise[blk].to(device=dev, dtype=torch.float32).reshape(B, P) for blk, _, P in shapes]
            buf.copy_(torch.cat([t.reshape(-1) for t in parts]))
        else:
            buf.uniform_()                                                           # torch.rand: [0, 1)
        return buf.data_ptr()


class ATSVisionTransformer(VisionTransformer):
    """models/ats.py:166-271: blocks in reduction_loc sample tokens by inverse-transform sampling on the CLS attention weighted
    by the value norms.  The reference's token count after such a block is data dependent (batch maximum of unique samples,
    ats.py:78); here it is the static bound K = sample_count, the surplus rows being masked keys (zero attention weight), which
    leaves every valid token and the logits unchanged.  Kept_Tokens is trimmed to the reference's batch-maximum width.

    `model.dynamic_width = True` (eval only, opt-in) makes the executor do what the reference does: after every sampling block it reads the
    batch maximum of unique ids back (one int, a stream synchronisation; no hipGraph replay) and runs the rest of the network on that many
    tokens -- fewer rows in every later block, the same valid tokens (tr_vit_config.ats_dynamic)."""
    _family = _lib.TR_FAMILY_ATS

    _features_every_block = False

    def _per_forward_config(self, cfg):
        super()._per_forward_config(cfg)
        cfg.ats_dynamic = 1 if (self.dynamic_width and not self.training) else 0

    def __init__(self, *a, args=None, **kw):
        super().__init__(*a, args=args, **kw)
        self.sample_loc = list(args.reduction_loc)
        P0 = self.patch_embed.num_patches
        sample_count = _expand_schedule(args.keep_rate, self.sample_loc, lambda r, idx: int(r ** (idx + 1) * P0) + 1,
                                        ("sample", "sample centers"))                                     # ats.py:204-205
        cnt = 0
        self.sample_count = [0] * self.depth
        for idx in range(self.depth):
            if idx in self.sample_loc:
                self.sample_count[idx] = int(sample_count[cnt])
                if self.sample_count[idx] < 1:
                    raise ValueError(f"block {idx}: the sampling schedule keeps {self.sample_count[idx]} tokens -- schedules that leave no patch token are not built")
                cnt += 1
        # static token bound of a sampling block: one token per grid point + CLS.  The grid (ats.py:48) is a float arange with an
        # exclusive end; for 42 sample counts up to 197 (7, 12, 14, ..., 126, ...) rounding admits the end point: K points, bound K + 1
        self._keep = [int(self.sample_steps(k).numel()) + 1 if k else 0 for k in self.sample_count]

    def get_reduction_count(self):
        return self.sample_loc

    @staticmethod
    def sample_steps(sample_count):
        """ats.py:48, verbatim."""
        return torch.arange(1 / (2 * sample_count), (2 * sample_count - 1) / (2 * sample_count), 2 / (2 * sample_count))

    def _stage_operands(self, j, loc):
        steps = lambda: self.sample_steps(self.sample_count[loc]).to(self.pos_embed.device)
        return "", (Op("w3", value=steps, grad=False),), dict(n_pad=self._keep[loc] - 1)       # (_keep: one token per grid point + CLS)

    def _decision_stages(self):
        out, n = [], self.patch_embed.num_patches + 1
        for blk, K in enumerate(self._keep):
            if K:
                out.append((blk, _lib.TR_DECISION_ATS, n, K))
                n = K
        return out

    def _viz_data(self, ws, B, tokens):
        kept = ws["kept"].cpu().numpy()
        decisions = {}
        for blk, K in enumerate(self._keep):
            if K:
                ids = self._stage_slab(kept, blk, B, K)
                width = int((ids[:, 1:] != 0).sum(axis=1).max())                      # pad_sequence to the batch maximum, ats.py:78
                decisions[blk] = ids[:, 1:1 + width] - 1                              # ats.py:253
        return {"Kept_Tokens": decisions, "Features": {}}


class Sinkhorn(nn.Module):
    """Parameter holder (sinkhorn.py:59-64): cluster centres v ~ N(0, 1)."""

    def __init__(self, embed_dim, cluster_centers, eps, iters):
        super().__init__()
        self.v = nn.Parameter(torch.randn(cluster_centers, embed_dim))
        self.eps, self.iters = eps, iters


class SinkhornVisionTransformer(SelfSlimmedVisionTransformer):
    """models/sinkhorn.py:89-200: before each block in reduction_loc the unit-norm patch tokens are softly assigned to K
    unit-norm learned centres by `cluster_iters` log-domain Sinkhorn iterations; outputs are assignment-weighted sums of the
    unit-norm tokens.  (The reference re-normalises `v` in place every forward, sinkhorn.py:73-76; here the normalised copy is
    made when the weights are packed and the parameter is left untouched.)"""
    _family = _lib.TR_FAMILY_SINKHORN
    _center_feats = True

    def _cluster_settings(self, args):
        self.sinkhorn_eps = float(args.sinkhorn_eps)
        self.sinkhorn_iters = int(args.cluster_iters)

    def _make_cluster_layer(self, count):
        return Sinkhorn(self.embed_dim, count, self.sinkhorn_eps, self.sinkhorn_iters)

    def _pre_pack(self):
        if self.training:                       # sinkhorn.py:72-76: the centres are re-normalised IN PLACE (no grad) at every forward
            with torch.no_grad():
                for m in self.cluster_layers:
                    m.v.copy_(torch.nn.functional.normalize(m.v, p=2, dim=-1))

    def _stage_operands(self, j, loc):
        v = self.cluster_layers[j].v
        n_pad, ld = self._soft_pad(self.cluster_count[j])
        # the operand is the unit-norm v, made once per repack for both copies; the gradient reaches v as if it were the unit vector (sinkhorn.py:76-77)
        rows = (Op("w1", "v", "w", rows=n_pad, grad_rows=n_pad, t_rows=ld, value=lambda: torch.nn.functional.normalize(v.detach().float(), p=2, dim=-1)),
                Op("b1", value=lambda: torch.zeros(n_pad, dtype=torch.float32, device=v.device), grad=False))
        return f"cluster_layers.{j}.", rows, dict(n_pad=n_pad)


class KMedoids(nn.Module):
    """kmedoids.py:135-149 (no parameters)."""

    def __init__(self, num_clusters, iters, equal_weights=False):
        super().__init__()
        self.cluster_count, self.iters, self.equal_weights = num_clusters, iters, equal_weights


class KMedoidsVisionTransformer(_ClusterBase):
    """models/kmedoids.py:152-272: before each block in reduction_loc the patch tokens are clustered by weighted K-Medoids
    (weights = column sums of the previous block's attention) and replaced by the medoid tokens themselves."""
    _blocks_last = True
    _family = _lib.TR_FAMILY_KMEDOIDS

    def _cluster_settings(self, args):
        self.num_patches = self.patch_embed.num_patches
        self.sinkhorn_iters = self.cluster_iters = int(args.cluster_iters)      # cfg.cluster_iters carries it to the executor
        self.equal_weight = bool(args.equal_weight)
        if 0 in self.cluster_loc:
            raise ValueError("kmedoids cannot reduce before block 0: there is no previous attention (kmedoids.py:240)")

    def _make_cluster_layer(self, count):
        return KMedoids(count, self.cluster_iters, self.equal_weight)

    def _per_forward_config(self, cfg):
        """args.equal_weight (kmedoids.py:43-47): every k_medoids_fit call draws its first medoid with
        `np.random.choice(np.arange(N), 1)` from numpy's GLOBAL generator -- drawn here, stage by stage in forward order, so a
        seeded run consumes the stream exactly like the reference; the executor takes the ids as inputs (and a captured graph is
        keyed on them through the noise key below)."""
        if not self.equal_weight:
            return
        draws = []
        for loc, _, p_in in self._stage_shapes():
            first = int(np.random.choice(np.arange(p_in), 1)[0])
            cfg.kmed_init[loc] = first + 1
            draws.append(first)
        self._kmed_draws = tuple(draws)


class PatchMerger(nn.Module):
    """Parameter holder (patchmerger.py:24-33)."""

    def __init__(self, embed_dim, cluster_centers, scaled_attention=False):
        super().__init__()
        self.scale = embed_dim ** -0.5 if scaled_attention else 1.
        self.norm = _ln_default(embed_dim)
        self.queries = nn.Parameter(torch.randn(cluster_centers, embed_dim))


class PatchMergerVisionTransformer(SelfSlimmedVisionTransformer):
    """models/patchmerger.py:42-150: before each block in reduction_loc, K learned queries attend over the LayerNorm-ed patch
    tokens (softmax over the tokens) and the outputs are the attention-weighted sums of the normalised tokens."""
    _family = _lib.TR_FAMILY_PATCHMERGER
    _center_feats = True

    def _make_cluster_layer(self, count):
        return PatchMerger(self.embed_dim, count)

    def _stage_operands(self, j, loc):
        m = self.cluster_layers[j]
        n_pad, ld = self._soft_pad(self.cluster_count[j])
        rows = (Op("ln_g", "norm.weight"), Op("ln_b", "norm.bias"), Op("w1", "queries", "w", rows=n_pad, grad_rows=n_pad, t_rows=ld),
                Op("b1", value=lambda: torch.zeros(n_pad, dtype=torch.float32, device=m.queries.device), grad=False))
        return f"cluster_layers.{j}.", rows, dict(scale=float(m.scale), n_pad=n_pad)


class HeuristicVisionTransformer(VisionTransformer):
    """models/heuristic.py:88-277: image-independent spatial pruning.  From every block in the reduction range on, the patch
    tokens farther than that block's radius (L1 / L2 / Linf distance from the grid centre) are masked as attention keys; no
    token is removed.  The radii are constructor-time geometry (prep_pattern / prep_pattern_stage_subset), computed on the
    host exactly as the reference does.  (The reference also masks those tokens as QUERIES, which turns their rows into the
    mean of V; here they attend like everyone else -- rows nothing ever reads: they stay masked as keys to the end.)"""
    _family = _lib.TR_FAMILY_HEURISTIC
    _features_every_block = False

    def __init__(self, *a, args=None, **kw):
        super().__init__(*a, args=args, **kw)
        self.heuristic_pattern = args.heuristic_pattern
        gh, gw = self.patch_embed.grid_size
        if gh != gw:
            raise ValueError(f"{type(self).__name__}: img_size {self.patch_embed.img_size} gives a {gh} x {gw} patch grid, but the heuristic's "
                             "distance grid is built on sqrt(num_patches) points per side (heuristic.py:158-162): a square grid only")
        if args.not_contiguous:
            self.reduction_loc = list(args.reduction_loc)
            self.keep_rate = list(args.keep_rate)
            if len(self.keep_rate) != 1:
                raise ValueError("heuristic with --not_contiguous defines its token targets for a single keep_rate only "
                                 "(heuristic.py:127-128)")
            num_tokens = [int(self.patch_embed.num_patches * self.keep_rate[0] ** (idx + 1)) for idx in range(len(self.reduction_loc))]
            self.distances, self.threshold, self.P = self.prep_pattern_stage_subset(num_tokens)
        else:
            self.min_radius = args.min_radius
            self.start_stage = int(min(args.reduction_loc))
            self.end_stage = int(max(args.reduction_loc))
            self.reduction_loc = [idx for idx in range(self.start_stage, self.end_stage + 1)]
            self.distances, self.threshold, self.P = self.prep_pattern()

    # ---- constructor-time geometry: one radius per block, a patch is visible while its distance to the grid centre is within it
    _NORMS = {"l1": lambda u, v: u.abs() + v.abs(), "l2": lambda u, v: (u * u + v * v).sqrt(), "linf": lambda u, v: torch.maximum(u.abs(), v.abs())}

    def _patch_radii(self):
        """[g, g] distance of every patch to the centre of the patch grid, in the norm named by --heuristic_pattern.  The grid
        coordinates are the reference's (g evenly spaced values from floor(-g/2) to floor(g/2), heuristic.py:158-162) so the
        radii -- and with them every mask -- are the same floats."""
        norm = self._NORMS.get(str(self.heuristic_pattern).lower())
        if norm is None:
            raise ValueError(f"heuristic_pattern {self.heuristic_pattern!r}: expected l1 | l2 | linf")
        g = int(self.patch_embed.num_patches ** 0.5)
        axis = torch.linspace((-g) // 2, g // 2, steps=g)
        return norm(axis[:, None].expand(g, g), axis[None, :].expand(g, g)), g

    def prep_pattern(self):
        """Contiguous range (heuristic.py:157-181): the radius shrinks linearly from the corner distance (everything visible) one
        block before the range to `min_radius` one block after it, and stays constant outside."""
        radii, g = self._patch_radii()
        if self.min_radius is None or self.min_radius <= 0:
            self.min_radius = radii[g // 2, g // 2]
        corner = float(radii[0, 0])
        n_stage = self.end_stage - self.start_stage + 1
        ramp = torch.linspace(corner, float(self.min_radius), n_stage + 2)            # ramp[0] = all visible, ramp[-1] = min_radius
        # the ramp starts one block BEFORE the range -- except for a range that starts at block 0, where the reference's left padding is
        # empty (F.pad(..., max(start_stage - 1, 0)), heuristic.py:178) and block 0 itself still sees everything
        pos = (torch.arange(self.depth + 2) - max(self.start_stage - 1, 0)).clamp(0, n_stage + 1)
        return radii, ramp[pos], g

    def prep_pattern_stage_subset(self, num_tokens):
        """Listed blocks only (heuristic.py:184-224): each stage takes, among the distinct radii of the grid, the one whose disc
        covers a patch count closest to its target (the smaller radius on a tie); a block uses the radius of the last stage at
        or before it, and everything is visible before the first one."""
        radii, g = self._patch_radii()
        levels = torch.unique(radii)                                                   # ascending
        covered = (radii.reshape(1, -1) <= levels.reshape(-1, 1)).sum(dim=1)            # patches inside each candidate disc
        targets = torch.as_tensor(list(num_tokens), dtype=covered.dtype)
        pick = (covered.reshape(1, -1) - targets.reshape(-1, 1)).abs().argmin(dim=1)    # first minimum = smallest radius
        table = torch.cat([levels[-1:], levels[pick]])
        is_stage = torch.zeros(self.depth, dtype=torch.long)
        is_stage[torch.as_tensor(sorted(self.reduction_loc), dtype=torch.long)] = 1
        return radii, table[torch.cumsum(is_stage, dim=0)], g

    def get_reduction_count(self):
        return self.reduction_loc

    def _block_mask(self, idx):
        return (self.distances <= self.threshold[idx]).reshape(self.P * self.P)

    def _stage_operands(self, j, loc):
        mask = lambda: torch.cat([torch.ones(1), self._block_mask(loc).float()]).to(self.pos_embed.device)      # CLS, then the patches in reach
        return "", (Op("w3", value=mask, grad=False),), dict(n_pad=self.P * self.P + 1)

    def _feature_blocks(self, tokens):
        return sorted(set(int(b) for b in self.reduction_loc) | {self.depth - 1})

    def _viz_data(self, ws, B, tokens):
        decisions = {}
        for idx in self.reduction_loc:
            ind = self._block_mask(idx).nonzero(as_tuple=True)[0]
            decisions[idx] = ind.unsqueeze(0).expand(B, -1).numpy().astype(np.int64)
        return {"Kept_Tokens_Abs": decisions}

    def _static_decisions(self, B, dev):
        """Kept_Tokens_Abs is constructor-time geometry: uploaded once per device, every image of a batch sees the same rows."""
        tabs = self._decision_tables.get(dev)
        if tabs is None:
            tabs = self._decision_tables[dev] = {idx: self._block_mask(idx).nonzero(as_tuple=True)[0].to(torch.int32).to(dev)
                                                 for idx in self.reduction_loc}
        return {"stages": tuple(sorted(tabs)), "kept": {idx: t.unsqueeze(0).expand(B, -1) for idx, t in tabs.items()},
                "kept_count": {idx: torch.full((B,), t.numel(), dtype=torch.int32, device=dev) for idx, t in tabs.items()}, "assign": {}}


class VisionTransformerTeacher(VisionTransformer):
    """models/dyvit.py:267-334: the DyViT distillation teacher -- a plain DeiT whose forward returns
    (head(norm(x)[:, 0]), norm(x)[:, 1:]): the logits and the final-norm patch-token features, always as a tuple.  The teacher is
    only ever run under `torch.no_grad()` (losses.py:122-123), so its forward is the inference executor whatever `self.training` says;
    its outputs carry no gradient."""

    def forward(self, x):
        # norm(x) of every row is the executor's final_tokens tap (forward_taps): one launch beside the forward, which keeps its graph
        # and its lazy norms -- the same bits as the residual stream after the last block pushed through a separate fp32 LayerNorm
        viz, self.viz_mode = self.viz_mode, False
        was_training, self.training = self.training, False          # the module flag only: the teacher has no train-mode behaviour
        try:
            logits, taps = self.forward_taps(x, cls_blocks=(), final_tokens=True)
        finally:
            self.viz_mode = viz
            self.training = was_training
        return logits, taps["final_tokens"][:, 1:]
