"""Training-mode forward/backward of the models through the HIP executors (csrc/tr_vit.hip, csrc/tr_train.hip).

The reference trains with `output = model(samples); loss = criterion(...); loss.backward()` (engine.py:50-76) and wraps the
model in DistributedDataParallel (train.py:405-407).  Here `model.train(); model(x)` runs `tr_vit_forward_train` (the forward
that keeps its activations on a tape) and returns logits that carry an autograd node; `loss.backward()` hands d logits to
`tr_vit_backward`, which writes every parameter gradient into ONE flat fp32 buffer.  `p.grad` of every parameter is a view
into that buffer, laid out in the order the backward finishes them (head, norm, blocks depth-1..0, embedding), so a
data-parallel reducer can all-reduce contiguous slices in place while the rest of the backward is still running
(dp.FlatGradReducer) -- no flatten/unflatten copies.
Frozen parameters (requires_grad False) cost no gradient work: a unit whose parameters are all frozen reaches the executor as NULL
pointers, and the backward stops at the lowest block that still has a trainable parameter at or below it (TrainState.grads_struct).
The input takes a gradient like any autograd leaf: when `x.requires_grad` is set (or a module in front of the model trains) the
backward runs `tr_vit_backward_dx`, which walks down to the embedding whatever is frozen and folds the patch projection's data gradient
back into the image; the node returns it in x's slot and autograd accumulates `x.grad`.  Eval mode is not differentiable.
`model.forward_dense_train(x)` is the same node with a dense request: `tr_vit_forward_train_dense` also leaves the final norm of every row,
the stream that entered it and the decisions in the eval slabs' format; the eval path's three launches (tr_stage_decisions, tr_dense_index,
tr_dense_gather) put the rows on the patch grid, and the map is the node's second output.  Its gradient goes through `tr_dense_scatter`
(the gather's adjoint, bf16 out) into `tr_vit_backward_dense`, which adds the final norm's backward of every row to the stream gradient.
`model.forward_dense_train(x, blocks=...)` asks for the maps of several blocks: `tr_vit_forward_train_levels` taps every chosen block where
eval's level taps run (one launch per level), `tr_dense_index_levels` and `tr_dense_gather_levels` build all maps, and each map is a further
output of the node.  In backward ONE `tr_dense_scatter_levels` launch takes the gradients of the maps that have one back to their rows, and
`tr_vit_backward_levels` injects each level's gradient into the stream gradient in front of its block.

PyTorch is plumbing: memory, the stream, the autograd hook and the loss.  No arithmetic of the model happens in torch.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import torch

from . import _lib, models
from .augment import AugmentedBatch


def _align4(n: int) -> int:
    """Slot size of a parameter in the flat gradient buffer: 64 floats (256 B), so every bucket boundary is 16-byte aligned and
    divisible by the world size (reduce-scatter shards)."""
    return (n + 63) // 64 * 64


def backward_order(model) -> List[Tuple[str, torch.nn.Parameter]]:
    """(name, parameter) in the order the backward pass finishes their gradients; buckets are contiguous runs of this list."""
    named = dict(model.named_parameters())
    order, seen = [], set()

    def take(prefix):
        for n in named:
            if (n == prefix or n.startswith(prefix + ".")) and n not in seen:
                seen.add(n)
                order.append((n, named[n]))

    take("head")
    take("norm")
    for i in reversed(range(model.depth)):
        take(f"blocks.{i}")
    for n in list(named):            # family modules (score predictors, cluster layers): finished before the embedding
        if n not in seen and not n.startswith(("pos_embed", "cls_token", "patch_embed")):
            take(n)
    take("pos_embed")
    take("cls_token")
    take("patch_embed")
    return order


class TrainState:
    """Per-model training state: flat gradient buffer + views, transposed weights, tape and workspaces (one batch size)."""

    def __init__(self, model):
        dev = model.pos_embed.device
        self.order = backward_order(model)
        self.named = dict(self.order)
        self.slots = {n: _align4(model._grad_slot_numel(n, p)) for n, p in self.order}
        self.offsets, off = {}, 0
        for n in self.slots:
            self.offsets[n] = off
            off += self.slots[n]
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        # where a parameter's view starts inside its slot: a no_embed_class model's pos_embed is rows 1 .. P of the [(P + 1), D] gradient
        # the executor writes (D floats in: still 256-byte aligned); row 0, the class row's, is scratch
        self.view_off = {"pos_embed": model.embed_dim} if getattr(model, "no_embed_class", False) else {}
        self.views = {n: self.flat[o + self.view_off.get(n, 0): o + self.view_off.get(n, 0) + p.numel()].view_as(p)
                      for (n, p), o in zip(self.order, self.offsets.values())}
        self.slot_scratch = [self.flat[self.offsets[n]: self.offsets[n] + k] for n, k in self.view_off.items()]
        # LayerScale: the executor's gradients of the FOLDED proj / fc2 operands land in a scratch buffer, depth * (D*D + D*Hd + 2D) floats;
        # tr_layerscale_unfold_grad turns them into the gradients of W, b and gamma in the flat buffer (ls_unfold)
        self.ls = None
        if hasattr(model.blocks[0], "ls1"):
            D, Hd = model.embed_dim, model.blocks[0].mlp.fc1.out_features
            per = D * D + D * Hd + 2 * D
            self.ls = dict(scratch=torch.zeros(model.depth * per, dtype=torch.float32, device=dev), per=per, D=D, Hd=Hd, items=[], tables={})
        # bucket boundaries: [head+norm+last block] ... per block ... [block 0 + embedding]; event index that completes each
        self.block_slices = self._block_slices(model)
        self.B = None
        self.tape = self.bws = None
        self.key = None
        self.events = None
        # the gradient side of the model's operand declaration (models.Op rows), read once.  ptr: the slot's start of every parameter, what the
        # executor writes; units: (block or None for the trunk, (field, name) of the two rows, gamma's name under LayerScale, where the unit's
        # folded gradients start inside the block's part of the scratch buffer); stage_grads: {block: [(field, name)]} of a family's stages
        self.ptr = {n: self.flat.data_ptr() + 4 * o for n, o in self.offsets.items()}
        self.units = [(None, (a.field, a.name), (b.field, b.name), None, 0) for a, b in model._trunk_units()]
        for i in range(model.depth):
            pre, off = f"blocks.{i}.", 0
            for a, b in models._BLOCK_UNITS:
                gamma = pre + a.gamma if a.gamma and self.ls is not None else None
                self.units.append((i, (a.field, pre + a.name), (b.field, pre + b.name), gamma, off))
                off += self.named[pre + a.name].numel() + self.named[pre + b.name].numel() if gamma else 0
        self.stage_grads = {loc: [(r.field, pre + r.name) for r in rows if r.grad] for loc, (pre, rows, _) in model._stages().items()}
        self._stage_names = {loc: [n for _, n in rows] for loc, rows in self.stage_grads.items() if rows}      # structure, not mask
        self._stage_of = {n: loc for loc, names in self._stage_names.items() for n in names}
        self.gen = 0                 # counts training forwards: the tape belongs to the LAST one (see _VitTrainFn.backward)
        self.dense = None            # forward_dense_train's buffers (dense_buffers): one set per model, like the tape
        self.levels = None           # forward_dense_train(blocks=...)'s buffers (level_buffers): one set per model and (B, L, norm)

    def _block_slices(self, model):
        """[(event_index, start, stop)] over the flat buffer: the slice event `e` of tr_vit_backward completes."""
        ends = {}
        for n in self.slots:
            if n.startswith("blocks."):
                e = int(n.split(".")[1])
            elif n.startswith(("head", "norm")):
                e = model.depth - 1                     # finished before the last block's event
            else:
                e = model.depth                          # embedding + family modules: the final event
            ends[e] = self.offsets[n] + self.slots[n]
        out, start = [], 0
        for e in sorted(ends, key=lambda k: ends[k]):
            out.append((e, start, ends[e]))
            start = ends[e]
        return out

    def grads_struct(self, model, want_dx=False):
        """tr_vit_weights-shaped struct whose pointers are the gradient views, read off `requires_grad` as it is NOW (built per
        backward, nothing cached but the declaration's rows).  A unit of tr_vit_backward (the two gradients one launch produces) whose
        parameters are all frozen is NULL: the executor leaves its work out.  A mixed unit (pos_embed trainable, cls_token frozen) keeps both
        pointers; the frozen half lands in its slot of the flat buffer and is discarded.  The unit of a LayerScale branch points into the scratch
        buffer instead (never at the real slots): the executor writes the gradients of the FOLDED operands there, NULL only when W, b and gamma are
        all frozen, and ls["items"] takes the unfold item (a frozen output is 0).  The pointers of a family's reduction stage are NULL only where
        the backward never arrives: below the lowest block that has a trainable parameter at or below it.
        want_dx: the input takes a gradient, so the backward goes all the way whatever is frozen (the floor is -1): every reduction stage is
        reached and keeps its pointers, a frozen stage parameter's slice is computed and discarded.
        Returns (struct, names of the frozen parameters the executor still writes)."""
        G = _lib.TrVitWeights()
        named, ptr, ls = self.named, self.ptr, self.ls
        discarded = []
        if ls is not None:
            ls["items"] = []
        for blk, (fa, a), (fb, b), g, off in self.units:
            ps = [named[n] for n in ((a, b) if g is None else (a, b, g))]
            if not any(p.requires_grad for p in ps):
                continue
            if g is None:
                discarded.extend(n for n in (a, b) if not named[n].requires_grad)
                ga, gb = ptr[a], ptr[b]
            else:
                D, cols = ps[0].shape
                ga = ls["scratch"].data_ptr() + 4 * (blk * ls["per"] + off)
                gb = ga + 4 * D * cols
                ls["items"].append((blk, (ga, gb) + tuple(p.data_ptr() for p in ps)
                                    + tuple(ptr[n] if p.requires_grad else 0 for n, p in zip((a, b, g), ps)) + (D, cols)))
            S = G if blk is None else G.blocks[blk]
            setattr(S, fa, ga)
            setattr(S, fb, gb)
        # the floor: the lowest block with a trainable parameter at or below it (-1: the embedding trains, the backward goes all the way).
        # Conservative for family modules: a stage's parameter counts at the stage's block, any other family parameter at block 0.
        floor = model.depth
        for n, p in self.order:
            if not p.requires_grad or n.startswith(("head.", "norm.")):
                continue
            if n.startswith("blocks."):
                floor = min(floor, int(n.split(".")[1]))
            elif n.startswith(("pos_embed", "cls_token", "patch_embed")):
                floor = -1
            else:
                floor = min(floor, self._stage_of.get(n, 0))
        if want_dx:
            floor = -1
        for loc, names in self._stage_names.items():
            if loc > floor or (loc == floor and any(named[n].requires_grad for n in names)):
                for f, n in self.stage_grads[loc]:
                    setattr(G.stage[loc], f, ptr[n])
                discarded.extend(n for n in names if not named[n].requires_grad)
        return G, discarded

    def ls_unfold(self, hi, lo, accumulate, dev):
        """LayerScale: the gradients of W, b and gamma of the blocks lo .. hi from the folded gradients the backward call just wrote -- one
        tr_layerscale_unfold_grad launch (nothing for a model without LayerScale, or a range whose branches are all frozen).  The item
        tables live on the device, one per (range, frozen pattern)."""
        if self.ls is None:
            return
        rows = tuple(it for blk, it in self.ls["items"] if lo <= blk <= hi)
        if not rows:
            return
        from . import ops
        tab = self.ls["tables"].get(rows)
        if tab is None:
            if len(self.ls["tables"]) >= 64:
                self.ls["tables"].clear()
            tab = self.ls["tables"][rows] = ops.layerscale_table(rows, ops.LS_UNFOLD_ITEM, dev)
        _lib.check(_lib.load().tr_layerscale_unfold_grad(tab["items"].data_ptr(), tab["shapes"], tab["n"], 1 if accumulate else 0,
                                                         torch.cuda.current_stream().cuda_stream), "tr_layerscale_unfold_grad")

    def transposed(self, model, pk):
        """The dgrad GEMM operands, all made by the model's own repack (models._pack with need_transposed): the bf16 transposed copies of
        the block matrices and of the patch weight are persistent buffers rewritten by the same fused launch as the operand copies; the reduction
        modules' few small matrices are transposed there too (models._pack_stages).  The struct is rebuilt whenever the pack generation changes."""
        if self.key == pk["gen"]:
            return self.wt
        WT = _lib.TrVitWeights()
        wt_fields = [a.field for a, _ in models._BLOCK_UNITS if a.kind == "wt"]
        for i, ts in enumerate(pk["tblocks"]):
            for f, t in zip(wt_fields, ts):
                setattr(WT.blocks[i], f, t.data_ptr())
        if pk.get("tpatch") is not None:      # the patch weight transposed [C*p*p, D]: the operand of the input gradient (tr_vit_backward_dx)
            WT.patch_w = pk["tpatch"].data_ptr()
        for (loc, f), t in model._stage_t.items():
            setattr(WT.stage[loc], f, t.data_ptr())
        self.wt, self.wt_keep, self.key = WT, dict(model._stage_t), pk["gen"]      # (the struct points into the stage tensors: kept with it)
        return WT

    def buffers(self, model, pk, B, dev):
        if self.B != B:
            lib = _lib.load()
            nt = lib.tr_vit_tape_bytes(C.byref(pk["cfg"]), B)
            nb = lib.tr_vit_backward_workspace_bytes(C.byref(pk["cfg"]), B)
            if nt == 0 or nb == 0:
                raise NotImplementedError(
                    f"{type(model).__name__}: this configuration has no training path in the HIP executor (built: every family, square and "
                    f"rectangular inputs, up to 640 tokens incl. the class token -- this model has {model.patch_embed.num_patches + 1}; bf16); "
                    "call model.eval() for inference")
            self.tape = torch.empty(nt, dtype=torch.uint8, device=dev)
            self.bws = torch.empty(nb, dtype=torch.uint8, device=dev)
            self.B = B
        return self.tape, self.bws

    def dense_buffers(self, model, B, dev):
        """What forward_dense_train owns beside the tape, for one batch size: the executor's caller-owned outputs (the final norm of every
        row, the stream entering it, the decision slabs) under their tr_vit_dense_train struct, the decision plan of the eval path
        (models._decision_plan: the stage table and tr_stage_decisions' record buffers), the index, one map per output dtype and the bf16
        token gradient tr_dense_scatter writes for the backward."""
        d = self.dense
        if d is None or d["B"] != B or d["dev"] != dev:
            P0, D = model.patch_embed.num_patches, model.embed_dim
            rows = B * (P0 + 1) * D
            empty = lambda n, dtype=torch.float32: torch.empty(n, dtype=dtype, device=dev)
            d = dict(B=B, dev=dev, tokens=empty(rows), stream=empty(rows), kept=empty(model.depth * B * (P0 + 1), torch.int32),
                     compl=empty(model.depth * B * (P0 + 1), torch.int32), index=empty(B * P0, torch.int32), feat={},
                     dtok=empty(rows, torch.bfloat16))
            dec = d["plan"] = model._decision_plan(d, B, dev)          # (keeps itself in d["dec"])
            d["struct"] = _lib.TrVitDenseTrain(d["tokens"].data_ptr(), d["stream"].data_ptr(), rows, d["kept"].data_ptr(), d["compl"].data_ptr(),
                                               d["kept"].numel(), dec["soft_ptr"], dec["soft_elems"])
            self.dense = d
        return d

    def level_buffers(self, model, B, dev, levels):
        """What forward_dense_train(blocks=...) owns beside the tape, for one (batch size, number of levels, norm): the level slabs of
        tr_vit_forward_train_levels (`tokens`: what the gather reads -- the final-normed rows, or with norm=False the summed rows; `stream`,
        norm=True only: the summed rows the norm's backward needs), the decision slabs and the eval path's decision plan as in dense_buffers,
        the indices [L, B, P0], one set of maps per output dtype and the token gradients tr_dense_scatter_levels writes (bf16 for norm=True,
        fp32 for norm=False).  A slab is B * N0 * D elements."""
        L, norm = len(levels.blocks), bool(levels.norm)
        d = self.levels
        if d is None or d["key"] != (B, dev, L, norm):
            P0, D = model.patch_embed.num_patches, model.embed_dim
            rows = B * (P0 + 1) * D
            empty = lambda n, dtype=torch.float32: torch.empty(n, dtype=dtype, device=dev)
            d = dict(key=(B, dev, L, norm), B=B, dev=dev, stride=rows, tokens=empty(L * rows), stream=empty(L * rows) if norm else None,
                     kept=empty(model.depth * B * (P0 + 1), torch.int32), compl=empty(model.depth * B * (P0 + 1), torch.int32),
                     index=empty(L * B * P0, torch.int32), feat={}, dtok=empty(L * rows, torch.bfloat16 if norm else torch.float32))
            dec = d["plan"] = model._decision_plan(d, B, dev)          # (keeps itself in d["dec"])
            d["struct"] = _lib.TrVitDenseTrain(None, None, 0, d["kept"].data_ptr(), d["compl"].data_ptr(), d["kept"].numel(), dec["soft_ptr"],
                                               dec["soft_elems"])
            self.levels = d
        mask = sum(1 << b for b in levels.blocks)
        d["taps"] = _lib.TrVitTrainLevels(mask, int(norm), d["tokens"].data_ptr(), None if d["stream"] is None else d["stream"].data_ptr(),
                                          d["tokens"].numel())
        d["mask"] = mask
        return d


TAPE_FIELDS = ("x0", "x1", "xn1", "qkv", "ao", "dattn", "x2", "xn2", "pre", "h", "idx", "idx2", "scores", "size",
               "n_pre", "n_att", "n_mlp", "kk")


def tape_layout(model, blk: int) -> dict:
    """Offsets / token counts of block `blk` on the tape of the last training forward."""
    st = model._train_state()
    out = (C.c_size_t * 18)()
    _lib.check(_lib.load().tr_vit_tape_layout(C.byref(model._packed["cfg"]), st.B, blk, out), "tr_vit_tape_layout")
    return dict(zip(TAPE_FIELDS, (int(v) for v in out)))


def train_decisions(model) -> dict:
    """{blk: decision tensors} of the last training forward, read back from the tape (int64 on the host side):
    Top-K / EViT: idx [B,K]; ToMe: (unm [B,na-r], src [B,r], dst [B,r]); DPC-KNN: (centres [B,K], assignment [B,P_in]); ATS: ids."""
    st = model._train_state()
    B, out = st.B, {}
    for blk in range(model.depth):
        lay = tape_layout(model, blk)
        k = lay["kk"]
        if k <= 0:
            continue
        raw = st.tape[lay["idx"]: lay["idx"] + 4 * B * lay["n_att"]].view(torch.int32)
        if model._family in (_lib.TR_FAMILY_TOPK, _lib.TR_FAMILY_EVIT):
            out[blk] = raw[: B * k].view(B, k).long()
        elif model._family == _lib.TR_FAMILY_TOME:
            na = (lay["n_att"] + 1) // 2
            out[blk] = (raw[: B * (na - k)].view(B, na - k).long(), raw[B * (na - k): B * na].view(B, k).long(),
                        raw[B * na: B * (na + k)].view(B, k).long())
        elif model._family == _lib.TR_FAMILY_DPCKNN:          # (centres [B,K], assignment [B,P_in])
            p_in = lay["n_pre"] - 1
            raw2 = st.tape[lay["idx2"]: lay["idx2"] + 4 * B * p_in].view(torch.int32)
            out[blk] = (raw[: B * k].view(B, k).long(), raw2.view(B, p_in).long())
        elif model._family == _lib.TR_FAMILY_KMEDOIDS:        # medoid ids [B,K]
            out[blk] = raw[: B * k].view(B, k).long()
        elif model._family == _lib.TR_FAMILY_ATS:             # ids [B,Ks]: CLS id 0 first, 1-based token ids, 0 padding
            out[blk] = raw[: B * k].view(B, k).long()
        elif model._family == _lib.TR_FAMILY_DYVIT:           # the Gumbel one-hot's first entry per patch token [B,P] (before * prev_decision)
            n = lay["n_att"]
            out[blk] = st.tape[lay["scores"]: lay["scores"] + 4 * B * n].view(torch.float32).view(B, n)[:, 1:].clone()
    return out


def drop_path_scales(model, B: int, dev):
    """DropPath (timm 0.4.12 drop_path, call sites topk.py:78,87,95): block i drops a branch of an image with probability
    dpr[i] = linspace(0, drop_path_rate, depth)[i] (topk.py:157) and scales the survivors by 1/keep_prob; two independent draws per
    block (attention branch, MLP branch).  Returns fp32 [2*depth, B] of scales, or None when drop_path_rate == 0.
    `model.drop_path_draws` (tests): the uniform draws [2*depth, B] to use instead of torch.rand (the reference's, replayed)."""
    if not model.drop_path_rate:
        return None
    dpr = torch.linspace(0, model.drop_path_rate, model.depth)
    keep = (1.0 - dpr).repeat_interleave(2).to(dev).unsqueeze(1)                      # [2*depth, 1]
    draws = getattr(model, "drop_path_draws", None)
    u = torch.rand(2 * model.depth, B, device=dev) if draws is None else draws.to(device=dev, dtype=torch.float32).reshape(2 * model.depth, B)
    scale = (keep + u).floor() / keep                                                   # x.div(keep) * floor(keep + rand)
    scale[keep.squeeze(1) >= 1.0] = 1.0                                                 # drop_prob 0 (block 0): DropPath is the identity
    return scale.contiguous()


def dropout_keep_mask(model, pk, B: int, dev):
    """Dropout (timm's drop_rate; train.py:46 --drop): the keep mask of one training forward, uint8 (1 = keep), one byte per element in
    the order the executor consumes it -- the embedded tokens [B,N0,D] (pos_drop, topk.py:186), then per block proj's output rows
    (proj_drop, :53), the Mlp's hidden layer and its output (timm Mlp's two nn.Dropout): the order in which the reference module draws.
    Returns None when drop_rate == 0.  `model.dropout_draws` (tests): the reference's recorded keep masks, in call order, used instead
    of a fresh Bernoulli(1 - p) draw on the device."""
    if not model.drop_rate:
        return None
    n = int(_lib.load().tr_vit_dropout_mask_bytes(C.byref(pk["cfg"]), B))
    if n == 0:
        raise NotImplementedError(f"{type(model).__name__}: no training path for this configuration")
    draws = getattr(model, "dropout_draws", None)
    if draws is not None:
        keep = torch.cat([torch.as_tensor(d).reshape(-1).to(torch.uint8) for d in draws]).to(dev)
        if keep.numel() != n:
            raise ValueError(f"dropout_draws hold {keep.numel()} elements, this forward consumes {n}")
        return keep.contiguous()
    return torch.empty(n, dtype=torch.uint8, device=dev).bernoulli_(1.0 - float(model.drop_rate))


class _VitTrainFn(torch.autograd.Function):
    """logits (+ DyViT's extra outputs) = model(x) with the backward wired to tr_vit_backward.  `anchor` only makes autograd call
    backward.  Outputs: (logits,) or for DyViT (logits, pred_0 .. pred_{S-1} [, features]): pred_j = the stage's hard keep decision
    [B,P] (straight-through differentiable, dyvit.py:223-225), features = the final norm of the patch tokens [B,P,D].
    dense (an eval_request.DenseOutput; not DyViT): forward_dense_train's request -- the outputs are (logits, map), the map as eval's
    forward_dense lays it out; the index stays in TrainState.dense.  Without it the inputs, outputs and launches are those above.
    levels (an eval_request.Levels, with dense): forward_dense_train(blocks=...) -- the outputs are (logits, map_0, ..., map_{L-1}) in
    ascending block order; indices and slabs stay in TrainState.levels."""

    @staticmethod
    def forward(ctx, anchor, x, model, fmt=_lib.TR_INPUT_F32, lut=None, aug=None, xe=None, dense=None, levels=None):
        lib = _lib.load()
        pk = model._pack(need_transposed=True)
        cfg = pk["cfg"]
        B = x.shape[0]
        # the input gradient is computed only when autograd wants it, and only for the fp32 image (uint8 pixels and augmented batches cannot
        # require one); the executor reads xe, train_forward's detached fp32 contiguous copy of the caller's tensor (made once)
        ctx.want_dx = bool(ctx.needs_input_grad[1]) and fmt == _lib.TR_INPUT_F32 and aug is None
        ctx.x_dtype = x.dtype
        if ctx.want_dx and not lib.tr_patch_embed_dgrad_hw_supported(cfg.in_chans, *cfg.image_hw, cfg.patch, cfg.embed_dim):
            raise NotImplementedError(
                f"{type(model).__name__}: the input requires a gradient, but the input gradient is built for patch 16, 1 or 3 channels and "
                f"embed_dim 128 / 192 / 384 / 768 (got patch {cfg.patch}, in_chans {cfg.in_chans}, embed_dim {cfg.embed_dim}); "
                "detach the input to train the parameters alone")
        if xe is not None:          # the executor's tensor of train_forward: x is the caller's own, here only for autograd
            x = xe
        st = model._train_state()
        tape, bws = st.buffers(model, pk, B, x.device)
        st.gen += 1
        ctx.gen = st.gen
        ws = model._workspace(B, x.device)
        logits = torch.empty(B, model._out_width, dtype=torch.float32, device=x.device)      # headless: the CLS features [B, D]
        tokens = (C.c_int * model.depth)()
        dyvit = model._family == _lib.TR_FAMILY_DYVIT
        distill = dyvit and bool(getattr(model, "dyvit_distillation", False))
        feats = torch.empty(B, model.patch_embed.num_patches + 1, model.embed_dim, dtype=torch.float32, device=x.device) if distill else None
        model._noise_slot = 0
        noise = model._gumbel_ptr(B, x.device) if dyvit else model._noise_ptr(B, x.device)
        ctx.drop = drop_path_scales(model, B, x.device)
        ctx.keep_mask = dropout_keep_mask(model, pk, B, x.device)
        dn = None
        if dense is not None:
            dn = st.dense_buffers(model, B, x.device) if levels is None else st.level_buffers(model, B, x.device, levels)
        with torch.cuda.device(x.device):
            rest = (logits.data_ptr(), ws["buf"].data_ptr(), ws["nbytes"], tape.data_ptr(), tape.numel(), noise,
                    None if feats is None else feats.data_ptr(), None if ctx.drop is None else ctx.drop.data_ptr(), tokens, B,
                    torch.cuda.current_stream().cuda_stream, None if ctx.keep_mask is None else ctx.keep_mask.data_ptr(),
                    float(model.drop_rate or 0.0))
            if dn is not None:       # the superset entry: any of the three inputs below, plus the dense request's caller-owned outputs
                table, aug_noise = aug if aug is not None else (None, None)
                entry = lib.tr_vit_forward_train_dense if levels is None else lib.tr_vit_forward_train_levels
                rc = entry(C.byref(cfg), C.byref(pk["W"]), x.data_ptr(), fmt, lut, None if table is None else table.data_ptr(),
                           aug_noise.data_ptr() if aug_noise is not None and aug_noise.numel() else None,
                           0 if aug_noise is None else aug_noise.numel(), *rest[:6], *rest[7:], C.byref(dn["struct"]),
                           *(() if levels is None else (C.byref(dn["taps"]),)))
            elif aug is not None:    # uint8 pixels + the device-side erase / mixup / cutmix table (augment.py): the columns of the augmented image
                table, aug_noise = aug
                rc = lib.tr_vit_forward_train_aug(C.byref(cfg), C.byref(pk["W"]), x.data_ptr(), fmt, lut, table.data_ptr(),
                                                  aug_noise.data_ptr() if aug_noise.numel() else None, aug_noise.numel(), *rest)
            elif fmt == _lib.TR_INPUT_F32:
                rc = lib.tr_vit_forward_train(C.byref(cfg), C.byref(pk["W"]), x.data_ptr(), *rest)
            else:      # uint8 pixels: the patch embedding normalizes them; the tape's column matrix is the one the fp32 image gives
                rc = lib.tr_vit_forward_train_pixels(C.byref(cfg), C.byref(pk["W"]), x.data_ptr(), fmt, lut, *rest)
        _lib.check(rc, "tr_vit_forward_train")
        model._last_tokens = list(tokens)
        ctx.model, ctx.B, ctx.pk = model, B, pk
        ctx.keep = (x, aug)
        ctx.n_pred, ctx.distill = 0, distill
        ctx.dense, ctx.levels = dense, levels
        if dense is not None:
            ctx.set_materialize_grads(False)      # a loss on one output alone: the other's gradient arrives as None and its path is skipped
        if model._out_width != model._out_cols:          # the padded classifier columns never leave the executor
            logits = logits[:, :model._out_cols].contiguous()
        if dn is not None and levels is not None:
            with torch.cuda.device(x.device):
                return (logits,) + _dense_maps(model, dn, dense, levels, list(tokens), B)
        if dn is not None:
            with torch.cuda.device(x.device):
                return logits, _dense_map(model, dn, dense, list(tokens), B)
        if not dyvit:
            return logits
        preds = []
        for blk in sorted(model.pruning_loc):
            lay = tape_layout(model, blk)
            n = lay["n_att"]
            pol = tape[lay["size"]: lay["size"] + 4 * B * n].view(torch.float32).view(B, n)
            preds.append(pol[:, 1:].clone())
        ctx.n_pred = len(preds)
        outs = [logits] + preds + ([feats[:, 1:].clone()] if distill else [])
        return tuple(outs)

    @staticmethod
    def backward(ctx, dlogits, *dextra):
        model, B, pk = ctx.model, ctx.B, ctx.pk
        lib = _lib.load()
        st = model._train_state()
        if ctx.gen != st.gen:
            # the tape, the Gumbel / DPC-KNN noise and the workspace belong to the model, not to the autograd node: a later train-mode
            # forward has overwritten the activations and decisions this backward would read
            raise RuntimeError(
                f"{type(model).__name__}: backward() of training forward #{ctx.gen}, but forward #{st.gen} has run since and overwritten "
                "the activation tape (one tape per model).  Call loss.backward() before the next model(x) in train mode; for several "
                "forwards per step (two views, accumulated losses) run forward + backward per view and let the gradients accumulate, or "
                "use model.eval() / torch.no_grad() for the forwards that need no gradient.")
        dev = st.flat.device
        if dlogits is None:
            dlogits = torch.zeros(B, model._out_cols, dtype=torch.float32, device=dev)
        dl = dlogits.detach().to(torch.float32).contiguous()
        if model._out_width != model._out_cols:          # zero gradient on the padded classifier columns
            dlp = torch.zeros(B, model._out_width, dtype=torch.float32, device=dev)
            dlp[:, :model._out_cols] = dl
            dl = dlp
        dpred = dfeat = dtok = lev = None
        if ctx.levels is not None and any(g is not None for g in dextra):
            # the gradients of the maps that have one, back on their levels' rows: ONE tr_dense_scatter_levels launch with the forward's indices
            # (the gen guard above keeps them the forward's).  A level without a gradient is a NULL entry: no tile, no injection below
            dn, P0, L = st.levels, model.patch_embed.num_patches, len(ctx.levels.blocks)
            dmaps = [None if g is None else g.detach() for g in dextra[:L]]
            kinds = {g.dtype for g in dmaps if g is not None}
            if kinds != {torch.bfloat16}:          # one dtype per launch: fp32 unless every gradient is bf16
                dmaps = [None if g is None else g.to(torch.float32) for g in dmaps]
            dmaps = [None if g is None else g.contiguous() for g in dmaps]
            ptrs = (C.c_void_p * L)(*[None if g is None else g.data_ptr() for g in dmaps])
            present = sum(1 << l for l, g in enumerate(dmaps) if g is not None)
            with torch.cuda.device(dev):
                _lib.check(lib.tr_dense_scatter_levels(ptrs, dn["index"].data_ptr(), dn["dtok"].data_ptr(), dn["stride"], dn["rows"], L,
                                                       _lib.TR_LAYOUT_NCHW if ctx.dense.fmt == "NCHW" else _lib.TR_LAYOUT_NHWC,
                                                       int(kinds == {torch.bfloat16}), int(ctx.levels.norm), B, P0, model.embed_dim,
                                                       torch.cuda.current_stream().cuda_stream), "tr_dense_scatter_levels")
            lev = _lib.TrVitLevelGrads(dn["mask"], int(ctx.levels.norm), present, dn["dtok"].data_ptr(),
                                       None if dn["stream"] is None else dn["stream"].data_ptr(), dn["stride"])
        elif ctx.levels is None and ctx.dense is not None and dextra[0] is not None:
            # the map's gradient back on the token rows: tr_dense_scatter with the forward's index (the gen guard above keeps it the
            # forward's), bf16 out -- the form the final norm's backward reads
            dn, P0 = st.dense, model.patch_embed.num_patches
            dmap = dextra[0].detach()
            if dmap.dtype not in (torch.float32, torch.bfloat16):
                dmap = dmap.to(torch.float32)
            dmap = dmap.contiguous()
            with torch.cuda.device(dev):
                _lib.check(lib.tr_dense_scatter(dmap.data_ptr(), dn["index"].data_ptr(), dn["dtok"].data_ptr(),
                                                _lib.TR_LAYOUT_NCHW if ctx.dense.fmt == "NCHW" else _lib.TR_LAYOUT_NHWC,
                                                int(dmap.dtype == torch.bfloat16), 1, B, P0, dn["rows"], model.embed_dim,
                                                torch.cuda.current_stream().cuda_stream), "tr_dense_scatter")
            dtok = dn["dtok"]
        if ctx.n_pred:
            P = model.patch_embed.num_patches
            gp = [torch.zeros(B, P, dtype=torch.float32, device=dev) if g is None else g.detach().to(torch.float32) for g in dextra[:ctx.n_pred]]
            dpred = torch.stack(gp).contiguous()                              # [stages, B, P]
            if ctx.distill and dextra[ctx.n_pred] is not None:
                dfeat = torch.zeros(B, P + 1, model.embed_dim, dtype=torch.float32, device=dev)
                dfeat[:, 1:] = dextra[ctx.n_pred].detach()
        # gradient views: when NO parameter holds a gradient yet (zero_grad(set_to_none=True), torch's default) the backward OVERWRITES
        # the flat buffer -- nothing to clear, nothing to read back; otherwise the slices of the parameters without a gradient are zeroed
        # and the backward accumulates (engine.py:41-84: gradient accumulation over micro-steps).  Every trainable parameter of the
        # executor is written exactly once per backward (csrc/tr_train.hip); parameters the executor does not touch keep the zeros they
        # were born with.  Frozen parameters (requires_grad False) take no part: their slices are neither cleared nor -- when their whole
        # unit is frozen (grads_struct) -- written.
        train = [(n, p) for n, p in st.order if p.requires_grad]
        fresh = [n for n, p in train if p.grad is None or p.grad.data_ptr() != st.views[n].data_ptr()]
        accumulate = 0 if len(fresh) == len(train) else 1
        G, discarded = st.grads_struct(model, want_dx=ctx.want_dx)
        if accumulate:
            for n in fresh + discarded:          # (a discarded slice is cleared so that it cannot grow without bound over the steps)
                st.views[n].zero_()
            for t in st.slot_scratch:            # (no_embed_class: the class row of the position gradient, discarded like them)
                t.zero_()
            if st.ls is not None:
                # the executor ADDS to what its gradient pointers hold: the folded-gradient scratch must not carry the last backward's values
                # into this one.  Cleared here, on accumulating calls only (a non-accumulating call overwrites it)
                st.ls["scratch"].zero_()
        WT = st.transposed(model, pk)
        reducer = model._grad_reducer
        reduce_now = reducer is not None and reducer.sync
        # one call for the whole model, or -- under a gradient reducer -- one call per bucket's block range, each followed by
        # that bucket's in-place reduction on the reducer's stream while the next range runs
        ranges = reducer.plan(st.block_slices, model.depth) if reduce_now else [(model.depth - 1, 0, 0, st.flat.numel())]
        if reduce_now:
            reducer.begin(st.flat) if hasattr(reducer, "begin") else setattr(reducer, "launched", [])
        stream = torch.cuda.current_stream().cuda_stream
        # the input gradient (x.requires_grad, or something learnable in front of the model): every range call takes dx so that all of them
        # walk down to the embedding whatever is frozen; only the call with lo == 0 writes it -- once, in full: autograd accumulates x.grad
        dx = torch.empty(ctx.keep[0].shape, dtype=torch.float32, device=dev) if ctx.want_dx else None
        with torch.cuda.device(dl.device):
            for hi, lo, start, stop in ranges:
                args = (C.byref(pk["cfg"]), C.byref(pk["W"]), C.byref(WT), C.byref(G), dl.data_ptr(),
                        None if dpred is None else dpred.data_ptr(), None if dfeat is None else dfeat.data_ptr(),
                        None if ctx.drop is None else ctx.drop.data_ptr(), st.tape.data_ptr(), st.tape.numel(), st.bws.data_ptr(), st.bws.numel(), accumulate, hi, lo, B, stream,
                        None if ctx.keep_mask is None else ctx.keep_mask.data_ptr(), float(model.drop_rate or 0.0))
                if lev is not None:      # every range call takes the levels; a level is consumed by the call whose range holds its block
                    rc = lib.tr_vit_backward_levels(*args, None if dx is None else dx.data_ptr(), None, 0, None, C.byref(lev))
                elif dtok is not None:   # every range call takes it; the one with hi == depth - 1 consumes it
                    rc = lib.tr_vit_backward_dense(*args, None if dx is None else dx.data_ptr(), dtok.data_ptr(), 1, st.dense["stream"].data_ptr())
                else:
                    rc = lib.tr_vit_backward(*args) if dx is None else lib.tr_vit_backward_dx(*args, dx.data_ptr())
                _lib.check(rc, "tr_vit_backward")
                st.ls_unfold(hi, lo, accumulate, dev)
                if reduce_now:
                    reducer.reduce_slice(st.flat, start, stop)
        if reduce_now:
            reducer.finish(st.flat)
        for n, p in st.order:
            if not p.requires_grad:
                continue
            if p.grad is None:
                p.grad = st.views[n]
            elif p.grad.data_ptr() != st.views[n].data_ptr():
                p.grad.add_(st.views[n])
        was_dirty = model._weights_dirty
        model.weights_changed()          # an optimizer step follows; fused optimizers do not bump the version counters the pack cache reads
        model._dirty_by_backward = not was_dirty      # dirt that was there before this backward is somebody else's: only a full repack clears it
        if dx is not None and dx.dtype != ctx.x_dtype:
            dx = dx.to(ctx.x_dtype)
        return None, dx, None, None, None, None, None, None, None


def _dense_maps(model, dn, dense, levels, tokens, B):
    """_dense_map for the levels of forward_dense_train(blocks=...): tr_stage_decisions, then ONE tr_dense_index_levels and ONE
    tr_dense_gather_levels for all levels (each level behind its own prefix of the stages; tr_dense_index_levels checks the stage table against
    the token counts the training forward had after each chosen block).  Returns the L maps, cloned out of their per-model buffer; the indices
    and the rows of every level stay in dn for the backward."""
    lib, dec, stream = _lib.load(), dn["plan"], torch.cuda.current_stream().cuda_stream
    D, P0, L = model.embed_dim, model.patch_embed.num_patches, len(levels.blocks)
    if dec["static"] is None and not dec["checked"]:
        model._decision_result(dec, B, tokens)                   # the stage table against the training forward's token counts, once
    if dec["n"]:
        _lib.check(lib.tr_stage_decisions(dn["kept"].data_ptr(), dn["compl"].data_ptr(), dn["kept"].numel(), dec["soft_ptr"], dec["soft_elems"],
                                          dec["table"], dec["n"], B, P0 + 1, dec["kept_ptr"], dec["kept_elems"], dec["count_ptr"],
                                          dec["assign_ptr"], dec["assign_elems"], stream), "tr_stage_decisions")
    feat = dn["feat"].get(dense.dtype)
    if feat is None:
        feat = dn["feat"][dense.dtype] = torch.empty(L * B * P0 * D, dtype=dense.dtype, device=dn["dev"])
    blocks = (C.c_int32 * L)(*levels.blocks)
    rows = dn["rows"] = (C.c_int32 * L)(*[tokens[b] for b in levels.blocks])
    _lib.check(lib.tr_dense_index_levels(dec["kept_ptr"], dec["kept_elems"], dec["assign_ptr"], dec["assign_elems"], dec["table"], dec["n"], B, P0,
                                         blocks, rows, L, dn["index"].data_ptr(), stream), "tr_dense_index_levels")
    _lib.check(lib.tr_dense_gather_levels(dn["tokens"].data_ptr(), dn["stride"], rows, L, dn["index"].data_ptr(), feat.data_ptr(),
                                          _lib.TR_LAYOUT_NCHW if dense.fmt == "NCHW" else _lib.TR_LAYOUT_NHWC, int(dense.dtype == torch.bfloat16),
                                          dense.fill, B, P0, D, stream), "tr_dense_gather_levels")
    h, w = model.patch_embed.grid_size
    return tuple(feat.clone().view((L, B, D, h, w) if dense.fmt == "NCHW" else (L, B, h, w, D)).unbind(0))


def _dense_map(model, dn, dense, tokens, B):
    """The eval path's launches behind the training executor (models._launch_outputs): the decision slabs -> record form, the records composed
    into one row per grid patch, the un-reduce of the final-normed rows.  Returns the map, cloned out of its per-model buffer; the index
    stays in dn["index"] for the backward."""
    lib, dec, stream = _lib.load(), dn["plan"], torch.cuda.current_stream().cuda_stream
    D, P0, n_last = model.embed_dim, model.patch_embed.num_patches, tokens[model.depth - 1]
    if dec["static"] is None and not dec["checked"]:
        model._decision_result(dec, B, tokens)                   # the stage table against the training forward's token counts, once
    if dec["n"]:
        _lib.check(lib.tr_stage_decisions(dn["kept"].data_ptr(), dn["compl"].data_ptr(), dn["kept"].numel(), dec["soft_ptr"], dec["soft_elems"],
                                          dec["table"], dec["n"], B, P0 + 1, dec["kept_ptr"], dec["kept_elems"], dec["count_ptr"],
                                          dec["assign_ptr"], dec["assign_elems"], stream), "tr_stage_decisions")
    feat = dn["feat"].get(dense.dtype)
    if feat is None:
        feat = dn["feat"][dense.dtype] = torch.empty(B * P0 * D, dtype=dense.dtype, device=dn["dev"])
    _lib.check(lib.tr_dense_index(dec["kept_ptr"], dec["kept_elems"], dec["assign_ptr"], dec["assign_elems"], dec["table"], dec["n"], B, P0,
                                  n_last, dn["index"].data_ptr(), stream), "tr_dense_index")
    _lib.check(lib.tr_dense_gather(dn["tokens"].data_ptr(), dn["index"].data_ptr(), feat.data_ptr(),
                                   _lib.TR_LAYOUT_NCHW if dense.fmt == "NCHW" else _lib.TR_LAYOUT_NHWC, int(dense.dtype == torch.bfloat16),
                                   dense.fill, B, P0, n_last, D, stream), "tr_dense_gather")
    dn["rows"] = n_last
    h, w = model.patch_embed.grid_size
    return feat.clone().view((B, D, h, w) if dense.fmt == "NCHW" else (B, h, w, D))


def train_forward(model, x: torch.Tensor, dense=None, levels=None):
    if model._family == _lib.TR_FAMILY_DYVIT and model._pool_mode() == _lib.TR_POOL_AVG:
        raise NotImplementedError("global_pool='avg' is not built for DyViT in train mode: training keeps the masked tokens in the stream under a "
                                  "differentiable policy (dyvit.py:221-229), so there is no token set to average over; DyViT eval, where the tokens "
                                  "are removed, pools like Top-K -- train with global_pool='' or call model.eval()")
    if not x.is_cuda:
        raise RuntimeError(f"input is on {x.device}: tokenreduction_amd has no CPU path (HIP kernels only)")
    if model.precision != "bf16":
        raise NotImplementedError("the training path is bf16 (fp32 accumulate); set model.precision = 'bf16'")
    if model.attn_drop_rate:
        raise NotImplementedError("attn_drop_rate (dropout on the attention probabilities, topk.py:49) is not built in the HIP training path; "
                                  "the reference's command line cannot set it either (train.py:46 exposes --drop only, which IS supported, "
                                  "as is --drop-path)")
    aug = None
    if isinstance(x, AugmentedBatch):       # (models.forward has materialized the batch unless pixel input is on)
        if x.mean_std != model.pixel_input:
            raise ValueError(f"the batch normalizes with (mean, std) = {x.mean_std}, the model with {model.pixel_input}: "
                             "give DeviceAugment the mean and std of model.set_pixel_input")
        aug, x = (x.table, x.noise), x.pixels
    want = (model.patch_embed.proj.in_channels, *model.patch_embed.img_size)
    if x.dim() != 4 or tuple(x.shape[1:]) != want:      # before any launch: the executor reads B * C * H * W elements, whatever it is given
        raise ValueError(f"expected [B, C, H, W] = [B,{want[0]},{want[1]},{want[2]}], got {tuple(x.shape)}")
    xe, fmt, lut = model._executor_input(x)
    # an fp32-format input that takes a gradient goes through autograd as the caller's own tensor (x.grad, a module in front of the model);
    # anything else -- uint8 pixels, an augmented batch, an input without requires_grad, torch.no_grad() -- as the executor's detached
    # tensor, as before
    anchor = torch.empty(0, dtype=torch.float32, device=xe.device, requires_grad=True)
    if fmt == _lib.TR_INPUT_F32 and aug is None and x.requires_grad and torch.is_grad_enabled():
        out = _VitTrainFn.apply(anchor, x, model, fmt, lut, aug, xe, dense, levels)
    else:
        out = _VitTrainFn.apply(anchor, xe, model, fmt, lut, aug, None, dense, levels)
    if levels is not None:           # forward_dense_train(blocks=...): eval's multi-level dictionary; index and cls carry no gradient
        (h, w), st, B, D = model.patch_embed.grid_size, model._train_state(), x.shape[0], model.embed_dim
        dn, L = st.levels, len(levels.blocks)
        slabs = dn["tokens"].view(L, -1)
        cls = torch.stack([slabs[l, :B * n * D].view(B, n, D)[:, 0] for l, n in enumerate(dn["rows"])], dim=1)      # (a strided copy)
        return out[0], {"features": list(out[1:]), "index": list(dn["index"].clone().view(L, B, h * w)), "blocks": levels.blocks,
                        "grid": (h, w), "cls": cls}
    if dense is not None:            # forward_dense_train: (out, the map); the index is a copy of the per-model buffer and carries no gradient
        h, w = model.patch_embed.grid_size
        st = model._train_state()
        return out[0], {"features": out[1], "index": st.dense["index"].clone().view(x.shape[0], h * w), "grid": (h, w)}
    if model._family != _lib.TR_FAMILY_DYVIT:
        return out
    # dyvit.py:257-261: (x, features, prev_decision.detach(), out_pred_prob) with the DyViT distillation scheme, else (x, out_pred_prob)
    n_st = len(model.pruning_loc)
    logits, preds = out[0], list(out[1: 1 + n_st])
    if getattr(model, "dyvit_distillation", False):
        return logits, out[1 + n_st], preds[-1].detach().unsqueeze(-1), preds
    return logits, preds
