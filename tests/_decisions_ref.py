"""numpy restatement of tr_stage_decisions (include/tokenreduction_hip.h, "Decision taps"): the executor's raw stage slabs -> the kept
lists / kept counts / assignment maps of validate.py's `Stage-{loc}` records, written image by image with no regard for speed.  Shared by the
CPU tests (on the committed fixtures) and the GPU tests (against the kernel).  Also: the raw slabs a forward would have written for the
decisions a fixture recorded (slabs_from_fixture), so the CPU tier can run the restatement on real decisions."""
import os

import numpy as np

PRUNE, EVIT, ATS, CENTRES, TOME, SOFT = range(6)
BAD = -2
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _through(lst, rel):
    """lst[rel] where rel indexes lst, BAD elsewhere."""
    rel = np.asarray(rel, dtype=np.int64)
    ok = (rel >= 0) & (rel < len(lst))
    out = np.full(rel.shape, BAD, dtype=np.int64)
    out[ok] = np.asarray(lst, dtype=np.int64)[rel[ok]]
    return out


def stage_decisions(kept_idx, compl_idx, soft, stages, B, N0):
    """kept_idx / compl_idx: flat int slabs (block blk at blk * B * N0), soft: flat fp32 (the SOFT stages' [B, k, P] back to back), stages:
    [(blk, kind, n_in, k)] in block order.  -> {"stages", "kept": {blk: [B, W]}, "kept_count": {blk: [B]}, "assign": {blk: [B, P]}}, int64."""
    out = {"stages": tuple(s[0] for s in stages), "kept": {}, "kept_count": {}, "assign": {}}
    prev = [None] * B                                         # per image: the previous stage's list (None: the input grid)
    soft_off = 0
    for blk, kind, n_in, k in stages:
        base, P = blk * B * N0, n_in - 1
        if kind in (PRUNE, EVIT, CENTRES):
            rel = np.asarray(kept_idx[base: base + B * k], dtype=np.int64).reshape(B, k)
            W = k + 1 if kind == EVIT else k
            rows = np.full((B, W), -1, dtype=np.int64)
            for b in range(B):
                v = _through(np.arange(P) if prev[b] is None else prev[b], rel[b])
                if kind == EVIT:
                    v[rel[b] == -1] = -1                       # numpy's prev[-1]: the trailing -1 of the list before
                rows[b, :k] = v
                prev[b] = rows[b].copy()
            out["kept"][blk], out["kept_count"][blk] = rows, np.full(B, W, dtype=np.int64)
            if kind == CENTRES:
                out["assign"][blk] = np.asarray(compl_idx[base: base + B * P], dtype=np.int64).reshape(B, P).copy()
        elif kind == ATS:
            ids = np.asarray(kept_idx[base: base + B * k], dtype=np.int64).reshape(B, k)[:, 1:]
            W = k - 1
            rows, count = np.full((B, W), -1, dtype=np.int64), np.zeros(B, dtype=np.int64)
            for b in range(B):
                valid = ids[b] != 0
                count[b] = valid.sum()
                if prev[b] is None:                            # as is, the padding as -1
                    rows[b, valid] = _through(np.arange(P), ids[b, valid] - 1)
                    prev[b] = rows[b].copy()
                else:                                          # the padding dropped, order kept
                    v = _through(prev[b], ids[b, valid] - 1)
                    rows[b, :len(v)] = v
                    prev[b] = v
            out["kept"][blk], out["kept_count"][blk] = rows, count
        elif kind == TOME:
            na, nb = (n_in + 1) // 2, n_in // 2
            r = min(k, (n_in - 1) // 2)
            slab = np.asarray(kept_idx[base: base + B * (na + r)], dtype=np.int64)
            unm, src, dst = slab[:B * (na - r)].reshape(B, na - r), slab[B * (na - r): B * na].reshape(B, r), slab[B * na:].reshape(B, r)
            maps = np.empty((B, n_in - 1), dtype=np.int64)
            for b in range(B):
                pos_a = np.full(na, BAD + 1, dtype=np.int64)
                for j, u in enumerate(unm[b]):
                    if 0 <= u < na:
                        pos_a[u] = j
                for u, d in zip(src[b], dst[b]):
                    if 0 <= u < na:
                        pos_a[u] = (na - r) + d if 0 <= d < nb else BAD + 1
                full = np.empty(n_in, dtype=np.int64)
                full[0::2] = pos_a
                full[1::2] = (na - r) + np.arange(nb)
                maps[b] = (full - 1)[1:]
            out["assign"][blk] = maps
        elif kind == SOFT:
            a = np.asarray(soft[soft_off: soft_off + B * k * P], dtype=np.float32).reshape(B, k, P)
            soft_off += B * k * P
            out["assign"][blk] = np.argmax(a, axis=1).astype(np.int64)
        else:
            raise ValueError(kind)
    return out


def ats_width(sample_count):
    """Static width of an ATS stage's id slab: one token per grid point of ats.py:48 plus CLS."""
    import torch
    return int(torch.arange(1 / (2 * sample_count), (2 * sample_count - 1) / (2 * sample_count), 2 / (2 * sample_count)).numel()) + 1


def slabs_from_fixture(name, case):
    """(kept_idx, compl_idx, soft, stages, B, N0, viz_data) for a golden fixture: the raw slabs the executor writes for the decisions the
    fixture recorded (tests/golden/<name>.npz holds them in viz_data form), and that viz_data."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    fam, locs = case["family"], list(case["reduction_loc"])
    P0 = (case.get("img_size", 224) // 16) ** 2
    N0, depth = P0 + 1, case["depth"]
    first = next(g[k] for k in g.files if k.split("_")[0] in ("kept", "assign", "keptabs"))
    B = first.shape[0]
    kept_idx, compl_idx = np.zeros(depth * B * N0, dtype=np.int32), np.zeros(depth * B * N0, dtype=np.int32)
    soft, stages, viz = [], [], {}
    n_in = N0

    def put(arr, blk, rows, at=0):
        flat = np.asarray(rows).reshape(-1)
        arr[blk * B * N0 + at: blk * B * N0 + at + flat.size] = flat

    for j, blk in enumerate(locs):
        if fam in ("topk", "dyvit", "evit"):
            rec = g[f"kept_{blk}"]
            rel = rec[:, :-1] if fam == "evit" else rec
            put(kept_idx, blk, rel)
            stages.append((blk, EVIT if fam == "evit" else PRUNE, n_in, rel.shape[1]))
            viz.setdefault("Kept_Tokens", {})[blk] = rec
            n_in = rel.shape[1] + (2 if fam == "evit" else 1)
        elif fam in ("dpcknn", "kmedoids"):
            rec, asg = g[f"kept_{blk}"], g[f"assign_{blk}"]
            put(kept_idx, blk, rec)
            put(compl_idx, blk, asg)
            stages.append((blk, CENTRES, n_in, rec.shape[1]))
            viz.setdefault("Kept_Tokens", {})[blk] = rec
            viz.setdefault("Assignment_Maps", {})[blk] = asg
            n_in = rec.shape[1] + 1
        elif fam == "ats":
            rec = g[f"kept_{blk}"]                             # [B, batch maximum], -1 padding (ats.py:78, :253)
            K = ats_width(int(case["keep_rate"][0] ** (j + 1) * P0) + 1)
            ids = np.zeros((B, K), dtype=np.int64)
            ids[:, 1:1 + rec.shape[1]] = rec + 1
            put(kept_idx, blk, ids)
            stages.append((blk, ATS, n_in, K))
            viz.setdefault("Kept_Tokens", {})[blk] = rec
            n_in = K
        elif fam == "tome":
            asg = g[f"assign_{blk}"]                           # (out - 1)[1:]; the CLS token is position 0 of the output
            n_out = (g[f"assign_{locs[j + 1]}"].shape[1] if j + 1 < len(locs) else int(asg.max()) + 1) + 1
            r, na = n_in - n_out, (n_in + 1) // 2
            full = np.concatenate([np.zeros((B, 1), dtype=np.int64), asg + 1], axis=1)
            pos_a = full[:, 0::2]
            unm, src, dst = np.zeros((B, na - r), np.int64), np.zeros((B, r), np.int64), np.zeros((B, r), np.int64)
            for b in range(B):
                merged = np.nonzero(pos_a[b] >= na - r)[0]
                alone = np.nonzero(pos_a[b] < na - r)[0]
                unm[b, pos_a[b, alone]] = alone
                src[b], dst[b] = merged, pos_a[b, merged] - (na - r)
            put(kept_idx, blk, unm)
            put(kept_idx, blk, src, B * (na - r))
            put(kept_idx, blk, dst, B * na)
            stages.append((blk, TOME, n_in, r))
            viz.setdefault("Assignment_Maps", {})[blk] = asg
            n_in = n_out
        elif fam in ("sit", "sinkhorn", "patchmerger"):
            # the fixture keeps the first 8 rows of the [B, K, P] matrix and the argmax over all K: rows 8 ... K-1 are filled in so that
            # the recorded assignment is the (first) maximum of every column -- below the recorded rows where one of them wins
            head, asg = g[f"soft_{blk}"], g[f"assign_{blk}"]
            K = int(P0 * case["keep_rate"][0] ** (j + 1))
            a = np.full((B, K, n_in - 1), -1.0, dtype=np.float32)
            a[:, :head.shape[1]] = head
            for b in range(B):
                late = np.nonzero(asg[b] >= head.shape[1])[0]
                a[b, asg[b, late], late] = head[b][:, late].max(axis=0) + 1.0
            soft.append(a.reshape(-1))
            stages.append((blk, SOFT, n_in, K))
            viz.setdefault("Assignment_Maps", {})[blk] = asg
            n_in = K + 1
        else:
            raise ValueError(fam)
    soft = np.concatenate(soft).astype(np.float32) if soft else np.zeros(0, dtype=np.float32)
    return kept_idx, compl_idx, soft, stages, B, N0, viz
