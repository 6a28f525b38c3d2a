"""numpy restatement of the dense feature maps (include/tokenreduction_hip.h, "Dense feature maps"): tr_dense_index and tr_dense_gather,
written image by image and patch by patch with no regard for speed, sharing nothing with the kernels.  Used by the CPU tests (on the
committed fixtures) and the GPU tests (against the kernels and the model)."""
import numpy as np

PRUNE, EVIT, ATS, CENTRES, TOME, SOFT = range(6)
MAPS = (CENTRES, TOME, SOFT)


def n_out(kind, n_in, k):
    """Patch rows that leave a stage."""
    if kind == EVIT:
        return k + 1
    if kind == ATS:
        return k - 1
    if kind == TOME:
        return n_in - 1 - min(k, (n_in - 1) // 2)
    return k


def dense_index(dec, stages, B, P0, n_last):
    """dec: {"kept": {blk: [B, W]}, "assign": {blk: [B, P_in]}} as forward_decisions / _decisions_ref.stage_decisions give it (numpy or
    anything np.asarray takes), stages: [(blk, kind, n_in, k)] in block order.  -> int32 [B, P0]: the row (1 ... n_last-1) of the last stream
    that stands for grid patch p, -1 where none does."""
    index = np.full((B, P0), -1, dtype=np.int32)
    rows = P0
    seen_map = False
    for blk, kind, n_in, k in stages:
        assert not (seen_map and kind not in MAPS), "a kept-only stage behind a stage with an assignment map"
        seen_map = seen_map or kind in MAPS
        rows = n_out(kind, n_in, k)
    assert rows == n_last - 1, (rows, n_last)
    for b in range(B):
        for p in range(P0):
            cur = p
            for blk, kind, n_in, k in stages:
                out = n_out(kind, n_in, k)
                if kind in MAPS:
                    a = np.asarray(dec["assign"][blk])[b]
                    assert len(a) == n_in - 1
                    if 0 <= cur < n_in - 1:
                        cur = int(a[cur])
                        if not 0 <= cur < out:
                            cur = -1
                    else:
                        cur = -1
                else:
                    lst = np.asarray(dec["kept"][blk])[b]
                    assert len(lst) == out
                    hits = np.nonzero(lst == p)[0]               # (0 <= p < P0: negative and large entries never match)
                    cur = int(hits[0]) if len(hits) else -1
            index[b, p] = cur + 1 if cur >= 0 else -1
    return index


def to_bf16_bits(a):
    """uint16 bits of fp32 `a` rounded to bf16, nearest even (no NaN expected)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    assert not np.isnan(a).any()
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def dense_gather(tokens, index, layout, dtype, fill):
    """tokens fp32 [B, n_rows, D], index int [B, P] -> [B, D, P] (layout "NCHW") or [B, P, D] ("NHWC"); dtype "fp32" (float32 array) or
    "bf16" (uint16 array holding the bits)."""
    tokens = np.asarray(tokens, dtype=np.float32)
    B, n_rows, D = tokens.shape
    P = index.shape[1]
    out = np.empty((B, P, D), dtype=np.float32)
    for b in range(B):
        for p in range(P):
            i = int(index[b, p])
            out[b, p] = tokens[b, i] if 0 <= i < n_rows else np.float32(fill)
    if layout == "NCHW":
        out = np.ascontiguousarray(out.transpose(0, 2, 1))
    else:
        assert layout == "NHWC", layout
    if dtype == "bf16":
        return to_bf16_bits(out)
    assert dtype == "fp32", dtype
    return out


def ats_valid_first(raw_ids):
    """The property the dense index of an ATS model rests on: in every row of a raw id slab [B, K] (column 0 the CLS id 0, then 1-based ids,
    0 = padding) the valid ids come first, strictly ascending, and the padding is at the END.  Asserts it."""
    ids = np.asarray(raw_ids)
    assert ids.ndim == 2 and (ids[:, 0] == 0).all(), "column 0 is the CLS id"
    for b, row in enumerate(ids[:, 1:]):
        n = int((row != 0).sum())
        assert (row[:n] > 0).all() and (row[n:] == 0).all(), f"image {b}: padding in front of a valid id"
        assert (np.diff(row[:n]) > 0).all(), f"image {b}: ids not sorted-unique"
    return True
