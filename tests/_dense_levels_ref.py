"""numpy restatement of the multi-level dense feature maps (include/tokenreduction_hip.h, tr_dense_index_levels / tr_dense_gather_levels), on
top of tests/_dense_ref.py: a level is the stream after one block, and stands behind the stages at or before that block."""
import numpy as np

from tests import _dense_ref as ref


def level_stages(stages, block):
    """The prefix of `stages` [(blk, kind, n_in, k)] that the stream after `block` is behind."""
    return [st for st in stages if st[0] <= block]


def level_rows(stages, P0, block):
    """Tokens (CLS included) of the stream after `block` according to the stage table."""
    pre = level_stages(stages, block)
    return (ref.n_out(*pre[-1][1:]) if pre else P0) + 1


def dense_index_levels(dec, stages, B, P0, level_blocks, rows=None):
    """-> int32 [L, B, P0]: level l's index is _dense_ref.dense_index on the stages with block <= level_blocks[l]; a level in front of every
    stage is the identity 1 ... P0.  rows (optional): the token counts the caller saw, checked against the table."""
    assert list(level_blocks) == sorted(set(level_blocks)), "level blocks strictly ascending"
    out = np.empty((len(level_blocks), B, P0), dtype=np.int32)
    done = {}                                                    # levels between the same pair of stages share a prefix: computed once
    for l, blk in enumerate(level_blocks):
        pre = level_stages(stages, blk)
        n = level_rows(stages, P0, blk)
        assert rows is None or rows[l] == n, (l, blk, rows[l], n)
        if len(pre) not in done:
            done[len(pre)] = ref.dense_index(dec, pre, B, P0, n) if pre else np.tile(np.arange(1, P0 + 1, dtype=np.int32), (B, 1))
        out[l] = done[len(pre)]
    return out


def dense_gather_levels(tokens, index, layout, dtype, fill):
    """tokens: a list of L fp32 arrays [B, n_rows_l, D]; index int [L, B, P] -> [L, B, D, P] or [L, B, P, D]: _dense_ref.dense_gather per level."""
    assert len(tokens) == index.shape[0]
    return np.stack([ref.dense_gather(tokens[l], index[l], layout, dtype, fill) for l in range(len(tokens))])
