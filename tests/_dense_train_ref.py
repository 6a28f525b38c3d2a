"""numpy restatement of tr_dense_scatter (include/tokenreduction_hip.h, "Dense feature maps"): the adjoint of tests/_dense_ref.dense_gather,
written image by image and patch by patch with no regard for speed, sharing nothing with the kernel.  The summation contract is spelled
out: fp32, one addition after the other in ascending p, starting from +0."""
import numpy as np

from tests._dense_ref import to_bf16_bits


def bf16_bits_to_f32(bits):
    """fp32 array of the values a uint16 array of bf16 bits holds."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def dense_scatter(dmap, index, n_rows, layout, dtype="fp32"):
    """dmap [B, D, P] (layout "NCHW") or [B, P, D] ("NHWC"): a float32 array, or a uint16 array holding bf16 bits; index int [B, P].
    -> dtokens [B, n_rows, D]: float32 (dtype "fp32") or the uint16 bits of its round-to-nearest-even bf16 ("bf16")."""
    dmap = np.asarray(dmap)
    g = bf16_bits_to_f32(dmap) if dmap.dtype == np.uint16 else dmap.astype(np.float32, copy=False)
    if layout == "NCHW":
        g = g.transpose(0, 2, 1)
    else:
        assert layout == "NHWC", layout
    B, P, D = g.shape
    assert index.shape == (B, P), (index.shape, g.shape)
    out = np.zeros((B, n_rows, D), dtype=np.float32)
    for b in range(B):
        for p in range(P):                                       # ascending p: the order of the additions of every row
            r = int(index[b, p])
            if 0 <= r < n_rows:
                out[b, r] = out[b, r] + g[b, p]                  # float32 + float32, rounded once per addition
    if dtype == "bf16":
        return to_bf16_bits(out)
    assert dtype == "fp32", dtype
    return out
