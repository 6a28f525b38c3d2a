"""Launch records of the HIP library's profiler (tr_profile_begin / tr_profile_end), shared by the tests that look at which kernels ran."""
import ctypes as C

import torch


def record(fn, cap=4096):
    """[(label, flops, bytes)] of the launches fn() enqueues through the library on the current stream, in launch order."""
    from tokenreduction_amd import _lib
    lib = _lib.load()
    labels = C.create_string_buffer(48 * cap)
    flops, nbytes = (C.c_double * cap)(), (C.c_double * cap)()
    assert lib.tr_profile_begin(torch.cuda.current_stream().cuda_stream) == 0
    try:
        fn()
    finally:
        n = lib.tr_profile_end(cap, labels, None, flops, nbytes)
    assert 0 <= n <= cap, n
    return [(labels.raw[48 * i:48 * (i + 1)].split(b"\0")[0].decode(), flops[i], nbytes[i]) for i in range(n)]


def labels(fn, cap=4096):
    return [rec[0] for rec in record(fn, cap)]


def forward_launches(model, x, cap=4096):
    """record() of one plain-launch forward of `model` (hipGraph replay off), after one warm-up forward."""
    graph, model.use_graph = model.use_graph, False
    try:
        model(x)
        torch.cuda.synchronize()
        recs = record(lambda: model(x), cap)
    finally:
        model.use_graph = graph
    assert recs
    return recs
