"""The tap entry points' host-side checks (no launch happens, so no GPU is needed): struct layout, NULL / shape / alignment refusals."""
import ctypes as C

from tokenreduction_amd import _lib


def test_taps_struct_layout_matches_the_header():
    assert C.sizeof(_lib.TrVitTaps) == 24                    # uint32 + padding, two pointers
    assert _lib.TrVitTaps.cls_out.offset == 8 and _lib.TrVitTaps.final_tokens_out.offset == 16
    assert len(_lib.SIGNATURES["tr_vit_forward_taps"][1]) == len(_lib.SIGNATURES["tr_vit_forward"][1]) + 1
    assert len(_lib.SIGNATURES["tr_vit_forward_pixels_taps"][1]) == len(_lib.SIGNATURES["tr_vit_forward_pixels"][1]) + 1


def test_tap_kernels_validate_before_launching():
    lib = _lib.load()
    p = 4096                                                  # any 16-byte aligned non-NULL address: nothing is dereferenced on the host
    assert lib.tr_cls_tap(None, 64, None, 0, None, 0, 0, p, 64, 1, 64, None) == -3
    assert lib.tr_cls_tap(p, 64, None, 0, p, 64, 0, p, 64, 1, 64, None) == -3          # a second operand without the first
    assert b"second pending operand" in lib.tr_last_error()
    assert lib.tr_cls_tap(p, 64, None, 0, None, 0, 0, p, 64, 1, 62, None) == -1         # D % 4
    assert lib.tr_cls_tap(p, 64, None, 0, None, 0, 0, p, 64, 1, 1028, None) == -1       # D > 1024
    assert lib.tr_cls_tap(p, 32, None, 0, None, 0, 0, p, 64, 1, 64, None) == -1         # stream stride below D
    assert lib.tr_cls_tap(p, 64, None, 0, None, 0, 0, p, 32, 1, 64, None) == -1         # destination stride below D
    assert lib.tr_cls_tap(p, 64, p + 8, 64, None, 0, 1, p, 64, 1, 64, None) == -1       # an fp32 operand at 8 bytes
    assert lib.tr_cls_tap(p, 64, p, 64, None, 0, 0, p + 4, 64, 1, 64, None) == -2       # destination not 16-byte aligned
    assert lib.tr_cls_tap(p, 64, None, 0, None, 0, 0, p, 64, 0, 64, None) == -1         # no rows
    assert lib.tr_final_tokens_f32(p, None, None, 0, p, p, None, 1, 64, 1e-6, None) == -3
    assert lib.tr_final_tokens_f32(p, None, p, 0, p, p, p, 1, 64, 1e-6, None) == -3
    assert lib.tr_final_tokens_f32(p, None, None, 0, p, p, p, 1, 2048, 1e-6, None) == -1
    assert lib.tr_final_tokens_f32(p, p + 4, None, 0, p, p, p, 1, 64, 1e-6, None) == -2


def test_forward_taps_needs_its_struct():
    lib = _lib.load()
    cfg, W = _lib.TrVitConfig(), _lib.TrVitWeights()
    args = (4096, 4096, 4096, 0, None, None, None, None, None, None, 1, None)
    assert lib.tr_vit_forward_taps(C.byref(cfg), C.byref(W), *args, None) == -3
    assert b"tr_vit_taps" in lib.tr_last_error()
    assert lib.tr_vit_forward_pixels_taps(C.byref(cfg), C.byref(W), 4096, 0, None, *args[1:], None) == -3
