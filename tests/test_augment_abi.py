"""C ABI of the device SSDAugmentation (tdrn_hip.h section ii-c), no GPU needed: the symbols and the record layout exist, and
null pointers, bad sizes, a missing or doubled draw source and an oversized max_truths return their codes before any launch."""
import ctypes as C

from tdrn_amd import _lib

E_ARG, E_UNSUPPORTED = -1, -4
p = 4096            # fake non-NULL device pointers: these paths return before anything is enqueued


def test_symbols_and_record_layout():
    lib = _lib.lib()
    assert hasattr(lib, "tdrn_augment_sample") and hasattr(lib, "tdrn_augment_apply")
    assert C.sizeof(_lib.AugmentParams) == 80 and C.sizeof(_lib.AugmentImage) == 16
    assert _lib.AugmentParams.kept.offset == 72 and _lib.AugmentParams.crop_x0.offset == 48


def _sample(hw=p, truths=p, off=p, T=10, Tmax=8, B=2, ids=p, tape=None, tape_off=None, params=p, out=p, out_off=p):
    return _lib.lib().tdrn_augment_sample(hw, truths, off, T, Tmax, B, 7, ids, tape, tape_off, params, out, out_off, None)


def test_sample_errors_before_any_launch():
    assert _sample(Tmax=513) == E_UNSUPPORTED
    assert _sample(hw=None) == E_ARG and _sample(off=None) == E_ARG
    assert _sample(params=None) == E_ARG and _sample(out_off=None) == E_ARG
    assert _sample(truths=None) == E_ARG and _sample(out=None) == E_ARG          # NULL rows only with T_total = 0
    assert _sample(B=0) == E_ARG and _sample(T=-1) == E_ARG and _sample(Tmax=-1) == E_ARG
    assert _sample(ids=None) == E_ARG                                            # no draw source
    assert _sample(tape=p, tape_off=p) == E_ARG                                  # two draw sources
    assert _sample(ids=None, tape=p) == E_ARG and _sample(ids=None, tape_off=p) == E_ARG


def _apply(images=p, params=p, B=2, mean=(C.c_float * 3)(104, 117, 123), S=320, to_rgb=1, out=p):
    return _lib.lib().tdrn_augment_apply(images, params, B, mean, S, to_rgb, out, None)


def test_apply_errors_before_any_launch():
    assert _apply(images=None) == E_ARG and _apply(params=None) == E_ARG and _apply(out=None) == E_ARG
    assert _apply(mean=None) == E_ARG
    assert _apply(B=0) == E_ARG and _apply(S=0) == E_ARG and _apply(S=-3) == E_ARG
    assert _apply(S=2049) == E_UNSUPPORTED and _apply(B=65536) == E_UNSUPPORTED
