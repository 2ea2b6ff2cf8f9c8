"""C ABI of the device pairSSDAugmentation (tdrn_hip.h section ii-d), no GPU needed: the symbols and the 112-byte pair record
exist with the single record embedded unchanged at offset 0, and every bad argument returns its code before any launch."""
import ctypes as C

from tdrn_amd import _lib

E_ARG, E_UNSUPPORTED = -1, -4
p = 4096            # fake non-NULL device pointers: these paths return before anything is enqueued


def test_symbols_and_record_layout():
    lib = _lib.lib()
    assert hasattr(lib, "tdrn_augment_pair_sample") and hasattr(lib, "tdrn_augment_pair_apply")
    Q = _lib.AugmentPairParams
    assert C.sizeof(Q) == 112 and Q.base.offset == 0 and Q.base.size == 80
    assert (Q.shift_x.offset, Q.shift_y.offset) == (80, 88)
    assert (Q.trans_x.offset, Q.trans_y.offset, Q.attempts.offset, Q.reserved.offset) == (96, 100, 104, 108)
    # the single record did not move
    assert C.sizeof(_lib.AugmentParams) == 80 and C.sizeof(_lib.AugmentImage) == 16
    assert _lib.AugmentParams.kept.offset == 72 and _lib.AugmentParams.crop_x0.offset == 48
    assert (_lib.AUGMENT_CROP_FALLBACK, _lib.AUGMENT_TAPE_EXHAUSTED, _lib.AUGMENT_TRANS_FALLBACK) == (1, 2, 4)


def test_python_record_size_matches():
    from tdrn_amd.utils import augmentations as A
    assert A.PAIR_PARAMS_BYTES == 112 and A.PARAMS_BYTES == 80
    assert A.pairSSDAugmentation is A.PairSSDAugmentation


def _sample(hw=p, truths=p, truths_t=None, off=p, T=10, Tmax=8, B=2, r=0.1, ids=p, tape=None, tape_off=None, params=p, out=p,
            out_t=p, out_off=p):
    return _lib.lib().tdrn_augment_pair_sample(hw, truths, truths_t, off, T, Tmax, B, r, 7, ids, tape, tape_off, params, out,
                                               out_t, out_off, None)


def test_sample_errors_before_any_launch():
    assert _sample(Tmax=513) == E_UNSUPPORTED and _sample(Tmax=513, truths_t=p) == E_UNSUPPORTED
    assert _sample(hw=None) == E_ARG and _sample(off=None) == E_ARG
    assert _sample(params=None) == E_ARG and _sample(out_off=None) == E_ARG
    assert _sample(truths=None) == E_ARG and _sample(out=None) == E_ARG and _sample(out_t=None) == E_ARG
    assert _sample(B=0) == E_ARG and _sample(T=-1) == E_ARG and _sample(Tmax=-1) == E_ARG
    assert _sample(ids=None) == E_ARG                                            # no draw source
    assert _sample(tape=p, tape_off=p) == E_ARG                                  # two draw sources
    assert _sample(ids=None, tape=p) == E_ARG and _sample(ids=None, tape_off=p) == E_ARG
    for r in (-0.01, 1.0, 1.5, float("nan"), float("inf")):                      # max_trans_ratio outside [0, 1)
        assert _sample(r=r) == E_ARG, r


def _apply(images=p, images_t=None, params=p, B=2, mean=(C.c_float * 3)(104, 117, 123), S=320, to_rgb=1, out=p, out_t=p):
    return _lib.lib().tdrn_augment_pair_apply(images, images_t, params, B, mean, S, to_rgb, out, out_t, None)


def test_apply_errors_before_any_launch():
    assert _apply(images=None) == E_ARG and _apply(params=None) == E_ARG
    assert _apply(out=None) == E_ARG and _apply(out_t=None) == E_ARG and _apply(mean=None) == E_ARG
    assert _apply(B=0) == E_ARG and _apply(S=0) == E_ARG and _apply(S=-3) == E_ARG
    assert _apply(S=2049) == E_UNSUPPORTED and _apply(B=65536) == E_UNSUPPORTED
    assert _apply(S=2049, images_t=p) == E_UNSUPPORTED
