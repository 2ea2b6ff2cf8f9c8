"""The argument checks of tdrn_amp_check_finite, tdrn_sgd_step_scaled and tdrn_amp_update (tdrn_hip.h section i-m): every
TDRN_E_ARG / TDRN_E_UNSUPPORTED case is decided on the host, before any launch, so each of them returns its code on a machine
without a GPU.  The device addresses here are made up; nothing reads them.  (That the symbols, the header and _lib._SIGS agree is
test_abi.py's check.)"""
import ctypes as C

import pytest

from tdrn_amd import _lib

E_ARG, E_UNSUPPORTED = -1, -4
P, G, B, HYPER, STATE = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # made-up device addresses
GOOD = (P, G, B, 8, 0)
BIG = 1 << 31


def _recs(*rows):
    arr = (_lib.SgdTensor * max(1, len(rows)))()
    for r, (p, g, b, numel, group) in zip(arr, rows):
        r.param, r.grad, r.momentum_buf, r.numel, r.group = p, g, b, numel, group
    return arr


def _addr(a):
    return C.c_void_p(a) if a else None


def _check(recs, n, state=STATE):
    return _lib.lib().tdrn_amp_check_finite(C.cast(recs, C.c_void_p) if recs is not None else None, n, _addr(state), None)


def _step(recs, n, hyper=HYPER, n_groups=1, state=STATE, flags=0):
    return _lib.lib().tdrn_sgd_step_scaled(C.cast(recs, C.c_void_p) if recs is not None else None, n, _addr(hyper), n_groups,
                                           _addr(state), flags, None)


def _update(state=STATE, growth=2.0, backoff=0.5, interval=2000):
    return _lib.lib().tdrn_amp_update(_addr(state), growth, backoff, interval, None)


@pytest.mark.parametrize("what,recs,n,kw", [
    ("null tensors_host", None, 1, {}),
    ("null hyper_dev", _recs(GOOD), 1, dict(hyper=0)),
    ("n_tensors < 0", _recs(GOOD), -1, {}),
    ("n_groups < 1", _recs(GOOD), 1, dict(n_groups=0)),
    ("n_groups < 1 with no tensors", _recs(), 0, dict(n_groups=0)),
    ("null state_dev", _recs(GOOD), 1, dict(state=0)),
    ("null state_dev with no tensors", _recs(), 0, dict(state=0)),
    ("state_dev 4 bytes off the 16-byte grid", _recs(GOOD), 1, dict(state=STATE + 4)),
    ("state_dev 8 bytes off the 16-byte grid", _recs(GOOD), 1, dict(state=STATE + 8)),
    ("group above range", _recs((P, G, B, 8, 1)), 1, {}),
    ("group above range, second of two groups", _recs(GOOD, (P, G, B, 8, 2)), 2, dict(n_groups=2)),
    ("group below range", _recs((P, G, B, 8, -1)), 1, {}),
    ("group out of range on a skipped tensor", _recs((P, 0, B, 8, 3)), 1, {}),
    ("negative numel", _recs((P, G, B, -1, 0)), 1, {}),
    ("negative numel on a tensor without grad", _recs((P, 0, B, -5, 0)), 1, {}),
    ("null param", _recs((0, G, B, 8, 0)), 1, {}),
    ("null momentum_buf", _recs((P, G, 0, 8, 0)), 1, {}),
    ("null param in the last of many", _recs(*([GOOD] * 200 + [(0, G, B, 8, 0)])), 201, {}),
    ("unknown flag bit", _recs(GOOD), 1, dict(flags=2)),
    ("unknown flag bit beside the known one", _recs(GOOD), 1, dict(flags=5)),
    ("an argument error behind a tensor that is too large", _recs((P, G, B, BIG, 0), (0, G, B, 8, 0)), 2, {}),
    ("a misaligned state behind a tensor that is too large", _recs((P, G, B, BIG, 0)), 1, dict(state=STATE + 4)),
])
def test_scaled_step_argument_errors_return_before_any_launch(what, recs, n, kw):
    assert _step(recs, n, **kw) == E_ARG, what


@pytest.mark.parametrize("what,recs,n,kw", [
    ("null tensors_host", None, 1, {}),
    ("n_tensors < 0", _recs(GOOD), -1, {}),
    ("null state_dev", _recs(GOOD), 1, dict(state=0)),
    ("null state_dev with no tensors", _recs(), 0, dict(state=0)),
    ("state_dev off the 16-byte grid", _recs(GOOD), 1, dict(state=STATE + 12)),
    ("negative group", _recs((P, G, B, 8, -1)), 1, {}),
    ("negative numel", _recs((P, G, B, -1, 0)), 1, {}),
    ("negative numel on a tensor without grad", _recs((P, 0, B, -5, 0)), 1, {}),
    ("a negative numel in the last of many", _recs(*([GOOD] * 200 + [(0, G, 0, -8, 0)])), 201, {}),
    ("an argument error behind a tensor that is too large", _recs((0, G, 0, BIG, 0), (0, G, 0, -1, 0)), 2, {}),
])
def test_check_finite_argument_errors_return_before_any_launch(what, recs, n, kw):
    assert _check(recs, n, **kw) == E_ARG, what


@pytest.mark.parametrize("numel", [BIG, BIG + 5, 1 << 40])
def test_two_to_the_31_elements_or_more_are_unsupported(numel):
    for call in (_step, _check):
        assert call(_recs((P, G, B, numel, 0)), 1) == E_UNSUPPORTED
        assert call(_recs(GOOD, (P, G, B, numel, 0)), 2) == E_UNSUPPORTED     # before the good tensor's launch
    assert _check(_recs((0, G, 0, numel, 0)), 1) == E_UNSUPPORTED             # the check asks for neither param nor momentum_buf


@pytest.mark.parametrize("what,kw", [
    ("null state_dev", dict(state=0)),
    ("state_dev off the 16-byte grid", dict(state=STATE + 4)),
    ("growth_factor 1", dict(growth=1.0)),
    ("growth_factor below 1", dict(growth=0.5)),
    ("growth_factor NaN", dict(growth=float("nan"))),
    ("backoff_factor 0", dict(backoff=0.0)),
    ("backoff_factor 1", dict(backoff=1.0)),
    ("backoff_factor above 1", dict(backoff=1.5)),
    ("backoff_factor negative", dict(backoff=-0.5)),
    ("backoff_factor NaN", dict(backoff=float("nan"))),
    ("growth_interval 0", dict(interval=0)),
    ("growth_interval negative", dict(interval=-3)),
    ("growth_interval 1 << 24", dict(interval=1 << 24)),
    ("growth_interval far above", dict(interval=(1 << 31) - 1)),
])
def test_update_argument_errors_return_before_any_launch(what, kw):
    assert _update(**kw) == E_ARG, what


def test_nothing_to_do_is_ok_without_a_device():
    """no tensors, or only skipped ones (numel 0, null grad: their other pointers may be null, as an empty tensor's are)"""
    skipped = ((0, 0, 0, 0, 0), (P, 0, B, 8, 0), (0, G, 0, 0, 0), (P, 0, B, 1 << 40, 0))
    for call in (_step, _check):
        assert call(_recs(), 0) == 0
        assert call(_recs(*skipped), 4) == 0
    assert _check(_recs((0, 0, 0, 8, 7)), 1) == 0             # any group >= 0: the check has no rows to hold it against
