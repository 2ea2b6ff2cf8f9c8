"""tdrn_sgd_step's argument checks (tdrn_hip.h section i-j): every TDRN_E_ARG / TDRN_E_UNSUPPORTED case is decided on the host,
before any launch, so each of them returns its code on a machine without a GPU.  The device addresses here are made up; nothing
reads them.  (That the symbol, the header and _lib._SIGS agree is test_abi.py's check.)"""
import ctypes as C
import re
import os

import pytest

from tdrn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -4
P, G, B, HYPER = 0x10000, 0x20000, 0x30000, 0x40000      # made-up device addresses


def _recs(*rows):
    arr = (_lib.SgdTensor * max(1, len(rows)))()
    for r, (p, g, b, numel, group) in zip(arr, rows):
        r.param, r.grad, r.momentum_buf, r.numel, r.group = p, g, b, numel, group
    return arr


def _call(recs, n, hyper=HYPER, n_groups=1, flags=0):
    return _lib.lib().tdrn_sgd_step(C.cast(recs, C.c_void_p) if recs is not None else None, n, C.c_void_p(hyper) if hyper else None,
                                    n_groups, flags, None)


GOOD = (P, G, B, 8, 0)


@pytest.mark.parametrize("what,recs,n,kw", [
    ("null tensors_host", None, 1, {}),
    ("null hyper_dev", _recs(GOOD), 1, dict(hyper=0)),
    ("n_tensors < 0", _recs(GOOD), -1, {}),
    ("n_groups < 1", _recs(GOOD), 1, dict(n_groups=0)),
    ("n_groups < 1 with no tensors", _recs(), 0, dict(n_groups=0)),
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
    ("an argument error behind a tensor that is too large", _recs((P, G, B, 1 << 31, 0), (0, G, B, 8, 0)), 2, {}),
])
def test_argument_errors_return_before_any_launch(what, recs, n, kw):
    assert _call(recs, n, **kw) == E_ARG, what


@pytest.mark.parametrize("numel", [1 << 31, (1 << 31) + 5, 1 << 40])
def test_two_to_the_31_elements_or_more_are_unsupported(numel):
    assert _call(_recs((P, G, B, numel, 0)), 1) == E_UNSUPPORTED
    assert _call(_recs(GOOD, (P, G, B, numel, 0)), 2) == E_UNSUPPORTED       # before the good tensor's launch


def test_nothing_to_do_is_ok_without_a_device():
    """no tensors, or only skipped ones (numel 0, null grad: their other pointers may be null, as an empty tensor's are)"""
    assert _call(_recs(), 0) == 0
    assert _call(_recs((0, 0, 0, 0, 0), (P, 0, B, 8, 0), (0, G, 0, 0, 0), (P, 0, B, 1 << 40, 0)), 4) == 0


def test_record_layout_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "tdrn_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} tdrn_sgd_tensor;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    fields = [(t.replace(" ", ""), n) for t, n in re.findall(r"(\w+\s*\*?)\s*(\w+);", body)]
    assert fields == [("float*", "param"), ("float*", "grad"), ("float*", "momentum_buf"), ("int64_t", "numel"),
                      ("int32_t", "group"), ("int32_t", "reserved")]
    assert [n for n, _ in _lib.SgdTensor._fields_] == [n for _, n in fields]
    assert C.sizeof(_lib.SgdTensor) == 40
    assert re.search(r"#define TDRN_SGD_ZERO_GRADS (\d+)", hdr).group(1) == str(_lib.SGD_ZERO_GRADS)
    assert "bitwise reproducible" in hdr[hdr.index("(i-j)"):hdr.index("(ii) NMS")]
