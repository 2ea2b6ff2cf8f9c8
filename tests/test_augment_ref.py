"""The numpy restatement of SSDAugmentation (tests/_augment_ref.py) against fixtures made by the reference's own
SSDAugmentation (tests/golden/make_golden_augment.py), and hand-worked known answers for the two cv2 legs it restates.
CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as R  # noqa: E402

F32 = np.float32


def _cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "augment_cases.npz"))
    n = len({k.split("_")[0] for k in z.files})
    return z, n


def test_fixture_covers_the_cases_asked_for(golden_dir):
    z, n = _cases(golden_dir)
    assert n == 24
    kinds = dict(expand=0, no_crop=0, mirror=0, pixels=0)
    for i in range(n):
        k = "c%02d_" % i
        H, W = z[k + "hw"]
        p, _, _ = R.sample(W, H, z[k + "target"][:, :4], z[k + "target"][:, 4], R.TapeDraws(z[k + "tape"]))
        kinds["expand"] += (p["canvas_w"], p["canvas_h"]) != (W, H)
        kinds["no_crop"] += p["crop"] == (0, 0, p["canvas_w"], p["canvas_h"])
        kinds["mirror"] += p["mirror"]
        kinds["pixels"] += (k + "pixels") in z.files
        assert 1 <= len(z[k + "target"]) <= 8
    assert all(v >= 3 for v in kinds.values()), kinds
    # case 1 keeps a crop whose left draw was uniform(W - w) with W - w < 1 (left in [W - w, 1)): the full width, fewer rows
    assert tuple(z["c01_canvas"]) == (30, 40) and z["c01_crop"][1] == 40 and z["c01_crop"][0] < 30


def test_restatement_reproduces_the_reference(golden_dir):
    z, n = _cases(golden_dir)
    for i in range(n):
        k = "c%02d_" % i
        H, W = (int(v) for v in z[k + "hw"])
        t = z[k + "target"]
        d = R.TapeDraws(z[k + "tape"])
        p, boxes, labels = R.sample(W, H, t[:, :4], t[:, 4], d)
        assert d.i == len(z[k + "tape"]) and not d.exhausted, i            # every draw consumed, in order
        assert (p["canvas_h"], p["canvas_w"]) == tuple(z[k + "canvas"]), i
        r = p["crop"]
        assert (r[3] - r[1], r[2] - r[0]) == tuple(z[k + "crop"]), i
        assert boxes.dtype == np.float64 and np.array_equal(boxes, z[k + "boxes"]), i       # bit for bit (fp64)
        assert np.array_equal(labels, z[k + "labels"]), i
        if k + "pixels" in z.files:
            x = R.apply(z[k + "image"], p, int(z[k + "S"]), (104, 117, 123), to_rgb=True)
            assert x.dtype == F32 and np.array_equal(x, z[k + "pixels"]), i                 # pixels exact


def test_tape_owners_follow_the_reference_order(golden_dir):
    """The recorded draws come from the transforms in the order the device sampler consumes them."""
    z, n = _cases(golden_dir)
    order = [0, 1, 2, 3, 4, 2, 5, 6, 7, 8]           # brightness, distort choice, contrast / sat / hue / contrast, ...
    for i in range(n):
        own = list(z["c%02d_owner" % i])
        ranks = [order.index(o) if o != 2 else None for o in own]
        seen = [r for r in ranks if r is not None]
        assert seen == sorted(seen), i
        assert own[-1] == 8                            # mirror is always the last draw


# ---------------------------------------------------------------- cv2 BGR <-> HSV, fp32, hand-worked
def hsv(b, g, r):
    return R.bgr2hsv(np.array([[[b, g, r]]], F32))[0, 0]


def bgr(h, s, v):
    return R.hsv2bgr(np.array([[[h, s, v]]], F32))[0, 0]


def test_bgr2hsv_known_answers():
    # grey: diff 0 -> s = 0, h = (g - b) * (60 / eps) = 0
    assert list(hsv(100, 100, 100)) == [0, 0, 100]
    # pure hues: s = 255 / (255 + eps) = 1 (eps is below half an ulp of 255)
    assert list(hsv(255, 0, 0)) == [240, 1, 255]          # blue:  (r - g) * d + 240
    assert list(hsv(0, 255, 0)) == [120, 1, 255]          # green: (b - r) * d + 120
    assert list(hsv(0, 0, 255)) == [0, 1, 255]            # red:   (g - b) * d
    # > 255: v = r = 360, diff = 120, d = 0.5, h = (240 - 300) * 0.5 = -30 -> 330; s = 120 / 360 in fp32
    assert list(hsv(300, 240, 360)) == [330, F32(120) / F32(360), 360]
    # negative: v = g = 0, diff = 120, s = 120 / FLT_EPSILON = 120 * 2^23, h = (b - r) * 0.5 + 120 = 150
    assert list(hsv(-60, 0, -120)) == [150, 120 * 2 ** 23, 0]
    # all negative: v = b = -10, vmin = -30, diff = 20, d = 3, s = 20 / 10 = 2, h = (r - g) * 3 + 240 = 210
    assert list(hsv(-10, -20, -30)) == [210, 2, -10]


def test_hsv2bgr_known_answers():
    assert list(bgr(37, 0, 80)) == [80, 80, 80]            # s = 0: grey whatever h
    assert list(bgr(0, 1, 255)) == [0, 0, 255]             # sector 0: (b, g, r) = (v(1-s), v(1-s(1-h)), v)
    assert list(bgr(0, 0.5, 200)) == [100, 100, 200]
    # h = 360: 360 * (6/360 in fp32) = 6.0000005 >= 6 -> 4.8e-7, sector 0: nearly red, b exactly v(1 - s) = 0
    b, g, r = bgr(360, 1, 100)
    assert b == 0 and r == 100 and 0 < g < 1e-4
    # h = 120 -> 2.0000002, sector 2 {3, 0, 1}: b = v(1 - s(1 - h)) ~ 0, g = v, r = v(1 - s) = 0
    b, g, r = bgr(120, 1, 255)
    assert g == 255 and r == 0 and 0 <= b < 1e-3
    # s > 1 and v < 0 are carried through without a clamp: sector 0, tab[1] = v(1 - s) = -10 * -1 = 10
    assert list(bgr(0, 2, -10)) == [10, 10, -10]


def test_hsv_round_trip_is_not_the_identity():
    rs = np.random.RandomState(0)
    x = rs.randint(0, 256, size=(64, 64, 3)).astype(F32)
    y = R.hsv2bgr(R.bgr2hsv(x))
    assert np.abs(y - x).max() < 1e-3 and not np.array_equal(y, x)


# ---------------------------------------------------------------- cv2.resize INTER_LINEAR, fp32
def test_resize_known_answers():
    x = np.arange(5 * 5 * 3, dtype=F32).reshape(5, 5, 3) * F32(1.5)
    assert np.array_equal(R.resize(x, 5), x)                                        # identity: f = d exactly, weights (1, 0)
    row = np.array([0, 10, 20, 50], F32)
    img = np.repeat(np.repeat(row[None, :, None], 4, 0), 3, 2)                      # 4x4, constant columns
    y = R.resize(img, 2)                                                            # 2:1: f = 0.5, 2.5 -> half and half
    assert np.array_equal(y[0, :, 0], np.array([5, 35], F32))
    img = np.repeat(np.repeat(np.array([0, 100], F32)[None, :, None], 2, 0), 3, 2)  # 1:2 with the border clamp
    y = R.resize(img, 4)                                                            # f = -0.25 (clamped), 0.25, 0.75, 1.25 (clamped)
    assert np.array_equal(y[0, :, 0], np.array([0, 25, 75, 100], F32))
    assert np.array_equal(y[1], y[0])


# ---------------------------------------------------------------- the generator regenerates the fixture byte for byte
def test_generator_regenerates_the_fixture(golden_dir, tmp_path):
    sys.path.insert(0, golden_dir)
    import ref_shim
    if not ref_shim.available():
        pytest.skip("the reference tree is not on this machine")
    subprocess.check_call([sys.executable, os.path.join(golden_dir, "make_golden_augment.py"), str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    with open(os.path.join(golden_dir, "augment_cases.npz"), "rb") as a, open(tmp_path / "augment_cases.npz", "rb") as b:
        assert a.read() == b.read()
