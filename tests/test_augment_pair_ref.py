"""The numpy restatement of the TRN pair chain (tests/_augment_pair_ref.py) against fixtures made by the reference's own
pull_translational_item and pairSSDAugmentation (tests/golden/make_golden_augment_pair.py), hand-worked known answers for the
translation rule and for the shifted frame's zero border, and the cross-check against the single chain.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as R  # noqa: E402
import _augment_pair_ref as P  # noqa: E402

F32 = np.float32
MEAN = (104, 117, 123)
FALLBACK_CASE = 5


def _cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "augment_pair_cases.npz"))
    return z, len({k.split("_")[0] for k in z.files})


def _replay(z, i):
    k = "c%02d_" % i
    H, W = (int(v) for v in z[k + "hw"])
    t = z[k + "target"]
    d = R.TapeDraws(z[k + "tape"])
    return k, H, W, t, d, P.sample_pair(W, H, t[:, :4], t[:, 4], d)


def test_fixture_covers_the_cases_asked_for(golden_dir):
    z, n = _cases(golden_dir)
    assert n == 16 and os.path.getsize(os.path.join(golden_dir, "augment_pair_cases.npz")) < 300 * 1024
    seen = dict(neg=0, pos=0, subpixel=0, second=0, third=0, fallback=0, border=0, drop_one=0, mirror=0, no_crop=0, tiny=0,
                pixels=0)
    for i in range(n):
        k, H, W, t, d, (p, b0, b1, l0, l1) = _replay(z, i)
        expand = (p["canvas_w"], p["canvas_h"]) != (W, H)
        crop = p["crop"] != (0, 0, p["canvas_w"], p["canvas_h"])
        fb = bool(p["status"] & P.ST_TRANS_FALLBACK)
        seen["neg"] += p["trans_x"] < 0 or p["trans_y"] < 0
        seen["pos"] += p["trans_x"] > 0 or p["trans_y"] > 0
        seen["subpixel"] += p["shift_x"] != 0 and p["trans_x"] == 0
        seen["second"] += p["attempts"] == 2
        seen["third"] += p["attempts"] == 3 and not fb
        seen["fallback"] += fb
        seen["border"] += expand and p["trans_x"] != 0 and p["trans_y"] != 0
        seen["mirror"] += p["mirror"]
        seen["no_crop"] += not crop
        seen["pixels"] += (k + "pixels0") in z.files
        assert fb == (i == FALLBACK_CASE)
        if crop:
            # a box whose centre is inside the rect in one frame only is dropped from both
            frac_t = P.translate(t[:, :4], R.TapeDraws(z[k + "tape"]), W, H)[1]
            masks = []
            for f in (t[:, :4], frac_t):
                b = f * (W, H, W, H) + (p["img_x"], p["img_y"]) * 2
                c = (b[:, :2] + b[:, 2:]) / 2.0
                r = p["crop"]
                masks.append((r[0] < c[:, 0]) & (r[1] < c[:, 1]) & (r[2] > c[:, 0]) & (r[3] > c[:, 1]))
            if (masks[0] != masks[1]).any():
                seen["drop_one"] += 1
                assert len(b0) == int((masks[0] & masks[1]).sum()) < int((masks[0] | masks[1]).sum())
    # case 10 keeps a crop whose left draw was uniform(W - w) with W - w < 1: the full width, fewer rows
    seen["tiny"] += tuple(z["c10_canvas"]) == (30, 40) and z["c10_crop"][1] == 40 and z["c10_crop"][0] < 30
    assert all(v >= 1 for v in seen.values()) and seen["pixels"] == 12, seen
    assert {int(z["c%02d_S" % i]) for i in range(12)} == {32, 48}
    assert all(max(z["c%02d_hw" % i]) <= 72 for i in range(12))


def test_restatement_reproduces_the_reference(golden_dir):
    z, n = _cases(golden_dir)
    for i in range(n):
        k, H, W, t, d, (p, b0, b1, l0, l1) = _replay(z, i)
        assert d.i == len(z[k + "tape"]) and not d.exhausted, i            # every draw consumed, in order
        assert (p["trans_x"], p["trans_y"]) == tuple(z[k + "trans"]) and p["attempts"] == int(z[k + "attempts"]), i
        assert (p["canvas_h"], p["canvas_w"]) == tuple(z[k + "canvas"]), i
        r = p["crop"]
        assert (r[3] - r[1], r[2] - r[0]) == tuple(z[k + "crop"]), i
        for got, name in ((b0, "boxes0"), (b1, "boxes1"), (l0, "labels0"), (l1, "labels1")):
            assert got.dtype == np.float64 and np.array_equal(got, z[k + name]), (i, name)      # bit for bit (fp64)
        assert len(b0) == len(b1) == p["kept"]
        if k + "pixels0" in z.files:
            x0, x1 = P.apply_pair(z[k + "image"], p, int(z[k + "S"]), MEAN, to_rgb=True)
            assert x0.dtype == F32 and np.array_equal(x0, z[k + "pixels0"]), i                  # pixels exact
            assert x1.dtype == F32 and np.array_equal(x1, z[k + "pixels1"]), i
    # the fallback's second truths are the first, unclipped, and its second frame is a copy
    assert np.array_equal(z["c05_boxes0"], z["c05_boxes1"]) and np.array_equal(z["c05_pixels0"], z["c05_pixels1"])


def test_tape_starts_with_the_translation_draws(golden_dir):
    z, n = _cases(golden_dir)
    for i in range(n):
        own = list(z["c%02d_owner" % i])
        a = int(z["c%02d_attempts" % i])
        assert own[:2 * a] == [0] * (2 * a) and 0 not in own[2 * a:], i      # rand() pairs first, then the chain's
        rest = own[2 * a:]
        assert rest == sorted(rest) and rest[0] == 1 and rest[-1] == 4, i    # distort, expand, crop, mirror (the last draw)


def test_identical_frames_reduce_to_the_single_chain(golden_dir):
    """Fed the first frame's truths as the second's, the pair chain consumes the single chain's draws and moves the boxes
    alike: the single fixture (the reference's SSDAugmentation) pins the pair restatement too."""
    z = np.load(os.path.join(golden_dir, "augment_cases.npz"))
    for i in range(len({k.split("_")[0] for k in z.files})):
        k = "c%02d_" % i
        H, W = (int(v) for v in z[k + "hw"])
        t = z[k + "target"]
        d = R.TapeDraws(z[k + "tape"])
        p, b0, b1, l0, l1 = P.sample_pair(W, H, t[:, :4], t[:, 4], d, frac_t=t[:, :4], labels_t=t[:, 4])
        ps = R.sample(W, H, t[:, :4], t[:, 4], R.TapeDraws(z[k + "tape"]))[0]
        assert d.i == len(z[k + "tape"]) and p["attempts"] == 0 and all(p[key] == ps[key] for key in ps), i
        assert np.array_equal(b0, z[k + "boxes"]) and np.array_equal(b1, z[k + "boxes"]), i
        assert np.array_equal(l0, z[k + "labels"]) and np.array_equal(l1, z[k + "labels"]), i


# ---------------------------------------------------------------- the translation rule, hand-worked (r = 0.1)
def test_translate_known_answers():
    box = np.array([[0.0, 0.1, 0.5, 0.6]])
    # attempt 1: x_trans = -0.1 + (0.3 * 2) * 0.1 = -0.04, y_trans = -0.1 + (0.9 * 2) * 0.1 = 0.08
    t, moved = P.translate(box, R.TapeDraws([0.3, 0.9]), W=40, H=30)
    assert t["attempts"] == 1 and not t["fallback"]
    assert abs(t["shift_x"] + 0.04) < 1e-15 and abs(t["shift_y"] - 0.08) < 1e-15
    assert (t["trans_x"], t["trans_y"]) == (-1, 2)               # int(-1.6) = -1 and int(2.4) = 2: toward zero, not floor
    assert moved[0, 0] == 0.0 and abs(moved[0, 2] - 0.46) < 1e-15              # x1 = -0.04 clipped to 0; the rest moved
    assert abs(moved[0, 1] - 0.18) < 1e-15 and abs(moved[0, 3] - 0.68) < 1e-15
    # u = 0.5 is no shift at all
    t, moved = P.translate(box, R.TapeDraws([0.5, 0.5]), W=40, H=30)
    assert (t["shift_x"], t["shift_y"], t["trans_x"], t["trans_y"]) == (0.0, 0.0, 0, 0) and np.array_equal(moved, box)
    # a sub-pixel shift moves the boxes and not the pixels: x_trans = -0.1 + 0.11 = 0.01, 0.01 * 40 = 0.4 -> 0
    t, moved = P.translate(box, R.TapeDraws([0.55, 0.5]), W=40, H=30)
    assert t["trans_x"] == 0 and abs(t["shift_x"] - 0.01) < 1e-15 and abs(moved[0, 0] - 0.01) < 1e-15


def test_translate_retries_and_falls_back():
    edge = np.array([[0.0, 0.2, 0.01, 0.4], [0.5, 0.5, 1.2, 0.9]])          # a centre at x = 0.005; a box past the right edge
    # attempt 1: u_x = 0 -> x_trans = -0.1, centre -0.095: rejected.  attempt 2: u = 0.5 -> -0.05 + (1 * 0.1) / 2 = 0: kept
    d = R.TapeDraws([0.0, 0.5, 0.5, 0.5])
    t, moved = P.translate(edge, d, W=40, H=30)
    assert t["attempts"] == 2 and not t["fallback"] and d.i == 4 and (t["shift_x"], t["trans_x"]) == (0.0, 0)
    assert np.array_equal(moved, np.clip(edge, 0, 1)) and moved[1, 2] == 1.0              # accepted: clipped
    # the ranges shrink: attempt 2 draws from +-0.05, attempt 3 from +-0.1 / 3
    t, _ = P.translate(np.array([[0.4, 0.4, 0.6, 0.6]]), R.TapeDraws([1.0, 1.0]), W=1000, H=1000)
    assert abs(t["shift_x"] - 0.1) < 1e-15 and t["trans_x"] in (99, 100)
    # three failures: six draws, no shift, the truths come back as they were -- NOT clipped
    d = R.TapeDraws([0.0, 0.5] * 3)
    t, moved = P.translate(edge, d, W=40, H=30)
    assert t["attempts"] == 3 and t["fallback"] and d.i == 6
    assert (t["shift_x"], t["shift_y"], t["trans_x"], t["trans_y"]) == (0.0, 0.0, 0, 0)
    assert np.array_equal(moved, edge) and moved[1, 2] == 1.2
    # a centre that lands exactly on 0 is outside: (0, 0.1) moved by -0.05 has the centre (-0.05 + 0.05) / 2 = 0
    t, _ = P.translate(np.array([[0.0, 0.2, 0.1, 0.4]]), R.TapeDraws([0.25, 0.5, 0.5, 0.5]), W=40, H=30)
    assert t["attempts"] == 2


def test_shifted_frame_has_a_zero_border():
    img = (np.arange(3 * 4 * 3) + 1).reshape(3, 4, 3).astype(np.uint8)          # no zero inside
    out = P.shift_frame(img, 1, -1)                                             # dst(x, y) = src(x - 1, y + 1)
    assert np.array_equal(out[0, 1], img[1, 0]) and np.array_equal(out[1, 3], img[2, 2])
    assert not out[:, 0].any() and not out[2].any() and out[:2, 1:].all()
    out = P.shift_frame(img, -2, 1)                                             # dst(x, y) = src(x + 2, y - 1)
    assert np.array_equal(out[1, 0], img[0, 2]) and np.array_equal(out[2, 1], img[1, 3])
    assert not out[0].any() and not out[:, 2:].any() and out[1:, :2].all()
    assert np.array_equal(P.shift_frame(img, 0, 0), img)
    assert not P.shift_frame(img, 4, 0).any() and not P.shift_frame(img, 0, -3).any()      # shifted out altogether


def test_black_border_is_distorted_like_a_pixel_and_only_the_canvas_gets_the_mean():
    """A black pixel goes through the HSV round trip (grey: s = 0) and comes out as (0 + brightness) * contrast."""
    p = R._params()
    p.update(brightness=F32(10), contrast_pre=F32(1.5), canvas_w=8, canvas_h=8, img_x=2, img_y=2, crop=(0, 0, 8, 8),
             trans_x=1, trans_y=0)
    img = np.full((4, 4, 3), 200, np.uint8)
    x0, x1 = P.apply_pair(img, p, 8, MEAN, to_rgb=False)
    assert np.array_equal(x1[:, 2:6, 2], np.full((3, 4), 15, F32) - np.array(MEAN, F32)[:, None])      # the border column
    assert np.array_equal(x1[:, 2:6, 3:6], x0[:, 2:6, 3:6]) and (x0[:, 2:6, 2:6] == x0[:, 2:3, 2:3]).all()
    assert not x1[:, :2].any() and not x1[:, :, :2].any() and not x0[:, 6:].any()                      # canvas: mean - mean


# ---------------------------------------------------------------- the generator regenerates the fixture byte for byte
def test_generator_regenerates_the_fixture(golden_dir, tmp_path):
    sys.path.insert(0, golden_dir)
    import ref_shim
    if not ref_shim.available():
        pytest.skip("the reference tree is not on this machine")
    subprocess.check_call([sys.executable, os.path.join(golden_dir, "make_golden_augment_pair.py"), str(tmp_path)],
                          stdout=subprocess.DEVNULL)
    with open(os.path.join(golden_dir, "augment_pair_cases.npz"), "rb") as a, open(tmp_path / "augment_pair_cases.npz", "rb") as b:
        assert a.read() == b.read()
