"""Generate tests/golden/augment_pair_cases.npz by running the REFERENCE's own VOCDetection.pull_translational_item and
pairSSDAugmentation on CPU (build container only).

    python tests/golden/make_golden_augment_pair.py [DIR]    # writes the fixture next to this file (or into DIR)

The reference is imported through ref_shim; nothing of it is copied.  The stand-ins that make it run without files:
  - the dataset is object.__new__(VOCDetection) with one id, a stub ET.parse, a target_transform that returns the case's
    truths and cv2.imread returning the synthetic frame;
  - one recorder around a seeded RandomState stands in for data.voc0712's `np.random` (through a proxy of the module's `np`)
    and for utils.augmentations' `random`; it logs every value drawn, in order (the tape: the translation's rand() values
    first, then the chain's) with the class that drew it.  choice(a) is restated as a[randint(len(a))], as in
    make_golden_augment.py (numpy 2 rejects the reference's call on its ragged tuple of modes);
  - cv2.cvtColor and cv2.resize are _augment_ref's fp32 legs; cv2.warpAffine is _augment_pair_ref.shift_frame, the integer
    shift with a zero border (cv2 is not installed; all three legs rest on hand-worked known answers).
Frames are regenerated from seeds (_augment_ref.case_image); truths are case_boxes, or hand-made with a centre close to an
edge where a retry or the fallback is wanted (_augment_pair_ref.edge_boxes).  A case's seed is the first one at or after
its base seed whose draws, run through the restatement, show the property the case is there for.

Stored per case cNN_: hw, S, seed, target (n, 5) fp64 in, the tape and its owners, trans (tx, ty as the reference passed them
to warpAffine; 0, 0 after three failures), attempts (pairs of rand() drawn), the canvas and crop shapes the reference's
pairExpand / pairRandomSampleCrop produced, boxes0 / boxes1 (k, 4) fp64 and labels0 / labels1 out; for the small frames also
the uint8 image and both fp32 outputs as pull_translational_item hands them on (RGB, CHW)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import ref_shim  # noqa: E402
import _augment_ref as R  # noqa: E402
import _augment_pair_ref as P  # noqa: E402
from make_golden_augment import save_npz  # noqa: E402

OWNERS = ("VOCDetection", "pairPhotometricDistort", "pairExpand", "pairRandomSampleCrop", "pairRandomMirror")
MEAN = (104, 117, 123)

# (H, W, truths, S, base seed, property); truths: n of case_boxes, or ("edge", n, margin); frames of at most SMALL a side keep
# their pixels
CASES = [
    (30, 40, 2, 32, 0, "neg_shift"), (40, 30, 3, 32, 10, "pos_shift"), (30, 40, 1, 32, 20, "subpixel"),
    (30, 36, ("edge", 2, 0.01), 32, 30, "attempt2"), (36, 30, ("edge", 3, 0.01), 32, 40, "attempt3"),
    (30, 40, ("edge", 2, 0.001), 32, 50, "fallback"), (32, 40, 2, 48, 60, "border_expand"), (40, 56, 5, 32, 70, "drop_one"),
    (40, 48, 4, 32, 80, "mirror"), (30, 40, 3, 32, 90, "no_crop"), (30, 40, 3, 32, 100, "tiny_crop"),
    (72, 32, 6, 32, 110, "any"),
    (375, 500, 3, 300, 200, "any"), (500, 353, 6, 300, 210, "drop_one"), (333, 500, 2, 320, 220, "border_expand"),
    (480, 640, ("edge", 4, 0.01), 320, 230, "attempt2"),
]
SMALL = 72
FALLBACK_CASE = 5


def case_truths(H, W, spec, base):
    if isinstance(spec, tuple):
        return P.edge_boxes(spec[1], spec[2], base)
    return R.case_boxes(H, W, spec, base)


class Recorder(object):
    """numpy.random stand-in: a seeded RandomState whose draws are logged in order with the class that made them."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.tape, self.owner, self.one_arg = [], [], []

    def _log(self, v, low=None):
        self.tape.append(float(v))
        name = type(sys._getframe(2).f_locals.get("self")).__name__
        self.owner.append(OWNERS.index(name) if name in OWNERS else -1)
        self.one_arg.append(low)
        return v

    def rand(self):
        return self._log(self.rs.rand())

    def randint(self, n):
        return self._log(self.rs.randint(n))

    def uniform(self, low=0.0, high=1.0):
        return self._log(self.rs.uniform(low, high), low if high == 1.0 and low != 0.0 else None)

    def choice(self, a):
        return a[self._log(self.rs.randint(len(a)))]


class NumpyProxy(object):
    """data.voc0712's `np` with `.random` replaced by the recorder."""

    def __init__(self, rec):
        self.random = rec

    def __getattr__(self, name):
        return getattr(np, name)


def centre_masks(p, target, W, H):
    """Per frame, which boxes keep their centre strictly inside the kept crop rect (fp64, the chain's op order)."""
    frac = target[:, :4]
    frac_t = frac.copy()
    if p["attempts"] and not p["status"] & P.ST_TRANS_FALLBACK:
        frac_t[:, 0::2] = frac_t[:, 0::2] + p["shift_x"]
        frac_t[:, 1::2] = frac_t[:, 1::2] + p["shift_y"]
        frac_t = np.clip(frac_t, 0.0, 1.0)
    r = p["crop"]
    out = []
    for f in (frac, frac_t):
        b = f.copy()
        b[:, 0::2] = b[:, 0::2] * W + p["img_x"]
        b[:, 1::2] = b[:, 1::2] * H + p["img_y"]
        c = (b[:, :2] + b[:, 2:]) / 2.0
        out.append((r[0] < c[:, 0]) & (r[1] < c[:, 1]) & (r[2] > c[:, 0]) & (r[3] > c[:, 1]))
    return out


def _has(kind, p, W, H, target, rec):
    expand = (p["canvas_w"], p["canvas_h"]) != (W, H)
    crop = p["crop"] != (0, 0, p["canvas_w"], p["canvas_h"])
    ok = not p["status"] & P.ST_TRANS_FALLBACK
    if kind == "any":
        return ok
    if kind == "neg_shift":
        return p["trans_x"] < 0 and p["trans_y"] < 0
    if kind == "pos_shift":
        return p["trans_x"] > 0 and p["trans_y"] > 0
    if kind == "subpixel":
        return ok and p["shift_x"] != 0 and p["trans_x"] == 0 and p["trans_y"] != 0
    if kind == "attempt2":
        return ok and p["attempts"] == 2
    if kind == "attempt3":
        return ok and p["attempts"] == 3
    if kind == "fallback":
        return not ok and crop
    if kind == "border_expand":
        return expand and not crop and abs(p["trans_x"]) >= 1 and abs(p["trans_y"]) >= 1 and p["canvas_w"] >= 3 * W
    if kind == "drop_one":
        m0, m1 = centre_masks(p, target, W, H)
        return crop and bool((m0 != m1).any())
    if kind == "mirror":
        return ok and p["mirror"] == 1 and crop
    if kind == "no_crop":
        return ok and not crop and not expand
    if kind == "tiny_crop":
        lows = [x for x in rec.one_arg if x is not None]          # the kept trial's left draw is uniform(W - w)
        return crop and len(lows) >= 2 and lows[-2] < 1.0
    raise KeyError(kind)


def find_seed(H, W, target, base, kind):
    for seed in range(base * 1000, base * 1000 + 100000):
        rec = Recorder(seed)
        p = P.sample_pair(W, H, target[:, :4], target[:, 4], rec)[0]
        if _has(kind, p, W, H, target, rec):
            return seed
    raise RuntimeError("no seed for %s" % kind)


def main(out_dir=HERE):
    ref_shim.install()
    cv2 = sys.modules["cv2"]
    cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = 40, 54
    cv2.cvtColor = lambda img, code: R.bgr2hsv(img) if code == 40 else R.hsv2bgr(img)
    cv2.resize = lambda img, dsize: R.resize(img, dsize[0]) if dsize[0] == dsize[1] else None
    import utils.augmentations as A
    import data.voc0712 as V

    class Tree(object):
        def getroot(self):
            return None
    V.ET = type("ET", (), {"parse": staticmethod(lambda path: Tree())})
    out = {}
    for i, (H, W, spec, S, base, kind) in enumerate(CASES):
        target = case_truths(H, W, spec, base)
        img = R.case_image(H, W, base)
        seed = find_seed(H, W, target, base, kind)
        rec = Recorder(seed)
        A.random = rec
        V.np = NumpyProxy(rec)
        trans = [0, 0]

        def warp(src, M, dsize):
            assert tuple(dsize) == (src.shape[1], src.shape[0]) and M.tolist()[0][:2] == [1, 0] and M.tolist()[1][:2] == [0, 1]
            trans[:] = [int(M[0, 2]), int(M[1, 2])]
            return P.shift_frame(src, trans[0], trans[1])
        cv2.imread = lambda path: img.copy()
        cv2.warpAffine = warp
        ds = object.__new__(V.VOCDetection)
        ds.ids, ds._annopath, ds._imgpath, ds.max_trans_ratio = ["x"], "%s", "%s", 0.1
        ds.target_transform = lambda t, w, h, img_id: target.tolist()
        ds.transform = aug = A.pairSSDAugmentation(S, MEAN)
        shapes = {}

        def spy(t, key):
            def call(im, b, l):
                r = t(im, b, l)
                assert r[0][0].shape == r[0][1].shape
                shapes[key] = r[0][0].shape[:2]
                return r
            return call
        ts = aug.augment.transforms
        ts[1], ts[2] = spy(ts[1], "canvas"), spy(ts[2], "crop")
        imgs, targets, h, w = ds.pull_translational_item(0)
        assert (h, w) == (H, W)
        k = "c%02d_" % i
        out[k + "hw"] = np.array([H, W])
        out[k + "S"] = np.array(S)
        out[k + "seed"] = np.array(seed)
        out[k + "target"] = target
        out[k + "tape"] = np.array(rec.tape, np.float64)
        out[k + "owner"] = np.array(rec.owner, np.int8)
        out[k + "trans"] = np.array(trans)
        out[k + "attempts"] = np.array(rec.owner.count(0) // 2)
        out[k + "canvas"] = np.array(shapes["canvas"])
        out[k + "crop"] = np.array(shapes["crop"])
        for f in (0, 1):
            out[k + "boxes%d" % f] = np.asarray(targets[f][:, :4], np.float64)
            out[k + "labels%d" % f] = np.asarray(targets[f][:, 4], np.float64)
        if max(H, W) <= SMALL:
            out[k + "image"] = img
            for f in (0, 1):
                out[k + "pixels%d" % f] = np.ascontiguousarray(imgs[f].numpy()).astype(np.float32)
        print("case %2d %4dx%-4d S=%d seed=%d %-13s draws=%3d attempts=%d trans=%s canvas=%s crop=%s kept=%d of %d" % (
            i, W, H, S, seed, kind, len(rec.tape), int(out[k + "attempts"]), tuple(trans), tuple(shapes["canvas"]),
            tuple(shapes["crop"]), len(targets[0]), len(target)))
    save_npz(os.path.join(out_dir, "augment_pair_cases.npz"), out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
