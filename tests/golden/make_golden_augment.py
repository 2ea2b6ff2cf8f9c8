"""Generate tests/golden/augment_cases.npz by running the REFERENCE's own SSDAugmentation on CPU (build container only).

    python tests/golden/make_golden_augment.py [DIR]    # writes the fixture next to this file (or into DIR)

The reference is imported through ref_shim, as make_golden.py does; nothing of it is copied.  Three stand-ins make it run:
  - the module's `random` (numpy.random) becomes a recorder around a seeded RandomState that logs every value drawn, in order
    (the tape) together with the transform that drew it.  numpy 2 rejects the reference's `choice` on its ragged tuple of
    modes, so choice(a) is restated as a[randint(len(a))], which is what numpy 1.x's legacy choice consumed;
  - cv2.cvtColor and cv2.resize are the restatement's fp32 legs (tests/_augment_ref.py; cv2 is not installed).
Inputs are regenerated from seeds (_augment_ref.case_image / case_boxes).  A case's seed is the first one at or after its
base seed whose draws show the property the case is there for (expand on, crop None, mirror, a crop with W - w < 1).

Stored per case cNN_: hw, S, target (n, 5) fp64 in, the tape and its owners, the canvas and crop shapes the reference's
Expand / RandomSampleCrop produced, boxes (k, 4) fp64 and labels out; for the small frames also the uint8 image and the
fp32 pixels as VOCDetection.pull_item hands them on (RGB, CHW).
"""
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

OWNERS = ("RandomBrightness", "PhotometricDistort", "RandomContrast", "RandomSaturation", "RandomHue",
          "RandomLightingNoise", "Expand", "RandomSampleCrop", "RandomMirror")

# (H, W, n boxes, S, base seed, property); S is the output size, small frames keep their pixels
CASES = [
    (30, 40, 1, 32, 0, "any"), (30, 40, 3, 32, 10, "tiny_crop"), (40, 48, 2, 32, 20, "expand"),
    (48, 64, 4, 48, 30, "no_crop"), (48, 64, 8, 48, 40, "mirror"), (60, 80, 5, 48, 50, "any"),
    (72, 56, 3, 48, 60, "expand_crop"), (36, 36, 2, 32, 70, "mirror_expand"), (30, 40, 6, 32, 80, "crop"),
    (375, 500, 2, 300, 100, "any"), (500, 353, 5, 300, 110, "expand"), (333, 500, 8, 300, 120, "no_crop"),
    (375, 500, 1, 300, 130, "mirror"), (480, 640, 7, 300, 140, "expand_crop"), (281, 500, 3, 300, 150, "crop"),
    (500, 375, 4, 300, 160, "any"), (375, 500, 6, 320, 170, "expand"), (400, 300, 2, 320, 180, "crop"),
    (500, 500, 8, 320, 190, "mirror_expand"), (338, 450, 3, 320, 200, "no_crop"), (375, 500, 5, 512, 210, "any"),
    (442, 500, 1, 512, 220, "crop"), (500, 333, 6, 512, 230, "expand_crop"), (366, 488, 4, 512, 240, "any"),
]
SMALL = 64          # frames with both sides at most this keep their pixels


class Recorder(object):
    """numpy.random stand-in: a seeded RandomState whose draws are logged in order with the transform that made them."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.tape, self.owner, self.one_arg = [], [], []

    def _log(self, v, low=None):
        self.tape.append(float(v))
        caller = sys._getframe(2).f_locals.get("self")
        self.owner.append(OWNERS.index(type(caller).__name__) if caller is not None else -1)
        self.one_arg.append(low)
        return v

    def randint(self, n):
        return self._log(self.rs.randint(n))

    def uniform(self, low=0.0, high=1.0):
        return self._log(self.rs.uniform(low, high), low if high == 1.0 and low != 0.0 else None)

    def choice(self, a):
        return a[self._log(self.rs.randint(len(a)))]


def _has(kind, p, W, H, rec):
    expand = (p["canvas_w"], p["canvas_h"]) != (W, H)
    crop = p["crop"] != (0, 0, p["canvas_w"], p["canvas_h"])
    ok = {"any": True, "expand": expand, "no_crop": not crop, "mirror": p["mirror"] == 1, "crop": crop,
          "expand_crop": expand and crop, "mirror_expand": expand and p["mirror"] == 1}
    if kind == "tiny_crop":
        lows = [x for x in rec.one_arg if x is not None]          # the kept trial's left draw is uniform(W - w)
        return crop and len(lows) >= 2 and lows[-2] < 1.0
    return ok[kind]


def find_seed(H, W, target, base, kind):
    for seed in range(base * 1000, base * 1000 + 100000):
        rec = Recorder(seed)
        p, _, _ = R.sample(W, H, target[:, :4], target[:, 4], rec)
        if _has(kind, p, W, H, rec):
            return seed
    raise RuntimeError("no seed for %s" % kind)


def main(out_dir=HERE):
    ref_shim.install()
    cv2 = sys.modules["cv2"]
    cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = 40, 54
    cv2.cvtColor = lambda img, code: R.bgr2hsv(img) if code == 40 else R.hsv2bgr(img)
    cv2.resize = lambda img, dsize: R.resize(img, dsize[0]) if dsize[0] == dsize[1] else None
    import utils.augmentations as A
    out = {}
    for i, (H, W, n, S, base, kind) in enumerate(CASES):
        target = R.case_boxes(H, W, n, base)
        img = R.case_image(H, W, base)
        seed = find_seed(H, W, target, base, kind)
        rec = Recorder(seed)
        A.random = rec
        aug = A.SSDAugmentation(S, (104, 117, 123))
        shapes = {}

        def spy(t, key):
            def call(im, b, l):
                r = t(im, b, l)
                shapes[key] = r[0].shape[:2]
                return r
            return call
        ts = aug.augment.transforms
        ts[3], ts[4] = spy(ts[3], "canvas"), spy(ts[4], "crop")
        x, boxes, labels = aug(img.copy(), target[:, :4].copy(), target[:, 4].copy())
        x = np.ascontiguousarray(x[:, :, (2, 1, 0)].transpose(2, 0, 1))          # VOCDetection.pull_item: RGB, CHW
        k = "c%02d_" % i
        out[k + "hw"] = np.array([H, W])
        out[k + "S"] = np.array(S)
        out[k + "seed"] = np.array(seed)
        out[k + "target"] = target
        out[k + "tape"] = np.array(rec.tape, np.float64)
        out[k + "owner"] = np.array(rec.owner, np.int8)
        out[k + "canvas"] = np.array(shapes["canvas"])
        out[k + "crop"] = np.array(shapes["crop"])
        out[k + "boxes"] = np.asarray(boxes, np.float64)
        out[k + "labels"] = np.asarray(labels, np.float64)
        if max(H, W) <= SMALL:
            out[k + "image"] = img
            out[k + "pixels"] = x.astype(np.float32)
        print("case %2d %4dx%-4d n=%d S=%d seed=%d %-13s draws=%3d canvas=%s crop=%s kept=%d" % (
            i, W, H, n, S, seed, kind, len(rec.tape), tuple(shapes["canvas"]), tuple(shapes["crop"]), len(boxes)))
    save_npz(os.path.join(out_dir, "augment_cases.npz"), out)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so a regeneration is byte-identical to the committed file."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
