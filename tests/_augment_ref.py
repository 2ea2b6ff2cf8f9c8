"""A numpy restatement of SSDAugmentation (tdrn_hip.h section ii-c), written from the stated semantics.

Two halves, as in the kernels: `sample` draws every decision from a draw source (numpy's legacy RandomState semantics for
randint / uniform, or a tape of the values the reference drew) and moves the boxes in fp64; `apply` makes the pixels of one
image from its parameters, materialising the distorted image, the expand canvas and the crop as the reference does.

The two cv2 legs the reference calls are restated here and pinned by hand-worked known answers (tests/test_augment_ref.py),
because cv2 is not installed in the build image:
  - cvtColor BGR2HSV / HSV2BGR on fp32: OpenCV's scalar float path (imgproc color_hsv), restated FROM MEMORY;
  - resize INTER_LINEAR on fp32: the float path (weights (1 - f, f) in fp32, horizontal pass then vertical), with the index
    and border rule of oracle.base_transform_u8's `coef`.
Used by the CPU tests against the reference fixtures, by the GPU tests as the oracle, and by scripts/augment_bench.py as the
single-core yardstick of a DataLoader worker."""
import numpy as np

F32, F64 = np.float32, np.float64
FLT_EPSILON = F32(np.finfo(np.float32).eps)
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
MAX_ROUNDS = 32                   # crop mode rounds before the device sampler falls back to no crop
ST_CROP_FALLBACK, ST_TAPE_EXHAUSTED = 1, 2


class TapeDraws(object):
    """Replays the values the reference drew, in its order: randint(n) -> int(value), uniform(...) -> value."""

    def __init__(self, tape):
        self.tape = np.asarray(tape, F64)
        self.i = 0
        self.exhausted = False

    def _next(self):
        if self.i >= len(self.tape):
            self.exhausted = True
            return 0.0
        v = float(self.tape[self.i])
        self.i += 1
        return v

    def randint(self, n):
        return int(self._next())

    def uniform(self, low, high=1.0):
        return self._next()


def _params():
    return dict(brightness=F32(0), contrast_pre=F32(1), contrast_post=F32(1), saturation=F32(1), hue=F32(0),
                perm=(0, 1, 2), canvas_w=0, canvas_h=0, img_x=0, img_y=0, crop=(0, 0, 0, 0), mirror=0, kept=0, status=0)


def sample(W, H, frac, labels, draws, max_rounds=None):
    """SSDAugmentation's decisions for one (H, W) image with truths `frac` (n, 4) fp64 fractions.
    Returns (params, boxes (k, 4) fp64 fractions of the output, labels (k,)).  max_rounds None = the reference's unbounded
    mode loop; an image with no truths gets no crop (the reference never augments one)."""
    p = _params()
    boxes = np.array(frac, F64).reshape(-1, 4)
    labels = np.asarray(labels, F64).reshape(-1)
    boxes[:, 0] *= W
    boxes[:, 2] *= W
    boxes[:, 1] *= H
    boxes[:, 3] *= H
    # PhotometricDistort: brightness, the contrast position, contrast / saturation / hue, lighting noise
    if draws.randint(2):
        p["brightness"] = F32(draws.uniform(-32, 32))
    pre = draws.randint(2)
    if pre and draws.randint(2):
        p["contrast_pre"] = F32(draws.uniform(0.5, 1.5))
    if draws.randint(2):
        p["saturation"] = F32(draws.uniform(0.5, 1.5))
    if draws.randint(2):
        p["hue"] = F32(draws.uniform(-18.0, 18.0))
    if not pre and draws.randint(2):
        p["contrast_post"] = F32(draws.uniform(0.5, 1.5))
    if draws.randint(2):
        p["perm"] = PERMS[draws.randint(6)]
    # Expand: a 1 means no expand
    cw, ch = W, H
    if not draws.randint(2):
        ratio = draws.uniform(1, 4)
        left = draws.uniform(0, W * ratio - W)
        top = draws.uniform(0, H * ratio - H)
        cw, ch = int(W * ratio), int(H * ratio)
        p["img_x"], p["img_y"] = int(left), int(top)
        boxes[:, :2] += (int(left), int(top))
        boxes[:, 2:] += (int(left), int(top))
    p["canvas_w"], p["canvas_h"] = cw, ch
    # RandomSampleCrop: the IoU test never rejects, so every mode but None samples alike
    rect = (0, 0, cw, ch)
    keep = np.ones(len(boxes), bool)
    rounds = 0
    while len(boxes):
        if max_rounds is not None and rounds == max_rounds:
            p["status"] |= ST_CROP_FALLBACK
            break
        rounds += 1
        if draws.randint(6) == 0:
            break
        done = False
        for _ in range(50):
            w = draws.uniform(0.3 * cw, cw)
            h = draws.uniform(0.3 * ch, ch)
            if getattr(draws, "exhausted", False):
                break
            if h / w < 0.5 or h / w > 2:
                continue
            left = draws.uniform(cw - w)
            top = draws.uniform(ch - h)
            r = (int(left), int(top), int(left + w), int(top + h))
            c = (boxes[:, :2] + boxes[:, 2:]) / 2.0
            m = (r[0] < c[:, 0]) & (r[1] < c[:, 1]) & (r[2] > c[:, 0]) & (r[3] > c[:, 1])
            if not m.any():
                continue
            rect, keep, done = r, m, True
            b = boxes[m].copy()
            b[:, :2] = np.maximum(b[:, :2], r[:2]) - r[:2]
            b[:, 2:] = np.minimum(b[:, 2:], r[2:]) - r[:2]
            boxes = b
            break
        if done or getattr(draws, "exhausted", False):
            break
    labels = labels[keep]
    p["crop"] = rect
    wc, hc = min(rect[2], cw) - rect[0], min(rect[3], ch) - rect[1]
    # RandomMirror
    if draws.randint(2):
        p["mirror"] = 1
        boxes = boxes.copy()
        boxes[:, 0::2] = wc - boxes[:, 2::-2]
    # ToPercentCoords
    boxes[:, 0] /= wc
    boxes[:, 2] /= wc
    boxes[:, 1] /= hc
    boxes[:, 3] /= hc
    p["kept"] = len(boxes)
    if getattr(draws, "exhausted", False):
        p["status"] |= ST_TAPE_EXHAUSTED
    return p, boxes, labels


# ---------------------------------------------------------------- the cv2 legs (fp32), restated
def bgr2hsv(img):
    """cv2.cvtColor(COLOR_BGR2HSV) on fp32, OpenCV's scalar float path (from memory): h in [0, 360], s, v unscaled."""
    img = np.asarray(img, F32)
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    diff = v - vmin
    s = diff / (np.abs(v) + FLT_EPSILON)
    d = (F64(60.0) / (diff + FLT_EPSILON).astype(F64)).astype(F32)       # (float)(60. / (diff + FLT_EPSILON))
    h = np.where(v == r, (g - b) * d, np.where(v == g, (b - r) * d + F32(120), (r - g) * d + F32(240)))
    h = np.where(h < 0, h + F32(360), h).astype(F32)
    return np.stack([h, s, v], -1).astype(F32)


HSCALE = F32(F32(6) / F32(360))


def hsv2bgr(img):
    """cv2.cvtColor(COLOR_HSV2BGR) on fp32, OpenCV's scalar float path (from memory)."""
    img = np.asarray(img, F32)
    h, s, v = img[..., 0] * HSCALE, img[..., 1], img[..., 2]
    h = h.astype(F32)
    while True:
        lo, hi = h < 0, h >= 6
        if not (lo.any() or hi.any()):
            break
        h = np.where(lo, h + F32(6), np.where(hi, h - F32(6), h)).astype(F32)
    sector = np.floor(h).astype(np.int64)
    h = (h - sector.astype(F32)).astype(F32)
    bad = (sector < 0) | (sector >= 6)
    sector[bad], h[bad] = 0, 0
    one = F32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], -1)
    idx = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector]     # (..., 3)
    out = np.take_along_axis(tab, idx, -1)
    out[s == 0] = v[s == 0][..., None]
    return out.astype(F32)


def coef(n_dst, n_src):
    """Source index pair and fp32 weights per destination index: oracle.base_transform_u8's rule, float weights."""
    d = np.arange(n_dst)
    f = ((d + 0.5) * (n_src / n_dst) - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    lo = s < 0
    f[lo], s[lo] = 0, 0
    hi = s >= n_src - 1
    f[hi], s[hi] = 0, n_src - 1
    return s, np.minimum(s + 1, n_src - 1), (F32(1) - f).astype(F32), f


def resize(img, S):
    """cv2.resize(img, (S, S)) for fp32 (H, W, C), INTER_LINEAR: horizontal then vertical, unfused fp32."""
    img = np.asarray(img, F32)
    H, W = img.shape[:2]
    x0, x1, a0, a1 = coef(S, W)
    y0, y1, b0, b1 = coef(S, H)
    h = img[:, x0] * a0[None, :, None] + img[:, x1] * a1[None, :, None]
    return (h[y0] * b0[:, None, None] + h[y1] * b1[:, None, None]).astype(F32)


# ---------------------------------------------------------------- pixels
def distort(img_u8, p):
    """PhotometricDistort of a uint8 (H, W, 3) BGR frame with parameters p (fp32, channels permuted)."""
    x = np.asarray(img_u8).astype(F32)
    x = x + p["brightness"]
    x = x * p["contrast_pre"]
    hsv = bgr2hsv(x)
    hsv[..., 1] *= p["saturation"]
    hsv[..., 0] += p["hue"]
    hue = hsv[..., 0]
    hue[hue > 360.0] -= F32(360)
    hue[hue < 0.0] += F32(360)
    x = hsv2bgr(hsv) * p["contrast_post"]
    return x[..., list(p["perm"])].astype(F32)


def apply(img_u8, p, S, mean=(104, 117, 123), to_rgb=True):
    """(3, S, S) fp32: distort, expand canvas, crop, mirror, resize, subtract the mean, optional BGR -> RGB, CHW."""
    mean = np.asarray(mean, F32)
    x = distort(img_u8, p)
    H, W = x.shape[:2]
    canvas = np.empty((p["canvas_h"], p["canvas_w"], 3), F32)
    canvas[:, :, :] = mean
    canvas[p["img_y"]:p["img_y"] + H, p["img_x"]:p["img_x"] + W] = x
    r = p["crop"]
    x = canvas[r[1]:r[3], r[0]:r[2]]
    if p["mirror"]:
        x = x[:, ::-1]
    x = resize(x, S) - mean
    if to_rgb:
        x = x[:, :, (2, 1, 0)]
    return np.ascontiguousarray(x.transpose(2, 0, 1)).astype(F32)


# ---------------------------------------------------------------- synthetic cases (shared by the fixture generator and tests)
def case_image(H, W, seed):
    """A deterministic uint8 BGR frame: smooth gradients plus noise, with saturated and grey patches (the HSV edge cases)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 255 // max(W - 1, 1)), (yy * 255 // max(H - 1, 1)), ((xx + yy) * 7) % 256], -1)
    img = (base + rs.randint(-20, 21, size=(H, W, 3))).clip(0, 255).astype(np.uint8)
    img[: H // 4, : W // 4] = (0, 0, 255)
    img[H // 4: H // 2, : W // 4] = 128
    img[: H // 4, W // 4: W // 2] = 255
    return img


def case_boxes(H, W, n, seed):
    """(n, 5) fp64 [x1, y1, x2, y2, label] fractions as AnnotationTransform makes them: (pixel - 1) / size."""
    rs = np.random.RandomState(seed + 1000)
    out = np.zeros((n, 5), F64)
    for i in range(n):
        x1, y1 = rs.randint(1, W - 4), rs.randint(1, H - 4)
        x2, y2 = rs.randint(x1 + 2, W + 1), rs.randint(y1 + 2, H + 1)
        out[i] = ((x1 - 1) / W, (y1 - 1) / H, (x2 - 1) / W, (y2 - 1) / H, rs.randint(20))
    return out
