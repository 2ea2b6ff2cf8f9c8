"""A numpy restatement of the TRN training pair chain (tdrn_hip.h section ii-d), written from the stated semantics:
VOCDetection.pull_translational_item's translated second frame and truths, then pairSSDAugmentation.

`translate` makes the second truths and the pixel shift from up to three attempts, `shift_frame` is the integer
cv2.warpAffine the reference calls ([[1, 0, tx], [0, 1, ty]] on uint8, zero border), `sample_pair` draws the shared decisions
with the two-frame centre test and moves both box sets in fp64, `apply_pair` makes both frames' pixels.  The unchanged legs
(the draw replay, the photometric distortion, the canvas / crop / mirror / resize of one frame) are _augment_ref's.

cv2 is not installed in the build image, so the warpAffine leg rests on hand-worked known answers
(tests/test_augment_pair_ref.py), like the cvtColor and resize legs of _augment_ref."""
import numpy as np

import _augment_ref as R

F32, F64 = R.F32, R.F64
ST_TRANS_FALLBACK = 4


def _rand(draws):
    """np.random.rand(): RandomState has it; a tape replays the value."""
    return draws.rand() if hasattr(draws, "rand") else draws.uniform(0.0, 1.0)


def translate(frac, draws, W, H, r=0.1):
    """voc0712.py:411-434.  frac (n, 4) fp64 fractions.  Returns (t, frac_t): t = dict(shift_x, shift_y, trans_x, trans_y,
    attempts, fallback); frac_t the second frame's truths (clipped on accept, a plain copy after three failures)."""
    frac = np.array(frac, F64).reshape(-1, 4)
    t = dict(shift_x=0.0, shift_y=0.0, trans_x=0, trans_y=0, attempts=0, fallback=False)
    for a in (1, 2, 3):
        u_x = _rand(draws)
        u_y = _rand(draws)
        x_trans = (-r / a) + ((u_x * 2) * r) / a
        y_trans = (-r / a) + ((u_y * 2) * r) / a
        moved = frac.copy()
        moved[:, 0] = moved[:, 0] + x_trans
        moved[:, 2] = moved[:, 2] + x_trans
        moved[:, 1] = moved[:, 1] + y_trans
        moved[:, 3] = moved[:, 3] + y_trans
        c = (moved[:, :2] + moved[:, 2:]) / 2.0
        t["attempts"] = a
        if ((c[:, 0] > 0.0) & (c[:, 1] > 0.0) & (c[:, 0] < 1.0) & (c[:, 1] < 1.0)).all():
            t.update(shift_x=float(x_trans), shift_y=float(y_trans), trans_x=int(x_trans * W), trans_y=int(y_trans * H))
            return t, np.clip(moved, 0.0, 1.0)
    t["fallback"] = True
    return t, frac.copy()


def shift_frame(img_u8, tx, ty):
    """cv2.warpAffine(img, [[1, 0, tx], [0, 1, ty]], (W, H)) on uint8: dst(x, y) = src(x - tx, y - ty), 0 outside."""
    img = np.asarray(img_u8)
    H, W = img.shape[:2]
    out = np.zeros_like(img)
    x0, x1 = max(tx, 0), min(W + tx, W)
    y0, y1 = max(ty, 0), min(H + ty, H)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = img[y0 - ty:y1 - ty, x0 - tx:x1 - tx]
    return out


def sample_pair(W, H, frac, labels, draws, r=0.1, frac_t=None, labels_t=None, max_rounds=None):
    """The pair chain's decisions for one (H, W) frame with truths `frac` (n, 4) fp64 fractions.  frac_t / labels_t: the
    second frame's truths when the caller has them (no translation, no translation draws).  Returns (params, boxes0, boxes1,
    labels0, labels1); params holds _augment_ref.sample's keys and shift_x, shift_y, trans_x, trans_y, attempts."""
    p = R._params()
    b0 = np.array(frac, F64).reshape(-1, 4)
    l0 = np.asarray(labels, F64).reshape(-1)
    t = dict(shift_x=0.0, shift_y=0.0, trans_x=0, trans_y=0, attempts=0, fallback=False)
    if frac_t is not None:
        b1 = np.array(frac_t, F64).reshape(-1, 4)
        l1 = np.asarray(labels_t, F64).reshape(-1)
    elif len(b0):
        t, b1 = translate(b0, draws, W, H, r)
        l1 = l0.copy()
    else:
        b1, l1 = b0.copy(), l0.copy()
    for k in ("shift_x", "shift_y", "trans_x", "trans_y", "attempts"):
        p[k] = t[k]
    if t["fallback"]:
        p["status"] |= ST_TRANS_FALLBACK
    for b in (b0, b1):
        b[:, 0] *= W
        b[:, 2] *= W
        b[:, 1] *= H
        b[:, 3] *= H
    # pairPhotometricDistort: one set of values
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
        p["perm"] = R.PERMS[draws.randint(6)]
    # pairExpand: a 1 means no expand; the canvas comes from frame 0
    cw, ch = W, H
    if not draws.randint(2):
        ratio = draws.uniform(1, 4)
        left = draws.uniform(0, W * ratio - W)
        top = draws.uniform(0, H * ratio - H)
        cw, ch = int(W * ratio), int(H * ratio)
        p["img_x"], p["img_y"] = int(left), int(top)
        for b in (b0, b1):
            b[:, :2] += (int(left), int(top))
            b[:, 2:] += (int(left), int(top))
    p["canvas_w"], p["canvas_h"] = cw, ch
    # pairRandomSampleCrop: a trial is kept when some box has its centre inside the rect in both frames
    rect = (0, 0, cw, ch)
    keep = np.ones(len(b0), bool)
    rounds = 0
    while len(b0):
        if max_rounds is not None and rounds == max_rounds:
            p["status"] |= R.ST_CROP_FALLBACK
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
            q = (int(left), int(top), int(left + w), int(top + h))
            m = np.ones(len(b0), bool)
            for b in (b0, b1):
                c = (b[:, :2] + b[:, 2:]) / 2.0
                m &= (q[0] < c[:, 0]) & (q[1] < c[:, 1]) & (q[2] > c[:, 0]) & (q[3] > c[:, 1])
            if not m.any():
                continue
            rect, keep, done = q, m, True
            cut = []
            for b in (b0, b1):
                b = b[m].copy()
                b[:, :2] = np.maximum(b[:, :2], q[:2]) - q[:2]
                b[:, 2:] = np.minimum(b[:, 2:], q[2:]) - q[:2]
                cut.append(b)
            b0, b1 = cut
            break
        if done or getattr(draws, "exhausted", False):
            break
    l0, l1 = l0[keep], l1[keep]
    p["crop"] = rect
    wc, hc = min(rect[2], cw) - rect[0], min(rect[3], ch) - rect[1]
    # pairRandomMirror, then percent coordinates of the crop's own size
    mirror = draws.randint(2)
    out = []
    for b in (b0, b1):
        if mirror:
            b = b.copy()
            b[:, 0::2] = wc - b[:, 2::-2]
        b[:, 0] /= wc
        b[:, 2] /= wc
        b[:, 1] /= hc
        b[:, 3] /= hc
        out.append(b)
    p["mirror"] = 1 if mirror else 0
    p["kept"] = len(out[0])
    if getattr(draws, "exhausted", False):
        p["status"] |= R.ST_TAPE_EXHAUSTED
    return p, out[0], out[1], l0, l1


def apply_pair(img_u8, p, S, mean=(104, 117, 123), to_rgb=True, img_t=None):
    """Both frames' (3, S, S) fp32 pixels.  img_t None: the second frame is the first shifted by (trans_x, trans_y)."""
    if img_t is None:
        img_t = shift_frame(img_u8, p["trans_x"], p["trans_y"])
    return R.apply(img_u8, p, S, mean, to_rgb), R.apply(img_t, p, S, mean, to_rgb)


def edge_boxes(n, margin, seed):
    """(n, 5) hand-made truths whose first box has its centre `margin` from the left and the top edge, so that translation
    attempts fail often (a centre must stay strictly inside (0, 1))."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 5), F64)
    out[0] = (0.0, 0.0, 2 * margin, 2 * margin, 3)
    for i in range(1, n):
        x1, y1 = rs.uniform(0.2, 0.5, 2)
        out[i] = (x1, y1, x1 + rs.uniform(0.1, 0.4), y1 + rs.uniform(0.1, 0.4), rs.randint(20))
    return out
