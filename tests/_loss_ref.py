"""A numpy restatement of MultiBoxLoss / RefineMultiBoxLoss (tdrn_hip.h section ii-b), written from the stated semantics.

Geometry (IoU, decode, encode) runs in fp32 with the reference's operation order, so conf_t comes out exactly; the
mining scores and the loss sums run in fp64.  Used by the CPU tests against the reference fixtures and by the GPU tests
as the oracle at sizes the fixtures do not cover."""
import numpy as np

F32 = np.float32


def _exp(x):
    return np.exp(x.astype(np.float64)).astype(F32)      # correctly rounded fp32 (numpy's own fp32 exp is not)


def _log(x):
    return np.log(x.astype(np.float64)).astype(F32)


def point_form(pri):
    half = pri[:, 2:] / F32(2)
    return np.concatenate([pri[:, :2] - half, pri[:, :2] + half], 1)


def decode(loc, pri, v):
    c = pri[:, :2] + loc[:, :2] * F32(v[0]) * pri[:, 2:]
    wh = pri[:, 2:] * _exp(loc[:, 2:] * F32(v[1]))
    lo = c - wh / F32(2)
    return np.concatenate([lo, wh + lo], 1)


def center_size(b):
    return np.concatenate([(b[:, 2:] + b[:, :2]) / F32(2), b[:, 2:] - b[:, :2]], 1)


def iou(truths, boxes):
    """[n, P] in fp32: clamp(min(x2) - max(x1), 0) * clamp(min(y2) - max(y1), 0) / ((area_a + area_b) - inter)."""
    a, b = truths[:, None, :], boxes[None, :, :]
    iw = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), F32(0))
    ih = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), F32(0))
    inter = iw * ih
    area_a = (truths[:, 2] - truths[:, 0]) * (truths[:, 3] - truths[:, 1])
    area_b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    return inter / ((area_a[:, None] + area_b[None, :]) - inter)


def encode(matched, pri, v):
    g_c = ((matched[:, :2] + matched[:, 2:]) / F32(2) - pri[:, :2]) / (F32(v[0]) * pri[:, 2:])
    g_wh = _log((matched[:, 2:] - matched[:, :2]) / pri[:, 2:]) / F32(v[1])
    return np.concatenate([g_c, g_wh], 1).astype(F32)


def match_one(threshold, target, priors, v, arm_loc=None):
    """(loc_t [P, 4], conf_t [P]) of one image; target [n, 5]."""
    P = priors.shape[0]
    target = np.asarray(target, F32).reshape(-1, 5)
    if target.shape[0] == 0:
        return np.zeros((P, 4), F32), np.zeros(P, np.int64)
    truths, labels = target[:, :4], target[:, 4]
    if arm_loc is None:
        boxes, anchors = point_form(priors), priors
    else:
        boxes = decode(np.asarray(arm_loc, F32), priors, v)
        anchors = center_size(boxes)
    ov = iou(truths, boxes)
    best_prior = ov.argmax(1)                         # lowest index on a tie
    best_truth = ov.argmax(0)
    best_ov = ov[best_truth, np.arange(P)]
    best_ov[best_prior] = F32(2)
    for j in range(len(best_prior)):                  # ascending j: the last truth of a shared prior wins
        best_truth[best_prior[j]] = j
    conf = (labels[best_truth] + F32(1)).astype(np.int64)
    conf[best_ov < F32(threshold)] = 0
    return encode(truths[best_truth], anchors, v), conf


def match_batch(threshold, targets, priors, v, arm_loc=None):
    out = [match_one(threshold, t, priors, v, None if arm_loc is None else arm_loc[b]) for b, t in enumerate(targets)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def mining_scores(conf, conf_t):
    """[B, P] fp64: log-sum-exp with the batch-global max minus the target logit, 0 on positives."""
    B, P = conf_t.shape
    x = conf.reshape(B * P, -1).astype(np.float64)
    g = x.max()
    with np.errstate(divide="ignore"):
        lse = np.log(np.exp(x - g).sum(1)) + g
    s = lse - x[np.arange(B * P), conf_t.reshape(-1)]
    s[conf_t.reshape(-1) > 0] = 0
    return s.reshape(B, P)


def select(conf, conf_t, negpos=3):
    """sel [B, P] uint8: 1 positive, 2 mined negative (rank in a stable descending sort < num_neg), 0 unused; and the
    smallest gap between the scores at either side of each image's num_neg boundary (inf where there is no boundary)."""
    B, P = conf_t.shape
    pos = conf_t > 0
    sel = pos.astype(np.uint8)
    gaps = np.full(B, np.inf)
    if conf is None:
        return sel, gaps
    s = mining_scores(conf, conf_t)
    for b in range(B):
        k = min(negpos * int(pos[b].sum()), P - 1)
        if k == 0:
            continue
        order = np.argsort(-s[b], kind="stable")
        neg = np.zeros(P, bool)
        neg[order[:k]] = True
        sel[b][neg & ~pos[b]] = 2
        gaps[b] = s[b][order[k - 1]] - s[b][order[k]]
    return sel, gaps


def losses(loc, conf, loc_t, conf_t, sel):
    """(loss_l, loss_c, N) in fp64; loss_c is None when conf is None."""
    N = float((conf_t > 0).sum())
    pos = sel == 1
    d = np.abs(loc.astype(np.float64) - loc_t)[pos]
    ll = np.where(d < 1, 0.5 * d * d, d - 0.5).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        if conf is None:
            return ll / N, None, N
        B, P = conf_t.shape
        x = conf.reshape(B, P, -1).astype(np.float64)[sel > 0]
        t = conf_t[sel > 0]
        m = x.max(1, keepdims=True)
        lse = np.log(np.exp(x - m).sum(1)) + m[:, 0]
        lc = (lse - x[np.arange(len(t)), t]).sum()
        return ll / N, lc / N, N


def grads(loc, conf, loc_t, conf_t, sel, g_l=1.0, g_c=1.0):
    """(grad_loc [B, P, 4], grad_conf [B, P, C] or None) in fp64."""
    B, P = conf_t.shape
    N = float((conf_t > 0).sum())
    gl = np.zeros((B, P, 4))
    pos = sel == 1
    gl[pos] = g_l / N * np.clip(loc.astype(np.float64)[pos] - loc_t[pos], -1, 1)
    if conf is None:
        return gl, None
    x = conf.reshape(B, P, -1).astype(np.float64)
    e = np.exp(x - x.max(2, keepdims=True))
    sm = e / e.sum(2, keepdims=True)
    sm[np.arange(B)[:, None], np.arange(P)[None, :], conf_t] -= 1
    gc = np.where((sel > 0)[..., None], g_c / N * sm, 0.0)
    return gl, gc


def synth_targets(rng, B, lo, hi, num_classes, counts=None):
    """VOC-like targets: B images with lo..hi truths (or `counts`), boxes inside the unit square, labels 0..C-2."""
    out = []
    for b in range(B):
        n = int(rng.integers(lo, hi + 1)) if counts is None else counts[b]
        c = rng.uniform(0.05, 0.95, (n, 2))
        wh = rng.uniform(0.02, 0.6, (n, 2))
        box = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0.0, 1.0)
        lab = rng.integers(0, num_classes - 1, (n, 1)).astype(np.float64)
        out.append(np.concatenate([box, lab], 1).astype(F32))
    return out


# Fixture cases of tests/golden/make_golden_loss.py: name -> (prior config, B, C, refine, only_loc, truth counts, seed).
# C = 2 with only_loc is the ARM criterion of train.py:185 (no arm_data: matched against the priors).
CASES = {
    "voc320_refine": ("VOC_320", 4, 21, True, False, (1, 60, 17, 33), 11),
    "voc320_plain": ("VOC_320", 2, 21, False, False, (24, 9), 12),
    "voc512_refine": ("VOC_512_RefineDet", 2, 21, True, False, (40, 5), 13),
    "c31_refine": ("VOC_320", 2, 31, True, False, (12, 28), 14),
    "c81_plain": ("VOC_320", 2, 81, False, False, (30, 3), 15),
    "arm_only_loc": ("VOC_320", 4, 2, False, True, (8, 60, 1, 21), 16),
}
TINY = np.array([-0.90, -0.90, -0.8999, -0.8999], F32)    # a truth that overlaps no prior (it takes prior 0)


def priors_of(cfg, golden_dir):
    return np.load("%s/priorbox_%s.npz" % (golden_dir, cfg))["priors"]


def case_inputs(name, P):
    """(loc [B,P,4], conf [B,P,C] or None, arm_loc [B,P,4] or None, targets) of a fixture case, from its seed.
    Every case's image 0 holds a duplicated truth (same box, another label: the two share a best prior) and its
    last image the tiny truth that overlaps no prior."""
    from tdrn_amd.utils import synth
    cfg, B, C, refine, only_loc, counts, seed = CASES[name]
    rng = synth._rng("loss_" + name, seed)
    targets = synth_targets(rng, B, 1, 60, max(C, 2), counts)
    dup = targets[0][:1].copy()
    dup[0, 4] = (dup[0, 4] + 1) % (max(C, 2) - 1)
    targets[0] = np.concatenate([targets[0], dup]).astype(F32)
    targets[-1] = np.concatenate([targets[-1], np.append(TINY, F32(0))[None]]).astype(F32)
    loc = (0.5 * rng.standard_normal((B, P, 4))).astype(F32)
    conf = None if only_loc else (1.5 * rng.standard_normal((B, P, C))).astype(F32)
    arm = (0.3 * rng.standard_normal((B, P, 4))).astype(F32) if refine else None
    return loc, conf, arm, targets


def loc_t_tolerance(refine):
    """(rtol, atol) for loc_t against the reference.  Plain matching: the decode tolerance of test_gpu_ops.  Refine: the
    anchors are decoded with exp, which torch, numpy and the device round differently in about 1 % of the cases (one
    ulp); the encode's (c_match - c_anchor) / (0.1 * w_anchor) amplifies that ulp of the anchor centre by up to 1 / (0.1 w)
    for a small anchor, so a few elements move by up to ~3e-5 absolute."""
    return (3e-6, 5e-5) if refine else (3e-6, 1e-7)


# ------------------------------------------------------------------------------------------------------------------
# Seeded case builders of the training fuzz (tests/test_gpu_train_fuzz.py; their claims are asserted on the CPU by
# tests/test_loss_ref.py).  Ties are made exact, not near: identical rows of conf give bit-identical mining scores in any
# deterministic implementation, and identical priors give bit-identical IoUs, so select / match_batch stay the oracle with
# no near-tie exemption.
# ------------------------------------------------------------------------------------------------------------------
FAR = np.array([-5.0, -5.0, 0.1, 0.1], F32)               # a prior that overlaps no truth of the unit square
TRUTH_COUNTS = (0, 1, 64, 65, 256, 257, 511, 512)         # around the 256-truth trips of the staging loops, up to the limit
CONF_MODES = ("gaussian", "zeros", "random", "zero_score", "neg_inf", "cap")
PATTERN_GAP = 1e-3                                        # least distance between the scores of two distinct patterns


def fuzz_priors(rng, P):
    """Synthetic center-size priors (test_gpu_fuzz._priors' distribution)."""
    c = rng.random((P, 2)).astype(F32)
    wh = (0.02 + 0.3 * rng.random((P, 2))).astype(F32)
    return np.concatenate([c, wh], 1)


def _background_scores(pats):
    """fp64 mining score of each pattern on a background row: log-sum-exp minus the background logit (the batch max cancels)."""
    x = pats.astype(np.float64)
    m = x.max(1, keepdims=True)
    return np.log(np.exp(x - m).sum(1)) + m[:, 0] - x[:, 0]


def _random_patterns(rng, K, C):
    """K rows whose background scores lie at least PATTERN_GAP apart and at least that far above 0 (the positives' score):
    the background logit spread over [-2, 2], the other logits N(0, 1)."""
    for _ in range(100):
        pats = rng.standard_normal((K, C)).astype(F32)
        pats[:, 0] = rng.permutation(np.linspace(-2.0, 2.0, K)).astype(F32) if K > 1 else F32(0)
        s = np.sort(np.concatenate([[0.0], _background_scores(pats)]))
        if np.diff(s).min() >= 10 * PATTERN_GAP:
            return pats
    raise AssertionError("no %d patterns of %d classes with distinct scores" % (K, C))


def pattern_conf(rng, B, P, C, K, shares=None, mode="random", num_neg=None):
    """(conf [B, P, C] fp32, pattern index [B, P]): every row of conf is one of K row patterns, pattern k on about
    shares[k] of the rows (uniform when None).
      zeros       K = 1, all logits 0: the zero-initialised head, every background row ties;
      random      K random patterns (_random_patterns);
      zero_score  pattern 0 is [0, -200, -200, ...] and every logit of the batch is <= 0: its exps beside the first vanish
                  against 1 in fp32 and in fp64, so its background score is exactly 0, the positives' score.  With num_neg
                  (the restatement's num_neg per image) image b gets num_neg[b] // 2 rows of the other patterns, which puts
                  the boundary inside the score-0 group;
      neg_inf     random patterns clipped to <= 2 and ONE element of the batch (row 0 of image 0, the last class) set to
                  1000: every other row's exps underflow to 0 in fp32 and fp64 alike (exp(-998)), score -inf.
    Returns the pattern index too, so a test can name the tie groups."""
    assert C >= 2 and K >= 1
    if mode == "zeros":
        assert K == 1
        return np.zeros((B, P, C), F32), np.zeros((B, P), np.int64)
    pats = _random_patterns(rng, K, C)
    p = None if shares is None else np.asarray(shares, np.float64) / np.sum(shares)
    idx = rng.choice(K, size=(B, P), p=p)
    if mode == "zero_score":
        pats = pats - np.maximum(pats.max(), F32(0)) - F32(0.5)         # a common shift keeps the scores; all logits < 0
        pats[0] = F32(-200)
        pats[0, 0] = F32(0)
        if num_neg is not None:
            idx[:] = 0
            for b in range(B):
                n_hot = min(int(num_neg[b]) // 2, P)
                idx[b, rng.choice(P, n_hot, replace=False)] = rng.integers(1, K, n_hot) if K > 1 else 0
    elif mode == "neg_inf":
        pats = np.minimum(pats, F32(2))
    conf = pats[idx].astype(F32)
    if mode == "neg_inf":
        conf[0, 0, C - 1] = F32(1000)
    return np.ascontiguousarray(conf), idx


def tiled_priors(base, copies, stride, P=None):
    """[P, 4]: prior i of base[:stride] at the indices i, i + stride, ..., i + (copies - 1) * stride (stride such as 300 or
    64 k + 1: the copies fall into other waves and other 256-prior chunks), rows behind copies * stride far away.  Every
    truth then has `copies` exactly tied best priors, of which the lowest index must win."""
    base = np.asarray(base, F32)[:stride]
    if len(base) < stride:
        base = np.concatenate([base, np.repeat(FAR[None], stride - len(base), 0)])
    P = copies * stride if P is None else P
    assert copies >= 2 and P >= copies * stride
    return np.ascontiguousarray(np.concatenate([np.tile(base, (copies, 1)), np.repeat(FAR[None], P - copies * stride, 0)]).astype(F32))


def tiled_arm(rng, B, copies, stride, P):
    """An ARM input for tiled_priors: equal rows for equal priors and the last two columns 0 (exp(0) = 1 is exact everywhere,
    so the decoded boxes, and with them the ties, are exact)."""
    a = np.zeros((B, stride, 4), F32)
    a[:, :, :2] = (0.3 * rng.standard_normal((B, stride, 2))).astype(F32)
    out = np.zeros((B, P, 4), F32)
    out[:, :copies * stride] = np.tile(a, (1, copies, 1))
    return out


def threshold_case(P=520, a=5, b=300):
    """(priors [P, 4], target [1, 5], a, b): prior A = (0.5, 0.5, 0.5, 0.5) at index a, prior B = (0.375, 0.5, 0.25, 0.5) at
    index b (another 256-prior chunk), every other prior far away, and the truth [0.25, 0.25, 0.5, 0.75] with label 6.  B is
    the truth's box (IoU 1, the forced match).  A: inter 0.125, union 0.25 + 0.125 - 0.125, IoU exactly 0.5 (all dyadic): a
    positive at threshold 0.5, background at nextafter(0.5, 1)."""
    pri = np.repeat(FAR[None], P, 0)
    pri[a] = (0.5, 0.5, 0.5, 0.5)
    pri[b] = (0.375, 0.5, 0.25, 0.5)
    return pri.astype(F32), np.array([[0.25, 0.25, 0.5, 0.75, 6.0]], F32), a, b


def truth_counts(rng, B):
    """B truth counts: as many of TRUTH_COUNTS as fit (all eight at B >= 8), image 0 never empty, the rest 1..40."""
    if B >= len(TRUTH_COUNTS):
        counts = list(TRUTH_COUNTS) + [int(v) for v in rng.integers(1, 41, B - len(TRUTH_COUNTS))]
        counts = [counts[i] for i in rng.permutation(B)]
    else:
        counts = [int(v) for v in rng.choice(TRUTH_COUNTS, B, replace=False)]
    if counts[0] == 0:
        j = int(np.argmax(counts))
        counts[0], counts[j] = counts[j], counts[0]
    if counts[0] == 0:
        counts[0] = 1
    return counts


def edge_targets(rng, counts, C, priors):
    """synth_targets(counts) with, where an image has the rows for it: the TINY truth last (it overlaps no prior and takes
    prior 0), the box of prior P - 1 before it (its best prior is P - 1, in the last, ragged chunk), and at n >= 12 one box
    at the rows 1, 3, 5, 7, 9 with labels that differ where C allows (they share a best prior; row 9 wins it)."""
    targets = synth_targets(rng, len(counts), 1, 1, max(C, 2), counts)
    last = point_form(priors[-1:])[0]
    for t in targets:
        n = len(t)
        if n >= 12:
            for k, r in enumerate((3, 5, 7, 9)):
                t[r, :4] = t[1, :4]
                t[r, 4] = (t[1, 4] + k + 1) % max(C - 1, 1)
        if n >= 2:
            t[n - 1] = np.append(TINY, F32(0))
        if n >= 3:
            t[n - 2, :4] = last
    return targets


def fragile_priors(threshold, target, priors, v, arm_loc):
    """[P] bool: the priors of one image whose conf_t one ulp of the ARM decode's exp can move: the best IoU within 1e-6 of
    another truth's (exact ties, as of identical truths, move together and do not count) or of the threshold."""
    target = np.asarray(target, F32).reshape(-1, 5)
    P = priors.shape[0]
    if len(target) == 0:
        return np.zeros(P, bool)
    boxes = point_form(priors) if arm_loc is None else decode(np.asarray(arm_loc, F32), priors, v)
    ov = iou(target[:, :4], boxes).astype(np.float64)
    best = ov.max(0)
    d = best[None, :] - ov
    near = ((d > 0) & (d <= 1e-6)).any(0)
    return near | (np.abs(best - float(F32(threshold))) <= 1e-6)


def mining_scores_f32(conf, conf_t):
    """The device's arithmetic for the mining score ([B, P] fp32): the batch max, correctly rounded fp32 exps summed one
    after the other in fp32, log, plus the max, minus the target logit; 0 on positives."""
    B, P = conf_t.shape
    x = conf.reshape(B * P, -1).astype(F32)
    g = x.max()
    s = _exp(x - g).cumsum(1, dtype=F32)[:, -1]
    with np.errstate(divide="ignore"):
        sc = (_log(s) + g) - x[np.arange(B * P), conf_t.reshape(-1)]
    sc[conf_t.reshape(-1) > 0] = 0
    return sc.reshape(B, P)


def select_from_scores(s, conf_t, negpos):
    """select's rule on given scores [B, P]: sel alone."""
    B, P = conf_t.shape
    pos = conf_t > 0
    sel = pos.astype(np.uint8)
    for b in range(B):
        k = min(negpos * int(pos[b].sum()), P - 1)
        if k == 0:
            continue
        neg = np.zeros(P, bool)
        neg[np.argsort(-s[b], kind="stable")[:k]] = True
        sel[b][neg & ~pos[b]] = 2
    return sel


FUZZ_SEEDS = tuple(range(32))
FUZZ_B = (1, 2, 3, 5, 32)
FUZZ_P = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 6375, 16320)
FUZZ_C = (2, 3, 21, 81, 201, 1024)
FUZZ_NEGPOS = (0, 1, 3, 7)
FUZZ_MAX_ELEMS = 12_000_000                      # B * P * C of a case (the fp64 oracle's arrays)
_GOLDEN_PRIORS = {6375: "VOC_320", 16320: "VOC_512_RefineDet"}


def _schedule(values, n, seed):
    """n draws that run through permutations of `values`: every value comes up about equally often, whatever n."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    while len(out) < n:
        out += [values[i] for i in rng.permutation(len(values))]
    return out[:n]


def fuzz_case(seed, golden_dir):
    """The drawn case of test_loss_fuzz_matches_restatement[seed]: a dict with B, P, C, negpos, refine, only_loc, mode, tiled
    (None or (copies, stride)), priors, targets, loc, conf (None with only_loc), arm (None when plain), exact_arm, and the
    restatement's conf_t of it.  P, B, C and the conf mode each run through every value (_schedule); the rest is drawn."""
    n = len(FUZZ_SEEDS)
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    B, P, C = _schedule(FUZZ_B, n, 1)[seed], _schedule(FUZZ_P, n, 2)[seed], _schedule(FUZZ_C, n, 3)[seed]
    mode = _schedule(CONF_MODES, n, 4)[seed]
    while B * P * C > FUZZ_MAX_ELEMS or (C == 1024 and B * P > 20000):
        C = FUZZ_C[FUZZ_C.index(C) - 1]
    only_loc = seed % 8 == 5
    if only_loc:
        C, mode = 2, "none"
    elif P < 63 and mode != "gaussian":           # one or two priors hold no tie group with members on both sides of a boundary
        mode = "gaussian"
    # the tie modes need a boundary (negpos > 0); the -inf group is reached only behind the positives' own ranks (negpos > 1)
    negpos = int(rng.choice({"gaussian": FUZZ_NEGPOS, "none": FUZZ_NEGPOS, "neg_inf": (3, 7), "cap": (7,)}.get(mode, (1, 3, 7))))
    refine = bool(rng.integers(0, 2))
    priors = priors_of(_GOLDEN_PRIORS[P], golden_dir) if P in _GOLDEN_PRIORS else fuzz_priors(rng, P)
    tiled = None
    if P >= 255 and rng.integers(0, 2):
        stride = int(rng.choice([s for s in (65, 129, 257, 300) if 2 * s <= P] or [P // 2]))
        tiled = (P // stride, stride)
        priors = tiled_priors(priors[rng.permutation(P)[:stride]], tiled[0], stride, P)
    counts = truth_counts(rng, B)
    if mode == "cap":
        counts = [max(c, min(512, max(64, P // 2))) for c in counts]      # negpos * num_pos > P - 1 needs many truths
    targets = edge_targets(rng, counts, C, priors)
    arm, exact_arm = None, False
    if refine:
        exact_arm = tiled is not None
        arm = tiled_arm(rng, B, tiled[0], tiled[1], P) if exact_arm else (0.3 * rng.standard_normal((B, P, 4))).astype(F32)
    loc = (0.5 * rng.standard_normal((B, P, 4))).astype(F32)
    conf_t = match_batch(0.5, targets, priors, (0.1, 0.2), arm)[1]
    conf = None
    if not only_loc:
        num_neg = np.minimum(negpos * (conf_t > 0).sum(1), P - 1)
        if mode == "gaussian":
            conf = (1.5 * rng.standard_normal((B, P, C))).astype(F32)
        elif mode == "zeros":
            conf = pattern_conf(rng, B, P, C, 1, mode="zeros")[0]
        else:
            K = int(rng.integers(3, 9))
            shares = rng.random(K) + 0.2
            conf = pattern_conf(rng, B, P, C, K, shares, "random" if mode == "cap" else mode, num_neg)[0]
    return dict(seed=seed, B=B, P=P, C=C, negpos=negpos, refine=refine, only_loc=only_loc, mode=mode, tiled=tiled, counts=counts,
                priors=priors, targets=targets, loc=loc, conf=conf, arm=arm, exact_arm=exact_arm, conf_t=conf_t)


def describe(k):
    return "seed=%d B=%d P=%d C=%d negpos=%d %s%s mode=%s tiled=%r truths=%r" % (
        k["seed"], k["B"], k["P"], k["C"], k["negpos"], "refine" if k["refine"] else "plain", " only_loc" if k["only_loc"] else "",
        k["mode"], k["tiled"], k["counts"] if len(k["counts"]) <= 8 else "%d..%d" % (min(k["counts"]), max(k["counts"])))
