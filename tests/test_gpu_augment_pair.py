"""pairSSDAugmentation on the device (tdrn_hip.h section ii-d) against the reference's own draws, the numpy restatement, the
merged single-frame kernels and a hand-written known answer.

Tape mode replays the draws recorded from the reference's pull_translational_item + pairSSDAugmentation
(tests/golden/augment_pair_cases.npz) and must give its decisions and both box sets bit for bit; the apply kernel must give
both frames' pixels bit for bit (the restatement reproduces the reference's exactly: tests/test_augment_pair_ref.py).  Fed
identical frames the pair entries must equal SSDAugmentation's.  Philox mode is checked for determinism, independence from the
batch, the invariants and the decision rates."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as R  # noqa: E402
import _augment_pair_ref as P  # noqa: E402
from tdrn_amd import _lib  # noqa: E402
from tdrn_amd.utils.augmentations import (PairSSDAugmentation, SSDAugmentation, pair_params_to_dicts,  # noqa: E402
                                          params_to_dicts)
from test_gpu_augment import MEAN, _dev, _rows  # noqa: E402
from test_gpu_caller_memory import Guarded  # noqa: E402

DEV = "cuda:0"
gpu = pytest.mark.gpu
SHARED = ("brightness", "contrast_pre", "contrast_post", "saturation", "hue", "perm", "canvas_w", "canvas_h", "img_x", "img_y",
          "mirror")
KEYS = SHARED + ("crop", "kept", "status", "shift_x", "shift_y", "trans_x", "trans_y", "attempts")
BASES = (0, 10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 200, 210, 220, 230)      # make_golden_augment_pair.CASES
FALLBACK_CASE = 5


def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "augment_pair_cases.npz"))
    cases = []
    for i in range(len({k.split("_")[0] for k in z.files})):
        k = "c%02d_" % i
        H, W = (int(v) for v in z[k + "hw"])
        c = dict(H=H, W=W, S=int(z[k + "S"]), target=z[k + "target"], tape=z[k + "tape"], pixels=None)
        c["img"] = z[k + "image"] if k + "image" in z.files else R.case_image(H, W, BASES[i])
        for name in ("boxes0", "boxes1", "labels0", "labels1"):
            c[name] = z[k + name]
        if k + "pixels0" in z.files:
            c["pixels"] = (z[k + "pixels0"], z[k + "pixels1"])
        cases.append(c)
    return cases


def _tt(targets):
    return [torch.from_numpy(np.ascontiguousarray(t)) for t in targets]


def _same_offsets(a, b):
    return a.offsets.data_ptr() == b.offsets.data_ptr() and a.T_total == b.T_total and a.max_truths == b.max_truths


class LogDraws(object):
    """A RandomState whose draws are logged: the restatement's run on it is replayed by the device in tape mode."""

    def __init__(self, seed):
        self.rs, self.tape = np.random.RandomState(seed), []

    def _log(self, v):
        self.tape.append(float(v))
        return v

    def rand(self):
        return self._log(self.rs.rand())

    def randint(self, n):
        return self._log(self.rs.randint(n))

    def uniform(self, low=0.0, high=1.0):
        return self._log(self.rs.uniform(low, high))


@gpu
def test_tape_mode_reproduces_the_reference(golden_dir):
    cases = _fixture(golden_dir)
    aug = PairSSDAugmentation(300, MEAN)
    params, packed, packed_t = aug.sample([(c["H"], c["W"]) for c in cases], _tt([c["target"] for c in cases]),
                                          torch.device(DEV), tape=[c["tape"] for c in cases])
    got = pair_params_to_dicts(params)
    assert _same_offsets(packed, packed_t) and packed.T_total == sum(len(c["target"]) for c in cases)
    rows, rows_t = _rows(packed), _rows(packed_t)
    for i, c in enumerate(cases):
        p = P.sample_pair(c["W"], c["H"], c["target"][:, :4], c["target"][:, 4], R.TapeDraws(c["tape"]))[0]
        for k in KEYS:
            assert got[i][k] == p[k], (i, k, got[i][k], p[k])
        assert got[i]["status"] == (_lib.AUGMENT_TRANS_FALLBACK if i == FALLBACK_CASE else 0), i
        assert np.array_equal(rows[i][:, :4], c["boxes0"].astype(np.float32)), i       # fp64 arithmetic, one cast at the end
        assert np.array_equal(rows_t[i][:, :4], c["boxes1"].astype(np.float32)), i
        assert np.array_equal(rows[i][:, 4], c["labels0"].astype(np.float32)), i
        assert np.array_equal(rows_t[i][:, 4], c["labels1"].astype(np.float32)), i


@gpu
def test_apply_matches_the_fixture_and_the_restatement_bit_for_bit(golden_dir):
    cases = _fixture(golden_dir)
    n_exact = n_all = 0
    groups = [(S, [c for c in cases if c["pixels"] is not None and c["S"] == S]) for S in (32, 48)]
    groups.append((300, [c for c in cases if c["pixels"] is None]))                 # the VOC-size cases, all at S = 300
    assert [len(g) for _, g in groups] == [11, 1, 4]
    for S, sub in groups:
        aug = PairSSDAugmentation(S, MEAN)
        x, x_t, _, _, params = aug.batch(_dev([c["img"] for c in sub]), _tt([c["target"] for c in sub]),
                                         tape=[c["tape"] for c in sub], return_params=True)
        x, x_t = x.cpu().numpy(), x_t.cpu().numpy()
        for i, (c, p) in enumerate(zip(sub, pair_params_to_dicts(params))):
            want = c["pixels"] if c["pixels"] is not None else P.apply_pair(c["img"], p, S, MEAN, to_rgb=True)
            for got, w in ((x[i], want[0]), (x_t[i], want[1])):
                n_exact += int((got == w).sum())
                n_all += w.size
                assert np.array_equal(got, w), (S, i, float(np.abs(got - w).max()), float((got == w).mean()))
    assert n_exact == n_all == 2 * 3 * (11 * 32 * 32 + 48 * 48 + 4 * 300 * 300)


@gpu
@pytest.mark.parametrize("mode", ["philox", "tape"])
def test_identical_frames_equal_the_single_chain(golden_dir, mode):
    B, S = 8, 48
    if mode == "tape":
        z = np.load(os.path.join(golden_dir, "augment_cases.npz"))
        ks = [k[:4] for k in sorted(z.files) if k.endswith("_image")]           # the seven frames the fixture keeps ...
        ks = (ks + ks)[:B]                                                      # ... and the first one's draws once more,
        imgs, targets = [z[k + "image"] for k in ks], [z[k + "target"] for k in ks]
        imgs[-1] = R.case_image(*imgs[-1].shape[:2], 999)                       # on another frame of its size
        src = dict(tape=[z[k + "tape"] for k in ks])
    else:
        rs = np.random.RandomState(3)
        hw = [(int(rs.randint(20, 65)), int(rs.randint(20, 65))) for _ in range(B)]
        imgs = [R.case_image(h, w, 300 + b) for b, (h, w) in enumerate(hw)]
        targets = [R.case_boxes(h, w, 1 + b % 4, 300 + b) for b, (h, w) in enumerate(hw)]
        src = dict(sample_ids=list(range(40, 40 + B)), seed=21)
    assert len(imgs) == B and all(max(im.shape[:2]) <= 64 for im in imgs)
    dimgs, tt = _dev(imgs), _tt(targets)
    x, packed, params = SSDAugmentation(S, MEAN).batch(dimgs, tt, return_params=True, **src)
    x0, x1, p0, p1, pair = PairSSDAugmentation(S, MEAN).batch(dimgs, tt, images_t=dimgs, targets_t=tt, return_params=True, **src)
    assert torch.equal(pair[:, :80], params)                                    # the embedded record, byte for byte
    assert not pair[:, 80:].any()                                               # no translation: shift 0, attempts 0
    assert torch.equal(x0, x) and torch.equal(x1, x)
    assert _same_offsets(p0, p1) and torch.equal(p0.offsets, packed.offsets)
    k = int(packed.offsets[-1])
    assert torch.equal(p0.truths[:k], packed.truths[:k]) and torch.equal(p1.truths[:k], packed.truths[:k])


@gpu
@pytest.mark.parametrize("u,want", [((0.1, 0.2), (-2, -1)), ((0.9, 0.75), (2, 1))])
def test_translated_frame_is_the_first_shifted_over_black(u, want):
    """A known answer that owes nothing to the restatement: every photometric switch off, no expand, mode None, no mirror and
    S = the frame's size, so the output is the frame's own pixels (through the HSV round trip) minus the mean."""
    # x_trans = -0.1 + (u * 2) * 0.1: 0.1 -> -0.08 (* 32 = -2.56 -> -2), 0.2 -> -0.06 (-1.92 -> -1); 0.9 -> 0.08 (2.56 -> 2),
    # 0.75 -> 0.05 (1.6 -> 1).  Then: brightness off, contrast last, saturation / hue / contrast / noise off, expand 1 = none,
    # mode 0 = None, no mirror.
    tape = [u[0], u[1], 0, 0, 0, 0, 0, 0, 1, 0, 0]
    img = R.case_image(32, 32, 7)
    assert img.min(axis=2).max() > 0                                            # some pixels are not black
    aug = PairSSDAugmentation(32, MEAN)
    x, x_t, _, _, params = aug.batch(_dev([img]), _tt([np.array([[0.3, 0.3, 0.7, 0.7, 1.0]])]), tape=[tape], return_params=True)
    p = pair_params_to_dicts(params)[0]
    tx, ty = want
    assert (p["trans_x"], p["trans_y"], p["attempts"], p["status"], p["cropped"], p["mirror"]) == (tx, ty, 1, 0, 0, 0)
    assert (p["canvas_w"], p["canvas_h"], p["crop"]) == (32, 32, (0, 0, 32, 32))
    x, x_t = x[0].cpu().numpy(), x_t[0].cpu().numpy()
    black = (0 - np.array(MEAN, np.float32))[::-1]                              # RGB planes
    n_in = 0
    for y in range(32):
        for xx in range(32):
            if 0 <= y - ty < 32 and 0 <= xx - tx < 32:
                assert np.array_equal(x_t[:, y, xx], x[:, y - ty, xx - tx]), (y, xx)
                n_in += 1
            else:
                assert np.array_equal(x_t[:, y, xx], black), (y, xx)
    assert n_in == (32 - abs(tx)) * (32 - abs(ty))


def _philox_inputs(n, seed):
    rs = np.random.RandomState(seed)
    hw = [(int(rs.randint(300, 501)), int(rs.randint(300, 501))) for _ in range(n)]
    # every fourth image has a box with its centre 0.01 from two edges, so that second and third attempts are common
    targets = [P.edge_boxes(1 + i % 3, 0.01, 60000 + i) if i % 4 == 0 else R.case_boxes(h, w, int(rs.randint(1, 9)), 60000 + i)
               for i, (h, w) in enumerate(hw)]
    return hw, targets


@gpu
def test_philox_determinism_invariants_and_rates():
    n, m, r = 4000, 2000, 0.1
    hw, targets = _philox_inputs(n, 13)
    tt = _tt(targets)
    dev = torch.device(DEV)
    aug = PairSSDAugmentation(320, MEAN, seed=777)
    ids = np.arange(n) + 5000
    params, packed, packed_t = aug.sample(hw, tt, dev, sample_ids=ids)
    params2, packed2, packed2_t = aug.sample(hw, tt, dev, sample_ids=ids)
    k = int(packed.offsets[-1])
    assert torch.equal(params, params2) and torch.equal(packed.offsets, packed2.offsets)
    assert torch.equal(packed.truths[:k], packed2.truths[:k]) and torch.equal(packed_t.truths[:k], packed2_t.truths[:k])
    # sample 5 of a batch of 17 equals the sample alone
    pa, ka, ka_t = aug.sample(hw[:17], tt[:17], dev, sample_ids=ids[:17])
    pb, kb, kb_t = aug.sample(hw[5:6], tt[5:6], dev, sample_ids=ids[5:6])
    assert torch.equal(pa, params[:17]) and torch.equal(pb[0], params[5])
    assert np.array_equal(_rows(ka)[5], _rows(kb)[0]) and np.array_equal(_rows(ka_t)[5], _rows(kb_t)[0])
    assert np.array_equal(_rows(kb)[0], _rows(packed)[5]) and np.array_equal(_rows(kb_t)[0], _rows(packed_t)[5])
    # invariants
    ps = pair_params_to_dicts(params)
    rows, rows_t = _rows(packed), _rows(packed_t)
    assert _same_offsets(packed, packed_t)
    for i, (p, (h, w)) in enumerate(zip(ps, hw)):
        for q in (rows[i], rows_t[i]):
            assert len(q) == p["kept"] and (q[:, :4] >= 0).all() and (q[:, :4] <= 1).all(), i
            assert (q[:, 0] <= q[:, 2]).all() and (q[:, 1] <= q[:, 3]).all(), i
        assert 1 <= p["kept"] <= len(targets[i]) and np.array_equal(rows[i][:, 4], rows_t[i][:, 4]), i
        assert abs(p["trans_x"]) <= r * w and abs(p["trans_y"]) <= r * h, i
        assert abs(p["shift_x"]) <= r / p["attempts"] and abs(p["shift_y"]) <= r / p["attempts"], i
        assert 1 <= p["attempts"] <= 3, i
        if p["status"] & _lib.AUGMENT_TRANS_FALLBACK:
            assert p["attempts"] == 3 and (p["shift_x"], p["shift_y"], p["trans_x"], p["trans_y"]) == (0, 0, 0, 0), i
        else:
            assert (p["trans_x"], p["trans_y"]) == (int(p["shift_x"] * w), int(p["shift_y"] * h)), i
    # the shared decisions are the single sampler's for the same seed and id
    single = params_to_dicts(SSDAugmentation(320, MEAN, seed=777).sample(hw, tt, dev, sample_ids=ids)[0])
    for i in range(n):
        for key in SHARED:
            assert ps[i][key] == single[i][key], (i, key)
    # rates: the restatement on numpy's legacy RandomState over the first m samples
    ref = [P.sample_pair(w, h, t[:, :4], t[:, 4], np.random.RandomState(90000 + i), r)[0]
           for i, ((h, w), t) in enumerate(zip(hw[:m], targets[:m]))]
    fb = _lib.AUGMENT_TRANS_FALLBACK
    checks = dict(no_crop=lambda d: d["crop"] == (0, 0, d["canvas_w"], d["canvas_h"]),
                  attempts1=lambda d: d["attempts"] == 1, attempts2=lambda d: d["attempts"] == 2,
                  attempts3=lambda d: d["attempts"] == 3 and not d["status"] & fb, fallback=lambda d: bool(d["status"] & fb))
    report = {}
    for name, f in checks.items():
        a, b = float(np.mean([f(d) for d in ps])), float(np.mean([f(d) for d in ref]))
        sd = np.sqrt(max(b * (1 - b), 1e-4) * (1.0 / n + 1.0 / m))
        report[name] = (round(a, 4), round(b, 4))
        assert abs(a - b) <= 5 * sd, (name, a, b, 5 * sd)             # 5 sigma of the two-sample difference
    crop_fallback = float(np.mean([bool(d["status"] & _lib.AUGMENT_CROP_FALLBACK) for d in ps]))
    assert crop_fallback < 0.001
    assert report["attempts2"][0] > 0.02 and report["fallback"][0] > 0        # the retries were exercised
    print("rates (device, restatement):", report, "crop fallback", crop_fallback)


def _ragged(B, seed, supplied):
    rs = np.random.RandomState(seed)
    imgs, targets, imgs_t, targets_t = [], [], [], []
    for b in range(B):
        H, W = int(rs.randint(17, 91)), int(rs.randint(17, 91))
        if H == W:
            W = W - 1 if W > 17 else W + 1
        n = int(rs.randint(1, 6))
        if B > 1 and b == 3:
            H, W, n = 60, 90, 70                                             # more truths than a wave has lanes
        if B > 1 and b == 9:
            n = 0                                                            # and an image with none
        imgs.append(R.case_image(H, W, seed * 100 + b))
        t = R.case_boxes(H, W, n, seed * 100 + b) if n else np.zeros((0, 5))
        targets.append(t)
        if supplied:
            imgs_t.append(R.case_image(H, W, seed * 100 + 50 + b))
            t2 = t.copy()
            t2[:, :4] = np.clip(t2[:, :4] + rs.uniform(-0.05, 0.05, (len(t), 1)), 0, 1)
            targets_t.append(t2)
    return imgs, targets, (imgs_t if supplied else None), (targets_t if supplied else None)


@gpu
@pytest.mark.parametrize("B,S,supplied", [(17, 33, False), (17, 48, True), (17, 32, False), (1, 32, False), (1, 33, True)])
def test_ragged_shapes_match_the_restatement(B, S, supplied):
    imgs, targets, imgs_t, targets_t = _ragged(B, 40 + B + S, supplied)
    want, tapes = [], []
    for b in range(B):
        d = LogDraws(7000 + 31 * S + b)
        h, w = imgs[b].shape[:2]
        t = targets[b]
        t2 = targets_t[b] if supplied else None
        want.append(P.sample_pair(w, h, t[:, :4], t[:, 4], d, 0.1, None if t2 is None else t2[:, :4],
                                  None if t2 is None else t2[:, 4], max_rounds=R.MAX_ROUNDS))
        tapes.append(d.tape)
    aug = PairSSDAugmentation(S, MEAN)
    x, x_t, packed, packed_t, params = aug.batch(_dev(imgs), _tt(targets), tape=tapes, images_t=_dev(imgs_t) if supplied else None,
                                                 targets_t=_tt(targets_t) if supplied else None, return_params=True)
    assert x.shape == x_t.shape == (B, 3, S, S) and _same_offsets(packed, packed_t)
    got = pair_params_to_dicts(params)
    rows, rows_t = _rows(packed), _rows(packed_t)
    x, x_t = x.cpu().numpy(), x_t.cpu().numpy()
    assert np.array_equal(np.diff(packed.offsets.cpu().numpy()), [w[0]["kept"] for w in want])
    for b, (p, b0, b1, l0, l1) in enumerate(want):
        for k in KEYS:
            assert got[b][k] == p[k], (b, k, got[b][k], p[k])
        assert np.array_equal(rows[b], np.hstack([b0, l0[:, None]]).astype(np.float32)), b
        assert np.array_equal(rows_t[b], np.hstack([b1, l1[:, None]]).astype(np.float32)), b
        w0, w1 = P.apply_pair(imgs[b], p, S, MEAN, True, imgs_t[b] if supplied else None)
        assert np.array_equal(x[b], w0), (b, float((x[b] == w0).mean()))
        assert np.array_equal(x_t[b], w1), (b, float((x_t[b] == w1).mean()))
    if B > 1:
        assert got[9]["kept"] == 0 and got[9]["attempts"] == 0 and got[9]["cropped"] == 0 and len(targets[3]) == 70
        if not supplied:
            assert any(g["trans_x"] or g["trans_y"] for g in got)


@gpu
def test_packed_pairs_feed_the_loss_without_a_sync():
    from tdrn_amd.data import mb_cfg
    from tdrn_amd.layers import PriorBox
    from tdrn_amd.layers.modules import RefineMultiBoxLoss
    B = 4
    rs = np.random.RandomState(8)
    hw = [(int(rs.randint(300, 501)), int(rs.randint(300, 501))) for _ in range(B)]
    imgs = [R.case_image(h, w, 800 + b) for b, (h, w) in enumerate(hw)]
    tt = [torch.from_numpy(R.case_boxes(h, w, 2 + b, 800 + b)).float() for b, (h, w) in enumerate(hw)]
    dimgs = _dev(imgs)
    aug = PairSSDAugmentation(320, MEAN, seed=5)
    pri = PriorBox(mb_cfg["VOC_320"]).forward().to(DEV)
    Pn = pri.size(0)
    g = torch.Generator(device="cpu").manual_seed(0)
    arm_loc = (0.1 * torch.randn(B, Pn, 4, generator=g)).to(DEV)            # static_net(images_ori)'s ARM output
    arm_conf = torch.randn(B, Pn, 2, generator=g).to(DEV)
    odm_loc = (0.1 * torch.randn(B, Pn, 4, generator=g)).to(DEV)            # net(images_trans)
    odm_conf = torch.randn(B, Pn, 21, generator=g).to(DEV)
    crit = RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False)
    x0, x0_t, _, packed0_t = aug.batch(dimgs, tt, list(range(B)))
    lists = [torch.from_numpy(r).to(DEV) for r in _rows(packed0_t)]
    ref = crit((odm_loc, odm_conf), pri, lists, (arm_loc, arm_conf))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, x_t, packed, packed_t = aug.batch(dimgs, tt, list(range(B)))
        got = crit((odm_loc, odm_conf), pri, packed_t, arm_data=(arm_loc, arm_conf))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(x, x0) and torch.equal(x_t, x0_t) and not torch.equal(x, x_t)
    for a, b in zip(got, ref):
        assert torch.equal(a, b), (a, b)
    assert all(torch.isfinite(v).item() for v in got)


@gpu
def test_outputs_stay_inside_guard_bands():
    B, S = 3, 48
    imgs, targets, _, _ = _ragged(B, 77, False)
    dimgs, tt = _dev(imgs), _tt(targets)
    aug = PairSSDAugmentation(S, MEAN, seed=17)
    x_ref, xt_ref, packed_ref, packed_t_ref, params_ref = aug.batch(dimgs, tt, list(range(B)), return_params=True)
    T = packed_ref.T_total
    ids = torch.arange(B, dtype=torch.int64, device=DEV)
    hw = torch.tensor([im.shape[:2] for im in imgs], dtype=torch.int32, device=DEV)
    rows = torch.cat([t.double() for t in tt if t.numel()]).to(DEV)
    counts = [len(t) for t in targets]
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)
    gp = Guarded((B, C.sizeof(_lib.AugmentPairParams)), torch.uint8)
    gr, gt = Guarded((T, 5), offset=4), Guarded((T, 5), offset=4)            # rows at a 4-byte offset
    go = Guarded((B + 1,), torch.int32)
    _lib.check(_lib.lib().tdrn_augment_pair_sample(_lib.ptr(hw), _lib.ptr(rows), None, _lib.ptr(off), T, max(counts), B, 0.1, 17,
                                                   _lib.ptr(ids), None, None, gp.ptr(), gr.ptr(), gt.ptr(), go.ptr(),
                                                   _lib.current_stream()))
    gx, gy = Guarded((B, 3, S, S), offset=4), Guarded((B, 3, S, S), offset=4)      # pixels at a 4-byte offset
    aug.apply(dimgs, params_ref, to_rgb=True, out=gx.t, out_t=gy.t)
    for what, g in (("records", gp), ("offsets", go), ("pixels", gx), ("pixels of frame 1", gy)):
        g.check(what)
    for what, g in (("rows", gr), ("rows of frame 1", gt)):
        g.check(what, full=False)                                               # written up to the kept count only
    assert torch.equal(gp.t, params_ref)
    assert torch.equal(go.t, packed_ref.offsets)
    k = int(packed_ref.offsets[-1])
    assert torch.equal(gr.t[:k], packed_ref.truths[:k])
    assert torch.equal(gt.t[:k], packed_t_ref.truths[:k])
    assert torch.equal(gx.t, x_ref) and torch.equal(gy.t, xt_ref)


@gpu
def test_one_pair_call_has_the_reference_signature():
    img = R.case_image(60, 80, 4)
    t = R.case_boxes(60, 80, 3, 4)
    aug = PairSSDAugmentation(48, MEAN, seed=9)
    imgs, boxes, labels = aug([torch.from_numpy(img), None], [t[:, :4], None], [t[:, 4], None])
    assert imgs[0].shape == imgs[1].shape == (48, 48, 3) and imgs[1].is_cuda
    assert boxes[0].shape == boxes[1].shape and boxes[0].shape[1] == 4 and torch.equal(labels[0], labels[1])
    img2 = R.case_image(60, 80, 5)
    imgs, boxes, labels = aug([torch.from_numpy(img), torch.from_numpy(img2)], [t[:, :4], t[:, :4]], [t[:, 4], t[:, 4]])
    assert imgs[0].shape == (48, 48, 3) and not torch.equal(imgs[0], imgs[1]) and torch.equal(boxes[0], boxes[1])
