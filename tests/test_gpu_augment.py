"""SSDAugmentation on the device (tdrn_hip.h section ii-c) against the reference's own draws and the numpy restatement.

Tape mode replays the draws recorded from the reference (tests/golden/augment_cases.npz) and must give its decisions and
boxes bit for bit; the apply kernel must give the restatement's pixels bit for bit (the restatement itself reproduces the
reference's pixels exactly: tests/test_augment_ref.py).  Philox mode is checked for determinism, independence from the batch,
the reference's invariants and its decision rates."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as R  # noqa: E402
from tdrn_amd import _lib  # noqa: E402
from tdrn_amd.layers.box_utils import PackedTargets  # noqa: E402
from tdrn_amd.utils.augmentations import SSDAugmentation, params_to_dicts  # noqa: E402
from test_gpu_caller_memory import Guarded  # noqa: E402

DEV = "cuda:0"
MEAN = (104, 117, 123)
gpu = pytest.mark.gpu
KEYS = ("brightness", "contrast_pre", "contrast_post", "saturation", "hue", "perm", "canvas_w", "canvas_h", "img_x", "img_y",
        "crop", "mirror", "kept", "status")


def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "augment_cases.npz"))
    cases = []
    for i in range(len({k.split("_")[0] for k in z.files})):
        k = "c%02d_" % i
        H, W = (int(v) for v in z[k + "hw"])
        img = z[k + "image"] if k + "image" in z.files else R.case_image(H, W, int(R_base(i)))
        cases.append(dict(H=H, W=W, S=int(z[k + "S"]), target=z[k + "target"], tape=z[k + "tape"], boxes=z[k + "boxes"],
                          labels=z[k + "labels"], img=img, pixels=z[k + "pixels"] if k + "pixels" in z.files else None))
    return cases


def R_base(i):
    """The base seed of fixture case i (make_golden_augment.CASES): the frame is case_image(H, W, base)."""
    return (0, 10, 20, 30, 40, 50, 60, 70, 80, 100, 110, 120, 130, 140, 150, 160, 170, 180, 190, 200, 210, 220, 230, 240)[i]


def _dev(imgs):
    return [torch.from_numpy(np.ascontiguousarray(im)).to(DEV) for im in imgs]


def _rows(packed):
    off = packed.offsets.cpu().numpy()
    t = packed.truths.cpu().numpy()
    return [t[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def _random_batch(B, seed, max_boxes=8, zero=()):
    rs = np.random.RandomState(seed)
    imgs, targets = [], []
    for b in range(B):
        H, W = int(rs.randint(300, 501)), int(rs.randint(300, 501))
        imgs.append(R.case_image(H, W, seed * 1000 + b))
        n = 0 if b in zero else int(rs.randint(1, max_boxes + 1))
        targets.append(R.case_boxes(H, W, n, seed * 1000 + b) if n else np.zeros((0, 5)))
    return imgs, targets


@gpu
def test_tape_mode_reproduces_the_reference(golden_dir):
    cases = _fixture(golden_dir)
    aug = SSDAugmentation(300, MEAN)
    imgs = _dev([c["img"] for c in cases])
    x, packed, params = aug.batch(imgs, [torch.from_numpy(c["target"]) for c in cases], tape=[c["tape"] for c in cases],
                                  return_params=True)
    got = params_to_dicts(params)
    rows = _rows(packed)
    assert packed.T_total == sum(len(c["target"]) for c in cases)
    for i, c in enumerate(cases):
        p, _, _ = R.sample(c["W"], c["H"], c["target"][:, :4], c["target"][:, 4], R.TapeDraws(c["tape"]))
        for k in KEYS:
            assert got[i][k] == p[k], (i, k, got[i][k], p[k])
        assert got[i]["status"] == 0
        assert np.array_equal(rows[i][:, :4], c["boxes"].astype(np.float32)), i        # fp64 arithmetic, one cast at the end
        assert np.array_equal(rows[i][:, 4], c["labels"].astype(np.float32)), i


@gpu
def test_apply_matches_the_restatement_bit_for_bit(golden_dir):
    cases = _fixture(golden_dir)
    n_exact = n_all = 0
    for S in sorted({c["S"] for c in cases}):
        sub = [c for c in cases if c["S"] == S]
        aug = SSDAugmentation(S, MEAN)
        x, _, params = aug.batch(_dev([c["img"] for c in sub]), [torch.from_numpy(c["target"]) for c in sub],
                                 tape=[c["tape"] for c in sub], return_params=True)
        x = x.cpu().numpy()
        for i, (c, p) in enumerate(zip(sub, params_to_dicts(params))):
            want = c["pixels"] if c["pixels"] is not None else R.apply(c["img"], p, S, MEAN, to_rgb=True)
            n_exact += int((x[i] == want).sum())
            n_all += want.size
            assert np.array_equal(x[i], want), (S, i, float(np.abs(x[i] - want).max()), float((x[i] == want).mean()))
    assert n_exact == n_all


@gpu
def test_philox_is_deterministic_and_independent_of_the_batch():
    imgs, targets = _random_batch(32, 5)
    dimgs = _dev(imgs)
    tt = [torch.from_numpy(t) for t in targets]
    ids = list(range(1000, 1032))
    aug = SSDAugmentation(320, MEAN, seed=1234)
    x1, p1, r1 = aug.batch(dimgs, tt, ids, return_params=True)
    x2, p2, r2 = aug.batch(dimgs, tt, ids, return_params=True)
    assert torch.equal(x1, x2) and torch.equal(r1, r2) and torch.equal(p1.offsets, p2.offsets)
    assert torch.equal(p1.truths[:int(p1.offsets[-1])], p2.truths[:int(p2.offsets[-1])])
    xs, ps, rs1 = aug.batch(dimgs[17:18], tt[17:18], ids[17:18], return_params=True)     # alone
    assert torch.equal(xs[0], x1[17]) and torch.equal(rs1[0], r1[17])
    assert np.array_equal(_rows(ps)[0], _rows(p1)[17])
    x3, _, r3 = aug.batch(dimgs, tt, ids, seed=99, return_params=True)                   # another seed, other draws
    assert not torch.equal(r3, r1)
    # and the pixels of Philox-drawn parameters are the restatement's
    x1 = x1.cpu().numpy()
    for b, p in list(enumerate(params_to_dicts(r1)))[:8]:
        assert np.array_equal(x1[b], R.apply(imgs[b], p, 320, MEAN, to_rgb=True)), b


def _check_sample_invariants(p, hw, target, r, i):
    """The reference's invariants on one image's decisions p (a params_to_dicts record) and moved boxes r, for a frame of
    hw = (h, w) with the truths `target`."""
    h, w = hw
    cw, ch = p["canvas_w"], p["canvas_h"]
    x0, y0, x1, y1 = p["crop"]
    assert cw >= w and ch >= h and p["img_x"] + w <= cw and p["img_y"] + h <= ch, i
    if p["cropped"]:
        ww, hh = x1 - x0, y1 - y0                 # int rect of a real w x h: |(x1 - x0) - w| < 1
        assert ww + 1 > 0.3 * cw and hh + 1 > 0.3 * ch and x1 <= cw and y1 <= ch, i
        assert (hh + 1) / max(ww - 1, 1e-9) >= 0.5 and (hh - 1) / (ww + 1) <= 2, i
        if cw - ww >= 2:                          # then W - w >= 1 and left = uniform(W - w, 1) >= 1
            assert x0 >= 1, i
        if ch - hh >= 2:
            assert y0 >= 1, i
        assert 1 <= p["kept"] <= len(target), i
    else:
        assert (x0, y0, x1, y1) == (0, 0, cw, ch) and p["kept"] == len(target), i
    assert len(r) == p["kept"] and (r[:, :4] >= 0).all() and (r[:, :4] <= 1).all(), i
    assert (r[:, 0] <= r[:, 2]).all() and (r[:, 1] <= r[:, 3]).all(), i


@gpu
def test_philox_invariants_and_rates_against_the_reference():
    n = 20000
    rs = np.random.RandomState(11)
    hw = [(int(rs.randint(300, 501)), int(rs.randint(300, 501))) for _ in range(n)]
    targets = [R.case_boxes(h, w, int(rs.randint(1, 9)), 50000 + i) for i, (h, w) in enumerate(hw)]
    aug = SSDAugmentation(320, MEAN, seed=777)
    params, packed = aug.sample(hw, [torch.from_numpy(t) for t in targets], torch.device(DEV), sample_ids=np.arange(n))
    ps = params_to_dicts(params)
    rows = _rows(packed)
    for i in range(n):
        _check_sample_invariants(ps[i], hw[i], targets[i], rows[i], i)
    # rates: the reference's own decision code (the restatement) on numpy's legacy RandomState, 4000 samples
    m = 4000
    ref = [R.sample(w, h, t[:, :4], t[:, 4], np.random.RandomState(90000 + i))[0]
           for i, ((h, w), t) in enumerate(zip(hw[:m], targets[:m]))]

    def rate(ds, f):
        return float(np.mean([f(d, s) for d, s in zip(ds, hw)]))
    checks = dict(mirror=lambda d, s: d["mirror"] == 1, expand=lambda d, s: (d["canvas_h"], d["canvas_w"]) != s,
                  no_crop=lambda d, s: d["crop"] == (0, 0, d["canvas_w"], d["canvas_h"]),
                  bright=lambda d, s: d["brightness"] != 0, contrast=lambda d, s: d["contrast_pre"] != 1 or d["contrast_post"] != 1,
                  hue=lambda d, s: d["hue"] != 0, sat=lambda d, s: d["saturation"] != 1)
    for k in range(6):
        checks["perm%d" % k] = (lambda kk: lambda d, s: d["perm"] == R.PERMS[kk])(k)
    report = {}
    for name, f in checks.items():
        a, b = rate(ps, f), rate(ref, f)
        sd = np.sqrt(max(b * (1 - b), 1e-4) * (1.0 / n + 1.0 / m))
        report[name] = (round(a, 4), round(b, 4))
        assert abs(a - b) <= 5 * sd, (name, a, b, 5 * sd)          # 5 sigma of the two-sample difference
    assert abs(rate(ps, checks["mirror"]) - 0.5) < 0.02 and abs(rate(ps, checks["expand"]) - 0.5) < 0.02
    assert abs(rate(ps, checks["perm0"]) - 7 / 12) < 0.02           # no lighting noise, or its identity permutation
    fallback = rate(ps, lambda d, s: d["status"] & _lib.AUGMENT_CROP_FALLBACK)
    assert fallback < 0.001
    assert abs(rate(ps, checks["no_crop"]) - (1 / 6 + fallback)) < 0.02
    print("rates (device, reference):", report, "fallback", fallback)


@gpu
def test_packed_targets_feed_the_loss_without_a_sync():
    from tdrn_amd.data import mb_cfg
    from tdrn_amd.layers import PriorBox
    from tdrn_amd.layers.modules import RefineMultiBoxLoss
    imgs, targets = _random_batch(32, 8)
    dimgs = _dev(imgs)
    tt = [torch.from_numpy(t).float() for t in targets]          # detection_collate's fp32 fractions
    aug = SSDAugmentation(320, MEAN, seed=5)
    pri = PriorBox(mb_cfg["VOC_320"]).forward().to(DEV)
    P = pri.size(0)
    g = torch.Generator(device="cpu").manual_seed(0)
    arm_loc = (0.1 * torch.randn(32, P, 4, generator=g)).to(DEV)
    arm_conf = torch.randn(32, P, 2, generator=g).to(DEV)
    odm_loc = (0.1 * torch.randn(32, P, 4, generator=g)).to(DEV)
    odm_conf = torch.randn(32, P, 21, generator=g).to(DEV)
    arm_crit = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, only_loc=True)
    odm_crit = RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False)
    x0, packed0 = aug.batch(dimgs, tt, list(range(32)))
    lists = [torch.from_numpy(r).to(DEV) for r in _rows(packed0)]
    ref_arm = (arm_crit(arm_loc, pri, lists),)
    ref_odm = odm_crit((odm_loc, odm_conf), pri, lists, (arm_loc, arm_conf))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, packed = aug.batch(dimgs, tt, list(range(32)))
        got_arm = (arm_crit(arm_loc, pri, PackedTargets(*packed)),)
        got_odm = odm_crit((odm_loc, odm_conf), pri, packed, (arm_loc, arm_conf))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert packed.T_total == sum(len(t) for t in targets) and packed.max_truths == max(len(t) for t in targets)
    assert torch.equal(x, x0)
    for a, b in zip(got_arm + got_odm, ref_arm + ref_odm):
        assert torch.equal(a, b), (a, b)
    assert all(torch.isfinite(v).item() for v in got_odm)


@gpu
@pytest.mark.parametrize("B,S", [(1, 320), (64, 320), (5, 512)])
def test_sizes_and_a_zero_box_image(B, S):
    imgs, targets = _random_batch(B, 20 + B, zero=(0,))
    aug = SSDAugmentation(S, MEAN, seed=3)
    x, packed, params = aug.batch(_dev(imgs), [torch.from_numpy(t) for t in targets], list(range(B)), return_params=True)
    assert x.shape == (B, 3, S, S) and torch.isfinite(x).all()
    ps = params_to_dicts(params)
    assert ps[0]["kept"] == 0 and ps[0]["cropped"] == 0 and ps[0]["crop"] == (0, 0, ps[0]["canvas_w"], ps[0]["canvas_h"])
    off = packed.offsets.cpu().numpy()
    assert off[0] == 0 and off[1] == 0 and np.array_equal(np.diff(off), [p["kept"] for p in ps])
    xh = x.cpu().numpy()
    for b in sorted({0, B // 2, B - 1}):
        assert np.array_equal(xh[b], R.apply(imgs[b], ps[b], S, MEAN, to_rgb=True)), b
    # BGR order on request: the same planes, swapped
    x_bgr = aug.apply(_dev(imgs), params, to_rgb=False)
    assert torch.equal(x_bgr, x.flip(1))


@gpu
def test_one_image_call_has_the_reference_signature():
    img = R.case_image(375, 500, 4)
    t = R.case_boxes(375, 500, 3, 4)
    aug = SSDAugmentation(300, MEAN, seed=9)
    out, boxes, labels = aug(torch.from_numpy(img), t[:, :4], t[:, 4])
    assert out.shape == (300, 300, 3) and out.is_cuda and boxes.shape[1] == 4 and labels.shape == boxes.shape[:1]


@gpu
def test_outputs_stay_inside_guard_bands():
    B, S = 6, 320
    imgs, targets = _random_batch(B, 31, zero=(2,))
    dimgs = _dev(imgs)
    tt = [torch.from_numpy(t) for t in targets]
    aug = SSDAugmentation(S, MEAN, seed=17)
    x_ref, packed_ref, params_ref = aug.batch(dimgs, tt, list(range(B)), return_params=True)
    T = packed_ref.T_total
    # sample: params, rows and offsets in guarded buffers (rows at a 4-byte offset)
    ids = torch.arange(B, dtype=torch.int64, device=DEV)
    hw = torch.tensor([im.shape[:2] for im in imgs], dtype=torch.int32, device=DEV)
    rows = torch.cat([t.double() for t in tt if t.numel()]).to(DEV)
    counts = [len(t) for t in targets]
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)
    gp = Guarded((B, C.sizeof(_lib.AugmentParams)), torch.uint8)
    gr = Guarded((T, 5), offset=4)
    go = Guarded((B + 1,), torch.int32)
    _lib.check(_lib.lib().tdrn_augment_sample(_lib.ptr(hw), _lib.ptr(rows), _lib.ptr(off), T, max(counts), B, 17, _lib.ptr(ids),
                                              None, None, gp.ptr(), gr.ptr(), go.ptr(), _lib.current_stream()))
    # apply: the output at a 4-byte offset
    gx = Guarded((B, 3, S, S), offset=4)
    aug.apply(dimgs, params_ref, to_rgb=True, out=gx.t)
    gp.check("records")
    gr.check("rows", full=False)                                                # written up to the kept count only
    go.check("offsets")
    gx.check("pixels")
    assert torch.equal(gp.t, params_ref)
    assert torch.equal(go.t, packed_ref.offsets)
    k = int(packed_ref.offsets[-1])
    assert torch.equal(gr.t[:k], packed_ref.truths[:k])
    assert torch.equal(gx.t, x_ref)
