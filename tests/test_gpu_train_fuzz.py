"""Seeded fuzz of the training kernels (loss.hip, deform_bwd.hip, augment.hip) against their CPU restatements, at the shapes
and ties the fixed cases of test_gpu_loss.py / test_gpu_deform_grad.py / test_gpu_augment.py do not reach.

Loss: the cases of _loss_ref.fuzz_case (exact ties of the mining score that straddle the num_neg boundary, rows at score 0 and
at -inf, the P - 1 cap, prior counts around every chunk and per-thread boundary, 0 .. 512 truths, exactly tied best priors in
other waves and chunks); tests/test_loss_ref.py asserts on the CPU that each case is what it claims.  Deformable backward:
_deform_grad_ref.fuzz_shape.  Augmentation: ragged frames from 16 to 1080 pixels at sizes that are no multiple of the apply
kernel's block.  Every failure message names the drawn shape."""
import os

import numpy as np
import pytest
import torch

import _augment_ref as AR
import _deform_grad_ref as gref
import _loss_ref as R
from tdrn_amd import _lib
from tdrn_amd.layers.box_utils import match_targets
from tdrn_amd.layers.modules.multibox_loss import multibox_loss
from test_gpu_augment import MEAN, _check_sample_invariants, _dev, _rows
from test_gpu_caller_memory import SENTINEL, Guarded
from test_gpu_deform_grad import _abi, _check, _cu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VAR = (0.1, 0.2)
E_UNSUPPORTED = -4


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _loss_run(priors, targets, loc, conf, arm, C, negpos, g=(0.7, 1.3), threshold=0.5):
    """(loc_t, conf_t, loss, sel, grad_loc, grad_conf) through match_targets / multibox_loss and autograd, upstream gradients g"""
    pri = _t(priors)
    loc_t, conf_t = match_targets([_t(t) for t in targets], pri, threshold, VAR, _t(arm))
    lg = _t(loc).requires_grad_(True)
    cg = None if conf is None else _t(conf).requires_grad_(True)
    loss, sel = multibox_loss(lg, cg, loc_t, conf_t, C, negpos)
    (loss * torch.tensor(g, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return (loc_t.cpu().numpy(), conf_t.cpu().numpy(), loss.detach().cpu().numpy(), sel.cpu().numpy(), lg.grad.cpu().numpy(),
            None if cg is None else cg.grad.cpu().numpy())


# ---------------------------------------------------------------------------------------------
# MultiBoxLoss / RefineMultiBoxLoss
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.FUZZ_SEEDS)
def test_loss_fuzz_matches_restatement(seed):
    k = R.fuzz_case(seed, GOLDEN)
    what = R.describe(k)
    B, P, C, negpos = k["B"], k["P"], k["C"], k["negpos"]
    loc, conf, arm, targets, priors = k["loc"], k["conf"], k["arm"], k["targets"], k["priors"]
    g = (0.7, 1.3)
    loc_t, conf_t, loss, sel, gl, gc = _loss_run(priors, targets, loc, conf, arm, C, negpos, g)

    # targets.  Plain matching and the exact ARM of the tiled cases are exact arithmetic: no exemption.  A random ARM input is
    # decoded with exp, whose last bit differs between implementations: only the priors of fragile_priors may differ.
    r_lt, r_ct = R.match_batch(0.5, targets, priors, VAR, arm)
    assert np.array_equal(r_ct, k["conf_t"])
    exempt = np.zeros((B, P), bool)
    if k["refine"] and not k["exact_arm"]:
        exempt = np.stack([R.fragile_priors(0.5, t, priors, VAR, arm[b]) for b, t in enumerate(targets)])
    share = exempt.sum() / float(B * P)
    print("%s: %d of %d priors left out of the conf_t comparison (%.4f %%)" % (what, exempt.sum(), B * P, 100 * share))
    assert share <= 0.0005, what
    bad = (conf_t != r_ct) & ~exempt
    assert not bad.any(), "%s: conf_t differs at %d priors, first (image, prior) %r" % (what, bad.sum(), np.argwhere(bad)[:5].tolist())
    rtol, atol = R.loc_t_tolerance(k["refine"])
    keep = ~exempt
    assert np.array_equal(np.isfinite(loc_t[keep]), np.isfinite(r_lt[keep])), what
    np.testing.assert_allclose(loc_t[keep], r_lt[keep], rtol=rtol, atol=atol, err_msg=what)

    # selection, on the device's own conf_t (equal to the restatement's but for the priors left out above)
    assert np.array_equal(sel == 1, conf_t > 0), what
    with np.errstate(invalid="ignore"):                       # (the gap inside a -inf group is inf - inf)
        r_sel, gaps = R.select(conf, conf_t, negpos)
    if k["mode"] == "gaussian":
        clear = gaps > 1e-5                                   # images whose num_neg boundary is not a near-tie of the scores
        assert clear.sum() >= B - 4, what
    else:
        clear = np.ones(B, bool)                              # exact ties only: no exemption
    bad = (sel != r_sel) & clear[:, None]
    assert not bad.any(), "%s: sel differs at %d rows, first (image, prior, got, want) %r" % (
        what, bad.sum(), [(int(b), int(p), int(sel[b, p]), int(r_sel[b, p])) for b, p in np.argwhere(bad)[:5]])
    if negpos == 0 or conf is None:
        assert not (sel == 2).any(), what

    # the sums and the gradients, on the device's own targets and selection
    ll, lc, N = R.losses(loc, conf, loc_t, conf_t, sel)
    rgl, rgc = R.grads(loc, conf, loc_t, conf_t, sel, *g)
    np.testing.assert_allclose(loss[0], ll, rtol=1e-5, err_msg=what)
    np.testing.assert_allclose(gl, rgl, atol=1e-6, err_msg=what)
    assert (gl[sel != 1] == 0).all(), what
    if conf is None:
        assert loss[1] == 0, what                             # only_loc: the slot keeps what the wrapper put there
        assert gc is None
    else:
        np.testing.assert_allclose(loss[1], lc, rtol=1e-5, err_msg=what)
        np.testing.assert_allclose(gc, rgc, atol=1e-6, err_msg=what)
        assert (gc[sel == 0] == 0).all(), what

    again = _loss_run(priors, targets, loc, conf, arm, C, negpos, g)
    for name, x, y in zip(("loc_t", "conf_t", "loss", "sel", "grad_loc", "grad_conf"), (loc_t, conf_t, loss, sel, gl, gc), again):
        if x is not None:
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs between two runs" % (what, name)


@pytest.mark.parametrize("refine", [False, True], ids=["plain", "refine"])
def test_iou_exactly_at_the_threshold(refine):
    pri, target, a, b = R.threshold_case()
    arm = np.zeros((1,) + pri.shape, np.float32) if refine else None
    loc = np.zeros((1,) + pri.shape, np.float32)
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    for thr, at_a in ((0.5, 7), (above, 0)):                  # `overlap < threshold` is background: AT the threshold stays positive
        loc_t, conf_t, _, sel, _, _ = _loss_run(pri, [target], loc, None, arm, 2, 3, threshold=thr)
        r_lt, r_ct = R.match_batch(thr, [target], pri, VAR, arm)
        assert r_ct[0, a] == at_a and r_ct[0, b] == 7
        assert np.array_equal(conf_t, r_ct), (thr, conf_t[0, [a, b]])
        np.testing.assert_allclose(loc_t, r_lt, rtol=3e-6, atol=1e-7)
        assert np.array_equal(sel == 1, r_ct > 0)


def test_513_truths_are_refused_and_nothing_is_written():
    rng = np.random.Generator(np.random.PCG64(1))
    P = 300
    pri = _t(R.fuzz_priors(rng, P))
    t513 = _t(R.synth_targets(rng, 1, 1, 1, 21, [513])[0])
    with pytest.raises(_lib.TdrnError) as e:
        match_targets([t513], pri, 0.5, VAR)
    assert e.value.code == E_UNSUPPORTED
    match_targets([t513[:512]], pri, 0.5, VAR)                # the limit itself is served
    lib = _lib.lib()
    assert lib.tdrn_match_workspace_bytes(1, P, 513) == 0
    nb = lib.tdrn_match_workspace_bytes(1, P, 512)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 513], dtype=torch.int32, device=DEV)
    loc_t, conf_t = Guarded((1, P, 4)), Guarded((1, P), torch.int32)
    rc = lib.tdrn_match(_lib.ptr(t513), _lib.ptr(off), 513, 513, 1, _lib.ptr(pri), P, None, 0.5, 0.1, 0.2, loc_t.ptr(), conf_t.ptr(),
                        _lib.ptr(ws), nb, _lib.current_stream(DEV))
    assert rc == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((loc_t.raw.view(torch.int32) == SENTINEL).all()) and bool((conf_t.raw.view(torch.int32) == SENTINEL).all())


def test_label_is_truncated_like_the_long_tensor_store():
    rng = np.random.Generator(np.random.PCG64(2))
    pri = R.fuzz_priors(rng, 257)
    t = R.synth_targets(rng, 1, 1, 1, 21, [6])[0]
    t[:, 4] = (3.7, 0.0, 0.999, 19.5, 2.0, 7.25)
    _, conf_t, _, _, _, _ = _loss_run(pri, [t], np.zeros((1, 257, 4), np.float32), None, None, 2, 3)
    _, r_ct = R.match_batch(0.5, [t], pri, VAR)
    assert np.array_equal(conf_t, r_ct)
    assert set(np.unique(conf_t)) <= {0, 4, 1, 20, 3, 8} and 4 in conf_t and 20 in conf_t      # 3.7 -> 4, 0.999 -> 1, 19.5 -> 20


def test_negpos_ratio_zero_mines_nothing():
    rng = np.random.Generator(np.random.PCG64(3))
    B, P, Cn = 3, 1025, 21
    pri = R.fuzz_priors(rng, P)
    targets = R.synth_targets(rng, B, 1, 1, Cn, [9, 0, 30])
    loc = (0.5 * rng.standard_normal((B, P, 4))).astype(np.float32)
    conf = (1.5 * rng.standard_normal((B, P, Cn))).astype(np.float32)
    loc_t, conf_t, loss, sel, gl, gc = _loss_run(pri, targets, loc, conf, None, Cn, 0)
    assert np.array_equal(sel, (conf_t > 0).astype(np.uint8)) and (sel == 1).sum() > 0
    ll, lc, _ = R.losses(loc, conf, loc_t, conf_t, (conf_t > 0).astype(np.uint8))        # the CE sum runs over the positives alone
    np.testing.assert_allclose(loss, [ll, lc], rtol=1e-5)
    assert (gc[conf_t == 0] == 0).all() and (gl[conf_t == 0] == 0).all() and np.abs(gc[conf_t > 0]).max() > 0
    mined = _loss_run(pri, targets, loc, conf, None, Cn, 3)
    assert (mined[3] == 2).sum() > 0 and mined[2][1] > loss[1]


# ---------------------------------------------------------------------------------------------
# deformable conv v1 backward
# ---------------------------------------------------------------------------------------------
def _deform_inputs(s, seed):
    rng = np.random.Generator(np.random.PCG64(6000 + seed))
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = s["k"], s["stride"], s["pad"], s["dil"]
    N, Cin, H, W, Cout, G = s["N"], s["Cin"], s["H"], s["W"], s["Cout"], s["G"]
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, kh, kw)) * (Cin * kh * kw) ** -0.5).astype(np.float32)
    off = (s["osc"] * rng.standard_normal((N, G * 2 * kh * kw, s["Ho"], s["Wo"]))).astype(np.float32)
    gout = rng.standard_normal((N, Cout, s["Ho"], s["Wo"])).astype(np.float32)
    dims = (N, Cin, H, W, Cout, kw, kh, sw, sh, pw, ph, dh, dw, G)
    return x, off, w, gout, dims


def _deform_compare(s, seed, what):
    x, off, w, gout, dims = _deform_inputs(s, seed)
    _, rgx, rgo, rgw = gref.grads(x, off, w, gout, s["stride"], s["pad"], s["dil"], s["G"])
    exempt = gref.near_decision(off, x.shape, w.shape, s["stride"], s["pad"], s["dil"], s["G"])
    gi, goff, gw = _abi(x, off, w, gout, dims)                # grad_offset starts as NaN: a missed entry shows
    _check(what + " grad_input", gi, rgx)
    n = _check(what + " grad_offset", goff, rgo, exempt)
    print("%s: %d of %d grad_offset entries left out (cap %d)" % (what, n, goff.numel(), max(2, goff.numel() // 1000)))
    assert n <= max(2, goff.numel() // 1000), (what, n)
    _check(what + " grad_weight", gw, rgw)


@pytest.mark.parametrize("seed", gref.FUZZ_SEEDS)
def test_deform_backward_fuzz_matches_oracle(seed):
    s = gref.fuzz_shape(seed)
    _deform_compare(s, seed, "seed=%d %r" % (seed, {k: v for k, v in s.items() if k not in ("Ho", "Wo")}))


def _wide(Cout, N, G):
    return dict(N=N, Cin=8, H=6, W=6, Cout=Cout, k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), G=G, cpg=8 // G, osc=1.0, Ho=6, Wo=6,
                M=N * 36)


@pytest.mark.parametrize("Cout,N,G", [(1100, 1, 1), (1900, 2, 2)])
def test_deform_backward_wide_cout_takes_the_8_pixel_tile(Cout, N, G):
    """Cout * 16 pixels * 4 bytes exceeds the 64 KiB of LDS: deform_bwd_data_kernel<8>."""
    assert Cout * 16 * 4 > 64 * 1024 > Cout * 8 * 4 + 4096
    _deform_compare(_wide(Cout, N, G), Cout, "Cout=%d N=%d G=%d" % (Cout, N, G))


def test_deform_backward_beyond_the_lds_budget_is_refused_by_both_entries():
    s = _wide(2100, 1, 1)
    x, off, w, gout, dims = (_cu(a) if isinstance(a, np.ndarray) else a for a in _deform_inputs(s, 0))
    lib = _lib.lib()
    N, Cin, H, W, Cout, kw, kh, sw, sh, pw, ph, dh, dw, G = dims
    nb = lib.tdrn_deform_conv_backward_workspace_bytes(N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, G)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    gi, goff, gw = Guarded(tuple(x.shape)), Guarded(tuple(off.shape)), Guarded(tuple(w.shape))
    st = _lib.current_stream(DEV)
    rc_in = lib.tdrn_deform_conv_backward_input(_lib.ptr(x), _lib.ptr(off), _lib.ptr(gout), gi.ptr(), goff.ptr(), _lib.ptr(w), *dims,
                                                _lib.ptr(ws), nb, st)
    rc_par = lib.tdrn_deform_conv_backward_parameters(_lib.ptr(x), _lib.ptr(off), _lib.ptr(gout), gw.ptr(), *dims, 1.0, _lib.ptr(ws), nb,
                                                      st)
    torch.cuda.synchronize()
    assert (rc_in, rc_par) == (E_UNSUPPORTED, E_UNSUPPORTED)
    for name, gbuf in (("grad_input", gi), ("grad_offset", goff), ("grad_weight", gw)):
        assert bool((gbuf.raw.view(torch.int32) == SENTINEL).all()), name + " was written by a refused call"


# ---------------------------------------------------------------------------------------------
# SSDAugmentation
# ---------------------------------------------------------------------------------------------
RAGGED_FRAMES = [(16, 1080), (1080, 16), (16, 16), (17, 17), (17, 255), (100, 257), (255, 100), (257, 720), (720, 1080), (1080, 720),
                 (1080, 1080)]


def test_augment_apply_ragged_frames():
    from tdrn_amd.utils.augmentations import SSDAugmentation, params_to_dicts
    hw = [f for f in RAGGED_FRAMES for _ in range(3)]         # three draws of every frame
    B = len(hw)
    imgs = [AR.case_image(h, w, 300 + i) for i, (h, w) in enumerate(hw)]
    targets = [AR.case_boxes(h, w, 1 + i % 5, 300 + i) for i, (h, w) in enumerate(hw)]
    dimgs = _dev(imgs)
    sampler = SSDAugmentation(300, MEAN, seed=4242)
    params, packed = sampler.sample(hw, [torch.from_numpy(t) for t in targets], torch.device(DEV), sample_ids=np.arange(B))
    ps = params_to_dicts(params)
    rows = _rows(packed)
    for i, p in enumerate(ps):
        _check_sample_invariants(p, hw[i], targets[i], rows[i], "image %d (%d x %d)" % (i, hw[i][0], hw[i][1]))
        x0, y0, x1, y1 = p["crop"]
        assert x1 - x0 >= 1 and y1 - y0 >= 1, (i, hw[i], p["crop"])
    assert any(p["cropped"] for p in ps) and any((p["canvas_h"], p["canvas_w"]) != s for p, s in zip(ps, hw))
    for S in (17, 300, 513):
        aug = SSDAugmentation(S, MEAN, seed=4242)
        x = aug.apply(dimgs, params, to_rgb=True)
        x_bgr = aug.apply(dimgs, params, to_rgb=False)
        assert x.shape == (B, 3, S, S) and torch.equal(x_bgr, x.flip(1))
        xh = x.cpu().numpy()
        for i, p in enumerate(ps):
            want = AR.apply(imgs[i], p, S, MEAN, to_rgb=True)
            assert np.array_equal(xh[i], want), "S=%d image %d (%d x %d) crop %r canvas %d x %d mirror %d: %d of %d pixels differ, by up to %g" % (
                S, i, hw[i][0], hw[i][1], p["crop"], p["canvas_h"], p["canvas_w"], p["mirror"], int((xh[i] != want).sum()), want.size,
                float(np.abs(xh[i] - want).max()))
