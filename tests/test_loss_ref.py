"""The numpy restatement of the training losses (tests/_loss_ref.py) against the reference's own outputs
(tests/golden/loss_*.npz, made by make_golden_loss.py): conf_t and sel equal, the rest within fp32 rounding.  CPU only."""
import os

import numpy as np
import pytest

import _loss_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VAR = (0.1, 0.2)


def _case(name):
    cfg, B, C, refine, only_loc, counts, seed = R.CASES[name]
    priors = R.priors_of(cfg, GOLDEN)
    loc, conf, arm, targets = R.case_inputs(name, priors.shape[0])
    return priors, loc, conf, arm, targets, np.load(os.path.join(GOLDEN, "loss_%s.npz" % name))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_matches_reference_fixture(name):
    priors, loc, conf, arm, targets, g = _case(name)
    B, P = loc.shape[:2]
    loc_t, conf_t = R.match_batch(0.5, targets, priors, VAR, arm)
    np.testing.assert_array_equal(conf_t, g["conf_t"])
    rtol, atol = R.loc_t_tolerance(arm is not None)
    np.testing.assert_allclose(loc_t, g["loc_t"], rtol=rtol, atol=atol)
    sel, gaps = R.select(conf, conf_t)
    np.testing.assert_array_equal(sel, g["sel"])
    ll, lc, N = R.losses(loc, conf, loc_t, conf_t, sel)
    np.testing.assert_allclose(ll, g["loss_l"], rtol=1e-5)
    gl, gc = R.grads(loc, conf, loc_t, conf_t, sel)
    gl = gl.reshape(B * P, 4)
    np.testing.assert_array_equal(np.nonzero(np.abs(gl).sum(1))[0], g["gloc_rows"])
    np.testing.assert_allclose(gl[g["gloc_rows"]], g["gloc"], atol=1e-7)
    if conf is not None:
        np.testing.assert_allclose(lc, g["loss_c"], rtol=1e-5)
        gc = gc.reshape(B * P, -1)
        np.testing.assert_array_equal(np.nonzero(np.abs(gc).sum(1))[0], g["gconf_rows"])
        np.testing.assert_allclose(gc[g["gconf_rows"]], g["gconf"], atol=1e-7)


def test_fixtures_pin_the_quirks():
    """Each quirk of the header is exercised by the fixtures: lowest-index argmax, forced matches with the last truth
    winning, the tiny truth taking prior 0, positives ranked into the negatives counted once."""
    priors, loc, conf, arm, targets, g = _case("voc320_plain")
    t0 = targets[0]
    ov = R.iou(t0[:, :4], R.point_form(priors))
    bp = ov.argmax(1)
    assert bp[0] == bp[-1]                                   # the duplicated truth shares its best prior ...
    assert g["conf_t"][0][bp[-1]] == int(t0[-1, 4]) + 1      # ... and the last one wins it
    assert g["conf_t"][0][bp[0]] != int(t0[0, 4]) + 1
    tl = targets[-1]
    assert R.iou(tl[-1:, :4], R.point_form(priors)).max() == 0
    assert g["conf_t"][-1][0] == int(tl[-1, 4]) + 1          # overlaps nothing: forced onto prior 0
    # most priors overlap no truth: they take truth 0 and background (loc_t encodes truth 0)
    lt, _ = R.match_one(0.5, t0, priors, VAR)
    far = ov.max(0) == 0
    assert far.sum() > 100
    np.testing.assert_array_equal(lt[far], R.encode(np.repeat(t0[:1, :4], far.sum(), 0), priors[far], VAR))


def test_zero_truth_image_adds_nothing():
    priors, loc, conf, arm, targets, g = _case("voc320_refine")
    loc_t, conf_t = R.match_batch(0.5, targets, priors, VAR, arm)
    with_empty = targets[:2] + [np.zeros((0, 5), np.float32)]
    lt2, ct2 = R.match_batch(0.5, with_empty, priors, VAR, arm[:3])
    assert (ct2[2] == 0).all() and (lt2[2] == 0).all()
    conf3 = np.concatenate([conf[:2], conf[:1]])
    loc3 = np.concatenate([loc[:2], loc[:1]])
    sel3, _ = R.select(conf3, ct2)
    assert (sel3[2] == 0).all()
    sel2, _ = R.select(conf[:2], conf_t[:2])
    a = R.losses(loc3, conf3, lt2, ct2, sel3)
    b = R.losses(loc[:2], conf[:2], loc_t[:2], conf_t[:2], sel2)
    np.testing.assert_allclose(a[:2], b[:2], rtol=1e-12)
