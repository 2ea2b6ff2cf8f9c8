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


# ------------------------------------------------------------------------------------------------------------------
# The training fuzz's cases (tests/test_gpu_train_fuzz.py) are what they claim: checked here, on the CPU, for every seed the
# GPU test uses, so that a green GPU run means the tie rule, the -inf rule and the cap really ran.
# ------------------------------------------------------------------------------------------------------------------
TIE_MODES = ("zeros", "random", "zero_score", "neg_inf")
_SUMMARY = {}


def _boundaries(s, conf_t, negpos):
    """per image: (k, score in front of the num_neg boundary, score behind it), or None where there is no boundary"""
    out = []
    for b in range(s.shape[0]):
        k = min(negpos * int((conf_t[b] > 0).sum()), s.shape[1] - 1)
        if k == 0:
            out.append(None)
            continue
        order = np.argsort(-s[b], kind="stable")
        out.append((k, s[b][order[k - 1]], s[b][order[k]]))
    return out


def _summary(seed):
    """every per-case claim asserted, and the few figures the coverage test needs"""
    if seed in _SUMMARY:
        return _SUMMARY[seed]
    k = R.fuzz_case(seed, GOLDEN)
    what = R.describe(k)
    B, P, C, negpos, mode = k["B"], k["P"], k["C"], k["negpos"], k["mode"]
    conf_t = k["conf_t"]
    out = dict(B=B, P=P, C=C, negpos=negpos, mode=mode, refine=k["refine"], only_loc=k["only_loc"], tiled=k["tiled"], counts=k["counts"],
               straddle=False, cap=False, unclear=0, fragile=0.0, last_prior=False, shared5=False)
    assert k["priors"].shape == (P, 4) and len(k["targets"]) == B and k["loc"].shape == (B, P, 4), what
    assert B * P * C <= R.FUZZ_MAX_ELEMS and (C < 1024 or B * P <= 20000), what
    assert max(k["counts"]) <= 512 and k["counts"][0] > 0, what
    if k["conf"] is not None:
        s = R.mining_scores(k["conf"], conf_t)
        with np.errstate(invalid="ignore"):          # the gap inside the -inf group is inf - inf
            sel, gaps = R.select(k["conf"], conf_t, negpos)
        bnd = _boundaries(s, conf_t, negpos)
        pos_n = (conf_t > 0).sum(1)
        out["cap"] = bool((negpos * pos_n > P - 1).any())
        sel32 = R.select_from_scores(R.mining_scores_f32(k["conf"], conf_t), conf_t, negpos)
        if mode == "gaussian":
            clear = gaps > 1e-5
            out["unclear"] = int((~clear).sum())
            assert clear.sum() >= B - 4, what
            np.testing.assert_array_equal(sel32[clear], sel[clear], what)
        else:
            np.testing.assert_array_equal(sel32, sel, what)      # the device's fp32 score orders the rows as the fp64 one does
            neg_scores = s[conf_t == 0]
            levels = np.unique(np.concatenate([[0.0], neg_scores[np.isfinite(neg_scores)]]))
            assert len(levels) == 1 or np.diff(levels).min() >= R.PATTERN_GAP, (what, np.diff(levels).min())
            with np.errstate(invalid="ignore"):
                tied = [bd is not None and bd[1] == bd[2] for bd in bnd]       # (-inf == -inf: the scores themselves, not the gap)
            out["straddle"] = any(tied)
            for b, bd in enumerate(bnd):
                if bd is not None and np.isfinite(bd[1]) and np.isfinite(bd[2]):
                    assert (gaps[b] == 0) == tied[b], what
        if mode in TIE_MODES:
            assert out["straddle"], what + ": no image's tie group straddles its num_neg boundary"
        if mode == "zero_score":
            assert k["conf"].max() <= 0, what
            assert ((s == 0) & (conf_t == 0)).any(), what
            assert any(bd is not None and bd[1] == 0 and bd[2] == 0 for bd in bnd), what + ": boundary outside the score-0 group"
            assert (sel[(s == 0) & (conf_t == 0)] == 2).any() and (sel[(s == 0) & (conf_t == 0)] == 0).any(), what
        if mode == "neg_inf":
            assert np.isneginf(s).any() and (k["conf"] == 1000).sum() == 1 and np.sort(k["conf"].ravel())[-2] <= 2, what
            assert any(bd is not None and np.isneginf(bd[1]) and np.isneginf(bd[2]) for bd in bnd), what + ": boundary outside the -inf group"
            assert np.isneginf(R.mining_scores_f32(k["conf"], conf_t)).sum() == np.isneginf(s).sum(), what
        if mode == "cap":
            assert out["cap"], what + ": num_neg never reaches P - 1"
    boxes_of = lambda b: R.point_form(k["priors"]) if k["arm"] is None else R.decode(k["arm"][b], k["priors"], VAR)
    if k["tiled"] is not None:
        for b, t in enumerate(k["targets"]):
            if len(t):
                ov = R.iou(t[:, :4], boxes_of(b))
                assert ((ov == ov.max(1, keepdims=True)).sum(1) >= 2).all(), what + ": a truth without a tied best prior"
    if k["refine"] and not k["exact_arm"]:
        frag = sum(int(R.fragile_priors(0.5, t, k["priors"], VAR, k["arm"][b]).sum()) for b, t in enumerate(k["targets"]))
        out["fragile"] = frag / float(B * P)
        assert frag <= 0.0005 * B * P, (what, frag)
    for b, t in enumerate(k["targets"]):
        n = len(t)
        if n >= 3 and not k["refine"] and k["tiled"] is None and P > 2:
            assert R.iou(t[n - 2:n - 1, :4], R.point_form(k["priors"])).argmax(1)[0] == P - 1, what
            out["last_prior"] = True
        if n >= 2:
            assert R.iou(t[n - 1:, :4], boxes_of(b)).max() == 0, what      # the tiny truth overlaps nothing
        if n >= 12:
            assert (t[[1, 3, 5, 7, 9], :4] == t[1, :4]).all(), what
            out["shared5"] = out["shared5"] or (C > 2 and len(set(t[[1, 3, 5, 7, 9], 4])) > 1)
    _SUMMARY[seed] = out
    return out


@pytest.mark.parametrize("seed", R.FUZZ_SEEDS)
def test_fuzz_case_is_well_posed(seed):
    _summary(seed)


def test_fuzz_cases_cover_what_the_kernels_branch_on():
    S = [_summary(seed) for seed in R.FUZZ_SEEDS]
    assert {s["B"] for s in S} == set(R.FUZZ_B)
    assert {s["P"] for s in S} == set(R.FUZZ_P)
    assert {s["C"] for s in S} == set(R.FUZZ_C)
    assert {s["negpos"] for s in S} == set(R.FUZZ_NEGPOS)
    for mode in R.CONF_MODES:
        assert sum(s["mode"] == mode for s in S) >= 3, mode
    assert any(s["only_loc"] for s in S) and any(s["refine"] and s["tiled"] for s in S) and any(s["refine"] and not s["tiled"] for s in S)
    assert any(not s["refine"] and s["tiled"] for s in S)
    assert {s["tiled"][1] for s in S if s["tiled"]} >= {65, 300}            # copies in other waves and in other chunks
    assert any(set(R.TRUTH_COUNTS) <= set(s["counts"]) for s in S)          # all eight counts in one batch
    assert any(s["last_prior"] for s in S) and any(s["shared5"] for s in S)
    assert max(s["fragile"] for s in S) <= 0.0005
    print("largest share of fragile priors: %.5f %%; unclear Gaussian images: %d" % (
        100 * max(s["fragile"] for s in S), sum(s["unclear"] for s in S)))


def test_threshold_case_sits_exactly_on_the_threshold():
    pri, target, a, b = R.threshold_case()
    assert a // 256 != b // 256
    for arm in (None, np.zeros_like(pri)):
        boxes = R.point_form(pri) if arm is None else R.decode(arm, pri, VAR)
        ov = R.iou(target[:, :4], boxes)[0]
        assert ov[a] == np.float32(0.5) and ov[b] == np.float32(1) and (np.delete(ov, [a, b]) == 0).all()
        _, ct = R.match_one(0.5, target, pri, VAR, arm)
        assert ct[a] == 7 and ct[b] == 7 and (ct > 0).sum() == 2
        _, ct = R.match_one(np.nextafter(np.float32(0.5), np.float32(1)), target, pri, VAR, arm)
        assert ct[a] == 0 and ct[b] == 7 and (ct > 0).sum() == 1


def test_tiled_priors_tie_every_truth():
    rng = np.random.Generator(np.random.PCG64(5))
    for stride, copies, P in ((300, 3, 1025), (65, 3, 257), (129, 4, 520)):
        pri = R.tiled_priors(R.fuzz_priors(rng, stride), copies, stride, P)
        assert pri.shape == (P, 4) and (pri[:stride] == pri[stride:2 * stride]).all() and (pri[copies * stride:] == R.FAR).all()
        t = R.synth_targets(rng, 1, 1, 1, 21, [40])[0]
        for arm in (None, R.tiled_arm(rng, 1, copies, stride, P)[0]):
            boxes = R.point_form(pri) if arm is None else R.decode(arm, pri, VAR)
            ov = R.iou(t[:, :4], boxes)
            assert ((ov == ov.max(1, keepdims=True)).sum(1) >= copies).all()
            assert (ov.argmax(1) < stride).all()                           # the lowest copy is the restatement's best prior
