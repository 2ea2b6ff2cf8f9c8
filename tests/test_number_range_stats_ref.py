"""The references, bounds and restatements of tests/_number_range_stats.py, checked without the library (CPU only).

BatchNorm's statistics: an fp32 numpy restatement of welford_chunk / welford_merge (bn_prims.h) in the kernel's chunk length stays
inside the bounds of save_mean and M2 at every (kappa, k, shape) the GPU test draws; a sum / sum-of-squares scheme leaves them at
kappa >= 2^12; a two-pass scheme that rounds the mean once still passes (the bounds belong to the kappa-linear class, not to one
algorithm).  The restatement with the merge as it was before the empty-record rule gives NaN where a mean exceeds 2^64.
L2Norm: torch's fp32 formula stays inside the bounds at every shape and eps; eps under the root, or the x t term dropped, does not.
Depthwise conv: the exact fmaf agrees with integer arithmetic on 10^5 triples; the nine-fmaf restatement equals torch's conv within
acc_bound.  Every drawn case: the ReLU-kink share is at most 1 %, and no reference is non-finite.
"""
import fractions

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _number_range_stats as S
from _number_range import acc_bound, f32_edges

CASES = [(c, d) for c in S.BN_SHAPES for d in S.BN_DRAWS]


def _channels(case, draw):
    x = S.bn_inputs(case, draw)[0]
    N, C, H, W = x.shape
    sp, per = S.bn_splits(N, C, H * W)
    L, K = S.bn_depth(N, H * W, sp, per)
    mean, m2, e_mean, (lo, hi) = S.bn_stat_bounds(x.double(), L, K)
    for c, (ka, k, _) in enumerate(S.bn_channel_plan(case, draw)):
        v = x[:, c].reshape(-1).numpy()
        yield c, ka, k, v, float(mean[c]), float(m2[c]), float(e_mean[c]), float(lo[c]), float(hi[c])


def test_every_kappa_and_scale_is_drawn():
    seen = {(ka, k) for case, draw in CASES for ka, k, _ in S.bn_channel_plan(case, draw)}
    assert seen == set(S.COMBOS)
    assert {w for case, draw in CASES for _, _, w in S.bn_channel_plan(case, draw)} == set(S.BN_WEIGHTS)
    assert S.bn_splits(4, 3, 1600)[0] > 1 and S.bn_splits(3, 4, 1023)[0] == 1


@pytest.mark.parametrize("case,draw", CASES)
def test_the_welford_restatement_stays_inside_the_bounds(case, draw):
    for c, ka, k, v, mean, m2, e_mean, lo, hi in _channels(case, draw):
        gm, g2 = S.welford_channel32(v)
        share_m = abs(gm - mean) / e_mean
        share_2 = abs(g2 - m2) / max(hi - m2, 1e-300)
        print("%s/%d channel %d kappa %g k %d: mean %.3e of its bound, M2 %.3e (relative error %.3e = %.3g kappa u)" % (
            case, draw, c, ka, k, share_m, share_2, abs(g2 - m2) / m2, abs(g2 - m2) / m2 / max(ka, 1.0) / S.U32))
        assert np.isfinite(gm) and np.isfinite(g2)
        assert share_m <= 1.0 and lo <= g2 <= hi, (case, draw, c, ka, k)


@pytest.mark.parametrize("case,draw", CASES)
def test_a_two_pass_scheme_with_a_once_rounded_mean_stays_inside_the_bounds(case, draw):
    for c, ka, k, v, mean, m2, e_mean, lo, hi in _channels(case, draw):
        gm, g2 = S.two_pass_channel32(v)
        assert abs(gm - mean) <= e_mean and lo <= g2 <= hi, (case, draw, c, ka, k)


def test_a_sum_of_squares_scheme_leaves_the_bounds_from_kappa_2_12():
    met = 0
    for case, draw in CASES:
        for c, ka, k, v, mean, m2, e_mean, lo, hi in _channels(case, draw):
            if ka < 2.0 ** 12 or len(v) < 100 or k == -100:
                # (two values per channel: sum x^2 - (sum x)^2 / 2 can come out right by chance; at k = -100 every squared deviation
                # is below 2^-149, M2 is 0 in any fp32 scheme and the bound is its underflow term alone)
                continue
            gm, g2 = S.sums_channel32(v)
            print("%s/%d channel %d kappa %g k %d: sum-of-squares M2 %.3e, reference %.3e, bounds [%.3e, %.3e]" % (
                case, draw, c, ka, k, g2, m2, lo, hi))
            if ka == 2.0 ** 12:
                assert not (lo <= g2 <= hi), (case, draw, c, ka, k)
            else:
                # at kappa = 2^20 the upper end is finite even where the lower end is 0: a sum of squares misses by 2^16 M2 or by sign
                assert not (np.isfinite(g2) and 0.0 < g2 <= hi), (case, draw, c, ka, k)
            met += 1
    assert met >= 6


def test_the_merge_without_the_empty_record_rule_gives_nan_past_2_64():
    """mean 2^67, sigma 2^49 (the issue's probe) and the drawn channel of kappa 2^20 at k = 55 (values near 2^75)"""
    gen = torch.Generator().manual_seed(1)
    v = ((4096.0 * 2 ** 6 + torch.randn(3069, generator=gen, dtype=torch.float64)).float().double() * 2.0 ** 49).float().numpy()
    assert np.isnan(S.welford_channel32(v, fixed=False)[1])
    gm, g2 = S.welford_channel32(v, fixed=True)
    m2 = float(((v.astype(np.float64) - v.astype(np.float64).mean()) ** 2).sum())
    assert np.isfinite(g2) and abs(g2 - m2) <= 0.5 * m2 and abs(gm - v.astype(np.float64).mean()) <= 16 * 2.0 ** -24 * 2.0 ** 68
    hit = [(case, draw, c) for case, draw in CASES for c, (ka, k, _) in enumerate(S.bn_channel_plan(case, draw)) if ka == 2.0 ** 20 and k == 55]
    assert hit
    for case, draw, c in hit:
        assert np.isnan(S.welford_channel32(S.bn_inputs(case, draw)[0][:, c].numpy(), fixed=False)[1])


@pytest.mark.parametrize("eps", S.BN_EPS)
@pytest.mark.parametrize("case,draw", CASES)
def test_every_drawn_batch_norm_case_meets_its_conditions(case, draw, eps):
    for relu in (False, True):
        ref = S.bn_reference(case, draw, eps, relu)
        print("%s/%d eps %g relu=%d: kink share %.4f, depth %r" % (case, draw, eps, relu, ref["kink_share"], ref["plan"]))
        assert ref["kink_share"] <= 0.01
        for name in ("save_mean", "save_invstd", "running_mean", "running_var", "output", "grad_input", "grad_weight", "grad_bias"):
            assert bool(torch.isfinite(ref[name][0]).all()), name
        # under the tiny eps a variance of 2^-120 (7.5e-7 eps) still shows in save_invstd: it is more than an fp32 rounding below
        # eps^-1/2, and the bound keeps the two apart
        if eps == 1e-30:
            for c, (ka, k, _) in enumerate(S.bn_channel_plan(case, draw)):
                if k == -60 and ka <= 120 and case != "m2":
                    top = float(np.float32(eps)) ** -0.5
                    assert float(ref["save_invstd"][2][c]) < top * (1 - 2.0 ** -24), (c, ka)
    S_, per = S.bn_splits(*[S.BN_SHAPES[case][i] for i in (0, 1)], S.BN_SHAPES[case][2] * S.BN_SHAPES[case][3])
    assert (S_ > 1) == (case == "multi_split")


@pytest.mark.parametrize("T", ["bf16", "fp16"])
@pytest.mark.parametrize("case", list(S.NHWC_SHAPES))
def test_every_resident_draw_meets_its_conditions(case, T):
    from _number_range import all16, cast_interval, to_bits, TYPES
    x = S.nhwc_inputs(case, T)[0]
    if case == "wide":
        seen = set(to_bits(x.to(TYPES[T])).reshape(-1).tolist())
        assert seen == set(torch.arange(65536)[torch.isfinite(all16(T)[1])].tolist())
        assert S.nhwc_splits(3, 1024, 100)[0] == 2
    for eps in S.BN_EPS:
        for relu in (False, True):
            ref, (ok, past, wild), _ = S.nhwc_reference(case, T, eps, relu)
            assert ref["kink_share"] <= 0.01
            if T == "fp16":
                assert bool(ok.all())                      # every finite fp16 input is inside the header's range
            for name in ("save_mean", "save_invstd", "running_mean", "running_var", "output", "grad_input", "grad_weight", "grad_bias"):
                r = ref[name][0]
                assert bool(torch.isfinite(r[:, ok] if r.dim() == 4 else r[ok]).all()), name
            for name in ("output", "grad_input"):
                _, lo, hi = ref[name]
                lo16, hi16 = cast_interval(T, lo[:, ok], hi[:, ok])
                print("%s %s eps %g relu=%d %-10s: kink share %.4f; %.1f %% of the intervals hold one value, %.1f %% of those are +-inf" % (
                    case, T, eps, relu, name, ref["kink_share"], 100 * float((lo16 == hi16).double().mean()),
                    100 * float(((lo16 == hi16) & torch.isinf(lo16)).double().sum() / max(1, int((lo16 == hi16).sum())))))
    # the fp32 restatement of the resident kernel's scheme (chunks of 4 rows, 32 row-lanes) inside the bounds, channel by channel
    N, C, H, W = x.shape
    L, K = S.bn_depth_nhwc(N * H * W, *S.nhwc_splits(N, C, H * W))
    mean, m2, e_mean, (lo, hi) = S.bn_stat_bounds(x.double(), L, K)
    ok = S.bn_range_classes(x.double())[0]
    for c in range(0, C, 37 if case == "wide" else 1):
        if not bool(ok[c]):
            continue
        gm, g2 = S.welford_channel32(x[:, c].reshape(-1).numpy(), chunk=4, lanes=32, wave=8)
        assert abs(gm - float(mean[c])) <= float(e_mean[c]) and float(lo[c]) <= g2 <= float(hi[c]), (c, gm, g2)


# ---- L2Norm ---------------------------------------------------------------------------------------------------------------------------
def _l2_inside(got, ref):
    bad = {}
    for name, (r, e) in ref.items():
        g = got[name].detach().double()
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(g).all()), name
        d = (g - r).abs()
        share = torch.where(d == 0, torch.zeros_like(d), d / e)
        bad[name] = float(share.max())
    return bad


@pytest.mark.parametrize("eps", S.L2_EPS)
@pytest.mark.parametrize("case", list(S.L2_SHAPES))
def test_the_fp32_l2norm_formula_stays_inside_the_bounds_and_the_doctored_ones_do_not(case, eps):
    x, w, go = S.l2_inputs(case)
    ref = S.l2_case_reference(case, eps)
    shares = _l2_inside(S.l2_formula32(x, w, go, eps), ref)
    print("%s eps %g: worst shares %r" % (case, eps, shares))
    assert max(shares.values()) <= 1.0, shares
    inside = _l2_inside(S.l2_formula32(x, w, go, eps, "eps_inside"), ref)
    print("%s eps %g eps inside the root: %r" % (case, eps, inside))
    assert inside["norm"] > 1.0 and inside["output"] > 1.0
    dropped = _l2_inside(S.l2_formula32(x, w, go, eps, "no_xt"), ref)
    print("%s eps %g x t dropped: %r" % (case, eps, dropped))
    assert dropped["grad_input"] > 1.0 and dropped["output"] <= 1.0


def test_the_l2norm_draw_crosses_eps_and_the_cancellation():
    for eps in S.L2_EPS:
        e = float(np.float32(eps))
        r = S.l2_case_reference("tiny_odd", eps)["norm"][0] - e
        assert bool(((r > 0.1 * e) & (r < 10 * e)).any()) and bool((r > 1e3 * e).any())
        if eps == 1e-10:
            assert bool((r < 1e-3 * e).any())
            # a pixel that is not zero whose fp32 norm is eps itself (r = norm - eps exactly 0), and one where r is a few ulps of eps
            assert bool(((r > 0) & (r < 2.0 ** -25 * e)).any()) and bool(((r > 2.0 ** -24 * e) & (r < 2.0 ** -10 * e)).any())


# ---- depthwise conv ----------------------------------------------------------------------------------------------------------------------
def test_the_exact_fmaf_agrees_with_integer_arithmetic_on_1e5_triples():
    rng = np.random.RandomState(5)
    n = 100000
    # exponents over the whole range so that results are subnormal, tie-prone (small integers) and overflowing too
    def draw(kind):
        if kind == 0:
            return (rng.randint(-(1 << 24), 1 << 24, n).astype(np.float64) * 2.0 ** rng.randint(-100, 80, n)).astype(np.float32)
        if kind == 1:
            return (rng.randint(-9, 10, n) * 2.0 ** rng.randint(-75, -60, n)).astype(np.float32)
        return rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    a = np.concatenate([draw(0)[:40000], draw(1)[:30000], draw(2)[:30000]])
    b = np.concatenate([draw(0)[:40000], draw(1)[:30000], draw(2)[:30000]])
    c = np.concatenate([draw(0)[:40000], (rng.randint(-(1 << 24), 1 << 24, 30000) * 2.0 ** -149).astype(np.float32), draw(2)[:30000]])
    keep = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    a, b, c = a[keep], b[keep], c[keep]
    got = S.fmaf32(a, b, c)
    Fr = fractions.Fraction
    want = np.array([S.f32_from_fraction(Fr(float(p)) * Fr(float(q)) + Fr(float(r))) for p, q, r in zip(a, b, c)], np.float64)
    sub = int(((np.abs(want) < 2.0 ** -126) & (want != 0)).sum())
    print("%d triples, %d subnormal results, %d infinite" % (len(a), sub, int(np.isinf(want).sum())))
    assert sub > 1000 and len(a) > 80000
    assert np.array_equal(got.astype(np.float64), want)
    # (the sign of an exact zero follows the float64 sum, which is IEEE's rule for the fused operation too)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [-100, 0, 100])
def test_the_nine_fmaf_restatement_is_torchs_depthwise_conv_within_acc_bound(k, stride):
    N, C, H, W = 2, 3, 9, 7
    x, w, b = S.dw_values((N, C, H, W), 0, 1), S.dw_values((C, 1, 3, 3), k, 2), S.dw_values((C,), k, 3)
    got = S.dw_forward_exact(x, w, b, stride)
    xt, wt, bt = (torch.from_numpy(t) for t in (x, w, b))
    ref = F.conv2d(xt.double(), wt.double(), bt.double(), stride, 1, 1, C)
    Sabs = F.conv2d(xt.double().abs(), wt.double().abs(), bt.double().abs(), stride, 1, 1, C)
    assert bool(((torch.from_numpy(got).double() - ref).abs() <= acc_bound("fp32", Sabs, 10)).all())
    t32 = F.conv2d(xt, wt, bt, stride, 1, 1, C)
    assert bool(((t32.double() - ref).abs() <= acc_bound("fp32", Sabs, 10)).all())
    go = S.dw_values(got.shape, 0, 4)
    gi = S.dw_backward_input_exact(go, w, H, W, stride)
    xr = xt.double().requires_grad_(True)
    F.conv2d(xr, wt.double(), None, stride, 1, 1, C).backward(torch.from_numpy(go).double())
    xa = xt.double().requires_grad_(True)
    F.conv2d(xa, wt.double().abs(), None, stride, 1, 1, C).backward(torch.from_numpy(go).double().abs())
    assert bool(((torch.from_numpy(gi).double() - xr.grad).abs() <= acc_bound("fp32", xa.grad, 9)).all())


def test_the_sgd_triples_bring_every_edge_value_to_every_tensor():
    e = set(f32_edges().view(torch.int32).tolist())
    for which in range(3):
        seen = set()
        for n in S.SGD_SIZES:
            for step in range(3):
                seen |= set(S.sgd_triples(n, step)[which].view(np.int32).tolist())
        assert seen <= e and len(seen) >= 30, (which, len(seen))
