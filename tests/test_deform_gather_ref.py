"""The CPU restatement of the 16-bit gather kernel (tests/_deform_gather_ref.py) proven on the CPU, before anything is held against
it on a GPU (tests/test_gpu_deform_gather16.py, check_stages of tests/test_gpu_pin16.py):

  * with the 16-bit rounding switched off it agrees with the CPU oracle (oracle.deform_conv_forward) on every stand-alone case;
  * its fp32 fused multiply-add is exact (against rational arithmetic, double-rounding ties included);
  * each of five deliberate errors leaves C_ACC * S + extra on far more than a handful of outputs, in both types: the tolerance of
    the GPU tests is not vacuous;
  * `near` (pixels at the discontinuity of the rejection test, which the GPU tests leave out) marks at most 10 % of every case.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc

import _deform_gather_ref as R

C_ACC = {"bf16": 2e-6, "fp16": 4e-5}     # tests/test_gpu_pin16.py: accumulation noise relative to S
HANDFUL = 5


def _case(i, dtype):
    x, w, off = R.case_inputs(R.CASES[i], R.SEEDS[i])
    return R.round16(x, dtype), R.round16(w, dtype), off


def _rn32(fr):
    """a rational number rounded once, nearest-even, to fp32"""
    if fr == 0:
        return np.float32(0)
    c = np.float32(float(fr))
    cands = {float(c): c for c in (c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf)))}
    best = sorted(cands.values(), key=lambda v: (abs(Fraction(float(v)) - fr), int(np.float32(v).view(np.uint32)) & 1))
    return best[0]


def test_fma32_is_one_rounding():
    """_fma32 against exact rational arithmetic: random operands of the kernel's kinds (fp32 weight in [0, 1], 16-bit value, fp32
    addend), and a constructed operand triple on which float64 addition followed by a cast to fp32 rounds the other way:
    w v + a = 1 + 2^-24 + 2^-54, half way between two fp32 values once float64 has dropped the last term."""
    rng = np.random.Generator(np.random.PCG64(5))
    n = 3000
    w = rng.random(n).astype(np.float32).astype(np.float64)
    for dtype in ("bf16", "fp16"):
        v = R.round16(rng.standard_normal(n), dtype)
        a = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 3, n))).astype(np.float32).astype(np.float64)
        got = R._fma32(w, v, a)
        for i in range(n):
            want = _rn32(Fraction(w[i]) * Fraction(v[i]) + Fraction(a[i]))
            assert got[i] == float(want), (dtype, w[i], v[i], a[i])
    w = np.array([2.0 ** -24 * (1 + 2.0 ** -10 + 2.0 ** -20)])
    v = np.array([-(1 - 2.0 ** -10)])                          # (fp16-representable)
    a = np.array([1 + 2.0 ** -23])
    assert float(np.float32(w[0])) == w[0] and R.round16(v, "fp16")[0] == v[0] and float(np.float32(a[0])) == a[0]
    exact = Fraction(w[0]) * Fraction(v[0]) + Fraction(a[0])
    assert exact == 1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 54)
    assert float(np.float32(w[0] * v[0] + a[0])) == 1.0        # float64, then fp32: the tie falls to even
    assert R._fma32(w, v, a)[0] == 1 + 2.0 ** -23 == float(_rn32(exact))


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_unrounded_reference_agrees_with_the_oracle(i):
    """round_blend=False (float64 blend with the fp32 sampling decisions and fp32 bilinear weights, float64 product) against the
    oracle on the 16-bit-representable inputs of both types: |helper - oracle| <= 1e-6 * S on every element, S = sum |blend| |w|.

    The 1e-6 is relative to the operation's scale S, not to each output: the oracle restates the reference in fp32 THROUGHOUT
    (orc_bilinear and the SGEMM loop of orc_deform_conv_forward accumulate in float), so its own error is a few 1e-7 of S whatever
    the output's size, and outputs that cancel to |y| << S carry it at any relative size.  Measured on these cases: at most 4.1e-7 S
    (the 25-tap case, K = 1600), while relative to the single output it is 1.3e-4 already on the zero-offset case, whose blend is
    exact, and up to 3.9e-2.  A swapped corner, a wrong tap or group is 1e-2 S and more (test_every_mutation_leaves_the_tolerance).
    Taps are rejected in both by the same fp32 comparison, so an all-rejected output is exactly 0 in both."""
    N, Cin, H, W, Cout, k, st, pad, dil, G, sigma = R.CASES[i]
    for dtype in ("bf16", "fp16"):
        x16, w16, off = _case(i, dtype)
        ref, S, extra, near = R.gather_ref(x16, off, w16, st, pad, dil, G, dtype, round_blend=False)
        want = orc.deform_conv_forward(x16.astype(np.float32), off, w16.astype(np.float32), st, pad, dil, G).astype(np.float64)
        assert ref.shape == want.shape and float(extra.max()) == 0.0
        d = np.abs(ref - want)
        nz = S > 0
        print("%s %s: max |d| / S %.2e, max |d| / |oracle| %.2e" % (R.CASE_IDS[i], dtype, float((d[nz] / S[nz]).max()),
                                                                  float((d[nz] / np.maximum(np.abs(want[nz]), 1e-300)).max())))
        assert (d <= 1e-6 * S).all(), (dtype, float((d[nz] / S[nz]).max()))
        assert (want[~nz] == 0).all() and (ref[~nz] == 0).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("i", [4, 1], ids=["5x5_cin64", "g8"])
def test_every_mutation_leaves_the_tolerance(i, dtype):
    """swapped corner weights, the next tap's weights, the previous group's channels, a dropped tap, a truncating rounding: each moves
    more than a handful of outputs outside C_ACC * S + extra of the unmutated restatement.  ("prev_group" is the identity with one
    group: it is asserted on the G = 8 case and must change nothing on the other.)"""
    N, Cin, H, W, Cout, k, st, pad, dil, G, sigma = R.CASES[i]
    x16, w16, off = _case(i, dtype)
    ref, S, extra, near = R.gather_ref(x16, off, w16, st, pad, dil, G, dtype)
    tol = C_ACC[dtype] * S + extra
    for m in R.MUTATIONS:
        mut = R.gather_ref(x16, off, w16, st, pad, dil, G, dtype, mutate=m)[0]
        err = np.abs(mut - ref)
        outside = int((err > tol).sum())
        print("%s %s %-10s: %d of %d outputs outside, worst %.1f x tolerance" % (R.CASE_IDS[i], dtype, m, outside, err.size,
                                                                                float((err / np.maximum(tol, 1e-300)).max())))
        if m == "prev_group" and G == 1:
            assert outside == 0 and float(err.max()) == 0.0
        else:
            assert outside > HANDFUL, (m, outside)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_near_marks_at_most_a_tenth(i):
    """the pixels the GPU tests leave out: at most 10 % of each case (sampling is in fp32 in both types: one count per case); with
    zero offsets every coordinate is an exact integer and nothing is near"""
    N, Cin, H, W, Cout, k, st, pad, dil, G, sigma = R.CASES[i]
    x16, w16, off = _case(i, "bf16")
    near = R.gather_ref(x16, off, w16, st, pad, dil, G, "bf16")[3]
    print("%s: near %d of %d output pixels" % (R.CASE_IDS[i], int(near.sum()), near.size))
    assert near.sum() * 10 <= near.size
    if sigma == 0.0:
        assert not near.any()


def test_near_rule_and_second_branch():
    """a coordinate 5e-5 off the border marks its pixel, the exact border does not; a second branch adds its result, S and `near`"""
    x16 = R.round16(np.random.Generator(np.random.PCG64(1)).standard_normal((1, 8, 4, 4)), "fp16")
    w16 = R.round16(np.ones((2, 8, 1, 1)), "fp16")
    off = np.zeros((1, 2, 4, 4), np.float32)
    off[0, 0, 0, 1] = -5e-5            # h_im = -5e-5: rejected, near
    off[0, 1, 2, 3] = 1.0              # w_im = 4.0 = W exactly: rejected, not near
    off[0, 0, 3, 0] = 5e-5             # inside, near the bottom clamp band? no: h_im = 3.00005, neither 0 nor H
    ref, S, extra, near = R.gather_ref(x16, off, w16, 1, 0, 1, 1, "fp16")
    assert near[0, 0, 1] and near.sum() == 1
    assert ref[0, 0, 0, 1] == 0 and ref[0, 0, 2, 3] == 0 and ref[0, 0, 3, 0] == x16[0, :, 3, 0].sum()
    off2 = np.zeros((1, 2, 4, 4), np.float32)
    off2[0, 1, 1, 1] = np.float32(3.0) - np.float32(1e-5)      # w_im = 4 - 1e-5: inside the clamp band, near W
    both = R.gather_ref(x16, off, w16, 1, 0, 1, 1, "fp16", second=dict(off=off2, w16=2 * w16, stride=1, padding=0, dilation=1, G=1))
    alone = R.gather_ref(x16, off2, 2 * w16, 1, 0, 1, 1, "fp16")
    assert np.array_equal(both[0], ref + alone[0]) and np.array_equal(both[1], S + alone[1])
    assert both[3][0, 1, 1] and both[3][0, 0, 1] and both[3].sum() == 2
    assert alone[0][0, 0, 1, 1] == 2 * x16[0, :, 1, 3].sum()   # (the [W-1, W) band: column W-1 with fraction 0)


@pytest.mark.parametrize("G", [1, 4])
def test_two_branches_on_slices_of_one_offset_tensor_agree_with_the_oracle(G):
    """what check (d) of tests/test_gpu_pin16.py feeds the restatement: a 3x3 / pad 1 and a 5x5 / pad 2 branch over one input, their
    offsets channel ranges of ONE tensor ([0, G 18) and [G 18, G 68)), weights of both concatenated from a 12-row and a 9-row block;
    unrounded, against the sum of two oracle calls (bound as in test_unrounded_reference_agrees_with_the_oracle)."""
    rng = np.random.Generator(np.random.PCG64(21))
    Cin, H, W = 32, 7, 6
    x16 = R.round16(rng.standard_normal((2, Cin, H, W)), "bf16")
    off = (1.5 * rng.standard_normal((2, G * 68, H, W))).astype(np.float32)
    specs, want = [], 0.0
    for k, pad, c0 in ((3, 1, 0), (5, 2, G * 18)):
        w16 = R.round16(np.concatenate([rng.standard_normal((12, Cin, k, k)), rng.standard_normal((9, Cin, k, k))], 0) * (Cin * k * k) ** -0.5, "bf16")
        o = np.ascontiguousarray(off[:, c0:c0 + G * 2 * k * k])
        specs.append(dict(off=o, w16=w16, stride=1, padding=pad, dilation=1, G=G))
        want = want + orc.deform_conv_forward(x16.astype(np.float32), o, w16.astype(np.float32), 1, pad, 1, G).astype(np.float64)
    ref, S, extra, near = R.gather_ref(x16, dtype="bf16", second=specs[1], round_blend=False, **specs[0])
    assert ref.shape == (2, 21, H, W) and (np.abs(ref - want) <= 1e-6 * S).all()
    both = R.gather_ref(x16, dtype="bf16", second=specs[1], **specs[0])
    one = [R.gather_ref(x16, dtype="bf16", **s) for s in specs]
    assert np.array_equal(both[0], one[0][0] + one[1][0]) and np.array_equal(both[3], one[0][3] | one[1][3])
