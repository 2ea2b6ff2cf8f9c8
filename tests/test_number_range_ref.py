"""tests/_number_range.py against torch on the CPU: the value sets hold what they say, rne_bits is torch's cast bit for bit,
cast_interval contains it, and torch's own fp32 conv sits inside acc_bound at the shapes and scales of the GPU sweep -- the reference
side is inside each bound before the GPU is asked to be."""
import math

import pytest
import torch

import _number_range as nr

TS = ("bf16", "fp16")


def _probe_values(T):
    return torch.cat([nr.ties(T).reshape(-1), nr.all16(T)[1]])


@pytest.mark.parametrize("T", TS)
def test_all16_decodes_like_torch(T):
    t16, f32 = nr.all16(T)
    assert t16.numel() == 65536 and torch.equal(nr.to_bits(t16), torch.arange(65536))
    ref = t16.float()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(f32), nan) and int(nan.sum()) == 2 * ((1 << nr.MANT_BITS[T]) - 1)
    assert torch.equal(nr.f32_bits(f32[~nan]), nr.f32_bits(ref[~nan]))                  # the sign of zero included


@pytest.mark.parametrize("T", TS)
def test_ties_are_midpoints_and_torch_rounds_them_to_even(T):
    t = nr.ties(T)
    n = {"fp16": 31744, "bf16": 32640}[T]
    assert tuple(t.shape) == (2, n, 3) and torch.equal(t[1], -t[0])
    h = nr.finite_patterns(T)
    lo = nr.decode64(T, h)
    mid, up, down = (t[0, :, i].double() for i in range(3))
    step = 2.0 * (mid - lo)                                                             # the spacing above h
    assert torch.equal(lo[1:], (lo + step)[:-1])                                        # mid is the midpoint to the successor
    assert bool((down < mid).all()) and bool((mid < up).all())
    if T == "fp16":
        assert float(mid[-1]) == 65520.0 and float(lo[-1]) == 65504.0
    even = torch.where(h % 2 == 0, h, h + 1)                                            # (the last h is odd: its even neighbour is inf)
    for sign, sbit in ((0, 0), (1, 32768)):
        cast = nr.to_bits(t[sign].to(nr.TYPES[T]))
        assert torch.equal(cast[:, 0], even + sbit)
        assert torch.equal(cast[:, 1], h + 1 + sbit) and torch.equal(cast[:, 2], h + sbit)
    assert int(even[-1]) == nr.inf_bits(T)


@pytest.mark.parametrize("T", TS)
def test_rne_bits_is_torchs_cast_bit_for_bit(T):
    v = torch.cat([_probe_values(T), nr.f32_edges(), torch.tensor([float("inf"), float("-inf"), float("nan"), -float("nan")])])
    got, ref16 = nr.rne_bits(T, v), v.to(nr.TYPES[T])
    ref = nr.to_bits(ref16)
    nan = torch.isnan(v)
    assert torch.equal(torch.isnan(nr.decode64(T, got)), nan) and torch.equal(torch.isnan(ref16), nan)
    assert torch.equal(got[~nan], ref[~nan])
    assert torch.equal(nr.f32_bits(nr.rne(T, v)[~nan]), nr.f32_bits(ref16.float()[~nan]))
    gen = torch.Generator().manual_seed(3)                                              # and on random fp32 bit patterns
    r = torch.randint(-2 ** 31, 2 ** 31, (200000,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32)
    keep = ~torch.isnan(r)
    assert torch.equal(nr.rne_bits(T, r)[keep], nr.to_bits(r.to(nr.TYPES[T]))[keep])


@pytest.mark.parametrize("T", TS)
def test_edges_hold_what_they_say(T):
    e = nr.edges(T)
    e_bits, m_bits = nr.EXP_BITS[T], nr.MANT_BITS[T]
    binades = (1 << e_bits) - 1
    assert e.numel() == binades * 5 * 4 * 2 and bool(torch.isfinite(e).all())
    have = set(nr.f32_bits(e).tolist())
    pool = set(nr.f32_bits(_probe_values(T)).tolist())
    assert have <= pool                                                                 # a subset of ties(T) u all16(T)
    mmax = (1 << m_bits) - 1
    for ex in range(binades):                                                           # every binade, the subnormal one included
        for ma in (0, 1, 2, mmax - 1, mmax):
            v = nr.decode64(T, torch.tensor([(ex << m_bits) | ma])).float()
            assert int(nr.f32_bits(v)) in have and int(nr.f32_bits(-v)) in have
    tiny_sub = 2.0 ** (2 - (1 << (e_bits - 1)) - m_bits)
    top = nr.decode64(T, torch.tensor([nr.inf_bits(T) - 1]))
    first_inf = (top + 2.0 ** ((1 << (e_bits - 1)) - 1 - m_bits) / 2).float()           # the largest finite value plus half a spacing
    for v in (torch.tensor([0.0]), torch.tensor([-0.0]), torch.tensor([tiny_sub]), torch.tensor([tiny_sub / 2]), top.float(), first_inf):
        assert int(nr.f32_bits(v.float())) in have, float(v)
    assert math.isinf(float(first_inf.to(nr.TYPES[T])))
    assert torch.isfinite(torch.nextafter(first_inf, torch.tensor([0.0])).to(nr.TYPES[T])).all()
    if T == "fp16":
        assert float(first_inf) == 65520.0 and tiny_sub == 2.0 ** -24


@pytest.mark.parametrize("T", TS)
def test_cast_interval_contains_torchs_cast(T):
    gen = torch.Generator().manual_seed(7)
    n = 100000
    # magnitudes over the whole range of T and beyond both ends, widths from 2^-60 of the value to the value itself
    top = {"fp16": 18.0, "bf16": 130.0}[T]
    expo = torch.rand(n, generator=gen, dtype=torch.float64) * (top + 160.0) - 160.0
    x = torch.randn(n, generator=gen, dtype=torch.float64) * torch.exp2(expo)
    width = x.abs() * torch.exp2(-60.0 * torch.rand(n, generator=gen, dtype=torch.float64))
    lo, hi = nr.cast_interval(T, x - width, x + width)
    assert bool((lo <= hi).all())
    for v in (x, x - width, x + width, x + width * (2 * torch.rand(n, generator=gen, dtype=torch.float64) - 1)):
        got = v.to(nr.TYPES[T]).double()                                                # torch goes through fp32
        assert bool(nr.inside(got, lo, hi).all())
        assert bool(nr.inside(v.float().to(nr.TYPES[T]).double(), lo, hi).all())
    assert bool((hi == float("inf")).any()) and bool((hi.abs() < 2.0 ** -14).any())    # both ends of the range were reached
    # a zero-width interval of a value T holds is that value; one past the overflow boundary is inf
    t16 = nr.all16(T)[1].double()
    fin = torch.isfinite(t16)
    lo, hi = nr.cast_interval(T, t16[fin], t16[fin])
    assert torch.equal(lo, t16[fin]) and torch.equal(hi, t16[fin])
    big = torch.tensor([1e39, 65520.0 if T == "fp16" else 3.4e38], dtype=torch.float64)
    lo, hi = nr.cast_interval(T, big, big)
    assert bool((lo == float("inf")).all()) and bool((hi == float("inf")).all())


def test_same_class():
    inf, nan = float("inf"), float("nan")
    a = torch.tensor([1.0, inf, -inf, nan, 0.0])
    assert nr.same_class(a, a.clone()).tolist() == [True, False, False, False, True]
    for bad in ([1.0, inf, -inf, 3.0, 0.0], [1.0, -inf, -inf, nan, 0.0], [inf, inf, -inf, nan, 0.0], [1.0, 65504.0, -inf, nan, 0.0]):
        with pytest.raises(AssertionError):
            nr.same_class(torch.tensor(bad), a)


def test_acc_bound_has_no_floor():
    S = torch.tensor([0.0, 2.0 ** -140, 1.0], dtype=torch.float64)
    for mode in ("fp32", "bf16", "fp16"):
        b = nr.acc_bound(mode, S, 55)
        assert float(b[0]) == 58 * 2.0 ** -149 and bool((b[1:] > b[:-1]).all())
    assert float(nr.acc_bound("fp32", S, 55)[2]) == 1.001 * 58 * 2.0 ** -24 + 58 * 2.0 ** -149


@pytest.mark.parametrize("family,case", nr.SWEEP_CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_torchs_fp32_conv_is_inside_acc_bound(family, case, mode):
    """the op in fp32 on the CPU (any summation order torch picks) against the float64 reference, elementwise, at every scale"""
    for scale, exps in nr.SCALES[mode].items():
        ref, S, bound = nr.sweep_reference(family, case, mode, scale)
        x, w, b, go = nr.scaled_inputs(family, case, exps)
        got = nr.autograd4(family, nr.rounded(x, mode), nr.rounded(w, mode), b, nr.rounded(go, mode))
        for name, g, r, bd in zip(nr.NAMES, got, ref, bound):
            nr.worst_share("%s %s %s %s %s" % (family, case, mode, scale, name), g, r, bd)


@pytest.mark.parametrize("k,pad", [(1, 0), (3, 1)])
def test_ref64_is_torchs_float64_autograd(k, pad):
    """the per-tap restatement the resident sweep uses (on the device for its two large cases) against torch's conv2d and autograd"""
    g = torch.Generator().manual_seed(k)
    x, w = torch.randn(2, 6, 9, 7, generator=g, dtype=torch.float64), torch.randn(4, 6, k, k, generator=g, dtype=torch.float64)
    b, go = torch.randn(4, generator=g, dtype=torch.float64), torch.randn(2, 4, 9, 7, generator=g, dtype=torch.float64)
    xx, ww, bb = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = torch.nn.functional.conv2d(xx, ww, bb, 1, pad)
    want = (y.detach(),) + torch.autograd.grad(y, (xx, ww, bb), go)
    S = nr.ref64(x.abs(), w.abs(), b.abs(), go.abs(), pad)
    for got, ref, s in zip(nr.ref64(x, w, b, go, pad), want, S):
        assert got.shape == ref.shape and bool(((got - ref).abs() <= 64 * 2.0 ** -53 * s).all())


def test_sweep_input_populations():
    """what section 3 asserts of the fp16 draws, here on the CPU too"""
    for family, case in nr.SWEEP_CASES:
        x, w, b, go = nr.unit_inputs(family, case)
        for t in (x, go):
            small = nr.rne("fp16", t * 2.0 ** -20)
            assert bool((small.abs() < 2.0 ** -14).all()) and float((small != 0).double().mean()) >= 0.9
            assert bool(torch.isfinite(nr.rne("fp16", t * 2.0 ** 13)).all())
            mid = nr.rne("fp16", t * 2.0 ** -12).abs()
            assert bool((mid < 2.0 ** -14).any()) and bool((mid >= 2.0 ** -14).any())   # straddles the smallest normal
