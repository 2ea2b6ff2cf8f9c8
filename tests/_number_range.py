"""Value sets and comparators for the tests that pin the training kernels' rounding over the whole number range
(test_number_range_ref.py, test_gpu_number_range.py, test_gpu_number_range_resident.py).  CPU only: nothing here touches the library.

T is "bf16" or "fp16".  A 16-bit value travels as its bit pattern (an int64 in 0 .. 65535) or as the exact fp32 it stands for.
Every bound a test of this family uses is one of three kinds: acc_bound (the fp32 accumulation before the one output rounding),
cast_interval (what that one rounding may give) or bit equality.  None has an absolute floor.
"""
import functools

import torch
import torch.nn.functional as F

from _conv_train_harness import C_ACC           # (the project's accumulation constants; importing them opens no device)

TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
EXP_BITS = {"bf16": 8, "fp16": 5}
MANT_BITS = {"bf16": 7, "fp16": 10}
F32_MIN_SUB = 2.0 ** -149


def _fmt(T):
    e, m = EXP_BITS[T], MANT_BITS[T]
    return e, m, (1 << (e - 1)) - 1


def inf_bits(T):
    e, m, _ = _fmt(T)
    return ((1 << e) - 1) << m


def decode64(T, bits):
    """bit patterns -> float64 values, from the fields alone (no torch cast)"""
    e, m, bias = _fmt(T)
    bits = bits.to(torch.int64)
    sign = 1.0 - 2.0 * ((bits >> (e + m)) & 1).double()
    ex, ma = (bits >> m) & ((1 << e) - 1), (bits & ((1 << m) - 1)).double()
    normal = torch.ldexp(1.0 + ma / (1 << m), (ex - bias).to(torch.int32))
    sub = torch.ldexp(ma / (1 << m), torch.full_like(ex, 1 - bias).to(torch.int32))
    v = torch.where(ex == 0, sub, normal)
    top = ex == (1 << e) - 1
    v = torch.where(top & (ma == 0), torch.full_like(v, float("inf")), v)
    v = torch.where(top & (ma != 0), torch.full_like(v, float("nan")), v)
    return sign * v


def from_bits(T, bits):
    """bit patterns -> the 16-bit tensor"""
    b = bits.to(torch.int64)
    return torch.where(b >= 32768, b - 65536, b).to(torch.int16).view(TYPES[T])


def to_bits(t16):
    """a 16-bit tensor -> bit patterns 0 .. 65535, in the tensor's logical order"""
    return t16.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def f32_bits(t):
    return t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def all16(T):
    """all 65536 bit patterns -> (the 16-bit tensor, the exact fp32 values)"""
    bits = torch.arange(65536, dtype=torch.int64)
    return from_bits(T, bits), decode64(T, bits).float()


def finite_patterns(T):
    """the finite non-negative bit patterns"""
    return torch.arange(inf_bits(T), dtype=torch.int64)


def _tie_triples(T, h):
    """patterns h (finite, non-negative) -> fp32 (len(h), 3): the midpoint to the successor, nextafter up, nextafter down.  The
    successor of the largest finite pattern is it plus the last spacing."""
    e, m, bias = _fmt(T)
    lo = decode64(T, h)
    last = h == inf_bits(T) - 1
    hi = torch.where(last, torch.full_like(lo, 2.0 ** (bias + 1)), decode64(T, torch.where(last, h, h + 1)))
    mid64 = (lo + hi) / 2
    mid = mid64.float()
    assert torch.equal(mid.double(), mid64), "a midpoint that fp32 does not hold"
    up = torch.nextafter(mid, torch.full_like(mid, float("inf")))
    down = torch.nextafter(mid, torch.full_like(mid, float("-inf")))
    return torch.stack([mid, up, down], 1)


def ties(T):
    """for every finite non-negative pattern: the midpoint to its successor and the two fp32 neighbours of the midpoint, in both
    signs -> fp32 (2, n, 3): [sign][pattern][mid, up, down] (up / down by magnitude)"""
    t = _tie_triples(T, finite_patterns(T))
    return torch.stack([t, -t], 0)


EDGE_MANTISSAS = (0, 1, 2, -2, -1)               # of every binade; negative: counted from the largest mantissa


def edge_patterns(T):
    """the finite non-negative patterns with mantissa 0, 1, 2, max - 1 or max, the subnormal binade included"""
    e, m, _ = _fmt(T)
    ex = torch.arange((1 << e) - 1, dtype=torch.int64)[:, None]
    ma = torch.tensor([k % (1 << m) for k in EDGE_MANTISSAS], dtype=torch.int64)[None, :]
    return ((ex << m) | ma).reshape(-1)


def edges(T):
    """fp32, every value finite: the edge patterns and their tie triples in both signs.  Among them +-0, the smallest subnormal and
    half of it (the midpoint above zero), the largest finite value and the first fp32 value that rounds to inf (the midpoint above
    the largest finite value: its even neighbour is inf)."""
    h = edge_patterns(T)
    pos = torch.cat([decode64(T, h).float(), _tie_triples(T, h).reshape(-1)])
    return torch.cat([pos, -pos])


def f32_edges():
    """fp32 values for the fp32 compute mode: +-0, subnormals (smallest, a few patterns, largest), the smallest normals, values of
    ordinary size and the largest finite ones, in both signs"""
    pats = [0, 1, 2, 3, 0x155555, 0x2AAAAA, 0x400000, 0x7FFFFE, 0x7FFFFF, 0x800000, 0x800001, 0xFFFFFF, 0x1000000,
            0x3F800000, 0x3F800001, 0x3FFFFFFF, 0x7F000000, 0x7F7FFFFE, 0x7F7FFFFF]
    p = torch.tensor(pats, dtype=torch.int64)
    p = torch.cat([p, p | 0x80000000])
    return torch.where(p >= 2 ** 31, p - 2 ** 32, p).to(torch.int32).view(torch.float32)


def rne_bits(T, f32):
    """round to nearest even, fp32 -> T, in integers on the fp32 bit patterns: subnormals of T are kept, a value past the largest
    finite one becomes +-inf, NaN stays NaN (one quiet pattern; compare NaN by NaN-ness).  Independent of torch's cast."""
    assert f32.dtype == torch.float32
    e, m, bias = _fmt(T)
    bits = f32_bits(f32)
    sign, a = bits >> 31, bits & 0x7FFFFFFF
    drop = 23 - m                                                  # fp32 mantissa bits that T does not have
    ex, ma = a >> 23, a & 0x7FFFFF
    sig = torch.where(ex > 0, ma | (1 << 23), ma)                  # the value is sig * 2^(E - 150), E = max(ex, 1)
    he = torch.clamp(ex, min=1) - 127 + bias                       # T's exponent field, were the value normal in T
    # normal in T: exponent and kept mantissa as one integer, so a carry out of the mantissa moves into the exponent
    t = (he << 23) + (sig - (1 << 23))
    normal = (t + ((1 << (drop - 1)) - 1) + ((t >> drop) & 1)) >> drop
    # subnormal in T (or an fp32 subnormal): shift the whole significand down to T's subnormal spacing 2^(1 - bias - m)
    shift = torch.clamp(drop + 1 - he, min=1, max=40)
    one = torch.ones_like(shift)
    q, rem, half = sig >> shift, sig & ((one << shift) - 1), one << (shift - 1)
    sub = q + ((rem > half) | ((rem == half) & ((q & 1) == 1))).to(torch.int64)
    r = torch.where((he >= 1) & (ex > 0), normal, sub)
    r = torch.clamp(r, max=inf_bits(T))                            # overflow -> inf
    r = torch.where(a > 0x7F800000, torch.full_like(r, inf_bits(T) | (1 << (m - 1))), r)
    return (sign << (e + m)) | r


def rne(T, f32):
    """rne_bits as values: fp32 -> the fp32 that T holds after the one rounding"""
    return decode64(T, rne_bits(T, f32)).float()


def rounded(t, mode):
    """a tensor as an op of compute mode `mode` uses it ("fp32": unchanged), through rne_bits"""
    return t if mode == "fp32" else rne(mode, t)


def f32_outward(lo64, hi64):
    """float64 ends -> fp32 ends, lo rounded down and hi rounded up"""
    lo, hi = lo64.float(), hi64.float()
    lo = torch.where(lo.double() > lo64, torch.nextafter(lo, torch.full_like(lo, float("-inf"))), lo)
    hi = torch.where(hi.double() < hi64, torch.nextafter(hi, torch.full_like(hi, float("inf"))), hi)
    return lo, hi


def cast_interval(T, lo64, hi64):
    """the closed interval of T values (as float64, +-inf included) that a value in [lo, hi] can round to, whichever fp32 it passes
    through: the ends go to fp32 outward and then through rne_bits (never float64 -> T directly, which rounds twice)"""
    lo, hi = f32_outward(lo64, hi64)
    return decode64(T, rne_bits(T, lo)), decode64(T, rne_bits(T, hi))


def inside(got64, lo, hi):
    """elementwise lo <= got <= hi (an infinite end admits the same infinity)"""
    return (got64 >= lo) & (got64 <= hi)


def acc_bound(mode, S, K):
    """the error allowed before the one output rounding for an fp32 sum of K terms whose absolute values sum to S.
    fp32 mode: 1.001 (K + 3) 2^-24 S + (K + 3) 2^-149 -- the first-order bound of K roundings in any summation order (split-K slabs,
    the bias and the `scale` fma are the + 3), plus one smallest subnormal per rounding for sums that leave the normal range.
    16-bit modes: C_ACC S + (K + 3) 2^-149.  No floor."""
    if mode == "fp32":
        return 1.001 * (K + 3) * 2.0 ** -24 * S + (K + 3) * F32_MIN_SUB
    return C_ACC[mode] * S + (K + 3) * F32_MIN_SUB


def terms(name, N, Cin, Cout, k, Ho, Wo):
    """K of acc_bound for one element of the tensor `name`"""
    return {"output": Cin * k * k + 1, "grad_input": Cout * k * k, "grad_weight": N * Ho * Wo, "grad_bias": N * Ho * Wo}[name]


def same_class(got, ref, what=""):
    """NaN must meet NaN, +inf +inf and -inf -inf -> the mask of the elements finite in both"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for name, g, r in (("NaN", torch.isnan(got), torch.isnan(ref)), ("+inf", got == float("inf"), ref == float("inf")),
                       ("-inf", got == float("-inf"), ref == float("-inf"))):
        bad = g != r
        assert not bool(bad.any()), "%s: %d elements where only one side is %s, first at %s (got %r, reference %r)" % (
            what, int(bad.sum()), name, tuple(bad.nonzero()[0].tolist()), float(got[bad][0]), float(ref[bad][0]))
    return torch.isfinite(got) & torch.isfinite(ref)


# ---- the scale sweep: the four dense conv families against float64, inputs multiplied by powers of two --------------------------------
SMALL = (2, 6, 9, 7, 4)                          # N, Cin, H, W, Cout: odd, H != W, two images, channel padding
RAGGED = (1, 192, 12, 11, 130)                   # test_gpu_conv_grad.py's ragged_tiles: several channel chunks
# family -> (entry prefix, k, dims of the C entries, weight shape, the op on (x, w, b))
FAMILIES = {
    "conv2d": ("tdrn_conv2d", 3, lambda N, Ci, H, W, Co: (N, Ci, H, W, Co, 3, 3, 1, 1, 1, 1, 1, 1),
               lambda Ci, Co: (Co, Ci, 3, 3), lambda x, w, b: F.conv2d(x, w, b, 1, 1)),
    "conv2d_strided": ("tdrn_conv2d_strided", 3, lambda N, Ci, H, W, Co: (N, Ci, H, W, Co, 3, 3, 2, 2, 1, 1, 1, 1),
                       lambda Ci, Co: (Co, Ci, 3, 3), lambda x, w, b: F.conv2d(x, w, b, 2, 1)),
    "conv5x5": ("tdrn_conv5x5", 5, lambda N, Ci, H, W, Co: (N, Ci, H, W, Co, 5, 5, 1, 1, 2, 2, 1, 1),
                lambda Ci, Co: (Co, Ci, 5, 5), lambda x, w, b: F.conv2d(x, w, b, 1, 2)),
    "conv_transpose2d": ("tdrn_conv_transpose2d", 2, lambda N, Ci, H, W, Co: (N, Ci, H, W, Co, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1),
                         lambda Ci, Co: (Ci, Co, 2, 2), lambda x, w, b: F.conv_transpose2d(x, w, b, 2)),
}
SWEEP_CASES = [(f, "small") for f in FAMILIES] + [("conv2d", "ragged")]
SHAPES = {"small": SMALL, "ragged": RAGGED}
# name -> the exponents of the powers of two on (x, w, grad_output); the bias takes x's times w's, the scale of the output it joins
_WIDE = {"x-100": (-100, 0, 0), "x+100": (100, 0, 0), "go-100": (0, 0, -100), "x-70_go-70": (-70, 0, -70)}
SCALES = {"fp32": _WIDE, "bf16": _WIDE,
          "fp16": {"x-12": (-12, 0, 0), "x-20": (-20, 0, 0), "x+13": (13, 0, 0), "go-12": (0, 0, -12), "go-20": (0, 0, -20),
                   "go+13": (0, 0, 13), "w-10_x-10": (-10, -10, 0)}}
NAMES = ("output", "grad_input", "grad_weight", "grad_bias")


def out_shape(family, shape):
    N, Ci, H, W, Co = shape
    op = FAMILIES[family][4]
    return tuple(op(torch.zeros(N, Ci, H, W), torch.zeros(FAMILIES[family][3](Ci, Co)), None).shape)


@functools.lru_cache(maxsize=None)
def unit_inputs(family, case):
    """the usual draw at unit scale: (x, w, b, grad_output) in fp32"""
    N, Ci, H, W, Co = SHAPES[case]
    k = FAMILIES[family][1]
    gen = torch.Generator().manual_seed(1000 + 10 * list(FAMILIES).index(family) + list(SHAPES).index(case))
    x = torch.randn(N, Ci, H, W, generator=gen)
    w = torch.randn(FAMILIES[family][3](Ci, Co), generator=gen) * (Ci * k * k) ** -0.5
    b = torch.randn(Co, generator=gen)
    go = torch.randn(out_shape(family, SHAPES[case]), generator=gen)
    return x, w, b, go


def scaled_inputs(family, case, exps):
    ax, aw, ago = exps
    x, w, b, go = unit_inputs(family, case)
    return x * 2.0 ** ax, w * 2.0 ** aw, b * 2.0 ** (ax + aw), go * 2.0 ** ago


def autograd4(family, x, w, b, go):
    """(output, grad_input, grad_weight, grad_bias) of the family's op by torch's CPU autograd, in the inputs' precision"""
    x, w, b = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = FAMILIES[family][4](x, w, b)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), go)
    return y.detach(), gx, gw, gb


@functools.lru_cache(maxsize=None)
def sweep_reference(family, case, mode, scale):
    """float64 autograd on the inputs as the op uses them -> (reference, S = the same op on absolute values, bound = acc_bound) per
    tensor of NAMES; computed once, never changed"""
    N, Ci, H, W, Co = SHAPES[case]
    k = FAMILIES[family][1]
    x, w, b, go = scaled_inputs(family, case, SCALES[mode][scale])
    xr, wr, gr = (rounded(t, mode).double() for t in (x, w, go))
    ref = autograd4(family, xr, wr, b.double(), gr)
    S = autograd4(family, xr.abs(), wr.abs(), b.double().abs(), gr.abs())
    Ho, Wo = go.shape[2:]
    bound = tuple(acc_bound(mode, s, terms(n, N, Ci, Co, k, Ho, Wo)) for n, s in zip(NAMES, S))
    return ref, S, bound


def worst_share(what, got, ref, bound):
    """print the worst share of the bound, then assert |got - ref| <= bound elementwise -> the share"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % what
    d = (got - ref).abs()
    share = torch.where(d == 0, torch.zeros_like(d), d / bound)          # (a zero bound admits a zero error only)
    worst = float(share.max())
    print("%s: max|d| %.3e  worst share of the bound %.3e" % (what, float(d.max()), worst))
    assert bool((d <= bound).all()), (what, worst)
    return worst


def ref64(x, w, b, go, pad):
    """stride-1 conv2d and its three gradients in float64 by one matmul per tap, on the tensors' device -> (y, gx, gw, gb), NCHW"""
    N, Ci, H, W = x.shape
    Co, k = w.shape[0], w.shape[2]
    xh, gh = x.permute(0, 2, 3, 1), go.permute(0, 2, 3, 1)
    xp = F.pad(xh, (0, 0, pad, pad, pad, pad))
    q = k - 1 - pad
    gp = F.pad(gh, (0, 0, q, q, q, q))
    y = b.expand(N, H, W, Co).clone()
    gx = torch.zeros_like(xh)
    gw = torch.zeros_like(w)
    for i in range(k):
        for j in range(k):
            xs = xp[:, i:i + H, j:j + W, :]
            y = y + xs @ w[:, :, i, j].t()
            gx = gx + gp[:, k - 1 - i:k - 1 - i + H, k - 1 - j:k - 1 - j + W, :] @ w[:, :, i, j]
            gw[:, :, i, j] = gh.reshape(-1, Co).t() @ xs.reshape(-1, Ci)
    return y.permute(0, 3, 1, 2), gx.permute(0, 3, 1, 2), gw, gh.reshape(-1, Co).sum(0)
