"""What the GPU tests of the transform-domain deformable conv share (tdrn_hip.h section i-l; DESIGN.md section 23;
test_gpu_deform_ts.py, test_gpu_deform_ts_scope.py; test_deform_ts_ref.py checks this file on the CPU): the C entries on plain
device buffers, inputs that are exact by construction, the float64 references and the derived bound, at any geometry of the op's
scope: kernel (kh, kw), stride (sh, sw), padding (ph, pw), dilation (dh, dw), so Ho x Wo outputs over an H x W map.

Inputs are exact by construction, so the bound is derived, not tuned: X, W and grad_output are exactly representable in the compute
type; offsets are fp32 multiples of 2^-6 with |offset| <= 16, so coordinates, fractions, the four bilinear weights and b * gO are exact
in fp32, and integer coordinates (offset 0 included), the [H-1, H) band and rejections are ordinary cases.  That holds at every
geometry used here: h_in + ti dh stays below 48 in magnitude (maps and dilated windows below 32, pad <= 2), so a coordinate stays
below 64 with 6 fractional bits (12 significant bits), a fraction has 6 bits, a bilinear weight at most 12 and b * gO at most
12 + 11 = 23 significant bits.  Far offsets (make_far: +-1e6, +-3e9, and the non-finite ones) are integers that fp32 holds; their
samples are rejected by the first comparison and nothing is computed from them.

Bound, elementwise, nothing exempted:  |got - ref| <= (U + 2 C_ACC) S + TINY.
  * each result passes through exactly one 16-bit rounding of an inexact intermediate (Y for output and grad_offset, Z for grad_input
    and grad_weight); U is a whole last-place unit, twice the rounding's half unit;
  * each result passes through two fp32 summation stages (GEMM, then blend / scatter / reduction), one C_ACC S each;
  * S is the same quantity on absolute values in float64: for output, grad_input and grad_weight the oracle run on |X|, |W|, |gO| (the
    bilinear weights are non-negative); for grad_offset it is restated here, sum_co |gO| sum_corners |db/dpos| Ybar with
    Ybar = sum_c |W| |X| (offset_S), zero along an axis inside its clamp band, where the derivative is zero.
The worst share of the bound is printed per result.

Only Ts and the functions that take device tensors need a GPU; everything else runs on the CPU."""
import collections
import functools

import torch

from tdrn_amd import _lib

from _conv_train_harness import C_ACC, DEV
from _deform_grad_ref import _schedule, grads
from _nhwc_harness import TINY, U, exact

MODES = ("bf16", "fp16")
REGIMES = ("half", "wide", "converging")
NAMES = ("output", "grad_input", "grad_offset", "grad_weight")


class Geom(collections.namedtuple("Geom", "N Cin H W Cout kh kw sh sw ph pw dh dw")):
    """one geometry of the op (G = 1); hashable, so a problem is computed once per (geometry, type, offsets)"""
    __slots__ = ()

    @property
    def Ho(self):
        return (self.H + 2 * self.ph - (self.dh * (self.kh - 1) + 1)) // self.sh + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.pw - (self.dw * (self.kw - 1) + 1)) // self.sw + 1

    @property
    def taps(self):
        return self.kh * self.kw

    @property
    def M(self):
        return self.N * self.Ho * self.Wo

    @property
    def NJ(self):
        """columns per lane: which instance of the sampling and backward kernels runs"""
        return (self.Cout + 63) // 64

    @property
    def YC(self):
        """columns of a row of Y: [taps][Cout rounded up to 8] padded to a multiple of 64"""
        return (self.taps * ((self.Cout + 7) // 8 * 8) + 63) // 64 * 64

    @property
    def stride(self):
        return (self.sh, self.sw)

    @property
    def padding(self):
        return (self.ph, self.pw)

    @property
    def dilation(self):
        return (self.dh, self.dw)

    @property
    def dims(self):
        """the C ABI's argument order: N, Cin, H, W, Cout, kW, kH, dW, dH, padW, padH, dilationH, dilationW, G"""
        return (self.N, self.Cin, self.H, self.W, self.Cout, self.kw, self.kh, self.sw, self.sh, self.pw, self.ph, self.dh, self.dw, 1)

    @property
    def smaller_than_kernel(self):
        """the reference's "input image is smaller than kernel" rule (H < kH or W < kW; only the padding makes the window fit): the
        gather op keeps the rule and refuses such a map, the transform-domain op covers it"""
        return self.H < self.kh or self.W < self.kw

    @property
    def name(self):
        return "%dx%dx%dx%d-co%d-k%dx%d-s%d%d-p%d%d-d%d%d" % self


def square(N, Cin, H, W, Cout, k, pad=None):
    """a square kernel at stride 1 and dilation 1, pad k // 2 unless given: the geometry of test_gpu_deform_ts.py's cases"""
    pad = k // 2 if pad is None else pad
    return Geom(N, Cin, H, W, Cout, k, k, 1, 1, pad, pad, 1, 1)


def _grid(g):
    """h_in (1, Ho, 1) and w_in (1, 1, Wo): the top-left input coordinate of every output pixel"""
    return (torch.arange(g.Ho) * g.sh - g.ph).view(1, g.Ho, 1), (torch.arange(g.Wo) * g.sw - g.pw).view(1, 1, g.Wo)


def make_offsets(g, offsets, gen):
    """offsets: a regime of REGIMES or a number, the sigma.  fp32 multiples of 2^-6 with |offset| <= 16; 10 % of the entries are 0
    and 10 % rounded to integers ("half": sigma 0.5, "wide": sigma max(H, W)); "converging": every sample of an image is aimed at one
    of two of its pixels, the maximal collision of the scatter's atomics."""
    N, taps, H, W, Ho, Wo = g.N, g.taps, g.H, g.W, g.Ho, g.Wo
    if offsets != "converging":
        sigma = {"half": 0.5, "wide": float(max(H, W))}.get(offsets, offsets)
        off = (torch.round(sigma * torch.randn(N, 2 * taps, Ho, Wo, generator=gen) * 64) / 64).clamp(-16, 16)
        kind = torch.rand(N, 2 * taps, Ho, Wo, generator=gen)
        off = torch.where(kind < 0.1, torch.zeros_like(off), off)                   # offset 0: the sample sits on its tap
        off = torch.where((kind >= 0.1) & (kind < 0.2), torch.round(off), off)      # other integer coordinates
        return off.float()
    targets = [(H // 2, W // 2), (max(H // 2 - 1, 0), max(W // 2 - 1, 0))]
    pick = torch.randint(0, 2, (N, taps, Ho, Wo), generator=gen)
    th = torch.tensor([targets[0][0], targets[1][0]])[pick].float()
    tw = torch.tensor([targets[0][1], targets[1][1]])[pick].float()
    off = torch.empty(N, 2 * taps, Ho, Wo)
    h_in, w_in = _grid(g)
    for t in range(taps):
        ti, tj = divmod(t, g.kw)
        off[:, 2 * t] = th[:, t] - (h_in + ti * g.dh).float()
        off[:, 2 * t + 1] = tw[:, t] - (w_in + tj * g.dw).float()
    assert float(off.abs().max()) <= 16
    return off


FAR = (1e6, -1e6, 3e9, -3e9)
NON_FINITE = (float("inf"), float("-inf"), float("nan"))


def make_far(off, values, seed):
    """-> (the offsets with 10 % of the entries replaced by draws from `values`, the boolean mask of those entries); the mask depends
    on the seed and the shape alone, so FAR and NON_FINITE land on the same entries"""
    gen = torch.Generator().manual_seed(seed)
    mask = torch.rand(off.shape, generator=gen) < 0.1
    pick = torch.randint(0, len(values), off.shape, generator=gen)
    return torch.where(mask, torch.tensor(values, dtype=torch.float32)[pick], off), mask


def sample_kinds(g, off):
    """boolean (N, taps, Ho, Wo) per sample, from the fp32 coordinates as the device forms them: accepted (not rejected); band (accepted,
    a coordinate in its [H-1, H) clamp band); integer (accepted, a coordinate on an integer: the one-sided derivative)"""
    h_in, w_in = _grid(g)
    acc, band, integer = [], [], []
    for t in range(g.taps):
        ti, tj = divmod(t, g.kw)
        h_im = (h_in + ti * g.dh).float() + off[:, 2 * t].float()
        w_im = (w_in + tj * g.dw).float() + off[:, 2 * t + 1].float()
        ok = (h_im >= 0) & (w_im >= 0) & (h_im < g.H) & (w_im < g.W)
        acc.append(ok)
        band.append(ok & ((h_im >= g.H - 1) | (w_im >= g.W - 1)))
        integer.append(ok & ((h_im == torch.floor(h_im)) | (w_im == torch.floor(w_im))))
    return dict(accepted=torch.stack(acc, 1), band=torch.stack(band, 1), integer=torch.stack(integer, 1))


def offset_S_square(x, off, w, go, k, pad):
    """offset_S as test_gpu_deform_ts.py had it, for a square kernel at stride 1 and dilation 1: kept, unchanged, as what the general
    offset_S must reproduce (tests/test_deform_ts_ref.py)"""
    N, Cin, H, W = x.shape
    Cout, taps, HW = w.shape[0], k * k, H * W
    ybar = torch.einsum("oct,ncq->ntoq", w.abs().double().reshape(Cout, Cin, taps), x.abs().double().reshape(N, Cin, HW))
    ago = go.abs().double().reshape(N, Cout, HW)
    h_in = (torch.arange(H) - pad).view(1, H, 1)
    w_in = (torch.arange(W) - pad).view(1, 1, W)
    S = torch.zeros(N, 2 * taps, H, W, dtype=torch.float64)
    for t in range(taps):
        ti, tj = divmod(t, k)
        oh, ow = off[:, 2 * t].float(), off[:, 2 * t + 1].float()
        h_im, w_im = (h_in + ti).float() + oh, (w_in + tj).float() + ow
        valid = (h_im >= 0) & (w_im >= 0) & (h_im < H) & (w_im < W)
        hm, wm = torch.tensor(float(ti)) + oh, torch.tensor(float(tj)) + ow
        height, width = H - h_in, W - w_in
        h_low, w_low = torch.floor(hm).long(), torch.floor(wm).long()
        ch, cw = h_low >= height - 1, w_low >= width - 1
        h_low = torch.where(ch, (height - 1).expand_as(h_low), h_low)
        w_low = torch.where(cw, (width - 1).expand_as(w_low), w_low)
        h_high, w_high = torch.where(ch, h_low, h_low + 1), torch.where(cw, w_low, w_low + 1)
        lh = torch.where(ch, torch.zeros_like(oh, dtype=torch.float64), (ti + oh.double()) - h_low.double())
        lw = torch.where(cw, torch.zeros_like(ow, dtype=torch.float64), (tj + ow.double()) - w_low.double())
        hh, hw = 1 - lh, 1 - lw
        r0, r1 = (h_in + h_low).clamp(0, H - 1), (h_in + h_high).clamp(0, H - 1)
        q0, q1 = (w_in + w_low).clamp(0, W - 1), (w_in + w_high).clamp(0, W - 1)

        def corner(r, q):
            idx = (r * W + q).reshape(N, 1, HW).expand(N, Cout, HW)
            return torch.gather(ybar[:, t], 2, idx)

        y1, y2, y3, y4 = corner(r0, q0), corner(r0, q1), corner(r1, q0), corner(r1, q1)
        f = lambda a: a.reshape(N, 1, HW)
        dh = (f(hw) * (y1 + y3) + f(lw) * (y2 + y4)) * f((~ch).double())
        dw = (f(hh) * (y1 + y2) + f(lh) * (y3 + y4)) * f((~cw).double())
        S[:, 2 * t] = (ago * dh).sum(1).reshape(N, H, W) * valid.double()
        S[:, 2 * t + 1] = (ago * dw).sum(1).reshape(N, H, W) * valid.double()
    return S


def offset_S(g, x, off, w, go):
    """sum_co |gO| sum_corners |db/dpos| Ybar, float64, (N, 2 taps, Ho, Wo): the sampling geometry as the device forms it (fp32
    coordinates, rejection, the [H-1, H) clamp: the rule of tests/_deform_grad_ref.py, with h_in = ho sh - ph and tap t at
    (ti dh, tj dw), (ti, tj) = divmod(t, kw)), the absolute values of the four corner derivatives of the bilinear weights.  Ybar lives
    on the H x W input pixels, everything else on the Ho x Wo output pixels."""
    N, Cin, H, W, Cout, taps, Ho, Wo = g.N, g.Cin, g.H, g.W, g.Cout, g.taps, g.Ho, g.Wo
    HW, P = H * W, Ho * Wo
    ybar = torch.einsum("oct,ncq->ntoq", w.abs().double().reshape(Cout, Cin, taps), x.abs().double().reshape(N, Cin, HW))
    ago = go.abs().double().reshape(N, Cout, P)
    h_in, w_in = _grid(g)
    S = torch.zeros(N, 2 * taps, Ho, Wo, dtype=torch.float64)
    for t in range(taps):
        ti, tj = divmod(t, g.kw)
        ti, tj = ti * g.dh, tj * g.dw
        oh, ow = off[:, 2 * t].float(), off[:, 2 * t + 1].float()
        h_im, w_im = (h_in + ti).float() + oh, (w_in + tj).float() + ow
        valid = (h_im >= 0) & (w_im >= 0) & (h_im < H) & (w_im < W)
        hm, wm = torch.tensor(float(ti)) + oh, torch.tensor(float(tj)) + ow
        height, width = H - h_in, W - w_in
        h_low, w_low = torch.floor(hm).long(), torch.floor(wm).long()
        ch, cw = h_low >= height - 1, w_low >= width - 1
        h_low = torch.where(ch, (height - 1).expand_as(h_low), h_low)
        w_low = torch.where(cw, (width - 1).expand_as(w_low), w_low)
        h_high, w_high = torch.where(ch, h_low, h_low + 1), torch.where(cw, w_low, w_low + 1)
        lh = torch.where(ch, torch.zeros_like(oh, dtype=torch.float64), (ti + oh.double()) - h_low.double())
        lw = torch.where(cw, torch.zeros_like(ow, dtype=torch.float64), (tj + ow.double()) - w_low.double())
        hh, hw = 1 - lh, 1 - lw
        r0, r1 = (h_in + h_low).clamp(0, H - 1), (h_in + h_high).clamp(0, H - 1)
        q0, q1 = (w_in + w_low).clamp(0, W - 1), (w_in + w_high).clamp(0, W - 1)

        def corner(r, q):
            idx = (r * W + q).reshape(N, 1, P).expand(N, Cout, P)
            return torch.gather(ybar[:, t], 2, idx)

        y1, y2, y3, y4 = corner(r0, q0), corner(r0, q1), corner(r1, q0), corner(r1, q1)
        f = lambda a: a.reshape(N, 1, P)
        dh = (f(hw) * (y1 + y3) + f(lw) * (y2 + y4)) * f((~ch).double())
        dw = (f(hh) * (y1 + y2) + f(lh) * (y3 + y4)) * f((~cw).double())
        # a rejected sample has S = 0 (where: a far offset's fraction may be huge, and 0 * inf would be NaN)
        S[:, 2 * t] = torch.where(valid, (ago * dh).sum(1).reshape(N, Ho, Wo), torch.zeros((), dtype=torch.float64))
        S[:, 2 * t + 1] = torch.where(valid, (ago * dw).sum(1).reshape(N, Ho, Wo), torch.zeros((), dtype=torch.float64))
    return S


@functools.lru_cache(maxsize=None)
def problem(g, mode, offsets, seed=0, far=None):
    """inputs (CPU fp32), float64 references and absolute-value sums, computed once and left unchanged.  offsets: see make_offsets.
    far: None, or the seed of make_far(off, FAR, seed): p["off"] then holds the far offsets, p["far"] the mask of the replaced entries
    and p["near"] the offsets before the replacement."""
    gen = torch.Generator().manual_seed(seed)
    x = exact(torch.randn(g.N, g.Cin, g.H, g.W, generator=gen), mode)
    w = exact(torch.randn(g.Cout, g.Cin, g.kh, g.kw, generator=gen) / 8, mode)
    go = exact(torch.randn(g.N, g.Cout, g.Ho, g.Wo, generator=gen), mode)
    off = make_offsets(g, offsets, gen)
    assert torch.equal(off * 64, torch.round(off * 64)) and off.dtype == torch.float32 and float(off.abs().max()) <= 16
    extra = {}
    if far is not None:
        near = off
        off, mask = make_far(near, FAR, far)
        assert off.dtype == torch.float32 and torch.equal(off[~mask], near[~mask]) and torch.equal(off, torch.round(off * 64) / 64)
        extra = dict(far=mask, near=near)
    ref = dict(zip(NAMES, grads(x, off, w, go, g.stride, g.padding, g.dilation, 1)))       # (out, grad_input, grad_offset, grad_weight)
    so, sgx, _, sgw = grads(x.abs(), off, w.abs(), go.abs(), g.stride, g.padding, g.dilation, 1)
    S = {"output": so, "grad_input": sgx, "grad_offset": offset_S(g, x, off, w, go), "grad_weight": sgw}
    return dict(x=x, w=w, off=off, go=go, ref=ref, S=S, kinds=sample_kinds(g, off), **extra)


def bound(mode, S):
    return (U[mode] + 2 * C_ACC[mode]) * S + TINY[mode]


SHARES = {}         # (group, mode, result) -> (the worst share seen, the case that gave it): what DESIGN.md section 23 tabulates


def within(what, mode, name, got, p, scale=1.0, group=None):
    d = (got.detach().cpu().double() - p["ref"][name]).abs()
    assert torch.isfinite(d).all(), "%s %s: non-finite values" % (what, name)
    b = scale * bound(mode, p["S"][name])
    share = float((d / b).max())
    print("%s %-11s max|d| %.3e  worst share of the bound %.3e" % (what, name, float(d.max()), share))
    if group is not None and share > SHARES.get((group, mode, name), (-1.0, None))[0]:
        SHARES[(group, mode, name)] = (share, what)
        print("WORST %s %s %s %.3f %s" % (group, mode, name, share, what))
    assert bool((d <= b).all()), (what, name, share)
    return share


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


def same_bits(p, q):
    return p.shape == q.shape and torch.equal(bits(p), bits(q))


class Ts(object):
    """the entries on plain device buffers"""

    def __init__(self, g, mode):
        self.lib, self.dt, self.g, self.dims = _lib.lib(), _lib.DTYPES[mode], g, g.dims
        self.nb = self.lib.tdrn_deform_conv_ts_workspace_bytes(*self.dims, self.dt)
        self.yb = self.lib.tdrn_deform_conv_ts_y_bytes(*self.dims, self.dt)
        assert self.nb > 0 and self.yb > 0
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)

    def inputs(self, p):
        return tuple(p[n].to(DEV) for n in ("x", "w", "off", "go"))

    def new_y(self):
        return torch.full((self.yb,), 0xFF, dtype=torch.uint8, device=DEV)

    def forward(self, x, w, off, out, y=None, ws=None):
        ws = self.ws if ws is None else ws
        _lib.check(self.lib.tdrn_deform_conv_ts_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(off), _lib.ptr(out), _lib.ptr(y), *self.dims,
                                                        self.dt, _lib.ptr(ws), self.nb, _lib.current_stream(DEV)))
        return out

    def backward(self, x, w, off, go, y, gi, goff, gw, ws=None):
        ws = self.ws if ws is None else ws
        _lib.check(self.lib.tdrn_deform_conv_ts_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(off), _lib.ptr(go), _lib.ptr(y), _lib.ptr(gi),
                                                         _lib.ptr(goff), _lib.ptr(gw), *self.dims, self.dt, _lib.ptr(ws), self.nb,
                                                         _lib.current_stream(DEV)))

    def all(self, p, y_given=True, off=None):
        """-> (output, grad_input, grad_offset, grad_weight, Y), every output pre-filled with NaN and Y with 0xFF bytes; off: offsets in
        place of the problem's"""
        x, w, o, go = self.inputs(p)
        off = o if off is None else off.to(DEV)
        nan = lambda t: torch.full_like(t, float("nan"))
        out, gi, goff, gw, y = nan(go), nan(x), nan(off), nan(w), self.new_y()
        self.forward(x, w, off, out, y)
        self.backward(x, w, off, go, y if y_given else None, gi, goff, gw)
        torch.cuda.synchronize()
        return out, gi, goff, gw, y


# ------------------------------------------------------------------------------------------------------------------------------------
# Shapes of the fuzz (tests/test_gpu_deform_ts_scope.py); tests/test_deform_ts_ref.py asserts on the CPU that they are inside the op's
# scope, reach what they are meant to reach and can tell a wrong kernel from a right one.
# ------------------------------------------------------------------------------------------------------------------------------------
TS_FUZZ_SEEDS = tuple(range(24))
# around Cp = Cout rounded up to 8 and the edges of `lane + 64 j < Cout`, 75 = the paired 21-class heads, 255 = the paired 81-class heads
# One value per seed.  The second line repeats eight of the sixteen values: with each value once and eight of them repeated at random,
# only four seeds had more than 192 couts, and a kernel that loses its fourth column per lane must fail in at least six.
TS_FUZZ_COUT = (1, 7, 8, 9, 63, 64, 65, 75, 127, 128, 129, 191, 192, 193, 255, 256,
                9, 65, 127, 129, 191, 193, 255, 256)
TS_FUZZ_SIGMA = (0.0, 0.5, 2.0, 6.0)


def ts_fuzz_shape(seed):
    """-> (Geom, the offsets' sigma).  Past 128 couts the kernels stay at 3 x 3 and below, so the float64 oracle stays quick."""
    import numpy as np
    n = len(TS_FUZZ_SEEDS)
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    Cout, sigma = _schedule(TS_FUZZ_COUT, n, 21)[seed], float(_schedule(TS_FUZZ_SIGMA, n, 22)[seed])
    Cin = int(rng.choice([64, 128, 192]))
    kmax = 3 if Cout > 128 else 5
    kh, kw = int(rng.integers(1, kmax + 1)), int(rng.integers(1, kmax + 1))
    sh, sw = int(rng.integers(1, 3)), int(rng.integers(1, 3))
    dh, dw = int(rng.integers(1, 3)), int(rng.integers(1, 3))
    ph, pw = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    N = int(rng.integers(1, 4))
    H = max(1, dh * (kh - 1) + 1 - 2 * ph) + int(rng.integers(0, 9))
    W = max(1, dw * (kw - 1) + 1 - 2 * pw) + int(rng.integers(0, 9))
    return Geom(N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw), sigma


# The inputs' seeds.  The smallest shapes have nine samples, so whether one of them lands in a clamp band is the offsets' luck: the base is
# the first of 70000, 71000, ... at which the conditions on the inputs hold that test_deform_ts_ref.py::test_fuzz_coverage asserts (at
# 70000 seed 19 has no sample in a band, at 71000 seed 6 accepts 4 % of its samples).  No kernel's result entered the choice.
TS_FUZZ_INPUT_SEED = 72000


def fuzz_problem(seed, mode):
    g, sigma = ts_fuzz_shape(seed)
    return g, problem(g, mode, sigma, TS_FUZZ_INPUT_SEED + 10 * seed + MODES.index(mode))


# ------------------------------------------------------------------------------------------------------------------------------------
# The fixed cases of tests/test_gpu_deform_ts_scope.py
# ------------------------------------------------------------------------------------------------------------------------------------
EDGE_COUTS = (1, 8, 9, 64, 65, 128, 129, 192, 193, 255, 256)       # Cp = Cout rounded up to 8, and the edges of `lane + 64 j < Cout`
# two images of 4 x 5 pixels (M = 40: ten full workgroups) under 3 x 3, pad 1; and 1 x 1 kernels for the two extremes of a row's padding:
# one cout = 8 live columns of 64, 256 couts = no padding at all
EDGES = tuple(square(2, 64, 4, 5, co, 3) for co in EDGE_COUTS) + (square(2, 64, 4, 5, 1, 1), square(2, 64, 4, 5, 256, 1))
# loc (12) + conf (243) columns of the paired 81-class heads; the second has 25 * 256 = 6400 columns per row
HEADS = (square(2, 256, 5, 5, 255, 3), square(1, 256, 3, 3, 255, 5))
HEAD_REGIMES = ("half", "converging")
FAR_GEOMS = (square(2, 64, 4, 5, 129, 3), ts_fuzz_shape(13)[0])      # three columns per lane at stride 1; and at stride 2, Ho != H
GRAPH_FUZZ_SEED = 18                                                # four columns per lane at stride 2, Ho != H
assert FAR_GEOMS[1].stride == (2, 2) and FAR_GEOMS[1].NJ == 3 and FAR_GEOMS[1].Ho != FAR_GEOMS[1].H
assert ts_fuzz_shape(GRAPH_FUZZ_SEED)[0].stride == (2, 2) and ts_fuzz_shape(GRAPH_FUZZ_SEED)[0].NJ >= 3
assert ts_fuzz_shape(GRAPH_FUZZ_SEED)[0].Ho != ts_fuzz_shape(GRAPH_FUZZ_SEED)[0].H


def edge_problem(g, mode):
    return problem(g, mode, "wide", 81000 + 10 * EDGES.index(g) + MODES.index(mode))


def head_problem(g, mode, regime):
    return problem(g, mode, regime, 82000 + 100 * HEADS.index(g) + 10 * HEAD_REGIMES.index(regime) + MODES.index(mode))


def far_problem(g, mode):
    """"half" offsets with 10 % of the entries replaced by +-1e6 / +-3e9; make_far(p["near"], NON_FINITE, far_seed(g)) puts the non-finite
    values on the same entries"""
    return problem(g, mode, "half", 83000 + 10 * FAR_GEOMS.index(g) + MODES.index(mode), far_seed(g))


def far_seed(g):
    return 84000 + FAR_GEOMS.index(g)


def fixed_problems(mode):
    """(name, Geom, problem) of every fixed case"""
    for g in EDGES:
        yield "edge " + g.name, g, edge_problem(g, mode)
    for g in HEADS:
        for regime in HEAD_REGIMES:
            yield "heads %s %s" % (g.name, regime), g, head_problem(g, mode, regime)
    for g in FAR_GEOMS:
        yield "far " + g.name, g, far_problem(g, mode)
