"""The 16-bit outputs of the resident entries (tdrn_hip.h section i-k) over the whole range of the type: the one rounding of a conv
output, of a BatchNorm output and the pool's comparison, at ties, in the subnormal range and at the overflow boundary.  Helpers and
bounds: tests/_number_range.py -- cast_interval (what the one rounding may give, with no `+ tiny`), acc_bound and bit equality.

Routes.  Every conv test runs on each kernel forward and backward_input can reach, at the smallest case that reaches it, and asserts
the route: `tile`, `k1` (conv_igemm) and `patch32` (conv3x3_patch) of test_gpu_nhwc_conv.py; `pw1x1` and `pp`: 48 images of 32 x 32
with 256 -> 256 channels are the 192 items of 256 pixels x 256 couts from which conv_route.hip hands a 1 x 1 layer to the wide GEMM and
a 3 x 3 layer to conv3x3_pp, in both directions.

a. Output ties.  Three of the input channels are nonzero and the weight has its centre tap only: the input holds (h, 16 half, 4 half)
   and the weight (1, 2^-4, v 2^-14) with half = half an ulp of h in the type and v = 0, +1, -1 by output channel, so an output element
   is exactly h + half + v delta, delta = 2^-12 half.  All operands are exact in the type, every partial sum in fp32, whatever the order.
   Expected: rne_bits, bit for bit: the tie to even, one fp32 step to either side of it, the subnormal spacing and largest + half an
   ulp -> inf, one pixel per edge pattern h and sign.
b. Scale sweep: section 3 of test_gpu_number_range.py on resident tensors.  output and grad_input must lie in cast_interval(ref - e,
   ref + e), e = acc_bound; grad_weight and grad_bias (fp32) within acc_bound.  The float64 reference is ref64 of tests/_number_range.py,
   on the CPU for the small cases and on the device for the two large ones (test_number_range_ref.py pins it to torch's autograd).
c. BatchNorm in eval mode at the fp16 scales with beta 0 and 2^-16, relu off and on, against float64 through cast_interval with
   e = 8 * 2^-24 (|x - mean| |a| + |beta|): sqrt, divide and multiply for a = gamma / sqrt(var + eps), one subtraction, one fma.
d. MaxPool2d 2 x 2 / 2 over every finite pattern of the type: forward and backward bit for bit with torch's on the float values.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import _number_range as nr
from _conv_train_harness import DEV
from _nhwc_harness import ConvAbi, bn_forward, pool_backward, pool_forward, resident

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

TS = ("bf16", "fp16")
#        name       N   Cin  H   W  Cout k pad  kernel
CASES = {"tile":    (1, 64,  8,  8,  64, 3, 1, "igemm"),
         "k1":      (2, 128, 7,  5,  64, 1, 0, "igemm"),
         "patch32": (1, 64,  16, 32, 64, 3, 1, "patch"),
         "pw1x1":   (48, 256, 32, 32, 256, 1, 0, "pw1x1"),
         "pp":      (48, 256, 32, 32, 256, 3, 1, "pp")}
LARGE = ("pw1x1", "pp")


def _abi(case, T):
    N, Ci, H, W, Co, k, pad, kernel = CASES[case]
    abi = ConvAbi((N, Ci, H, W, Co, k, k, 1, 1, pad, pad, 1, 1), T)
    assert (abi.route(0), abi.route(1)) == (kernel, kernel), (case, T, abi.route(0), abi.route(1))
    return abi


def _bits_nchw(t16):
    """a resident tensor -> bit patterns in NCHW order, on its device"""
    return nr.to_bits(t16.detach().contiguous())


# ---- a. output ties ---------------------------------------------------------------------------------------------------------------------------
def _tie_table(T):
    """per edge pattern and sign: (h, half an ulp above h) in float64, signed -> (n, 2)"""
    h = nr.edge_patterns(T)
    lo = nr.decode64(T, h)
    last = h == nr.inf_bits(T) - 1
    hi = nr.decode64(T, torch.where(last, h, h + 1))
    half = torch.where(last, (lo - nr.decode64(T, h - 1)) / 2, (hi - lo) / 2)
    t = torch.stack([lo, half], 1)
    return torch.cat([t, -t])


@pytest.mark.parametrize("dgrad", [0, 1], ids=["forward", "backward_input"])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("case", list(CASES))
def test_output_ties_round_to_even(case, T, dgrad):
    N, Ci, H, W, Co, k, pad, _ = CASES[case]
    abi = _abi(case, T)
    cin, cout = (Co, Ci) if dgrad else (Ci, Co)                       # channels of the launch's input and of its output
    chans = (1, cin // 2 + 3, cin - 1)                                # the three nonzero channels, in different 16-channel groups
    v = torch.tensor([0.0, 1.0, -1.0], dtype=torch.float64)[torch.arange(cout) % 3]
    wsel = torch.zeros(cout, cin, k, k, dtype=torch.float64)
    wsel[:, chans[0], k // 2, k // 2] = 1.0
    wsel[:, chans[1], k // 2, k // 2] = 2.0 ** -4
    wsel[:, chans[2], k // 2, k // 2] = v * 2.0 ** -14
    w = (wsel.transpose(0, 1) if dgrad else wsel).contiguous().float()         # OIHW of the layer; the centre tap is its own mirror
    table = _tie_table(T)
    P = N * H * W
    bias = torch.zeros(Co, device=DEV)
    differ = total = 0
    for first in range(0, table.shape[0], P):
        part = table[first:first + P]
        src = torch.zeros(P, cin, dtype=torch.float64)
        src[:part.shape[0], chans[0]] = part[:, 0]
        src[:part.shape[0], chans[1]] = part[:, 1] * 16
        src[:part.shape[0], chans[2]] = part[:, 1] * 4
        want64 = src @ wsel[:, :, k // 2, k // 2].t()                  # three exact products, exact sums: (P, cout)
        src32, want32 = src.float(), want64.float()
        assert torch.equal(src32.double(), src) and torch.equal(nr.rne(T, src32), src32), "operands the type does not hold"
        assert torch.equal(want32.double(), want64) and torch.equal(nr.rne(T, w), w)
        exp = part[:, :1] + part[:, 1:] + (part[:, 1:] * 2.0 ** -12) * v[None, :]
        assert torch.equal(want64[:part.shape[0]], exp)                # h + half + v delta
        t = resident(src32.view(N, H, W, cin).permute(0, 3, 1, 2), T)
        if dgrad:
            got = abi.backward_input(t, w.to(DEV), torch.full((N, Ci, H, W), float("nan"), dtype=nr.TYPES[T], device=DEV)
                                     .contiguous(memory_format=torch.channels_last))
        else:
            got = abi.forward(t, w.to(DEV), bias, torch.full((N, Co, H, W), float("nan"), dtype=nr.TYPES[T], device=DEV)
                              .contiguous(memory_format=torch.channels_last))
        torch.cuda.synchronize()
        got_bits = nr.to_bits(got.detach().permute(0, 2, 3, 1).contiguous()).cpu().view(P, cout)
        want_bits = nr.rne_bits(T, want32)
        bad = got_bits != want_bits
        total += bad.numel()
        if bool(bad.any()):
            differ += int(bad.sum())
            i = bad.nonzero()[0]
            print("%s %s dgrad %d: exact %r (v %d) got %#06x want %#06x" % (case, T, dgrad, float(want64[i[0], i[1]]), int(v[i[1]]),
                                                                          int(got_bits[i[0], i[1]]), int(want_bits[i[0], i[1]])))
    print("%s %s %s: %d output elements, %d differ from rne_bits" % (case, T, "backward_input" if dgrad else "forward", total, differ))
    assert differ == 0


# ---- b. the scale sweep ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unit_draw(case):
    """the usual draw at unit scale (x, w, b, grad_output), once per case, where the reference of the case is computed"""
    N, Ci, H, W, Co, k, pad, _ = CASES[case]
    g = torch.Generator().manual_seed(2000 + list(CASES).index(case))
    draw = (torch.randn(N, Ci, H, W, generator=g), torch.randn(Co, Ci, k, k, generator=g) * (Ci * k * k) ** -0.5,
            torch.randn(Co, generator=g), torch.randn(N, Co, H, W, generator=g))
    return tuple(t.to(DEV if case in LARGE else "cpu") for t in draw)


def _sweep_inputs(case, T, exps):
    """the draw times the powers of two, exact in the type (the bias, fp32, takes the scale of the output it joins)"""
    ax, aw, ago = exps
    x, w, b, go = _unit_draw(case)
    return nr.rne(T, x * 2.0 ** ax), nr.rne(T, w * 2.0 ** aw), b * 2.0 ** (ax + aw), nr.rne(T, go * 2.0 ** ago)


def _in_interval(what, T, got16, ref, e):
    lo, hi = nr.cast_interval(T, ref - e, ref + e)
    got = nr.decode64(T, _bits_nchw(got16))
    ok = nr.inside(got, lo, hi)
    print("%s: %d elements, %d outside the interval, %d pinned to one value, %d +-inf allowed, %d subnormal or zero" % (
        what, ok.numel(), int((~ok).sum()), int((lo == hi).sum()), int(torch.isinf(hi).sum() + torch.isinf(lo).sum()),
        int((got.abs() < 2.0 ** (2 - (1 << (nr.EXP_BITS[T] - 1)))).sum())))
    assert bool(ok.all()), (what, "%d of %d outside cast_interval" % (int((~ok).sum()), ok.numel()),
                            [(float(a), float(l), float(h)) for a, l, h in list(zip(got[~ok], lo[~ok], hi[~ok]))[:4]])


@pytest.mark.parametrize("T,scale", [(T, scale) for T in TS for scale in nr.SCALES[T]])
@pytest.mark.parametrize("case", list(CASES))
def test_scale_sweep_rounds_once_without_a_floor(case, T, scale):
    N, Ci, H, W, Co, k, pad, _ = CASES[case]
    abi = _abi(case, T)
    K = {n: nr.terms(n, N, Ci, Co, k, H, W) for n in nr.NAMES}
    x, w, b, go = _sweep_inputs(case, T, nr.SCALES[T][scale])
    xr, gor, wd, bd = resident(x, T), resident(go, T), w.to(DEV), b.to(DEV)
    y = abi.forward(xr, wd, bd, torch.full_like(gor, float("nan")))
    gx = abi.backward_input(gor, wd, torch.full_like(xr, float("nan")))
    gw, gb = abi.backward_parameters(xr, gor, torch.zeros_like(wd), torch.zeros_like(bd))
    torch.cuda.synchronize()
    ins = [t.double() for t in (x, w, b, go)]
    ref = nr.ref64(*ins, pad)
    S = nr.ref64(*(t.abs() for t in ins), pad)
    failed = []
    for name, got, r, s in zip(nr.NAMES, (y, gx, gw, gb), ref, S):
        what = "%s %s %s %s" % (case, T, scale, name)
        e = nr.acc_bound(T, s, K[name])
        try:
            if name in ("output", "grad_input"):
                _in_interval(what, T, got.to(r.device), r.contiguous(), e.contiguous())
            else:
                nr.worst_share(what, got, r.cpu(), e.cpu())
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed


# ---- c. BatchNorm, eval mode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("T", TS)
def test_batch_norm_eval_rounds_once_at_the_ends_of_the_range(T, relu):
    N, C, H, W = 2, 128, 9, 7
    eps = 1e-5
    failed = []
    for a in (-12, -20, 13):
        for beta in (0.0, 2.0 ** -16):
            g = torch.Generator().manual_seed(31 + a)
            x = nr.rne(T, torch.randn(N, C, H, W, generator=g) * 2.0 ** a)
            mean = torch.randn(C, generator=g) * 0.25 * 2.0 ** a
            var = torch.rand(C, generator=g) + 0.5
            gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
            bt = torch.full((C,), beta)
            xr = resident(x, T)
            out = torch.full_like(xr, float("nan"))
            sm, si = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            rm, rv = mean.to(DEV), var.to(DEV)
            bn_forward(xr, gamma.to(DEV), bt.to(DEV), rm, rv, out, sm, si, False, 0.1, eps, relu, T)
            torch.cuda.synchronize()
            assert torch.equal(rm.cpu(), mean) and torch.equal(rv.cpu(), var)                  # eval mode moves no buffer
            sh = (1, C, 1, 1)
            a64 = (gamma.double() / torch.sqrt(var.double() + eps)).view(sh)
            d = x.double() - mean.double().view(sh)
            z = d * a64 + bt.double().view(sh)
            e = 8 * 2.0 ** -24 * (d.abs() * a64.abs() + bt.double().abs().view(sh))
            lo, hi = z - e, z + e
            if relu:
                lo, hi = lo.clamp_min(0.0), hi.clamp_min(0.0)
            try:
                lo16, hi16 = nr.cast_interval(T, lo, hi)
                got = nr.decode64(T, _bits_nchw(out).cpu())
                ok = nr.inside(got, lo16, hi16)
                print("batch_norm %s relu %d x * 2^%d beta %g: %d elements, %d outside, %d subnormal or zero, %d +-inf allowed" % (
                    T, relu, a, beta, ok.numel(), int((~ok).sum()), int((got.abs() < 2.0 ** (2 - (1 << (nr.EXP_BITS[T] - 1)))).sum()),
                    int(torch.isinf(hi16).sum() + torch.isinf(lo16).sum())))
                assert bool(ok.all()), ("batch_norm %s relu %d 2^%d beta %g" % (T, relu, a, beta), int((~ok).sum()),
                                        [(float(p), float(q), float(r)) for p, q, r in list(zip(got[~ok], lo16[~ok], hi16[~ok]))[:4]])
            except AssertionError as err:
                failed.append(str(err))
    assert not failed, failed


# ---- d. MaxPool2d ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
def test_max_pool_orders_every_finite_pattern_like_torch(T):
    H, W = {"fp16": (16, 62), "bf16": (34, 30)}[T]
    top = nr.inf_bits(T)
    every = torch.cat([torch.arange(top), 32768 + torch.arange(top)])                         # every finite pattern, both signs
    assert every.numel() == 64 * H * W
    g = torch.Generator().manual_seed(17)
    # two images, each every finite pattern once in an order of its own.  The first window of channel 0 holds negative subnormals beside
    # the two zeros, -0 ahead of +0 in one image and behind it in the other: compared as integers the patterns order otherwise
    # (-0 = 0x8000 below every negative value as a signed word, above every positive one as an unsigned word)
    window = [0, 64, W * 64, (W + 1) * 64]                                                    # its four slots in [H][W][C] order
    images = []
    for special in ([0x8001, 0x8000, 0x0000, 0x8002], [0x8002, 0x0000, 0x8000, 0x8001]):
        pats = every[torch.randperm(every.numel(), generator=g)]
        for pos, val in zip(window, special):
            j = int((pats == val).nonzero()[0])
            pats[pos], pats[j] = pats[j].clone(), pats[pos].clone()
        assert pats[window].tolist() == special and torch.equal(torch.sort(pats)[0], torch.sort(every)[0])
        images.append(pats)
    pats = torch.stack(images)
    x16 = nr.from_bits(T, pats).view(2, H, W, 64).permute(0, 3, 1, 2)
    xf = x16.float().requires_grad_(True)
    want = F.max_pool2d(xf, 2, 2)
    assert nr.to_bits(want.detach().to(nr.TYPES[T]))[:, 0, 0, 0].tolist() == [0x8000, 0x0000]   # the first of the equal zeros wins
    go16 = nr.from_bits(T, pats.reshape(-1)[:2 * 64 * (H // 2) * (W // 2)]).view(2, 64, H // 2, W // 2)
    (want_gi,) = torch.autograd.grad(want, xf, go16.float())
    xr, gor = resident(x16, T), resident(go16, T)
    out = torch.full_like(gor, float("nan"))
    code = torch.full((2, H // 2, W // 2, 64), 255, dtype=torch.uint8, device=DEV)
    gi = torch.full_like(xr, float("nan"))
    pool_forward(xr, out, code, (2, 2, 0, 0), T)
    pool_backward(gor, code, gi, (2, 2, 0, 0), T)
    torch.cuda.synchronize()
    assert torch.equal(_bits_nchw(out).cpu(), nr.to_bits(want.detach().to(nr.TYPES[T]))), "forward"
    assert torch.equal(nr.f32_bits(out.float().cpu()), nr.f32_bits(want.detach())), "forward, as fp32"
    assert torch.equal(_bits_nchw(gi).cpu(), nr.to_bits(want_gi.to(nr.TYPES[T]))), "backward"
