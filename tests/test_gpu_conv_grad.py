"""Dense conv2d with gradients (tdrn_hip.h section i-c; Conv2dFunction / conv2d / Conv2d) against torch's CPU autograd in
float64.

Oracle: torch.nn.functional.conv2d on the CPU in float64, differentiated by autograd, fed the exact inputs the op used: in the
16-bit modes input, weight and grad_output are rounded to the type first (bias is not).

Bounds.  fp32 mode: |got - ref| <= 1e-4 * max(1, max|ref|), as in test_gpu_deform_grad.py.  16-bit modes: the inputs are
exact, the products are exact in fp32, so only the fp32 accumulation is left: |got - ref| <= c * S elementwise, S = the same
convolution on absolute values (wgrad: sum_p |GO| |X|; forward: + |bias|), c = C_ACC of test_gpu_pin16.py (2e-6 bf16,
4e-5 fp16).  Outputs are fp32: no output-rounding term, no element is exempted.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from _conv_train_harness import C_ACC, DEV, DT, NAMES, Guarded, check  # noqa: F401
from _conv_train_harness import Abi as _Abi, bits_equal as _bits_equal, round_to as _round
from tdrn_amd.model import networks

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))      # (the float64 references of the deep_* cases: the GPU hosts' threads oversubscribe)

# N, Cin, H, W, Cout, k, pad, dil
CASES = {
    "first_conv_3ch": (1, 3, 8, 8, 4, 3, 1, 1),            # channel padding 3 -> 64
    "odd_two_images": (2, 6, 9, 7, 4, 3, 1, 1),            # H != W, odd sizes, two images
    "tiny_images": (3, 32, 5, 5, 256, 3, 1, 1),            # images smaller than a pixel chunk: padding across image boundaries
    "ragged_tiles": (1, 192, 12, 11, 130, 3, 1, 1),        # several cin and cout tiles, ragged last tile
    "k800": (2, 64, 20, 20, 75, 3, 1, 1),                  # K = 800, no multiple of the chunk
    "dil2": (1, 16, 9, 9, 8, 3, 2, 2),
    "conv6": (1, 16, 13, 13, 24, 3, 6, 6),                 # conv6's geometry: most taps in the padding
    "valid": (1, 8, 10, 9, 8, 3, 0, 1),                    # valid conv: pad' = 2 in dgrad, Ho x Wo = 8 x 7
    "1x1": (2, 140, 6, 6, 12, 1, 0, 1),
    "k6400_split": (4, 64, 40, 40, 64, 3, 1, 1),           # K = 6400: more than one K split (DESIGN 11 lists conv_wgrad_splits = 25)
    # beyond the issue's table
    "full_pad2": (2, 70, 12, 10, 40, 3, 2, 1),             # pad = dil (k - 1): Ho x Wo = 14 x 12 > H x W, pad' = 0 in dgrad, K = 336
    "dil30": (1, 8, 40, 40, 8, 3, 30, 30),                 # a dilation larger than the image: eight of nine taps all padding, K = 1600
    # the kernel variants of a real training step (test_conv_grad_variants.py asserts which one each case reaches).  M = 127 * 127
    # = 63 * 256 + 1 pixels: the last 256-row tile holds one row
    "deep_fwd": (1, 8, 127, 127, 1000, 3, 1, 1),           # forward on the 3-stage 256x128 tile, Cout < Npad = 1024
    "deep_fwd_scalar": (1, 8, 127, 127, 1001, 3, 1, 1),    # ... with o_cs % 4 != 0: the scalar-store epilogue
    "deep_dgrad": (1, 1000, 127, 127, 8, 3, 1, 1),         # the input gradient on 256x128, through the rotated packing
    "deep_1x1": (1, 8, 127, 127, 1000, 1, 0, 1),           # one K-step (16-bit) or two (fp32): fewer than the ring has stages
    "deep_dil6": (1, 8, 127, 127, 1000, 3, 6, 6),          # conv6's geometry on the deep tile: border tiles with dead taps
    "two_big_images": (2, 6, 41, 41, 10, 3, 1, 1),         # 1681 > 1600 pixels an image: batch-major rows, a tile across the image boundary
}
# the autograd test leaves this one to the ABI test: the same kernels through the same wrapper, 3.8 s of float64 reference saved
AUTOGRAD_CASES = [c for c in CASES if c != "deep_fwd_scalar"]
# seeds: the first twelve cases keep the inputs they always had (their rank among themselves), the later ones follow in table order
SEED_ORDER = sorted(list(CASES)[:12]) + list(CASES)[12:]


def _dims(case):
    N, Cin, H, W, Cout, k, pad, dil = CASES[case]
    return (N, Cin, H, W, Cout, k, k, 1, 1, pad, pad, dil, dil)


def _out_hw(case):
    N, Cin, H, W, Cout, k, pad, dil = CASES[case]
    return H + 2 * pad - dil * (k - 1), W + 2 * pad - dil * (k - 1)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    N, Cin, H, W, Cout, k, pad, dil = CASES[case]
    Ho, Wo = _out_hw(case)
    gen = torch.Generator().manual_seed(SEED_ORDER.index(case) + 11)
    x = torch.randn(N, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, k, k, generator=gen) * (Cin * k * k) ** -0.5
    b = torch.randn(Cout, generator=gen)
    go = torch.randn(N, Cout, Ho, Wo, generator=gen)
    return x, w, b, go


@functools.lru_cache(maxsize=None)
def _reference(case, mode):
    """float64 CPU autograd on the inputs as the op uses them -> ((y, gx, gw, gb), (Sy, Sgx, Sgw, Sgb)); computed once, never changed"""
    N, Cin, H, W, Cout, k, pad, dil = CASES[case]
    x, w, b, go = _inputs(case)
    xr, wr, gr = (_round(t, mode).double() for t in (x, w, go))

    def run(xx, ww, bb, gg):
        xx, ww, bb = (t.clone().requires_grad_(True) for t in (xx, ww, bb))
        y = F.conv2d(xx, ww, bb, 1, pad, dil)
        gx, gw, gb = torch.autograd.grad(y, (xx, ww, bb), gg)
        return y.detach(), gx, gw, gb
    return run(xr, wr, b.double(), gr), run(xr.abs(), wr.abs(), b.double().abs(), gr.abs())


def _check(case, mode, names, got):
    check(_reference, case, mode, names, got)


def Abi(case, mode):
    """the four C entries on plain device buffers"""
    return _Abi("tdrn_conv2d", _dims(case), _inputs(case), mode)


@pytest.mark.parametrize("mode", list(DT))
@pytest.mark.parametrize("case", list(CASES))
def test_conv2d_abi_matches_float64_autograd(case, mode):
    _check(case, mode, NAMES, Abi(case, mode).all())


@pytest.mark.parametrize("mode", list(DT))
@pytest.mark.parametrize("case", AUTOGRAD_CASES)
def test_conv2d_autograd_matches_float64_autograd(case, mode):
    N, Cin, H, W, Cout, k, pad, dil = CASES[case]
    x, w, b, go = (t.to(DEV) for t in _inputs(case))
    x, w, b = (t.requires_grad_(True) for t in (x, w, b))
    y = networks.conv2d(x, w, b, padding=pad, dilation=dil, compute=mode)
    y.backward(go)
    _check(case, mode, NAMES, (y, x.grad, w.grad, b.grad))


def test_conv2d_parameter_gradients_accumulate_and_the_rest_is_overwritten():
    a = Abi("k800", "fp32")
    gw, gb = a.backward_parameters(torch.zeros_like(a.w), torch.zeros_like(a.b))
    gw1, gb1 = gw.clone(), gb.clone()
    a.backward_parameters(gw, gb, scale=0.5)
    # fl(g + fl(0.5 s)) against 1.5 g with g = fl(s): two roundings of fp32
    for got, one in ((gw, gw1), (gb, gb1)):
        assert float((got - 1.5 * one).abs().max()) <= 4 * 2.0 ** -24 * float(one.abs().max())
    out = a.forward(torch.full_like(a.go, float("nan")))
    out2 = a.forward(torch.full_like(a.go, float("nan")))
    gi = a.backward_input(torch.full_like(a.x, float("nan")))
    gi2 = a.backward_input(torch.full_like(a.x, float("nan")))
    assert torch.equal(out, out2) and torch.equal(gi, gi2)
    assert bool(torch.isfinite(out2).all()) and bool(torch.isfinite(gi2).all())
    _check("k800", "fp32", ("grad_weight", "grad_bias"), (gw1, gb1))


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_conv2d_is_bitwise_reproducible(mode):
    for case in ("k6400_split", "deep_fwd"):
        a = Abi(case, mode)
        first = [t.clone() for t in a.all()]
        # other work on the device in between must not change the arithmetic
        Abi("ragged_tiles", mode).all()
        second = a.all()
        for name, p, q in zip(NAMES, first, second):
            assert _bits_equal(p, q), (case, name)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", ["ragged_tiles", "odd_two_images", "1x1", "full_pad2", "deep_fwd", "two_big_images"])
def test_conv2d_writes_only_the_callers_buffers(case, mode):
    a = Abi(case, mode)
    want = [t.clone() for t in a.all()]
    ws = Guarded(nbytes=a.nb)                      # exactly the queried size
    a.ws = ws.t
    assert ws.t.data_ptr() % 256 == 0
    out = Guarded(a.go.shape, offset=4)            # 4 bytes behind a 256-byte boundary
    gi = Guarded(a.x.shape, offset=4)
    gw = Guarded(a.w.shape, offset=4, init=torch.zeros_like(a.w))
    gb = Guarded(a.b.shape, offset=4, init=torch.zeros_like(a.b))
    assert out.t.data_ptr() % 256 == 4
    a.forward(out.t)
    a.backward_input(gi.t)
    a.backward_parameters(gw.t, gb.t)
    for name, g, w in zip(NAMES, (out, gi, gw, gb), want):
        g.check("%s %s %s" % (case, mode, name))
        assert _bits_equal(g.t, w), name
    ws.check("%s %s workspace" % (case, mode), full=False)


def test_conv2d_autograd_plumbing():
    case, mode = "odd_two_images", "fp32"
    N, Cin, H, W, Cout, k, pad, dil = CASES[case]
    x0, w0, b0, _ = (t.to(DEV) for t in _inputs(case))
    for need in ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        x, w, b = (t.clone().requires_grad_(n) for t, n in zip((x0, w0, b0), need))
        y = networks.conv2d(x, w, b, padding=pad, dilation=dil, compute=mode)
        assert y.requires_grad
        y.sum().backward()                           # a stride-0 grad_output
        for t, n in zip((x, w, b), need):
            assert (t.grad is not None) == n
    with torch.no_grad():
        assert networks.conv2d(x0.clone().requires_grad_(True), w0, b0, padding=pad).grad_fn is None
    assert networks.conv2d(x0, w0, b0, padding=pad).grad_fn is None
    # the gradient of sum(y), and bias=None
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y = networks.conv2d(x, w, None, padding=pad, dilation=dil, compute=mode)
    y.sum().backward()
    xr, wr = x0.cpu().double().requires_grad_(True), w0.cpu().double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, 1, pad, dil)
    yr.sum().backward()
    for got, ref in ((y, yr), (x.grad, xr.grad), (w.grad, wr.grad)):
        assert float((got.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))
    # geometry the ABI rejects raises (no fallback): stride is not even an argument, k = 5 is refused
    with pytest.raises(RuntimeError):
        networks.conv2d(x0, torch.zeros(Cout, Cin, 5, 5, device=DEV), None, padding=2)
    # a module left on the CPU: its parameters must not reach the library as host pointers
    with pytest.raises(NotImplementedError):
        networks.Conv2d(Cin, Cout, 3, padding=1)(x0)
    m = networks.Conv2d(Cin, Cout, 3, padding=1).to(DEV)
    m(x0).mean().backward()
    assert m.weight.grad is not None and m.bias.grad is not None


def test_conv2d_short_training_run_follows_float64():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 10, 10, generator=gen)
    target = torch.randn(2, 8, 10, 10, generator=gen)
    w1 = torch.randn(32, 16, 3, 3, generator=gen) * (16 * 9) ** -0.5
    b1 = torch.randn(32, generator=gen) * 0.1
    w2 = torch.randn(8, 32, 1, 1, generator=gen) * 32 ** -0.5
    b2 = torch.randn(8, generator=gen) * 0.1

    def loop(params, x, target, conv):
        losses = []
        for _ in range(3):
            h = torch.relu(conv(x, params[0], params[1], 1))
            loss = ((conv(h, params[2], params[3], 0) - target) ** 2).mean()
            grads = torch.autograd.grad(loss, params)
            with torch.no_grad():
                for p, g in zip(params, grads):
                    p -= 0.5 * g
            losses.append(float(loss))
        return losses

    ours = [t.clone().to(DEV).requires_grad_(True) for t in (w1, b1, w2, b2)]
    ref = [t.clone().double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    l_ours = loop(ours, x.to(DEV), target.to(DEV), lambda i, w, b, p: networks.conv2d(i, w, b, padding=p, compute="fp32"))
    l_ref = loop(ref, x.double(), target.double(), lambda i, w, b, p: F.conv2d(i, w, b, 1, p))
    assert l_ours[0] > l_ours[1] > l_ours[2], l_ours
    assert l_ref[0] > l_ref[1] > l_ref[2], l_ref
    for p, r in zip(ours, ref):
        d = float((p.detach().cpu().double() - r.detach()).abs().max())
        assert d <= 1e-4 * max(1.0, float(r.abs().max())), d
