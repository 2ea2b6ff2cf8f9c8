"""The dense 3x3 stride-2 conv with gradients (tdrn_hip.h section i-g; the `stride` argument of Conv2dFunction / conv2d / Conv2d)
against torch's CPU autograd in float64.

Oracle: torch.nn.functional.conv2d(x, w, b, 2, pad) on the CPU in float64, differentiated by autograd, fed the exact inputs the op
used: in the 16-bit modes input, weight and grad_output are rounded to the type first (bias is not).

Bounds, the project's own (test_gpu_conv_grad.py), unchanged.  fp32 mode: |got - ref| <= 1e-4 * max(1, max|ref|).  16-bit modes: the
inputs are exact and the products are exact in fp32, so only the fp32 accumulation is left: |got - ref| <= c * S elementwise, S = the
same op on absolute values, c = C_ACC of test_gpu_pin16.py (2e-6 bf16, 4e-5 fp16).  Outputs are fp32: no element is exempted.

Which kernel variant each case reaches is asserted without a GPU in test_conv_strided_abi.py.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from _conv_train_harness import C_ACC, DEV, DT, NAMES, Guarded, check  # noqa: F401
from _conv_train_harness import Abi as _Abi, bits_equal as _bits_equal, round_to as _round
from tdrn_amd.model import networks

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

# N, Cin, H, W, Cout, pad
CASES = {
    "odd_sizes": (2, 6, 9, 7, 4, 1),           # odd sizes; 20 pixels per image, so a 64-pixel wgrad chunk crosses images
    "even_sizes": (1, 70, 8, 6, 40, 1),        # even sizes; two cin tiles; the bottom pad row is unused
    "pad0_untouched": (2, 8, 8, 6, 8, 0),      # the last input row and column are touched by no output: grad_input there is exactly 0
    "pad2_a": (2, 8, 8, 7, 8, 2),              # Hd > H
    "pad2_b": (1, 8, 9, 6, 8, 2),
    "one_pixel_a": (3, 70, 2, 2, 40, 1),       # 1 x 1 outputs
    "one_pixel_b": (1, 8, 3, 3, 8, 0),
    "mobilenet_first": (2, 3, 32, 32, 32, 1),  # MobileNet's first conv, Cin = 3
    "extras": (2, 256, 10, 10, 512, 1),        # the extras layer; forward and dgrad split-K
    "k_split": (4, 64, 40, 40, 64, 1),         # K = 1600: several wgrad splits
    "k_ragged": (2, 64, 41, 37, 20, 1),        # K = 798: ragged last split; Cout = 20 leaves 44 padded channels in its tile
    "odd_wo": (1, 8, 5, 13, 10, 1),            # odd Wo: the dword path of the dilate kernel; Cout % 4 != 0: the scalar epilogue
}


def _out_hw(case):
    N, Cin, H, W, Cout, pad = CASES[case]
    return (H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1


def _dims(case):
    N, Cin, H, W, Cout, pad = CASES[case]
    return (N, Cin, H, W, Cout, 3, 3, 2, 2, pad, pad, 1, 1)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    N, Cin, H, W, Cout, pad = CASES[case]
    Ho, Wo = _out_hw(case)
    gen = torch.Generator().manual_seed(list(CASES).index(case) + 301)
    x = torch.randn(N, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * (9 * Cin) ** -0.5
    b = torch.randn(Cout, generator=gen)
    go = torch.randn(N, Cout, Ho, Wo, generator=gen)
    return x, w, b, go


@functools.lru_cache(maxsize=None)
def _reference(case, mode):
    """float64 CPU autograd on the inputs as the op uses them -> ((y, gx, gw, gb), (Sy, Sgx, Sgw, Sgb)); computed once, never changed"""
    pad = CASES[case][5]
    x, w, b, go = _inputs(case)
    xr, wr, gr = (_round(t, mode).double() for t in (x, w, go))

    def run(xx, ww, bb, gg):
        xx, ww, bb = (t.clone().requires_grad_(True) for t in (xx, ww, bb))
        y = F.conv2d(xx, ww, bb, 2, pad)
        gx, gw, gb = torch.autograd.grad(y, (xx, ww, bb), gg)
        return y.detach(), gx, gw, gb
    return run(xr, wr, b.double(), gr), run(xr.abs(), wr.abs(), b.double().abs(), gr.abs())


def _check(case, mode, names, got):
    check(_reference, case, mode, names, got)


def Abi(case, mode):
    """the four C entries on plain device buffers"""
    return _Abi("tdrn_conv2d_strided", _dims(case), _inputs(case), mode)


# 1. the four C entries, every case x type
@pytest.mark.parametrize("mode", list(DT))
@pytest.mark.parametrize("case", list(CASES))
def test_conv2d_strided_abi_matches_float64_autograd(case, mode):
    got = Abi(case, mode).all()
    _check(case, mode, NAMES, got)
    if case == "pad0_untouched":
        # input row 7 and column 5 lie under no window (Ho = 3 covers rows 0..6, Wo = 2 columns 0..4): exact zeros, any sign bit
        gi = got[1]
        assert float(gi[:, :, 7, :].abs().max()) == 0.0 and float(gi[:, :, :, 5].abs().max()) == 0.0
        assert float(gi[:, :, :7, :5].abs().min()) > 0.0


# 2. scale and accumulation
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_conv2d_strided_parameter_gradients_accumulate_bitwise(mode):
    a = Abi("k_ragged", mode)
    g_w, g_b = a.backward_parameters(torch.zeros_like(a.w), torch.zeros_like(a.b))
    gen = torch.Generator().manual_seed(7)
    old_w, old_b = torch.randn(a.w.shape, generator=gen).to(DEV), torch.randn(a.b.shape, generator=gen).to(DEV)
    got_w, got_b = a.backward_parameters(old_w.clone(), old_b.clone(), scale=0.5)
    # one fused multiply-add per element: fl(old + 0.5 s) with g = s exactly (scale 1 into zeros) and 0.5 g exact
    assert _bits_equal(got_w, old_w + 0.5 * g_w) and _bits_equal(got_b, old_b + 0.5 * g_b)
    assert float((got_w - old_w).abs().max()) > 0 and float((got_b - old_b).abs().max()) > 0
    # without a bias gradient the weight gradient keeps its bits
    only_w, none = a.backward_parameters(torch.zeros_like(a.w), None)
    assert none is None and _bits_equal(only_w, g_w)
    # bias = NULL is a zero bias: the two forwards differ by the bias, up to the one rounding of the sum
    no_bias = a.forward(torch.full_like(a.go, float("nan")), bias=False)
    with_bias = a.forward(torch.full_like(a.go, float("nan")))
    assert float((with_bias - no_bias - a.b.view(1, -1, 1, 1)).abs().max()) <= 4 * 2.0 ** -24 * float(with_bias.abs().max())


# 3. autograd
@pytest.mark.parametrize("mode", list(DT))
@pytest.mark.parametrize("case", ["odd_sizes", "pad2_a", "extras", "k_ragged"])
def test_conv2d_stride2_autograd_matches_float64_autograd(case, mode):
    pad = CASES[case][5]
    x, w, b, go = (t.to(DEV) for t in _inputs(case))
    x, w, b = (t.requires_grad_(True) for t in (x, w, b))
    y = networks.conv2d(x, w, b, padding=pad, compute=mode, stride=2)
    y.backward(go)
    _check(case, mode, NAMES, (y, x.grad, w.grad, b.grad))


def test_conv2d_stride2_autograd_plumbing():
    case, mode = "odd_sizes", "fp32"
    N, Cin, H, W, Cout, pad = CASES[case]
    x0, w0, b0, go0 = (t.to(DEV) for t in _inputs(case))
    for need in ((True, True, True), (True, False, False), (False, True, True), (False, True, False), (False, False, True),
                 (True, True, False), (True, False, True)):
        x, w, b = (t.clone().requires_grad_(n) for t, n in zip((x0, w0, b0), need))
        y = networks.conv2d(x, w, b, pad, 1, mode, (2, 2))
        assert y.requires_grad
        y.backward(go0)
        for t, n, name in zip((x, w, b), need, NAMES[1:]):
            assert (t.grad is not None) == n
            if n:
                _check(case, mode, (name,), (t.grad,))
    with torch.no_grad():
        assert networks.conv2d(x0.clone().requires_grad_(True), w0, b0, pad, stride=2).grad_fn is None
    assert networks.conv2d(x0, w0, b0, pad, stride=2).grad_fn is None
    # no bias; a stride-0 grad_output (sum().backward())
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y = networks.conv2d(x, w, None, pad, compute=mode, stride=2)
    y.sum().backward()
    xr, wr = x0.cpu().double().requires_grad_(True), w0.cpu().double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, 2, pad)
    yr.sum().backward()
    for got, want in ((y.detach(), yr.detach()), (x.grad, xr.grad), (w.grad, wr.grad)):
        assert float((got.cpu().double() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    # the module: nn.Conv2d's parameters, the same arithmetic
    m = networks.Conv2d(Cin, Cout, 3, padding=pad, stride=2).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w0)
        m.bias.copy_(b0)
    x = x0.clone().requires_grad_(True)
    y = m(x)
    y.backward(go0)
    _check(case, mode, NAMES, (y, x.grad, m.weight.grad, m.bias.grad))
    # geometry the library refuses raises; nothing falls back
    for kw in (dict(stride=3), dict(stride=(2, 1)), dict(stride=2, dilation=2, padding=2), dict(stride=2, padding=3)):
        with pytest.raises(RuntimeError, match="outside what libtdrn_hip covers"):
            networks.conv2d(x0, w0, b0, **dict(dict(padding=pad), **kw))
    with pytest.raises(RuntimeError, match="outside what libtdrn_hip covers"):
        networks.conv2d(x0, torch.zeros(Cout, Cin, 1, 1, device=DEV), b0, stride=2)          # k = 1 at stride 2
    with pytest.raises(NotImplementedError):
        networks.Conv2d(Cin, Cout, 3, padding=pad, stride=2)(x0)             # a module left on the CPU


def test_stride1_through_the_keyword_keeps_its_bits():
    gen = torch.Generator().manual_seed(11)
    x0, w0, b0 = torch.randn(2, 6, 9, 7, generator=gen).to(DEV), torch.randn(4, 6, 3, 3, generator=gen).to(DEV), torch.randn(4, generator=gen).to(DEV)
    go = torch.randn(2, 4, 9, 7, generator=gen).to(DEV)
    runs = []
    for call in (lambda x, w, b: networks.conv2d(x, w, b, 1, 1, "bf16"), lambda x, w, b: networks.conv2d(x, w, b, 1, 1, "bf16", stride=1),
                 lambda x, w, b: networks.conv2d(x, w, b, 1, 1, "bf16", (1, 1)),
                 lambda x, w, b: networks.Conv2dFunction.apply(x, w, b, 1, 1, "bf16")):
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        y = call(x, w, b)
        y.backward(go)
        runs.append((y.detach(), x.grad, w.grad, b.grad))
    for r in runs[1:]:
        for p, q in zip(runs[0], r):
            assert _bits_equal(p, q)


# 4. bitwise reproducibility, caller buffers on any 4-byte boundary, the workspace exactly as queried and full of NaN bytes
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", ["odd_sizes", "pad0_untouched", "pad2_a", "extras", "k_ragged", "odd_wo"])
def test_conv2d_strided_is_bitwise_reproducible_on_any_callers_buffers(case, mode):
    a = Abi(case, mode)
    want = [t.clone() for t in a.all()]
    Abi("one_pixel_a", mode).all()                 # other work on the device in between must not change the arithmetic
    for name, p, q in zip(NAMES, want, a.all()):
        assert _bits_equal(p, q), (case, name, "second run")
    # every caller tensor 4 bytes behind a 256-byte boundary; the workspace exactly the queried size, pre-filled with 0xFF bytes (a
    # NaN in fp32, bf16 and fp16 alike: a zero of the dilated image that the kernel did not store itself would poison grad_input),
    # guard bands all round
    ws = Guarded(nbytes=a.nb)
    assert ws.t.data_ptr() % 256 == 0
    ws.t.fill_(0xFF)
    ins = [Guarded(t.shape, offset=4, init=t) for t in (a.x, a.w, a.b, a.go)]
    a.ws = ws.t
    a.x, a.w, a.b, a.go = (g.t for g in ins)
    out, gi = Guarded(a.go.shape, offset=4), Guarded(a.x.shape, offset=4)
    gw, gb = Guarded(a.w.shape, offset=4, init=torch.zeros_like(a.w)), Guarded(a.b.shape, offset=4, init=torch.zeros_like(a.b))
    assert all(g.t.data_ptr() % 256 == 4 for g in ins + [out, gi, gw, gb])
    # backward_input first: the dilated image is then built on the untouched NaN bytes
    a.backward_input(gi.t)
    a.forward(out.t)
    a.backward_parameters(gw.t, gb.t)
    for name, g, w in zip(NAMES, (out, gi, gw, gb), want):
        g.check("%s %s %s" % (case, mode, name))
        assert _bits_equal(g.t, w), (case, name, "buffers on a 4-byte boundary")
    for name, g in zip(("input", "weight", "bias", "grad_output"), ins):
        g.check("%s %s %s" % (case, mode, name))
    ws.check("%s %s workspace" % (case, mode), full=False)


# 5. no allocation, no synchronisation: the three entries captured on a side stream, one stream, no parallel branches
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_conv2d_strided_replays_under_graph_capture(mode):
    a = Abi("extras", mode)
    want = [t.clone() for t in a.all()]
    out, gi = torch.full_like(a.go, float("nan")), torch.full_like(a.x, float("nan"))
    gw, gb = torch.zeros_like(a.w), torch.zeros_like(a.b)

    def work():
        gw.zero_()
        gb.zero_()
        a.forward(out)
        a.backward_input(gi)
        a.backward_parameters(gw, gb)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()                                     # warm-up on the side stream: lazy initialisation happens outside the capture
    side.synchronize()
    for name, p, q in zip(NAMES, want, (out, gi, gw, gb)):
        assert _bits_equal(p, q), (name, "side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        work()
    for k in range(2):
        out.fill_(float("nan"))
        gi.fill_(float("nan"))
        a.ws.fill_(0xFF)                           # NaN bytes in every type: the entries write what they read on every replay
        graph.replay()
        torch.cuda.synchronize()
        for name, p, q in zip(NAMES, want, (out, gi, gw, gb)):
            assert _bits_equal(p, q), (name, "replay %d" % k)
    del graph
