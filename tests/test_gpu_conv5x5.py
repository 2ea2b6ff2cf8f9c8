"""The dense 5x5 conv with gradients (tdrn_hip.h section i-i; Conv5x5Function / conv5x5 / Conv5x5) against torch's CPU autograd in
float64.

Oracle: torch.nn.functional.conv2d(x, w, b, padding=2) on the CPU in float64, differentiated by autograd, fed the exact inputs the op
used: in the 16-bit modes input, weight and grad_output are rounded to the type first (bias is not).

Bounds, the project's own (_conv_train_harness.py), unchanged.  fp32 mode: |got - ref| <= 1e-4 * max(1, max|ref|).  16-bit modes:
|got - ref| <= c * S elementwise, S = the same op on absolute values, c = C_ACC (2e-6 bf16, 4e-5 fp16).  No element is exempted.

What each case is in the suite for is asserted without a GPU in test_conv5x5_abi.py.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from _conv_train_harness import DEV, DT, NAMES, Guarded, check
from _conv_train_harness import Abi as _Abi, bits_equal as _bits_equal, round_to as _round
from tdrn_amd.model import networks

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

# N, Cin, H, W, Cout
CASES = {
    "one_pixel": (2, 6, 1, 1, 12),             # 24 of the 25 taps, and four of the five kernel rows, lie in the padding
    "two_by_two": (3, 70, 2, 2, 12),           # the kernel is larger than the image; two cin tiles
    "three_by_three": (2, 6, 3, 3, 63),        # no pixel sees the whole kernel
    "five_n3": (3, 6, 5, 5, 75),               # 25 pixels per image: a 64-pixel wgrad chunk crosses two image boundaries; two cout tiles
    "odd_sizes": (1, 6, 7, 9, 75),             # not square
    "m800": (2, 64, 20, 20, 12),               # K = 800: the last split holds half a chunk
    "k_split": (4, 64, 40, 40, 64),            # K = 6400: 25 K splits
    # odm_loc_2 / odm_conf_2 (21 classes) on the pyramid of a 192 px frame, batch 2
    "loc_24": (2, 256, 24, 24, 12), "loc_12": (2, 256, 12, 12, 12), "loc_6": (2, 256, 6, 6, 12), "loc_3": (2, 256, 3, 3, 12),
    "conf_24": (2, 256, 24, 24, 63), "conf_12": (2, 256, 12, 12, 63), "conf_6": (2, 256, 6, 6, 63), "conf_3": (2, 256, 3, 3, 63),
}


def _dims(case):
    N, Cin, H, W, Cout = CASES[case]
    return (N, Cin, H, W, Cout, 5, 5, 1, 1, 2, 2, 1, 1)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    N, Cin, H, W, Cout = CASES[case]
    gen = torch.Generator().manual_seed(list(CASES).index(case) + 501)
    x = torch.randn(N, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 5, 5, generator=gen) * (25 * Cin) ** -0.5
    b = torch.randn(Cout, generator=gen)
    go = torch.randn(N, Cout, H, W, generator=gen)
    return x, w, b, go


@functools.lru_cache(maxsize=None)
def _reference(case, mode):
    """float64 CPU autograd on the inputs as the op uses them -> ((y, gx, gw, gb), (Sy, Sgx, Sgw, Sgb)); computed once, never changed"""
    x, w, b, go = _inputs(case)
    xr, wr, gr = (_round(t, mode).double() for t in (x, w, go))

    def run(xx, ww, bb, gg):
        xx, ww, bb = (t.clone().requires_grad_(True) for t in (xx, ww, bb))
        y = F.conv2d(xx, ww, bb, padding=2)
        gx, gw, gb = torch.autograd.grad(y, (xx, ww, bb), gg)
        return y.detach(), gx, gw, gb
    return run(xr, wr, b.double(), gr), run(xr.abs(), wr.abs(), b.double().abs(), gr.abs())


def _check(case, mode, names, got):
    check(_reference, case, mode, names, got)


def Abi(case, mode):
    """the four C entries on plain device buffers"""
    return _Abi("tdrn_conv5x5", _dims(case), _inputs(case), mode)


# 1. the four C entries, every case x type
@pytest.mark.parametrize("mode", list(DT))
@pytest.mark.parametrize("case", list(CASES))
def test_conv5x5_abi_matches_float64_autograd(case, mode):
    _check(case, mode, NAMES, Abi(case, mode).all())


# 2. scale and accumulation, bias / no bias, grad_bias NULL
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_conv5x5_parameter_gradients_accumulate_bitwise(mode):
    a = Abi("m800", mode)
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


# 3. autograd: the raw entries' bits, every needs_input_grad mask, a stride-0 grad_output, the module
@pytest.mark.parametrize("mode", list(DT))
@pytest.mark.parametrize("case", ["five_n3", "m800", "conf_6"])
def test_conv5x5_autograd_equals_the_raw_entries_bitwise(case, mode):
    want = Abi(case, mode).all()
    x, w, b, go = (t.to(DEV) for t in _inputs(case))
    x, w, b = (t.requires_grad_(True) for t in (x, w, b))
    y = networks.conv5x5(x, w, b, compute=mode)
    y.backward(go)
    for name, p, q in zip(NAMES, want, (y.detach(), x.grad, w.grad, b.grad)):
        assert _bits_equal(p, q), (case, mode, name)
    _check(case, mode, NAMES, (y, x.grad, w.grad, b.grad))


def test_conv5x5_autograd_plumbing():
    case, mode = "five_n3", "fp32"
    N, Cin, H, W, Cout = CASES[case]
    x0, w0, b0, go0 = (t.to(DEV) for t in _inputs(case))
    for need in ((True, True, True), (True, False, False), (False, True, True), (False, True, False), (False, False, True),
                 (True, True, False), (True, False, True)):
        x, w, b = (t.clone().requires_grad_(n) for t, n in zip((x0, w0, b0), need))
        y = networks.conv5x5(x, w, b, mode)
        assert y.requires_grad
        y.backward(go0)
        for t, n, name in zip((x, w, b), need, NAMES[1:]):
            assert (t.grad is not None) == n
            if n:
                _check(case, mode, (name,), (t.grad,))
    with torch.no_grad():
        assert networks.conv5x5(x0.clone().requires_grad_(True), w0, b0).grad_fn is None
    assert networks.conv5x5(x0, w0, b0).grad_fn is None
    # no bias; a stride-0 grad_output (sum().backward())
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y = networks.conv5x5(x, w, None, compute=mode)
    y.sum().backward()
    xr, wr = x0.cpu().double().requires_grad_(True), w0.cpu().double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, padding=2)
    yr.sum().backward()
    for got, want in ((y.detach(), yr.detach()), (x.grad, xr.grad), (w.grad, wr.grad)):
        assert float((got.cpu().double() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    # the module: nn.Conv2d's parameters, the same arithmetic
    m = networks.Conv5x5(Cin, Cout).to(DEV)
    m.load_state_dict(torch.nn.Conv2d(Cin, Cout, 5, padding=2).state_dict())
    with torch.no_grad():
        m.weight.copy_(w0)
        m.bias.copy_(b0)
    x = x0.clone().requires_grad_(True)
    y = m(x)
    y.backward(go0)
    _check(case, mode, NAMES, (y, x.grad, m.weight.grad, m.bias.grad))
    # another weight shape raises and names what is covered; conv2d keeps refusing 5x5; nothing falls back
    with pytest.raises(RuntimeError, match="kernel 5 x 5, stride 1, padding 2"):
        networks.conv5x5(x0, torch.zeros(Cout, Cin, 3, 3, device=DEV), b0)
    with pytest.raises(RuntimeError, match="outside what libtdrn_hip covers"):
        networks.conv2d(x0, w0, b0, padding=2)
    with pytest.raises(NotImplementedError):
        networks.Conv5x5(Cin, Cout)(x0)                 # a module left on the CPU


# 4. bitwise reproducibility, caller buffers 4 / 8 / 12 bytes behind a 256-byte boundary, the workspace exactly as queried and full
# of NaN bytes
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case,offset", [("one_pixel", 4), ("five_n3", 8), ("m800", 12), ("conf_12", 4), ("loc_3", 12)])
def test_conv5x5_is_bitwise_reproducible_on_any_callers_buffers(case, offset, mode):
    a = Abi(case, mode)
    want = [t.clone() for t in a.all()]
    Abi("two_by_two", mode).all()                  # other work on the device in between must not change the arithmetic
    for name, p, q in zip(NAMES, want, a.all()):
        assert _bits_equal(p, q), (case, name, "second run")
    ws = Guarded(nbytes=a.nb)
    assert ws.t.data_ptr() % 256 == 0
    ws.t.fill_(0xFF)
    ins = [Guarded(t.shape, offset=offset, init=t) for t in (a.x, a.w, a.b, a.go)]
    a.ws = ws.t
    a.x, a.w, a.b, a.go = (g.t for g in ins)
    out, gi = Guarded(a.go.shape, offset=offset), Guarded(a.x.shape, offset=offset)
    gw = Guarded(a.w.shape, offset=offset, init=torch.zeros_like(a.w))
    gb = Guarded(a.b.shape, offset=offset, init=torch.zeros_like(a.b))
    assert all(g.t.data_ptr() % 256 == offset for g in ins + [out, gi, gw, gb])
    a.backward_input(gi.t)
    a.forward(out.t)
    a.backward_parameters(gw.t, gb.t)
    for name, g, w in zip(NAMES, (out, gi, gw, gb), want):
        g.check("%s %s %s" % (case, mode, name))
        assert _bits_equal(g.t, w), (case, name, "buffers %d bytes behind a boundary" % offset)
    for name, g in zip(("input", "weight", "bias", "grad_output"), ins):
        g.check("%s %s %s" % (case, mode, name))
    ws.check("%s %s workspace" % (case, mode), full=False)


# 5. no allocation, no synchronisation: the three entries captured on a side stream and replayed once, in a fresh child process
# (tests/_conv5x5_graph_worker.py says why), which is what this test is about
def test_conv5x5_replays_under_graph_capture():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_conv5x5_graph_worker.py"), "bf16", "fp32"], cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, "rc %d\n%s\n%s" % (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-4000:])
    assert p.stdout.decode().split("\n")[:2] == ["replayed bf16", "replayed fp32"]
