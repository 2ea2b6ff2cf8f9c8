"""ConvTranspose2d(kernel 2, stride 2) with gradients (tdrn_hip.h section i-f; ConvTranspose2dFunction / conv_transpose2d /
ConvTranspose2d) against torch's CPU autograd in float64.

Oracle: torch.nn.functional.conv_transpose2d(x, w, b, 2) on the CPU in float64, differentiated by autograd, fed the exact inputs the
op used: in the 16-bit modes input, weight and grad_output are rounded to the type first (bias is not).

Bounds, the project's own (test_gpu_conv_grad.py).  fp32 mode: |got - ref| <= 1e-4 * max(1, max|ref|).  16-bit modes: the inputs are
exact and the products are exact in fp32, so only the fp32 accumulation is left: |got - ref| <= c * S elementwise, S = the same op
on absolute values, c = C_ACC of test_gpu_pin16.py (2e-6 bf16, 4e-5 fp16).  Outputs are fp32: no element is exempted.

Which kernel variant each case reaches is asserted without a GPU in test_conv_transpose_abi.py.
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

# N, Cin, H, W, Cout
CASES = {
    "tcb_small": (2, 256, 5, 5, 256),          # the real channels; the input gradient runs split-K
    "odd_ragged": (2, 6, 5, 7, 10),            # channel padding; Cout % 4 != 0: the scalar epilogue with phases; odd W: dword loads
    "one_pixel": (3, 70, 1, 1, 40),            # M = 3
    "ragged_tiles": (1, 192, 6, 5, 130),       # several cin tiles; padding rows inside each phase block; 4 CoPad = 768
    "k_split": (4, 64, 20, 20, 64),            # several wgrad splits; two 16-pixel tiles a row
    "k_ragged": (2, 64, 21, 19, 20),           # M = 798, a short last split
    "splitk_fwd": (2, 512, 5, 5, 64),          # forward split-K through four phases
    "deep_fwd": (1, 8, 23, 167, 1000),         # M = 3841; the 3-stage tile with phases and columns past Cout
}


def _dims(case):
    N, Cin, H, W, Cout = CASES[case]
    return (N, Cin, H, W, Cout, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    N, Cin, H, W, Cout = CASES[case]
    gen = torch.Generator().manual_seed(list(CASES).index(case) + 101)
    x = torch.randn(N, Cin, H, W, generator=gen)
    w = torch.randn(Cin, Cout, 2, 2, generator=gen) * Cin ** -0.5
    b = torch.randn(Cout, generator=gen)
    go = torch.randn(N, Cout, 2 * H, 2 * W, generator=gen)
    return x, w, b, go


@functools.lru_cache(maxsize=None)
def _reference(case, mode):
    """float64 CPU autograd on the inputs as the op uses them -> ((y, gx, gw, gb), (Sy, Sgx, Sgw, Sgb)); computed once, never changed"""
    x, w, b, go = _inputs(case)
    xr, wr, gr = (_round(t, mode).double() for t in (x, w, go))

    def run(xx, ww, bb, gg):
        xx, ww, bb = (t.clone().requires_grad_(True) for t in (xx, ww, bb))
        y = F.conv_transpose2d(xx, ww, bb, 2)
        gx, gw, gb = torch.autograd.grad(y, (xx, ww, bb), gg)
        return y.detach(), gx, gw, gb
    return run(xr, wr, b.double(), gr), run(xr.abs(), wr.abs(), b.double().abs(), gr.abs())


def _check(case, mode, names, got):
    check(_reference, case, mode, names, got)


def Abi(case, mode):
    """the four C entries on plain device buffers"""
    return _Abi("tdrn_conv_transpose2d", _dims(case), _inputs(case), mode)


# 1. the four C entries, every case x type
@pytest.mark.parametrize("mode", list(DT))
@pytest.mark.parametrize("case", list(CASES))
def test_conv_transpose2d_abi_matches_float64_autograd(case, mode):
    _check(case, mode, NAMES, Abi(case, mode).all())


# 2. scale and accumulation
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_conv_transpose2d_parameter_gradients_accumulate_bitwise(mode):
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
@pytest.mark.parametrize("case", ["tcb_small", "odd_ragged", "ragged_tiles", "k_ragged"])
def test_conv_transpose2d_autograd_matches_float64_autograd(case, mode):
    x, w, b, go = (t.to(DEV) for t in _inputs(case))
    x, w, b = (t.requires_grad_(True) for t in (x, w, b))
    y = networks.conv_transpose2d(x, w, b, compute=mode)
    y.backward(go)
    _check(case, mode, NAMES, (y, x.grad, w.grad, b.grad))


def test_conv_transpose2d_autograd_plumbing():
    case, mode = "odd_ragged", "fp32"
    N, Cin, H, W, Cout = CASES[case]
    x0, w0, b0, go0 = (t.to(DEV) for t in _inputs(case))
    ref = _reference(case, mode)[0]
    for need in ((True, True, True), (True, False, False), (False, True, True), (False, True, False), (False, False, True)):
        x, w, b = (t.clone().requires_grad_(n) for t, n in zip((x0, w0, b0), need))
        y = networks.conv_transpose2d(x, w, b, compute=mode)
        assert y.requires_grad
        y.backward(go0)
        for t, n, name in zip((x, w, b), need, NAMES[1:]):
            assert (t.grad is not None) == n
            if n:
                _check(case, mode, (name,), (t.grad,))
    with torch.no_grad():
        assert networks.conv_transpose2d(x0.clone().requires_grad_(True), w0, b0).grad_fn is None
    assert networks.conv_transpose2d(x0, w0, b0).grad_fn is None
    # no bias; a stride-0 grad_output (sum().backward())
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y = networks.conv_transpose2d(x, w, None, compute=mode)
    y.sum().backward()
    xr, wr = x0.cpu().double().requires_grad_(True), w0.cpu().double().requires_grad_(True)
    yr = F.conv_transpose2d(xr, wr, None, 2)
    yr.sum().backward()
    for got, want in ((y.detach(), yr.detach()), (x.grad, xr.grad), (w.grad, wr.grad)):
        assert float((got.cpu().double() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    # a non-contiguous input and a non-contiguous grad_output: the values count, not the strides
    xt = x0.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    got = go0.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not xt.is_contiguous() and not got.is_contiguous()
    w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    y = networks.conv_transpose2d(xt, w, b, compute=mode)
    y.backward(got)
    _check(case, mode, NAMES, (y, xt.grad, w.grad, b.grad))
    # the module: nn.ConvTranspose2d's parameters, the same arithmetic
    m = networks.ConvTranspose2d(Cin, Cout, 2, 2).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w0)
        m.bias.copy_(b0)
    x = x0.clone().requires_grad_(True)
    y = m(x)
    y.backward(go0)
    _check(case, mode, NAMES, (y, x.grad, m.weight.grad, m.bias.grad))
    # geometry the library refuses raises and names what is covered; nothing falls back
    for bad in (networks.ConvTranspose2d(Cin, Cout, 3, 2).to(DEV), networks.ConvTranspose2d(Cin, Cout, 2, 1).to(DEV),
                networks.ConvTranspose2d(Cin, Cout, 2, 2, padding=1).to(DEV)):
        with pytest.raises(RuntimeError, match="kernel 2 x 2, stride 2"):
            bad(x0)
    with pytest.raises(RuntimeError, match="stride 2"):
        networks.conv_transpose2d(x0, w0, b0, stride=1)
    with pytest.raises(NotImplementedError):
        networks.ConvTranspose2d(Cin, Cout)(x0)             # a module left on the CPU


# 4. bitwise reproducibility, caller buffers on any 4-byte boundary, the workspace exactly as queried
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", ["tcb_small", "odd_ragged", "ragged_tiles", "k_split", "deep_fwd"])
def test_conv_transpose2d_is_bitwise_reproducible_on_any_callers_buffers(case, mode):
    a = Abi(case, mode)
    want = [t.clone() for t in a.all()]
    Abi("one_pixel", mode).all()                   # other work on the device in between must not change the arithmetic
    for name, p, q in zip(NAMES, want, a.all()):
        assert _bits_equal(p, q), (case, name, "second run")
    # every caller tensor 4 bytes behind a 256-byte boundary, the workspace exactly the queried size, guard bands all round
    ws = Guarded(nbytes=a.nb)
    assert ws.t.data_ptr() % 256 == 0
    ins = [Guarded(t.shape, offset=4, init=t) for t in (a.x, a.w, a.b, a.go)]
    a.ws = ws.t
    a.x, a.w, a.b, a.go = (g.t for g in ins)
    out, gi = Guarded(a.go.shape, offset=4), Guarded(a.x.shape, offset=4)
    gw, gb = Guarded(a.w.shape, offset=4, init=torch.zeros_like(a.w)), Guarded(a.b.shape, offset=4, init=torch.zeros_like(a.b))
    assert all(g.t.data_ptr() % 256 == 4 for g in ins + [out, gi, gw, gb])
    a.forward(out.t)
    a.backward_input(gi.t)
    a.backward_parameters(gw.t, gb.t)
    for name, g, w in zip(NAMES, (out, gi, gw, gb), want):
        g.check("%s %s %s" % (case, mode, name))
        assert _bits_equal(g.t, w), (case, name, "buffers on a 4-byte boundary")
    for name, g in zip(("input", "weight", "bias", "grad_output"), ins):
        g.check("%s %s %s" % (case, mode, name))
    ws.check("%s %s workspace" % (case, mode), full=False)


# 5. a TCB block of the library's own ops
def test_tcb_block_matches_float64_autograd():
    gen = torch.Generator().manual_seed(23)
    C = 256
    trans, top = torch.randn(2, C, 10, 10, generator=gen), torch.randn(2, C, 5, 5, generator=gen)
    w1, w2 = (torch.randn(C, C, 3, 3, generator=gen) * (9 * C) ** -0.5 for _ in range(2))
    wu = torch.randn(C, C, 2, 2, generator=gen) * C ** -0.5
    b1, bu, b2 = (torch.randn(C, generator=gen) * 0.1 for _ in range(3))
    go = torch.randn(2, C, 10, 10, generator=gen)
    leaves = (trans, top, w1, b1, wu, bu, w2, b2)

    def block(t, conv, convt):
        trans, top, w1, b1, wu, bu, w2, b2 = t
        return conv(torch.relu(conv(trans, w1, b1) + convt(top, wu, bu)), w2, b2)

    ours = [t.clone().to(DEV).requires_grad_(True) for t in leaves]
    y = block(ours, lambda x, w, b: networks.conv2d(x, w, b, padding=1), lambda x, w, b: networks.conv_transpose2d(x, w, b))
    grads = torch.autograd.grad(y, ours, go.to(DEV))
    ref = [t.clone().double().requires_grad_(True) for t in leaves]
    yr = block(ref, lambda x, w, b: F.conv2d(x, w, b, 1, 1), lambda x, w, b: F.conv_transpose2d(x, w, b, 2))
    grads_r = torch.autograd.grad(yr, ref, go.double())
    names = ("output", "g trans", "g top", "g w1", "g b1", "g w_up", "g b_up", "g w2", "g b2")
    for name, got, want in zip(names, (y,) + tuple(grads), (yr,) + tuple(grads_r)):
        d = float((got.detach().cpu().double() - want.detach()).abs().max())
        bound = 1e-4 * max(1.0, float(want.abs().max()))
        print("tcb block %-8s max|d| %.3e  bound %.3e" % (name, d, bound))
        assert d <= bound, (name, d, bound)


# 6. no allocation, no synchronisation: the three entries captured on a side stream, one stream, no parallel branches
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_conv_transpose2d_replays_under_graph_capture(mode):
    a = Abi("tcb_small", mode)
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
        a.ws.fill_(0x4B)                           # the entries zero what they need on every replay
        graph.replay()
        torch.cuda.synchronize()
        for name, p, q in zip(NAMES, want, (out, gi, gw, gb)):
            assert _bits_equal(p, q), (name, "replay %d" % k)
    del graph
