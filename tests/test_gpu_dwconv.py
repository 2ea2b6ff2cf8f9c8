"""The depthwise 3x3 conv with gradients (tdrn_hip.h section i-h; DepthwiseConv2dFunction / depthwise_conv2d / DepthwiseConv2d)
against torch's CPU autograd in float64.

Oracle: torch.nn.functional.conv2d(x, w, b, stride, 1, groups=C) on the CPU in float64, differentiated by autograd.
Bound: the harness's fp32 bound |got - ref| <= 1e-4 * max(1, max|ref|) (_conv_train_harness.compare); no element is exempted.  The
op has no 16-bit mode.  Inputs are unit-scale normal values from a fixed generator; the worst share of the bound is printed.

The cases are the smallest at which each path can go wrong; what each reaches in the weight gradient's split rule is asserted from
the rule restated in test_dwconv_abi.py.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from _conv_train_harness import DEV, NAMES, Guarded, compare
from _conv_train_harness import Abi as _Abi, bits_equal as _bits_equal
from tdrn_amd.model import networks

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
MODE = "fp32"

# (N, C, H, W) at stride 1 and 2 unless a stride is named
SHAPES = [
    ("one_pixel", (1, 1, 1, 1), (1, 2)),          # every tap but the centre in the padding
    ("tiny", (3, 1, 2, 3), (1, 2)),
    ("odd", (2, 5, 7, 9), (1, 2)),                # odd sizes; at stride 2 the last row and column are touched by one tap only
    ("even", (2, 5, 8, 6), (1, 2)),               # even sizes
    ("c70", (1, 70, 1, 1), (1, 2)),               # C is no multiple of anything
    ("c32", (2, 32, 5, 5), (1, 2)),
    ("wide", (1, 3, 64, 130), (1, 2)),            # W across more than one wave of a row
    ("c1030", (1, 1030, 4, 6), (1, 2)),
    ("k_ragged", (8, 64, 33, 31), (1, 2)),        # K spans several wgrad splits, with a ragged last split at stride 2
    ("last1024", (2, 1024, 6, 6), (1,)),           # the model's own last layers at 192 px
    ("last256", (2, 256, 6, 6), (2,)),
]
CASES = {"%s_s%d" % (name, s): shape + (s,) for name, shape, strides in SHAPES for s in strides}


def _out_hw(case):
    N, C, H, W, s = CASES[case]
    return (H - 1) // s + 1, (W - 1) // s + 1


def _dims(case):
    N, C, H, W, s = CASES[case]
    return (N, C, H, W, 3, 3, s, s, 1, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    N, C, H, W, s = CASES[case]
    Ho, Wo = _out_hw(case)
    gen = torch.Generator().manual_seed(list(CASES).index(case) + 901)
    return (torch.randn(N, C, H, W, generator=gen), torch.randn(C, 1, 3, 3, generator=gen), torch.randn(C, generator=gen),
            torch.randn(N, C, Ho, Wo, generator=gen))


@functools.lru_cache(maxsize=None)
def _reference(case, bias=True):
    """float64 CPU autograd -> (y, gx, gw, gb); computed once, never changed"""
    N, C, H, W, s = CASES[case]
    x, w, b, go = (t.double() for t in _inputs(case))
    x, w, b = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(x, w, b if bias else None, s, 1, 1, C)
    gx, gw = torch.autograd.grad(y, (x, w), go, retain_graph=True)
    return y.detach(), gx, gw, go.sum((0, 2, 3))


def _check(case, names, got, bias=True):
    ref = _reference(case, bias)
    return max(compare(case, MODE, name, g, ref[NAMES.index(name)], None) for name, g in zip(names, got))


def Abi(case):
    return _Abi("tdrn_dwconv2d", _dims(case), _inputs(case), MODE)


def test_the_cases_cover_the_split_rule():
    import test_dwconv_abi as A
    rules = {case: A.wgrad_splits(*CASES[case]) for case in CASES}
    assert any(S > 1 and K % per != 0 for S, per, K in rules.values())
    assert any(S == 1 for S, per, K in rules.values())
    assert rules["k_ragged_s2"] == (3, 726, 2176) and rules["k_ragged_s1"][0] == 8 and rules["one_pixel_s1"] == (1, 1, 1)


# 1. the four C entries, every case: outputs NaN-prefilled and fully overwritten (Abi.all)
@pytest.mark.parametrize("case", list(CASES))
def test_dwconv_abi_matches_float64_autograd(case):
    got = Abi(case).all()
    worst = _check(case, NAMES, got)
    print("%s: worst share of the bound %.3e" % (case, worst))
    if case == "even_s2":
        # Ho = 4 covers input rows -1 .. 7 and Wo = 3 columns -1 .. 5: at pad 1 no input row or column is ever left out
        assert float(got[1].abs().min()) > 0.0


# 2. bias present and NULL, grad_bias NULL, += scale on a non-zero grad_weight
def test_dwconv_bias_scale_and_accumulation_bitwise():
    case = "k_ragged_s2"
    a = Abi(case)
    g_w, g_b = a.backward_parameters(torch.zeros_like(a.w), torch.zeros_like(a.b))
    gen = torch.Generator().manual_seed(7)
    old_w, old_b = torch.randn(a.w.shape, generator=gen).to(DEV), torch.randn(a.b.shape, generator=gen).to(DEV)
    got_w, got_b = a.backward_parameters(old_w.clone(), old_b.clone(), scale=0.5)
    # one fused multiply-add per element: fl(old + 0.5 s) with g = s exactly (scale 1 into zeros) and 0.5 g exact
    assert _bits_equal(got_w, old_w + 0.5 * g_w) and _bits_equal(got_b, old_b + 0.5 * g_b)
    assert float((got_w - old_w).abs().max()) > 0 and float((got_b - old_b).abs().max()) > 0
    only_w, none = a.backward_parameters(torch.zeros_like(a.w), None)
    assert none is None and _bits_equal(only_w, g_w)
    no_bias = a.forward(torch.full_like(a.go, float("nan")), bias=False)
    torch.cuda.synchronize()
    _check(case, ("output",), (no_bias,), bias=False)
    _check(case, ("output",), (a.forward(torch.full_like(a.go, float("nan"))),))


# 3. autograd: the same bits as the raw entries; every needs_input_grad combination; a stride-0 grad_output; the module
@pytest.mark.parametrize("case", ["odd_s1", "odd_s2", "k_ragged_s2", "last1024_s1"])
def test_depthwise_autograd_gives_the_entries_bits(case):
    s = CASES[case][4]
    want = Abi(case).all()
    x, w, b, go = (t.to(DEV) for t in _inputs(case))
    x, w, b = (t.requires_grad_(True) for t in (x, w, b))
    y = networks.depthwise_conv2d(x, w, b, stride=s, padding=1)
    y.backward(go)
    for name, p, q in zip(NAMES, want, (y.detach(), x.grad, w.grad, b.grad)):
        assert _bits_equal(p, q), (case, name)
    y2 = networks.DepthwiseConv2dFunction.apply(x, w, b, (s, s), (1, 1))
    assert _bits_equal(y2.detach(), want[0])


def test_depthwise_autograd_plumbing():
    case = "odd_s2"
    N, C, H, W, s = CASES[case]
    x0, w0, b0, go0 = (t.to(DEV) for t in _inputs(case))
    for need in ((True, True, True), (True, False, False), (False, True, True), (False, True, False), (False, False, True),
                 (True, True, False), (True, False, True)):
        x, w, b = (t.clone().requires_grad_(n) for t, n in zip((x0, w0, b0), need))
        y = networks.depthwise_conv2d(x, w, b, s)
        assert y.requires_grad
        y.backward(go0)
        for t, n, name in zip((x, w, b), need, NAMES[1:]):
            assert (t.grad is not None) == n
            if n:
                _check(case, (name,), (t.grad,))
    with torch.no_grad():
        assert networks.depthwise_conv2d(x0.clone().requires_grad_(True), w0, b0, s).grad_fn is None
    assert networks.depthwise_conv2d(x0, w0, b0, s).grad_fn is None
    # no bias; a stride-0 grad_output (sum().backward())
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    y = networks.depthwise_conv2d(x, w, None, s)
    y.sum().backward()
    xr, wr = x0.cpu().double().requires_grad_(True), w0.cpu().double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, s, 1, 1, C)
    yr.sum().backward()
    for name, got, want in (("output", y.detach(), yr.detach()), ("grad_input", x.grad, xr.grad), ("grad_weight", w.grad, wr.grad)):
        compare(case + " sum", MODE, name, got, want, None)
    # the module: nn.Conv2d(groups=C)'s state dict loads, the same arithmetic
    r = torch.nn.Conv2d(C, C, 3, s, 1, groups=C, bias=True)
    with torch.no_grad():
        r.weight.copy_(w0)
        r.bias.copy_(b0)
    m = networks.DepthwiseConv2d(C, stride=s, bias=True)
    m.load_state_dict(r.state_dict())
    m = m.to(DEV)
    x = x0.clone().requires_grad_(True)
    y = m(x)
    y.backward(go0)
    _check(case, NAMES, (y, x.grad, m.weight.grad, m.bias.grad))
    # geometry the library refuses raises with the covered list; nothing falls back
    for kw in (dict(stride=3), dict(stride=(2, 1)), dict(padding=0), dict(padding=2), dict(padding=(1, 0))):
        with pytest.raises(RuntimeError, match="outside what libtdrn_hip covers.*kernel 3 x 3, stride 1 or 2, padding 1"):
            networks.depthwise_conv2d(x0, w0, b0, **kw)
    with pytest.raises(RuntimeError, match="outside what libtdrn_hip covers"):
        networks.depthwise_conv2d(x0, torch.zeros(C, 1, 5, 5, device=DEV), b0, 1, 2)
    with pytest.raises(RuntimeError, match="expected"):
        networks.depthwise_conv2d(x0, torch.zeros(C, 2, 3, 3, device=DEV), b0)
    with pytest.raises(NotImplementedError):
        networks.DepthwiseConv2d(C, stride=s)(x0.cpu())             # a module left on the CPU


# 4. bitwise reproducibility, caller buffers on byte offsets 4, 8 and 12, the workspace exactly as queried and full of NaN bytes
@pytest.mark.parametrize("case", ["odd_s1", "odd_s2", "wide_s1", "k_ragged_s1", "k_ragged_s2", "c1030_s2"])
def test_dwconv_is_bitwise_reproducible_on_any_callers_buffers(case):
    a = Abi(case)
    want = [t.clone() for t in a.all()]
    Abi("c70_s1").all()                 # other work on the device in between must not change the arithmetic
    for name, p, q in zip(NAMES, want, a.all()):
        assert _bits_equal(p, q), (case, name, "second run")
    plain = (a.x, a.w, a.b, a.go)
    for offset in (4, 8, 12):
        ws = Guarded(nbytes=a.nb)
        ws.t.fill_(0xFF)
        ins = [Guarded(t.shape, offset=offset, init=t) for t in plain]
        a.ws = ws.t
        a.x, a.w, a.b, a.go = (g.t for g in ins)
        out, gi = Guarded(a.go.shape, offset=offset), Guarded(a.x.shape, offset=offset)
        gw = Guarded(a.w.shape, offset=offset, init=torch.zeros_like(a.w))
        gb = Guarded(a.b.shape, offset=offset, init=torch.zeros_like(a.b))
        assert all(g.t.data_ptr() % 16 == offset for g in ins + [out, gi, gw, gb])
        a.backward_input(gi.t)
        a.forward(out.t)
        a.backward_parameters(gw.t, gb.t)
        for name, g, w in zip(NAMES, (out, gi, gw, gb), want):
            g.check("%s %s offset %d" % (case, name, offset))
            assert _bits_equal(g.t, w), (case, name, "buffers at byte offset %d" % offset)
        for name, g in zip(("input", "weight", "bias", "grad_output"), ins):
            g.check("%s %s offset %d" % (case, name, offset))
        ws.check("%s workspace" % case, full=False)


# 5. no allocation, no synchronisation: the three entries captured on a side stream, one stream, no parallel branches
def test_dwconv_replays_under_graph_capture():
    a = Abi("k_ragged_s2")
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
    out.fill_(float("nan"))
    gi.fill_(float("nan"))
    a.ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    for name, p, q in zip(NAMES, want, (out, gi, gw, gb)):
        assert _bits_equal(p, q), (name, "replay")
    del graph
