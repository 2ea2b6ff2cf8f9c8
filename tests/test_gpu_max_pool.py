"""Trainable MaxPool2d (tdrn_hip.h section i-e; MaxPool2dFunction / max_pool2d / MaxPool2d) against torch on the CPU.

Oracle: F.max_pool2d(..., return_indices=True) and its autograd on the CPU, in fp32 for the exact comparisons and in float64 for
the summed one.

Checks.  Forward: bitwise equal (as int32).  Codes: (ho s - p + code // k) W + wo s - p + code % k is torch's index.  Backward of
2x2 / 2: bitwise equal, so every zero is +0.0 and the rows and columns no floor-mode window covers are +0.0 too.  Backward of
3x3 / 1 / 1 (up to nine windows add into one element): within 1e-4 * max(1, max|ref|) of float64, the project's fp32 bound, and
bitwise equal between two runs.

Every case runs on a randn input and on a draw from {-1, -0.0, 0.0, 0.0, 0.5, 2}, where most windows hold ties and zeros of both
signs.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tdrn_amd import _lib
from tdrn_amd.model import networks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FLOOR, CEIL, K3 = (2, 2, 0, 0), (2, 2, 0, 1), (3, 1, 1, 0)       # kernel, stride, pad, ceil_mode
# N, C, H, W, geometry
CASES = {
    "odd_floor": (2, 3, 7, 9, FLOOR),            # uncovered last row and column, 63-float planes
    "odd_ceil": (2, 3, 7, 9, CEIL),              # clipped windows, 4x5 output
    "aligned": (3, 5, 8, 12, FLOOR),             # the pure 16-byte path
    "conv7_in": (2, 70, 10, 10, FLOOR),          # W mod 4 = 2, more than 64 channels
    "one_window": (1, 2, 2, 2, FLOOR),           # one output per plane
    "one_element": (1, 2, 1, 1, CEIL),           # a window clipped to one element
    "wide": (1, 2, 64, 130, FLOOR),              # many pieces inside one plane
    "many_planes": (4, 3, 40, 40, FLOOR),        # more than one workgroup
    "k3_small": (2, 5, 5, 5, K3),                # every border kind
    "k3_conv7_in": (2, 70, 10, 10, K3),
    "k3_one": (1, 3, 1, 1, K3),                  # eight of nine slots out of bounds
    "k3_odd": (2, 3, 7, 9, K3),
}
KINDS = ("randn", "ties")
TIE_VALUES = (-1.0, -0.0, 0.0, 0.0, 0.5, 2.0)


@functools.lru_cache(maxsize=None)
def _inputs(case, kind):
    """x and grad_output (CPU, fp32)"""
    N, C, H, W, geo = CASES[case]
    gen = torch.Generator().manual_seed(sorted(CASES).index(case) * 2 + KINDS.index(kind) + 41)
    if kind == "randn":
        x = torch.randn(N, C, H, W, generator=gen)
    else:
        x = torch.tensor(TIE_VALUES)[torch.randint(len(TIE_VALUES), (N, C, H, W), generator=gen)]
    k, s, p, ceil = geo
    Ho, Wo = F.max_pool2d(x, k, s, p, ceil_mode=bool(ceil)).shape[2:]
    return x, torch.randn(N, C, Ho, Wo, generator=gen)


def _oracle(x, go, geo, dtype):
    k, s, p, ceil = geo
    xr = x.to(dtype).clone().requires_grad_(True)
    y, idx = F.max_pool2d(xr, k, s, p, ceil_mode=bool(ceil), return_indices=True)
    gi, = torch.autograd.grad(y, xr, go.to(dtype))
    return y.detach(), idx, gi


@functools.lru_cache(maxsize=None)
def _reference(case, kind):
    """computed once, never changed"""
    x, go = _inputs(case, kind)
    geo = CASES[case][4]
    y, idx, gi = _oracle(x, go, geo, torch.float32)
    return {"output": y, "index": idx, "grad_input": gi, "grad_input64": _oracle(x, go, geo, torch.float64)[2]}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _index_of(code, geo, W):
    k, s, p, _ = geo
    Ho, Wo = code.shape[2:]
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    c = code.cpu().long()
    return (ho * s - p + c // k) * W + wo * s - p + c % k


def _forward(x, geo, out, code):
    N, C, H, W = x.shape
    _lib.check(_lib.lib().tdrn_max_pool_forward(_lib.ptr(x), _lib.ptr(out), _lib.ptr(code), N, C, H, W, *geo, _lib.current_stream(DEV)))


def _backward(go, code, gi, geo):
    N, C, H, W = gi.shape
    _lib.check(_lib.lib().tdrn_max_pool_backward(_lib.ptr(go), _lib.ptr(code), _lib.ptr(gi), N, C, H, W, *geo, _lib.current_stream(DEV)))


def _run(x, go, geo):
    """the C entries on plain device buffers, outputs started at NaN / 255"""
    x, go = x.to(DEV), go.to(DEV)
    out = torch.full(go.shape, float("nan"), device=DEV)
    code = torch.full(go.shape, 255, dtype=torch.uint8, device=DEV)
    gi = torch.full(x.shape, float("nan"), device=DEV)
    _forward(x, geo, out, code)
    _backward(go, code, gi, geo)
    torch.cuda.synchronize()
    return {"output": out, "code": code, "grad_input": gi}


def _compare(tag, got, ref, geo, W):
    assert torch.equal(_bits(got["output"].cpu()), _bits(ref["output"])), "%s: output bits" % tag
    assert torch.equal(_index_of(got["code"], geo, W), ref["index"]), "%s: codes" % tag
    gi = got["grad_input"].cpu()
    if geo[0] == 2:
        assert torch.equal(_bits(gi), _bits(ref["grad_input"])), "%s: grad_input bits" % tag
    else:
        r = ref["grad_input64"]
        d, bound = float((gi.double() - r).abs().max()), 1e-4 * max(1.0, float(r.abs().max()))
        print("%s grad_input max|d| %.3e  share of the bound %.4f" % (tag, d, d / bound))
        assert d <= bound, (tag, d, bound)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(CASES))
def test_max_pool_abi_matches_torch_cpu(case, kind):
    x, go = _inputs(case, kind)
    geo = CASES[case][4]
    _compare("%s %s" % (case, kind), _run(x, go, geo), _reference(case, kind), geo, x.shape[3])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(CASES))
def test_max_pool_autograd_matches_torch_cpu(case, kind):
    x, go = _inputs(case, kind)
    k, s, p, ceil = geo = CASES[case][4]
    xg = x.to(DEV).requires_grad_(True)
    y = networks.max_pool2d(xg, k, s, p, bool(ceil))
    code = y.grad_fn.saved_tensors[0]                # all the backward keeps: no input, no int64 indices
    assert len(y.grad_fn.saved_tensors) == 1 and code.dtype == torch.uint8 and code.shape == y.shape
    y.backward(go.to(DEV))
    ref = _reference(case, kind)
    _compare("%s %s autograd" % (case, kind), {"output": y.detach(), "code": code, "grad_input": xg.grad}, ref, geo, x.shape[3])


def test_max_pool_inference_only_forward_gives_the_same_output():
    for case in ("odd_ceil", "k3_odd", "aligned"):
        x, go = _inputs(case, "ties")
        out = torch.full(go.shape, float("nan"), device=DEV)
        _forward(x.to(DEV), CASES[case][4], out, None)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out.cpu()), _bits(_reference(case, "ties")["output"])), case


@pytest.mark.parametrize("geo", [FLOOR, K3])
def test_max_pool_nan_wins_and_the_last_nan_is_selected(geo):
    nan = float("nan")
    if geo is FLOOR:
        x = torch.tensor([[nan, 5.0, 1.0, 2.0], [nan, 1.0, 3.0, nan]]).view(1, 1, 2, 4)      # windows: two NaNs and a 5 | one NaN last
    else:
        x = torch.tensor([[1.0, nan, 1.0], [7.0, 1.0, nan], [1.0, 1.0, 1.0]]).view(1, 1, 3, 3)
    k, s, p, ceil = geo
    Ho, Wo = F.max_pool2d(x, k, s, p).shape[2:]
    go = torch.arange(1.0, 1.0 + Ho * Wo).view(1, 1, Ho, Wo)
    y, idx, gi = _oracle(x, go, geo, torch.float32)
    got = _run(x, go, geo)
    out = got["output"].cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(y)) and bool(torch.isnan(out).any())
    assert torch.equal(_index_of(got["code"], geo, x.shape[3]), idx)
    if geo is FLOOR:
        assert bool(torch.isnan(out).all()) and _index_of(got["code"], geo, 4).flatten().tolist() == [4, 7]      # the last NaN of each window
    assert torch.equal(got["grad_input"].cpu(), gi)
    # the whole gradient of a window lands on its selected NaN
    assert torch.equal(got["grad_input"].cpu().flatten()[idx.flatten()] != 0, torch.ones(Ho * Wo, dtype=torch.bool))


@pytest.mark.parametrize("case", ["k3_conv7_in", "k3_odd"])
def test_max_pool_k3_backward_is_bitwise_reproducible(case):
    x, go = _inputs(case, "ties")
    first = _run(x, go, K3)
    xo, goo = _inputs("many_planes", "randn")
    _run(xo, goo, FLOOR)                      # other work on the device in between
    second = _run(x, go, K3)
    for name in ("output", "grad_input"):
        assert torch.equal(_bits(first[name]), _bits(second[name])), name
    assert torch.equal(first["code"], second["code"])


SENTINEL = 0x7FBADBAD          # a NaN pattern no kernel computes; none of its bytes is a code (0..8)
GUARD = 4096


class Guarded(object):
    """`nbytes` of device memory that start `offset` bytes behind a 256-byte boundary, between two guard bands of a NaN pattern no
    kernel computes (the pattern of test_gpu_batch_norm.py); `offset` may be any byte for a uint8 tensor"""

    def __init__(self, shape, offset, dtype=torch.float32, init=None):
        n = int(torch.Size(shape).numel()) * (4 if dtype == torch.float32 else 1)
        total = 2 * GUARD + 256 + offset + n
        self.raw = torch.full(((total + 3) // 4,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.uint8)
        self.pristine = self.raw.clone()
        base = (-self.raw.data_ptr()) % 256 + GUARD
        self.lo, self.hi, self.dtype = base + offset, base + offset + n, dtype
        body = self.raw[self.lo:self.hi]
        self.t = (body.view(torch.float32) if dtype == torch.float32 else body).view(shape)
        assert self.t.data_ptr() % 256 == offset
        if init is not None:
            self.t.copy_(init)

    def check(self, what, written=True):
        torch.cuda.synchronize()
        assert torch.equal(self.raw[:self.lo], self.pristine[:self.lo]), "%s: bytes in front of the buffer were written" % what
        assert torch.equal(self.raw[self.hi:], self.pristine[self.hi:]), "%s: bytes behind the end of the buffer were written" % what
        if written and self.dtype == torch.float32:
            assert int((self.t.contiguous().view(torch.int32) == SENTINEL).sum()) == 0, "%s: elements never written" % what
        elif written:
            assert int((self.t > 8).sum()) == 0, "%s: codes never written" % what


@pytest.mark.parametrize("code_offset", [4, 1])
@pytest.mark.parametrize("case", ["odd_ceil", "conv7_in", "k3_odd"])
def test_max_pool_writes_only_the_callers_buffers(case, code_offset):
    geo = CASES[case][4]
    for kind in KINDS:
        x, go = _inputs(case, kind)
        want = _run(x, go, geo)
        gx, ggo = Guarded(x.shape, 4, init=x), Guarded(go.shape, 4, init=go)
        out, code, gi = Guarded(go.shape, 4), Guarded(go.shape, code_offset, torch.uint8), Guarded(x.shape, 4)
        _forward(gx.t, geo, out.t, code.t)
        _backward(ggo.t, code.t, gi.t, geo)
        for name, g in (("output", out), ("code", code), ("grad_input", gi)):
            g.check("%s %s %s" % (case, kind, name))
        assert torch.equal(_bits(out.t), _bits(want["output"])) and torch.equal(_bits(gi.t), _bits(want["grad_input"]))
        assert torch.equal(code.t, want["code"])
        gx.check("input", written=False)
        ggo.check("grad_output", written=False)
        assert torch.equal(gx.t.cpu(), x) and torch.equal(ggo.t.cpu(), go)


def test_max_pool_autograd_plumbing():
    x0, _ = _inputs("odd_ceil", "ties")
    x0 = x0.to(DEV)
    x = x0.clone().requires_grad_(True)
    y = networks.max_pool2d(x, 2, 2, 0, True)
    assert y.requires_grad
    y.sum().backward()                               # a stride-0 grad_output
    xr = x0.cpu().clone().requires_grad_(True)
    F.max_pool2d(xr, 2, 2, 0, ceil_mode=True).sum().backward()
    assert torch.equal(_bits(x.grad.cpu()), _bits(xr.grad))
    with torch.no_grad():
        assert networks.max_pool2d(x0.clone().requires_grad_(True), 2).grad_fn is None
    assert networks.max_pool2d(x0, 2).grad_fn is None
    assert networks.max_pool2d(x0, 2).shape == (2, 3, 3, 4)             # stride defaults to the kernel size
    with pytest.raises(NotImplementedError):
        networks.max_pool2d(x0.cpu(), 2)
    for bad in ((2, 1, 0), (3, 2, 0), (2, 2, 1), (3, 1, 0), ((2, 3), 2, 0)):
        with pytest.raises(NotImplementedError, match="kernel_size 2, stride 2, padding 0"):
            networks.max_pool2d(x0, *bad)
    with pytest.raises(ValueError):
        networks.max_pool2d(x0[0], 2)
    with pytest.raises(ValueError):
        networks.max_pool2d(x0.double(), 2)
    # a non-contiguous input and a non-contiguous grad_output
    xt = x0.transpose(2, 3).clone().requires_grad_(True)
    y = networks.max_pool2d(xt.transpose(2, 3), 2)
    g = torch.randn(y.shape[0], y.shape[1], y.shape[3], y.shape[2], device=DEV).transpose(2, 3)
    y.backward(g)
    xr = x0.cpu().clone().requires_grad_(True)
    F.max_pool2d(xr, 2).backward(g.cpu())
    assert torch.equal(_bits(xt.grad.transpose(2, 3).cpu()), _bits(xr.grad))


def test_max_pool_modules_agree_with_nn_maxpool2d():
    for args, kw in (((2, 2), {"ceil_mode": True}), ((3, 1, 1), {})):
        ours, ref = networks.MaxPool2d(*args, **kw), torch.nn.MaxPool2d(*args, **kw)
        assert list(ours.state_dict()) == []
        for kind in KINDS:
            x = _inputs("odd_ceil", kind)[0].to(DEV)
            assert torch.equal(_bits(ours(x)), _bits(ref(x))), (args, kind)
