"""MaxPool2d on resident tensors (tdrn_hip.h section i-k: tdrn_max_pool_nhwc_*, networks.max_pool2d_nhwc) and the layout boundary
(to_nhwc / from_nhwc).  Selection is exact, so the yardstick is the existing fp32 NCHW op on the same values, bit for bit: output and
codes (the fp32 op's codes are NCHW: permuted before comparing), and grad_input = the fp32 backward's result rounded once to the type."""
import pytest
import torch

from tdrn_amd.model import networks

from _conv_train_harness import DEV
from _nhwc_harness import TYPES, GuardedResident, exact, pool_backward, pool_forward, raw_equal, resident

pytestmark = pytest.mark.gpu
MODES = ("bf16", "fp16")
GEOS = {"floor2": (2, 2, 0, 0), "ceil2": (2, 2, 0, 1), "k3": (3, 1, 1, 0)}
SHAPES = [(2, 64, 7, 9), (1, 192, 10, 6), (1, 64, 1, 5), (3, 64, 2, 2)]


def values(shape, mode, seed):
    """few distinct values (ties everywhere), both zeros, infinities and NaNs"""
    g = torch.Generator().manual_seed(seed)
    x = exact(torch.randint(-3, 4, shape, generator=g).float() * 0.5, mode)
    r = torch.rand(shape, generator=g)
    x[r < 0.10] = -0.0
    x[(r >= 0.10) & (r < 0.13)] = float("nan")
    x[(r >= 0.13) & (r < 0.16)] = float("-inf")
    x[(r >= 0.16) & (r < 0.18)] = float("inf")
    return x


def same_values(p, q):
    """bit for bit, a NaN matching any NaN"""
    p, q = p.float(), q.float()
    nan = torch.isnan(p)
    return torch.equal(nan, torch.isnan(q)) and torch.equal(p[~nan].view(torch.int32), q[~nan].view(torch.int32))


def fp32_pool(x, geo):
    """the existing op's entries on the same values -> (output, codes NCHW, a backward from codes)"""
    from tdrn_amd import _lib
    lib = _lib.lib()
    N, Cc, H, W = x.shape
    Ho, Wo = (lib.tdrn_max_pool_output_size(n, *geo) for n in (H, W))
    xd = x.to(DEV)
    out = torch.empty(N, Cc, Ho, Wo, device=DEV)
    code = torch.empty(N, Cc, Ho, Wo, dtype=torch.uint8, device=DEV)
    _lib.check(lib.tdrn_max_pool_forward(_lib.ptr(xd), _lib.ptr(out), _lib.ptr(code), N, Cc, H, W, *geo, _lib.current_stream(DEV)))

    def backward(go):
        gi = torch.empty(N, Cc, H, W, device=DEV)
        _lib.check(lib.tdrn_max_pool_backward(_lib.ptr(go), _lib.ptr(code), _lib.ptr(gi), N, Cc, H, W, *geo, _lib.current_stream(DEV)))
        return gi
    return out, code, backward


# (a 2x2 floor window does not fit a one-row map)
COMBOS = [(s, g) for s in SHAPES for g in sorted(GEOS) if not (g == "floor2" and min(s[2:]) < 2)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,geo", COMBOS, ids=["%s-%s" % ("x".join(map(str, s)), g) for s, g in COMBOS])
def test_pool_equals_the_fp32_op(shape, geo, mode):
    g = GEOS[geo]
    x = values(shape, mode, SHAPES.index(shape) * 3 + sorted(GEOS).index(geo))
    out32, code32, backward32 = fp32_pool(x, g)
    N, Cc, Ho, Wo = out32.shape
    xr = resident(x, mode)
    out = GuardedResident((N, Cc, Ho, Wo), mode)
    n = N * Ho * Wo * Cc
    raw = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    code = raw[33:33 + n]                                                   # codes on an odd byte, between two guard bands
    pool_forward(xr, out.t, code, g, mode)
    out.check("pool %s output" % geo)
    assert same_values(out.t, out32)
    assert torch.equal(code.view(N, Ho, Wo, Cc).permute(0, 3, 1, 2), code32)
    assert bool((raw[:33] == 0xAB).all()) and bool((raw[33 + n:] == 0xAB).all())
    # backward: finite grad_output, every element of grad_input written once
    gen = torch.Generator().manual_seed(7)
    go = exact(torch.randn(N, Cc, Ho, Wo, generator=gen), mode)
    gi = GuardedResident(shape, mode)
    pool_backward(resident(go, mode), code, gi.t, g, mode)
    gi.check("pool %s grad_input" % geo)
    want = backward32(go.to(DEV)).to(TYPES[mode])
    assert raw_equal(gi.t, want.contiguous(memory_format=torch.channels_last))
    # without codes: the same output
    out2 = torch.empty_like(out.t)
    pool_forward(xr, out2, None, g, mode)
    torch.cuda.synchronize()
    assert same_values(out2, out32)


def test_python_pool_op():
    mode, shape = "bf16", (2, 64, 7, 9)
    x = values(shape, mode, 11)
    x[torch.isnan(x) | torch.isinf(x)] = 1.0
    for geo in GEOS.values():
        k, s, p, ceil = geo
        out32, _, backward32 = fp32_pool(x, geo)
        xr = resident(x, mode).requires_grad_(True)
        y = networks.max_pool2d_nhwc(xr, k, s, p, bool(ceil))
        assert y.grad_fn is not None and y.is_contiguous(memory_format=torch.channels_last) and same_values(y.detach(), out32)
        go = exact(torch.randn(out32.shape, generator=torch.Generator().manual_seed(2)), mode)
        y.backward(go.to(DEV))                                              # fp32 NCHW grad_output: made resident by the wrapper
        assert raw_equal(xr.grad, backward32(go.to(DEV)).to(TYPES[mode]).contiguous(memory_format=torch.channels_last))
        assert networks.max_pool2d_nhwc(xr.detach(), k, s, p, bool(ceil)).grad_fn is None
    with pytest.raises(NotImplementedError):
        networks.max_pool2d_nhwc(resident(x, mode), 3, 2, 1)
    with pytest.raises(NotImplementedError):
        networks.max_pool2d_nhwc(resident(x, mode).cpu(), 2, 2)
    with pytest.raises(ValueError):
        networks.max_pool2d_nhwc(x.to(DEV), 2, 2)                           # fp32 is max_pool2d's


@pytest.mark.parametrize("mode", MODES)
def test_layout_round_trip_and_gradients(mode):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 128, 5, 7, generator=g).to(DEV)                      # NOT exact in the type: to_nhwc rounds once
    r = networks.to_nhwc(x, mode)
    assert r.dtype == TYPES[mode] and r.shape == x.shape and r.is_contiguous(memory_format=torch.channels_last) and r.grad_fn is None
    assert raw_equal(r, x.to(TYPES[mode]).contiguous(memory_format=torch.channels_last))
    back = networks.from_nhwc(r)
    assert back.dtype == torch.float32 and back.is_contiguous() and torch.equal(back, r.float())
    assert raw_equal(networks.to_nhwc(back, TYPES[mode]), r)                # the identity on 16-bit values
    # gradients pass through both: each is the other's backward
    xg = x.clone().requires_grad_(True)
    y = networks.from_nhwc(networks.to_nhwc(xg, mode))
    go = torch.randn(x.shape, generator=g).to(DEV)
    y.backward(go)
    assert torch.equal(xg.grad, go.to(TYPES[mode]).float())
    with pytest.raises(RuntimeError):
        networks.to_nhwc(x[:, :70], mode)
    with pytest.raises(NotImplementedError):
        networks.to_nhwc(x.cpu(), mode)
    with pytest.raises(ValueError):
        networks.to_nhwc(x, torch.float32)
