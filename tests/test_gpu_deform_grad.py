"""Deformable conv v1 backward on the GPU (tdrn_hip.h section i-b, ConvOffset2dFunction) against the CPU gradient
oracle (tests/_deform_grad_ref.py): parity through the C ABI and through autograd, the accumulation contract, run-to-run
reproducibility, the reference smoke script's shape class, the autograd plumbing and a short training run."""
import numpy as np
import pytest
import torch

import _deform_grad_ref as gref
from tdrn_amd import _lib
from tdrn_amd.model.networks import ConvOffset2d, ConvOffset2dFunction, conv_offset2d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [
    # N, Cin, H, W, Cout, k, stride, pad, dil, G, offset scale  (the shape classes of test_gpu_ops.DEFORM_CASES)
    (2, 6, 9, 7, 4, 3, 1, 1, 1, 1, 0.0),
    (1, 6, 9, 7, 4, 3, 1, 1, 1, 1, 1.0),
    (2, 32, 10, 10, 12, 3, 1, 1, 1, 1, 1.5),
    (1, 64, 20, 20, 75, 3, 1, 1, 1, 1, 1.0),
    (1, 64, 12, 11, 63, 5, 1, 2, 1, 1, 2.0),
    (2, 64, 8, 8, 12, 3, 1, 1, 1, 8, 1.0),
    (1, 24, 13, 9, 10, 3, 2, 1, 1, 2, 1.0),
    (1, 16, 9, 9, 8, 3, 1, 2, 2, 1, 1.0),
    (1, 8, 6, 6, 140, 1, 1, 0, 1, 1, 0.7),
    (3, 256, 5, 5, 75, 3, 1, 1, 1, 1, 3.0),
    (2, 16, 11, 13, 9, (3, 5), 1, (1, 2), 1, 1, 1.0),
    (1, 32, 14, 9, 12, (1, 3), (2, 1), (0, 1), 1, 2, 1.5),
    # ODM heads (fused loc + conf width) and a TRN head (8 deformable groups, Cin 512)
    (2, 256, 20, 20, 75, 3, 1, 1, 1, 1, 2.0),
    (2, 256, 20, 20, 75, 5, 1, 2, 1, 1, 2.0),
    (1, 512, 10, 10, 63, 3, 1, 1, 1, 8, 2.0),
]


def _pr(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _rand(shape, seed, scale=1.0):
    return (scale * np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)).astype(np.float32)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(case):
    N, Cin, H, W, Cout, k, st, pad, dil, G, osc = case
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pr(k), _pr(st), _pr(pad), _pr(dil)
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    x, w = _rand((N, Cin, H, W), 1), _rand((Cout, Cin, kh, kw), 2, (Cin * kh * kw) ** -0.5)
    off = _rand((N, G * 2 * kh * kw, Ho, Wo), 3, osc)
    gout = _rand((N, Cout, Ho, Wo), 4)
    dims = (N, Cin, H, W, Cout, kw, kh, sw, sh, pw, ph, dh, dw, G)
    return x, off, w, gout, st, pad, dil, G, dims


def _abi(x, off, w, gout, dims, gi=None, gw=None, scale=1.0, what="both"):
    """the two C entries on fresh (or given) output buffers; returns (grad_input, grad_offset, grad_weight) on the GPU"""
    lib = _lib.lib()
    N, Cin, H, W, Cout, kw, kh, sw, sh, pw, ph, dh, dw, G = dims
    nb = lib.tdrn_deform_conv_backward_workspace_bytes(N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, G)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    x, off, w, gout = (t if torch.is_tensor(t) else _cu(t) for t in (x, off, w, gout))
    gi = torch.zeros_like(x) if gi is None else gi
    goff = torch.full_like(off, float("nan"))            # overwritten: NaN shows any entry the kernel misses
    gw = torch.zeros_like(w) if gw is None else gw
    st = _lib.current_stream(x.device)
    if what in ("both", "input"):
        _lib.check(lib.tdrn_deform_conv_backward_input(_lib.ptr(x), _lib.ptr(off), _lib.ptr(gout), _lib.ptr(gi), _lib.ptr(goff),
                                                       _lib.ptr(w), *dims, _lib.ptr(ws), nb, st), "backward_input")
    if what in ("both", "params"):
        _lib.check(lib.tdrn_deform_conv_backward_parameters(_lib.ptr(x), _lib.ptr(off), _lib.ptr(gout), _lib.ptr(gw), *dims,
                                                            scale, _lib.ptr(ws), nb, st), "backward_parameters")
    torch.cuda.synchronize()
    return gi, goff, gw


def _check(name, got, ref, exempt=None):
    got = got.detach().cpu().double()
    d = (got - ref).abs()
    tol = 1e-4 * max(1.0, float(ref.abs().max()))
    bad = d > tol
    n_exempt = 0
    if exempt is not None:
        n_exempt = int((bad & exempt).sum())
        bad = bad & ~exempt
    assert not bool(torch.isnan(got).any()), name + ": NaN (an entry was never written)"
    assert int(bad.sum()) == 0, "%s: %d entries off by up to %.3e (tol %.3e)" % (name, int(bad.sum()), float(d[bad].max()), tol)
    return n_exempt


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_backward_matches_oracle_abi_and_autograd(case):
    x, off, w, gout, st, pad, dil, G, dims = _case(case)
    _, rgx, rgo, rgw = gref.grads(x, off, w, gout, st, pad, dil, G)
    exempt = gref.near_decision(off, x.shape, w.shape, st, pad, dil, G)
    gi, goff, gw = _abi(x, off, w, gout, dims)
    _check("grad_input", gi, rgx)
    n = _check("grad_offset", goff, rgo, exempt)
    assert n <= max(2, goff.numel() // 1000), n
    _check("grad_weight", gw, rgw)
    # the same through autograd
    xt, ot, wt = (_cu(a).requires_grad_(True) for a in (x, off, w))
    y = conv_offset2d(xt, ot, wt, st, pad, dil, G)
    y.backward(_cu(gout))
    _check("autograd grad_input", xt.grad, rgx)
    _check("autograd grad_offset", ot.grad, rgo, exempt)
    _check("autograd grad_weight", wt.grad, rgw)


def test_accumulation_semantics():
    x, off, w, gout, st, pad, dil, G, dims = _case((2, 32, 10, 10, 12, 3, 1, 1, 1, 1, 1.5))
    gi1, go1, gw1 = _abi(x, off, w, gout, dims)
    gi2, go2, _ = _abi(x, off, w, gout, dims, gi=gi1.clone(), what="input")     # += onto the first result
    torch.testing.assert_close(gi2, 2 * gi1, rtol=1e-5, atol=1e-6)
    assert torch.equal(go2, go1)                                                 # grad_offset is overwritten
    pre = _cu(_rand(w.shape, 9))
    _, _, gw = _abi(x, off, w, gout, dims, gw=pre.clone(), scale=0.5, what="params")
    torch.testing.assert_close(gw, pre + 0.5 * gw1, rtol=1e-5, atol=1e-6)


def test_reproducibility():
    x, off, w, gout, st, pad, dil, G, dims = _case((2, 256, 20, 20, 75, 3, 1, 1, 1, 1, 2.0))
    a = _abi(x, off, w, gout, dims)
    b = _abi(x, off, w, gout, dims)
    assert torch.equal(a[1], b[1]), "grad_offset differs between two runs"
    assert torch.equal(a[2], b[2]), "grad_weight differs between two runs"
    assert float((a[0] - b[0]).abs().max()) <= 1e-6 * float(a[0].abs().max())


def test_reference_smoke_script_shape_class():
    # utils/deformconv/test.py: N = 1, 6 -> 4 channels, G = 2, offsets from an nn.Conv2d, output.backward(output.data);
    # on a 64 x 64 map instead of 512 x 512 (the fp64 CPU oracle takes minutes at the full size)
    torch.manual_seed(0)
    N, C, S, G = 1, 6, 64, 2
    conv = torch.nn.Conv2d(C, G * 2 * 9, 3, 1, 1, bias=False).to(DEV)
    dcn = ConvOffset2d(C, 4, (3, 3), stride=1, padding=1, num_deformable_groups=G).to(DEV)
    x = torch.randn(N, C, S, S, device=DEV, requires_grad=True)
    offset = conv(x)
    output = dcn(x, offset)
    output.backward(output.data)
    # oracle: the same graph in fp64 on the CPU
    xr = x.detach().cpu().double().requires_grad_(True)
    cw = conv.weight.detach().cpu().double().requires_grad_(True)
    dw = dcn.weight.detach().cpu().double().requires_grad_(True)
    offr = torch.nn.functional.conv2d(xr, cw, padding=1)
    # the product's offsets are fp32: the oracle samples where the device sampled, and differentiates through its conv
    offr = offr + (offset.detach().cpu().double() - offr.detach())
    outr = gref.deform_conv(xr, offr, dw, 1, 1, 1, G)
    outr.backward(output.detach().cpu().double())
    _check("deformable weight", dcn.weight.grad, dw.grad)
    _check("offset conv weight", conv.weight.grad, cw.grad)
    _check("input", x.grad, xr.grad)


def test_sum_backward_with_stride0_grad():
    x, off, w, _, st, pad, dil, G, _ = _case((1, 16, 9, 9, 8, 3, 1, 2, 2, 1, 1.0))
    xt, ot, wt = (_cu(a).requires_grad_(True) for a in (x, off, w))
    conv_offset2d(xt, ot, wt, st, pad, dil, G).sum().backward()
    _, rgx, rgo, rgw = gref.grads(x, off, w, np.ones((1, 8, 9, 9), np.float32), st, pad, dil, G)
    _check("grad_input", xt.grad, rgx)
    _check("grad_offset", ot.grad, rgo, gref.near_decision(off, x.shape, w.shape, st, pad, dil, G))
    _check("grad_weight", wt.grad, rgw)


def test_needs_input_grad_is_honoured():
    x, off, w, gout, st, pad, dil, G, _ = _case((2, 32, 10, 10, 12, 3, 1, 1, 1, 1, 1.5))
    for flags in [(True, False, False), (False, True, False), (False, False, True), (True, True, False)]:
        ts = [_cu(a).requires_grad_(f) for a, f in zip((x, off, w), flags)]
        got = torch.autograd.grad(ConvOffset2dFunction.apply(*ts, st, pad, dil, G), [t for t in ts if t.requires_grad],
                                  _cu(gout))
        assert len(got) == sum(flags) and all(g is not None for g in got)
    # only the offset requires grad: no weight gradient is formed
    ot = _cu(off).requires_grad_(True)
    wt = _cu(w).requires_grad_(True)
    y = conv_offset2d(_cu(x), ot, wt, st, pad, dil, G)
    gi, goff, gw = y.grad_fn.apply(_cu(gout))[:3]
    assert gi is None and goff is not None and gw is not None
    y2 = ConvOffset2dFunction.apply(_cu(x), ot, _cu(w), st, pad, dil, G)
    gi, goff, gw = y2.grad_fn.apply(_cu(gout))[:3]
    assert gi is None and goff is not None and gw is None


def test_forward_bits_identical_with_and_without_autograd():
    x, off, w, _, st, pad, dil, G, _ = _case((1, 64, 12, 11, 63, 5, 1, 2, 1, 1, 2.0))
    plain = conv_offset2d(_cu(x), _cu(off), _cu(w), st, pad, dil, G)
    assert plain.grad_fn is None
    y = conv_offset2d(_cu(x).requires_grad_(True), _cu(off), _cu(w), st, pad, dil, G)
    assert y.grad_fn is not None
    assert torch.equal(plain, y.detach())
    with torch.no_grad():
        z = conv_offset2d(_cu(x).requires_grad_(True), _cu(off).requires_grad_(True), _cu(w), st, pad, dil, G)
    assert z.grad_fn is None and torch.equal(plain, z)


def test_bf16_forward_gets_the_fp32_backward():
    x, off, w, gout, st, pad, dil, G, _ = _case((2, 64, 8, 8, 12, 3, 1, 1, 1, 8, 1.0))
    res = []
    for compute in ("fp32", "bf16"):
        ts = [_cu(a).requires_grad_(True) for a in (x, off, w)]
        conv_offset2d(*ts, st, pad, dil, G, compute=compute).backward(_cu(gout))
        res.append([t.grad for t in ts])
    (gi_a, go_a, gw_a), (gi_b, go_b, gw_b) = res
    assert torch.equal(go_a, go_b) and torch.equal(gw_a, gw_b)
    assert float((gi_a - gi_b).abs().max()) <= 1e-6 * float(gi_a.abs().max())     # (float atomics: arrival order)


def test_cpu_tensors_raise_not_implemented():
    x, off, w, gout, st, pad, dil, G, _ = _case((1, 6, 9, 7, 4, 3, 1, 1, 1, 1, 1.0))
    with pytest.raises(NotImplementedError):
        conv_offset2d(torch.from_numpy(x).requires_grad_(True), torch.from_numpy(off), torch.from_numpy(w), st, pad, dil, G)
    y = conv_offset2d(_cu(x).requires_grad_(True), _cu(off), _cu(w), st, pad, dil, G)
    with pytest.raises(NotImplementedError):
        y.grad_fn.apply(torch.from_numpy(gout))


def test_training_steps_track_the_oracle():
    # offset conv -> ConvOffset2d, 20 SGD steps on the GPU and the same steps on the fp64 CPU oracle
    torch.manual_seed(1)
    C, Cout, S, G, lr = 8, 4, 12, 2, 0.05
    conv = torch.nn.Conv2d(C, G * 18, 3, 1, 1, bias=False)
    torch.nn.init.normal_(conv.weight, std=0.05)
    dcn = ConvOffset2d(C, Cout, 3, padding=1, num_deformable_groups=G)
    x = torch.randn(2, C, S, S)
    target = torch.randn(2, Cout, S, S)
    cw_g, dw_g = conv.weight.detach().to(DEV).requires_grad_(True), dcn.weight.detach().to(DEV).requires_grad_(True)
    cw_r, dw_r = conv.weight.detach().double().requires_grad_(True), dcn.weight.detach().double().requires_grad_(True)
    xg, tg, xr, tr = x.to(DEV), target.to(DEV), x.double(), target.double()
    for _ in range(20):
        offg = torch.nn.functional.conv2d(xg, cw_g, padding=1)
        loss = ((conv_offset2d(xg, offg, dw_g, 1, 1, 1, G) - tg) ** 2).mean()
        gc, gd = torch.autograd.grad(loss, (cw_g, dw_g))
        offr = torch.nn.functional.conv2d(xr, cw_r, padding=1)
        offr = offr + (offg.detach().cpu().double() - offr.detach())     # sample where the device sampled
        lr_ = ((gref.deform_conv(xr, offr, dw_r, 1, 1, 1, G) - tr) ** 2).mean()
        rc, rd = torch.autograd.grad(lr_, (cw_r, dw_r))
        with torch.no_grad():
            cw_g -= lr * gc
            dw_g -= lr * gd
            cw_r -= lr * rc
            dw_r -= lr * rd
    for g, r in ((cw_g, cw_r), (dw_g, dw_r)):
        rel = float((g.detach().cpu().double() - r).abs().max()) / max(1e-12, float(r.abs().max()))
        assert rel <= 1e-4, rel
