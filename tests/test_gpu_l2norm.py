"""Trainable L2Norm (tdrn_hip.h section i-e; L2NormFunction / l2norm / L2Norm) against the module's formula on the CPU in float64
with autograd: y = weight x / (sqrt(sum_c x^2) + eps).

Bounds (derived, not tuned).  output, grad_input and grad_weight: |got - ref| <= 1e-4 * max(1, max|ref|), the project's fp32 bound
(test_gpu_batch_norm.py, test_gpu_conv_grad.py).  norm: 1e-5 relative; a plain sequential fp32 sum over the channels stays below
8e-7 on these cases, so any sane summation order has a tenfold margin.  The smallest pixel norm over all cases is 0.030: no case
has a zero pixel but the one that is built for it.  There is no C = 1 case: its true input gradient is a cancellation of two terms of
size weight go / |x| to about 0, which no fp32 evaluation of the formula holds to 1e-4.

At an all-zero pixel the function is weight x / eps and the library returns its true gradient weight go / eps, where torch's autograd
gives NaN (sqrt'(0) * 0): a deliberate, documented difference.
"""
import functools

import pytest
import torch

from tdrn_amd import _lib
from tdrn_amd.layers.modules.l2norm import L2Norm as TorchL2Norm
from tdrn_amd.model import networks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-10

# N, C, H, W
CASES = {
    "tiny_odd": (2, 5, 7, 9),
    "one_pixel": (3, 70, 1, 1),
    "small_maps": (2, 70, 5, 5),
    "conv4_3_like": (2, 512, 10, 10),        # 128 channels per wave, the layers' own count
    "ragged_c": (1, 1030, 4, 6),             # past what a lane keeps in registers, no multiple of anything
    "wide": (1, 3, 64, 130),
    "many_pixels": (4, 6, 40, 40),           # 100 tiles, tiles across image boundaries
}


@functools.lru_cache(maxsize=None)
def _inputs(case, zero_pixel=False):
    """x, weight, grad_output (CPU, fp32)"""
    N, C, H, W = CASES[case]
    gen = torch.Generator().manual_seed(sorted(CASES).index(case) + 61)
    x = torch.randn(N, C, H, W, generator=gen)
    w = 8 + 4 * torch.rand(C, generator=gen)
    go = torch.randn(N, C, H, W, generator=gen)
    if zero_pixel:
        x[1, :, 3, 4] = 0.0
    return x, w, go


def _formula(x, w):
    norm = x.pow(2).sum(dim=1, keepdim=True).sqrt() + EPS
    return w.view(1, -1, 1, 1) * (x / norm), norm[:, 0]


@functools.lru_cache(maxsize=None)
def _reference(case, zero_pixel=False):
    """float64 CPU autograd; computed once, never changed"""
    x, w, go = _inputs(case, zero_pixel)
    x64, w64 = x.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
    y, norm = _formula(x64, w64)
    gx, gw = torch.autograd.grad(y, (x64, w64), go.double())
    return {"output": y.detach(), "norm": norm.detach(), "grad_input": gx, "grad_weight": gw}


def _check(tag, ref, got, mask=None):
    """got: {name: tensor}.  Prints every measured share of its bound before asserting.  mask (N, H, W): the pixels compared"""
    for name, g in got.items():
        r, g = ref[name], g.detach().cpu().double()
        if mask is not None and name in ("output", "grad_input"):
            keep = mask[:, None].expand_as(r)
            r, g = r[keep], g[keep]
        elif mask is not None and name == "norm":
            r, g = r[mask], g[mask]
        d = (g - r).abs()
        assert torch.isfinite(d).all(), "%s %s: non-finite values" % (tag, name)
        bound = 1e-5 * r.abs() if name == "norm" else torch.full_like(r, 1e-4 * max(1.0, float(r.abs().max())))
        share = float((d / bound).max())
        print("%s %-12s max|d| %.3e  worst share of the bound %.4f" % (tag, name, float(d.max()), share))
        assert share <= 1.0, (tag, name, float(d.max()), share)


class Abi(object):
    """the C entries on plain device buffers"""

    def __init__(self, case, zero_pixel=False):
        self.lib, self.dims = _lib.lib(), CASES[case]
        self.nb = self.lib.tdrn_l2norm_workspace_bytes(*self.dims)
        assert self.nb > 0
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.ref = _reference(case, zero_pixel)
        self.x, self.w, self.go = (t.to(DEV) for t in _inputs(case, zero_pixel))
        self.st = _lib.current_stream(DEV)

    def forward(self, out, norm):
        _lib.check(self.lib.tdrn_l2norm_forward(_lib.ptr(self.x), _lib.ptr(self.w), _lib.ptr(out), _lib.ptr(norm), *self.dims, EPS, self.st))

    def backward(self, norm, gi, gw, scale=1.0):
        _lib.check(self.lib.tdrn_l2norm_backward(_lib.ptr(self.x), _lib.ptr(self.go), _lib.ptr(self.w), _lib.ptr(norm), _lib.ptr(gi),
                                                 _lib.ptr(gw), *self.dims, EPS, scale, _lib.ptr(self.ws), self.nb, self.st))

    def all(self):
        N, C, H, W = self.dims
        nan = float("nan")
        r = {"output": torch.full_like(self.x, nan), "norm": torch.full((N, H, W), nan, device=DEV),
             "grad_input": torch.full_like(self.x, nan), "grad_weight": torch.zeros_like(self.w)}
        self.forward(r["output"], r["norm"])
        self.backward(r["norm"], r["grad_input"], r["grad_weight"])
        torch.cuda.synchronize()
        return r


NAMES = ("output", "norm", "grad_input", "grad_weight")


def test_l2norm_cases_have_no_zero_pixel():
    smallest = min(float(_reference(case)["norm"].min()) for case in CASES)
    print("smallest pixel norm over all cases: %.4f" % smallest)
    assert smallest > 0.02


@pytest.mark.parametrize("case", list(CASES))
def test_l2norm_abi_matches_float64_autograd(case):
    a = Abi(case)
    _check(case, a.ref, a.all())


@pytest.mark.parametrize("case", list(CASES))
def test_l2norm_autograd_matches_float64_autograd(case):
    ref = _reference(case)
    x, w, go = (t.to(DEV) for t in _inputs(case))
    x, w = x.requires_grad_(True), w.requires_grad_(True)
    y = networks.l2norm(x, w, EPS)
    y.backward(go)
    _check("%s autograd" % case, ref, {"output": y, "grad_input": x.grad, "grad_weight": w.grad})


def test_l2norm_zero_pixel_has_the_true_gradient():
    a = Abi("tiny_odd", zero_pixel=True)
    r = a.all()
    for name in NAMES:
        assert bool(torch.isfinite(r[name]).all()), name
    assert bool((r["output"][1, :, 3, 4] == 0).all())
    assert float(r["norm"][1, 3, 4]) == pytest.approx(EPS, rel=1e-6)
    want = a.w.cpu().double() * a.go.cpu().double()[1, :, 3, 4] / EPS
    rel = float(((r["grad_input"][1, :, 3, 4].cpu().double() - want) / want).abs().max())
    print("zero pixel grad_input: worst relative error %.3e (bound 1e-6)" % rel)
    assert rel <= 1e-6
    # every other pixel as usual; the bound's max|ref| is taken over those pixels (the reference is NaN at the zero pixel)
    mask = torch.ones(a.dims[0], a.dims[2], a.dims[3], dtype=torch.bool)
    mask[1, 3, 4] = False
    assert bool(torch.isnan(a.ref["grad_input"][1, :, 3, 4]).all()) and bool(torch.isfinite(a.ref["grad_weight"]).all())
    _check("tiny_odd zero pixel", a.ref, r, mask)


def test_l2norm_grad_weight_accumulates_and_the_rest_is_overwritten():
    a = Abi("many_pixels")
    r = a.all()                                   # output, norm and grad_input started at NaN
    for name in NAMES:
        assert bool(torch.isfinite(r[name]).all()), name
    g = r["grad_weight"].clone()
    pre = torch.linspace(-3.0, 5.0, a.dims[1], device=DEV)
    gw = pre.clone()
    a.backward(r["norm"], None, gw, scale=0.5)
    torch.cuda.synchronize()
    # fl(pre + 0.5 s) against pre + 0.5 g with g = fl(s): two roundings of fp32
    assert float((gw - (pre + 0.5 * g)).abs().max()) <= 4 * 2.0 ** -24 * float((pre.abs() + g.abs()).max())
    # a NULL grad_input, or a NULL grad_weight (with no workspace at all), leaves the other result's bits unchanged
    gw3 = torch.zeros_like(a.w)
    a.backward(r["norm"], None, gw3)
    gi3 = torch.full_like(a.x, float("nan"))
    _lib.check(a.lib.tdrn_l2norm_backward(_lib.ptr(a.x), _lib.ptr(a.go), _lib.ptr(a.w), _lib.ptr(r["norm"]), _lib.ptr(gi3), None, *a.dims,
                                          EPS, 1.0, None, 0, a.st))
    torch.cuda.synchronize()
    assert torch.equal(gw3.view(torch.int32), g.view(torch.int32))
    assert torch.equal(gi3.view(torch.int32), r["grad_input"].view(torch.int32))
    # a NULL norm leaves the output the same
    out = torch.full_like(a.x, float("nan"))
    a.forward(out, None)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), r["output"].view(torch.int32))


@pytest.mark.parametrize("case", ["many_pixels", "conv4_3_like"])
def test_l2norm_is_bitwise_reproducible(case):
    a = Abi(case)
    first = a.all()
    Abi("ragged_c").all()                 # other work on the device in between must not change the arithmetic
    second = a.all()
    for name in NAMES:
        assert torch.equal(first[name].view(torch.int32), second[name].view(torch.int32)), name


SENTINEL = 0x7FBADBAD
GUARD = 4096


class Guarded(object):
    """`nbytes` of device memory that start `offset` bytes behind a 256-byte boundary, between two guard bands of a NaN pattern no
    kernel computes (the pattern of test_gpu_batch_norm.py)"""

    def __init__(self, shape=None, offset=0, nbytes=None, init=None):
        n = int(nbytes) if nbytes is not None else 4 * int(torch.Size(shape).numel())
        total = 2 * GUARD + 256 + offset + n
        self.raw = torch.full(((total + 3) // 4,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.uint8)
        base = (-self.raw.data_ptr()) % 256 + GUARD
        self.lo, self.hi = base + offset, base + offset + n
        body = self.raw[self.lo:self.hi]
        self.t = body if shape is None else body.view(torch.float32).view(shape)
        if init is not None:
            self.t.copy_(init)

    def check(self, what, full=True):
        torch.cuda.synchronize()
        words = self.raw.view(torch.int32)
        assert self.lo % 4 == 0 and self.hi % 4 == 0
        assert bool((words[:self.lo // 4] == SENTINEL).all()), "%s: bytes in front of the buffer were written" % what
        assert bool((words[self.hi // 4:] == SENTINEL).all()), "%s: bytes behind the end of the buffer were written" % what
        if full:
            assert int((words[self.lo // 4:self.hi // 4] == SENTINEL).sum()) == 0, "%s: elements never written" % what


@pytest.mark.parametrize("case", ["tiny_odd", "conv4_3_like", "wide"])
def test_l2norm_writes_only_the_callers_buffers(case):
    a = Abi(case)
    want = a.all()
    N, C, H, W = a.dims
    ws = Guarded(nbytes=a.nb)                      # exactly the queried size
    a.ws = ws.t
    assert ws.t.data_ptr() % 256 == 0
    x, go, w = Guarded(a.x.shape, 4, init=a.x), Guarded(a.x.shape, 4, init=a.go), Guarded(a.w.shape, 4, init=a.w)
    a.x, a.go, a.w = x.t, go.t, w.t
    g = {"output": Guarded(a.x.shape, 4), "norm": Guarded((N, H, W), 4), "grad_input": Guarded(a.x.shape, 4),
         "grad_weight": Guarded(a.w.shape, 4, init=torch.zeros(C))}
    assert all(v.t.data_ptr() % 256 == 4 for v in list(g.values()) + [x, go, w])
    a.forward(g["output"].t, g["norm"].t)
    a.backward(g["norm"].t, g["grad_input"].t, g["grad_weight"].t)
    for name in NAMES:
        g[name].check("%s %s" % (case, name))
        assert torch.equal(g[name].t.contiguous().view(torch.int32), want[name].view(torch.int32)), name
    ws.check("%s workspace" % case, full=False)
    for name, b in (("input", x), ("grad_output", go), ("weight", w)):
        b.check("%s %s" % (case, name))


def test_l2norm_autograd_plumbing():
    x0, w0, go = (t.to(DEV) for t in _inputs("tiny_odd"))
    ref = _reference("tiny_odd")
    for need in ((True, False), (False, True), (True, True)):
        x, w = x0.clone().requires_grad_(need[0]), w0.clone().requires_grad_(need[1])
        y = networks.l2norm(x, w)
        assert y.requires_grad
        y.backward(go.transpose(2, 3).contiguous().transpose(2, 3))          # a non-contiguous grad_output
        assert (x.grad is not None) == need[0] and (w.grad is not None) == need[1]
        got = {"output": y}
        if need[0]:
            got["grad_input"] = x.grad
        if need[1]:
            got["grad_weight"] = w.grad
        _check("plumbing %r" % (need,), ref, got)
    x = x0.clone().requires_grad_(True)
    networks.l2norm(x, w0).sum().backward()              # a stride-0 grad_output
    assert bool(torch.isfinite(x.grad).all())
    with torch.no_grad():
        assert networks.l2norm(x0.clone().requires_grad_(True), w0).grad_fn is None
    assert networks.l2norm(x0, w0).grad_fn is None
    with pytest.raises(ValueError):
        networks.l2norm(x0[0], w0)
    with pytest.raises(ValueError):
        networks.l2norm(x0.double(), w0.double())
    with pytest.raises(RuntimeError):
        networks.l2norm(x0, w0[:3])
    # a module left on the CPU: its weight must not reach the library as a host pointer
    m = networks.L2Norm(5, 10)
    with pytest.raises(NotImplementedError):
        m(x0)
    with pytest.raises(NotImplementedError):
        networks.l2norm(x0.cpu(), w0)


def test_l2norm_module_loads_and_follows_the_reference_module():
    ref = TorchL2Norm(512, 10)
    with torch.no_grad():
        ref.weight.uniform_(8, 12)
    ours = networks.L2Norm(512, 10)
    ours.load_state_dict(ref.state_dict(), strict=True)
    ref, ours = ref.to(DEV), ours.to(DEV)
    x = _inputs("conv4_3_like")[0].to(DEV)
    want, got = ref(x).detach(), ours(x).detach()
    d, bound = float((got - want).abs().max()), 1e-4 * max(1.0, float(want.abs().max()))
    print("module forward against the torch formula on the GPU: max|d| %.3e  bound %.3e" % (d, bound))
    assert d <= bound
    ours(x).mean().backward()
    assert ours.weight.grad is not None and ours.weight.grad.shape == (512,)


def test_short_training_run_with_pool_and_l2norm_follows_float64():
    """the construction of test_batch_norm_short_training_run_follows_float64 with MaxPool2d(2, 2) and L2Norm(32, 10) behind the
    BatchNorm: three plain SGD steps in our modules, in torch's fp32 modules on the same GPU and in float64 on the CPU"""
    seed = 6
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 16, 10, 10, generator=gen)
    target = torch.randn(2, 8, 5, 5, generator=gen)

    def torch_net():
        return torch.nn.Sequential(torch.nn.Conv2d(16, 32, 3, padding=1), torch.nn.BatchNorm2d(32), torch.nn.ReLU(), torch.nn.MaxPool2d(2, 2),
                                   TorchL2Norm(32, 10), torch.nn.Conv2d(32, 8, 1))
    torch.manual_seed(seed)
    ref = torch_net()
    with torch.no_grad():
        ref[1].weight.copy_(0.5 + torch.rand(32, generator=gen))
        ref[1].bias.copy_(0.2 * torch.randn(32, generator=gen))
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    ref = ref.double()
    # condition on the reference alone: a pool window with a positive maximum has its top two values more than 1e-4 apart in every
    # float64 step (a near-tie may legitimately fall either way in fp32)
    gaps = []

    def gap(module, args, out):
        v = out.detach().unfold(2, 2, 2).unfold(3, 2, 2).reshape(-1, 4).sort(1, descending=True).values
        pos = v[:, 0] > 0
        gaps.append(float((v[pos, 0] - v[pos, 1]).min()))
    ref[2].register_forward_hook(gap)

    tch = torch_net()
    tch.load_state_dict(state)
    tch = tch.to(DEV)

    class Ours(torch.nn.Module):
        def __init__(self):
            super(Ours, self).__init__()
            self.c1, self.bn, self.pool = networks.Conv2d(16, 32, 3, padding=1), networks.BatchNorm2d(32, relu=True), networks.MaxPool2d(2, 2)
            self.l2, self.c2 = networks.L2Norm(32, 10), networks.Conv2d(32, 8, 1)

        def forward(self, v):
            return self.c2(self.l2(self.pool(self.bn(self.c1(v)))))
    ours = Ours()
    names = {"0": "c1", "1": "bn", "4": "l2", "5": "c2"}
    ours.load_state_dict({names[k.split(".")[0]] + "." + k.split(".", 1)[1]: v for k, v in state.items()})
    ours = ours.to(DEV)

    def loop(net, x, target):
        net.train()
        losses = []
        for _ in range(3):
            loss = ((net(x) - target) ** 2).mean()
            grads = torch.autograd.grad(loss, list(net.parameters()))
            with torch.no_grad():
                for p, g in zip(net.parameters(), grads):
                    p -= 0.1 * g
            losses.append(float(loss.detach()))
        return losses

    l_ours, l_tch, l_ref = loop(ours, x.to(DEV), target.to(DEV)), loop(tch, x.to(DEV), target.to(DEV)), loop(ref, x.double(), target.double())
    print("pool windows' smallest top-two gaps in the float64 steps: %r" % (gaps,))
    assert len(gaps) == 3 and min(gaps) > 1e-4, "a near-tie in a pool window of the float64 net: change the seed (%r)" % (gaps,)
    for l in (l_ours, l_tch, l_ref):
        assert l[0] > l[1] > l[2], l
    so, st, sr = ours.state_dict(), tch.state_dict(), ref.state_dict()
    assert len(so) == len(sr)
    for ko, kr in zip(so, sr):
        if kr.endswith("num_batches_tracked"):
            continue
        r = sr[kr]
        d_ours = float((so[ko].cpu().double() - r).abs().max())
        d_torch = float((st[kr].cpu().double() - r).abs().max())
        bound = max(4 * d_torch, 1e-5 * max(1.0, float(r.abs().max())))
        print("training run %-22s ours %.3e  torch-GPU %.3e  bound %.3e" % (kr, d_ours, d_torch, bound))
        assert d_ours <= bound, (kr, d_ours, d_torch, bound)
