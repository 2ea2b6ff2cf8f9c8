"""BatchNorm2d with a fused ReLU (tdrn_hip.h section i-d; BatchNormFunction / batch_norm / BatchNorm2d) against torch's CPU
autograd in float64.

Oracle: F.batch_norm (+ F.relu) on the CPU in float64, differentiated by autograd; nn.BatchNorm2d in float64 for the running
buffers after one training forward.

Bounds (derived, not tuned).  output and the three gradients: |got - ref| <= 1e-4 * max(1, max|ref|), the project's fp32 bound
(test_gpu_conv_grad.py, test_gpu_deform_grad.py).  save_mean and the updated running_mean: 1e-5 * max(1, |ref|) elementwise;
save_invstd and the updated running_var: 1e-5 relative.  A chunked fp32 Welford scheme stays below 7.2 % of the first and 6 % of
the others on these shapes; a sum / sum-of-squares kernel misses them by one to three orders of magnitude on the offset_mean cases.

ReLU kink: an element whose float64 pre-activation lies within tau = 1e-4 * max(1, max|y_ref|) of zero may fall on either side in
fp32.  grad_output is set to exactly 0 there, for the op and the oracle alike, so no element is exempted from any comparison; the
reference alone decides which elements those are, and they are at most 1 % of a case (expected: about 1e-4).
"""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tdrn_amd import _lib
from tdrn_amd.model import networks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, MOMENTUM = 1e-5, 0.1

# N, C, H, W, input mean, input std
CASES = {
    "tiny_odd": (2, 5, 7, 9, 0.0, 1.0),                  # H W = 63: no plane but the first is 16-byte aligned
    "m2": (2, 3, 1, 1, 0.0, 1.0),                        # the smallest legal count, unbiased factor 2
    "one_pixel_maps": (6, 70, 1, 1, 0.0, 1.0),           # H W = 1, more than 64 channels
    "small_maps": (2, 70, 5, 5, 0.0, 1.0),               # H W = 25
    "conv7_like": (3, 130, 10, 10, 0.0, 1.0),            # aligned 400-byte planes, ragged channel count
    "multi_split": (4, 3, 40, 40, 0.0, 1.0),             # more than one split (DESIGN 12 lists 2)
    "one_wide_plane": (1, 2, 64, 130, 0.0, 1.0),         # N = 1: the splits cut inside a plane
    "offset_mean": (3, 4, 33, 31, 30.0, 0.25),           # cancellation in the variance; H W = 1023
    "offset_mean_split": (32, 2, 40, 40, 30.0, 0.25),    # cancellation across the split merge
}
TRAIN_CASES = list(CASES)
# eval mode only: one value per channel is legal there
CASES["one_pixel_n1"] = (1, 70, 1, 1, 0.0, 1.0)
EVAL_CASES = ["tiny_odd", "conv7_like", "one_pixel_maps", "one_pixel_n1"]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """x, gamma, beta, grad_output, and non-trivial starting values of the running buffers (CPU, fp32)"""
    N, C, H, W, mean, std = CASES[case]
    gen = torch.Generator().manual_seed(sorted(CASES).index(case) + 23)
    x = mean + std * torch.randn(N, C, H, W, generator=gen)
    w = 0.5 + torch.rand(C, generator=gen)
    b = 0.2 * torch.randn(C, generator=gen)
    go = torch.randn(N, C, H, W, generator=gen)
    rm = mean + 0.5 * torch.randn(C, generator=gen)
    rv = 0.5 + torch.rand(C, generator=gen)
    return x, w, b, go, rm, rv


@functools.lru_cache(maxsize=None)
def _reference(case, relu, training):
    """float64 CPU autograd -> dict of references and the grad_output both sides use; computed once, never changed"""
    N, C, H, W, _, _ = CASES[case]
    x, w, b, go, rm, rv = _inputs(case)
    x64, w64, b64 = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    z = F.batch_norm(x64, None if training else rm.double(), None if training else rv.double(), w64, b64, training, MOMENTUM, EPS)
    y = F.relu(z) if relu else z
    go_used = go.clone()
    if relu:
        tau = 1e-4 * max(1.0, float(y.detach().abs().max()))
        near = z.detach().abs() <= tau
        share = float(near.double().mean())
        assert share <= 0.01, "%s: %.2f %% of the elements sit on the ReLU kink: change the seed" % (case, 100 * share)
        go_used[near] = 0.0
    gx, gw, gb = torch.autograd.grad(y, (x64, w64, b64), go_used.double())
    ref = {"output": y.detach(), "grad_input": gx, "grad_weight": gw, "grad_bias": gb, "go": go_used}
    if training:
        m = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).double()
        m.load_state_dict({"weight": w.double(), "bias": b.double(), "running_mean": rm.double(), "running_var": rv.double(),
                           "num_batches_tracked": torch.tensor(0)})
        m.train()(x.double())
        xd = x.double()
        ref.update(save_mean=xd.mean((0, 2, 3)), save_invstd=(xd.var((0, 2, 3), unbiased=False) + EPS).rsqrt(),
                   running_mean=m.running_mean.clone(), running_var=m.running_var.clone())
    else:
        ref.update(save_mean=rm.double(), save_invstd=(rv.double() + EPS).rsqrt(), running_mean=rm.double(), running_var=rv.double())
    return ref


KIND = {"output": "fp32", "grad_input": "fp32", "grad_weight": "fp32", "grad_bias": "fp32", "save_mean": "abs5", "running_mean": "abs5",
        "save_invstd": "rel5", "running_var": "rel5"}


def _check(tag, ref, got):
    """got: {name: tensor}.  Prints every measured ratio to its bound before asserting"""
    for name, g in got.items():
        r = ref[name]
        d = (g.detach().cpu().double() - r).abs()
        assert torch.isfinite(d).all(), "%s %s: non-finite values" % (tag, name)
        if KIND[name] == "fp32":
            bound = torch.full_like(r, 1e-4 * max(1.0, float(r.abs().max())))
        elif KIND[name] == "abs5":
            bound = 1e-5 * r.abs().clamp_min(1.0)
        else:
            bound = 1e-5 * r.abs()
        ratio = float((d / bound).max())
        print("%s %-12s max|d| %.3e  worst ratio to the bound %.4f" % (tag, name, float(d.max()), ratio))
        assert ratio <= 1.0, (tag, name, float(d.max()), ratio)


class Abi(object):
    """the C entries on plain device buffers"""

    def __init__(self, case, relu, training=True):
        N, C, H, W, _, _ = CASES[case]
        self.lib, self.dims, self.relu, self.training = _lib.lib(), (N, C, H, W), int(relu), int(training)
        self.nb = self.lib.tdrn_batch_norm_workspace_bytes(*self.dims)
        assert self.nb > 0
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.ref = _reference(case, bool(relu), bool(training))
        self.x, self.w, self.b, _, self.rm0, self.rv0 = (t.to(DEV) for t in _inputs(case))
        self.go = self.ref["go"].to(DEV)
        self.st = _lib.current_stream(DEV)

    def forward(self, out, save_mean, save_invstd, rm, rv):
        _lib.check(self.lib.tdrn_batch_norm_forward(_lib.ptr(self.x), _lib.ptr(self.w), _lib.ptr(self.b), _lib.ptr(rm), _lib.ptr(rv),
                                                    _lib.ptr(out), _lib.ptr(save_mean), _lib.ptr(save_invstd), *self.dims, self.training,
                                                    MOMENTUM, EPS, self.relu, _lib.ptr(self.ws), self.nb, self.st))

    def backward(self, save_mean, save_invstd, gi, gw, gb, scale=1.0):
        _lib.check(self.lib.tdrn_batch_norm_backward(_lib.ptr(self.x), _lib.ptr(self.go), _lib.ptr(self.w), _lib.ptr(self.b),
                                                     _lib.ptr(save_mean), _lib.ptr(save_invstd), _lib.ptr(gi), _lib.ptr(gw), _lib.ptr(gb),
                                                     *self.dims, self.training, self.relu, scale, _lib.ptr(self.ws), self.nb, self.st))

    def all(self):
        nan = float("nan")
        r = {"output": torch.full_like(self.x, nan), "save_mean": torch.full_like(self.w, nan), "save_invstd": torch.full_like(self.w, nan),
             "running_mean": self.rm0.clone(), "running_var": self.rv0.clone(), "grad_input": torch.full_like(self.x, nan),
             "grad_weight": torch.zeros_like(self.w), "grad_bias": torch.zeros_like(self.w)}
        self.forward(r["output"], r["save_mean"], r["save_invstd"], r["running_mean"], r["running_var"])
        self.backward(r["save_mean"], r["save_invstd"], r["grad_input"], r["grad_weight"], r["grad_bias"])
        torch.cuda.synchronize()
        return r


NAMES = ("output", "save_mean", "save_invstd", "running_mean", "running_var", "grad_input", "grad_weight", "grad_bias")


def _design_table():
    """DESIGN.md section 12's table of split counts: {case: ((N, C, H, W), splits)}"""
    rows = {}
    for m in re.finditer(r"^\| `(\w+)` \| (\d+), (\d+), (\d+), (\d+) \| \d+ \| \d+ \| (\d+) \|", open(os.path.join(ROOT, "DESIGN.md")).read(),
                         re.M):
        rows[m.group(1)] = (tuple(int(m.group(i)) for i in range(2, 6)), int(m.group(6)))
    return rows


def _splits(dims):
    """from the query: 12 C splits + 8 C bytes (tdrn_hip.h)"""
    nb, C = _lib.lib().tdrn_batch_norm_workspace_bytes(*dims), dims[1]
    assert (nb - 8 * C) % (12 * C) == 0
    return (nb - 8 * C) // (12 * C)


def test_batch_norm_split_counts_are_the_design_table():
    table = _design_table()
    for case in TRAIN_CASES:
        dims = CASES[case][:4]
        assert table[case][0] == dims, case
        assert _splits(dims) == table[case][1], case
    assert _splits(CASES["multi_split"][:4]) > 1 and _splits(CASES["offset_mean_split"][:4]) > 1
    assert _splits(CASES["one_wide_plane"][:4]) > 1           # one plane, cut inside


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", TRAIN_CASES)
def test_batch_norm_abi_matches_float64_autograd(case, relu):
    a = Abi(case, relu)
    _check("%s relu=%d" % (case, relu), a.ref, a.all())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", EVAL_CASES)
def test_batch_norm_eval_mode_uses_the_running_buffers_and_leaves_them_alone(case, relu):
    a = Abi(case, relu, training=False)
    r = a.all()
    for name, start in (("running_mean", a.rm0), ("running_var", a.rv0)):
        assert torch.equal(r[name].view(torch.int32), start.view(torch.int32)), name
    assert torch.equal(r["save_mean"], a.rm0)
    _check("%s eval relu=%d" % (case, relu), a.ref, r)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", TRAIN_CASES)
def test_batch_norm_autograd_matches_float64_autograd(case, relu):
    ref = _reference(case, relu, True)
    x, w, b, _, rm, rv = (t.to(DEV) for t in _inputs(case))
    x, w, b = (t.requires_grad_(True) for t in (x, w, b))
    y = networks.batch_norm(x, rm, rv, w, b, True, MOMENTUM, EPS, relu=relu)
    y.backward(ref["go"].to(DEV))
    _check("%s autograd relu=%d" % (case, relu), ref, {"output": y, "grad_input": x.grad, "grad_weight": w.grad, "grad_bias": b.grad,
                                                       "running_mean": rm, "running_var": rv})


def test_batch_norm_module_in_both_modes():
    case = "tiny_odd"
    N, C, H, W, _, _ = CASES[case]
    x, w, b, _, rm, rv = _inputs(case)
    state = {"weight": w, "bias": b, "running_mean": rm, "running_var": rv, "num_batches_tracked": torch.tensor(0)}
    for relu in (False, True):
        m = networks.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM, relu=relu)
        m.load_state_dict(state)
        m = m.to(DEV)
        xg = x.to(DEV).requires_grad_(True)
        ref = _reference(case, relu, True)
        y = m(xg)
        y.backward(ref["go"].to(DEV))
        assert int(m.num_batches_tracked) == 1 and m._batches == 1
        _check("%s module train relu=%d" % (case, relu), ref,
               {"output": y, "grad_input": xg.grad, "grad_weight": m.weight.grad, "grad_bias": m.bias.grad,
                "running_mean": m.running_mean, "running_var": m.running_var})
        # eval mode, from the starting buffers again
        m.load_state_dict(state)
        m.eval()
        m.zero_grad()
        xg = x.to(DEV).requires_grad_(True)
        ref = _reference(case, relu, False)
        y = m(xg)
        y.backward(ref["go"].to(DEV))
        assert int(m.num_batches_tracked) == 0
        assert torch.equal(m.running_mean.cpu(), rm) and torch.equal(m.running_var.cpu(), rv)
        _check("%s module eval relu=%d" % (case, relu), ref,
               {"output": y, "grad_input": xg.grad, "grad_weight": m.weight.grad, "grad_bias": m.bias.grad})


def test_batch_norm_module_cumulative_average():
    case = "tiny_odd"
    N, C, H, W, _, _ = CASES[case]
    x, w, b, _, rm, rv = _inputs(case)
    state = {"weight": w, "bias": b, "running_mean": rm, "running_var": rv, "num_batches_tracked": torch.tensor(0)}
    m = networks.BatchNorm2d(C, eps=EPS, momentum=None)
    m.load_state_dict(state)
    m = m.to(DEV)
    r = torch.nn.BatchNorm2d(C, eps=EPS, momentum=None).double()
    r.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in state.items()})
    gen = torch.Generator().manual_seed(77)
    for step in range(3):
        xs = x * (1.0 + 0.5 * step) + 0.3 * step + 0.1 * torch.randn(x.shape, generator=gen)
        with torch.no_grad():
            y = m(xs.to(DEV))
        yr = r(xs.double())
        assert int(m.num_batches_tracked) == step + 1 == int(r.num_batches_tracked)
        ref = {"output": yr.detach(), "running_mean": r.running_mean.clone(), "running_var": r.running_var.clone()}
        _check("cumulative step %d" % step, ref, {"output": y, "running_mean": m.running_mean, "running_var": m.running_var})


@pytest.mark.parametrize("relu", [0, 1])
def test_batch_norm_constant_channel(relu):
    a = Abi("small_maps", relu)
    a.x = a.x.clone()
    a.x[:, 0] = 0.7
    r = a.all()
    for name in NAMES:
        assert bool(torch.isfinite(r[name]).all()), name
    beta0 = float(a.b[0])
    want = max(beta0, 0.0) if relu else beta0
    y64 = F.batch_norm(a.x.cpu().double(), None, None, a.w.cpu().double(), a.b.cpu().double(), True, MOMENTUM, EPS)
    bound = 1e-4 * max(1.0, float((F.relu(y64) if relu else y64).abs().max()))
    d = float((r["output"][:, 0].double() - want).abs().max())
    print("constant channel relu=%d: max|d| %.3e  bound %.3e" % (relu, d, bound))
    assert d <= bound
    assert float((r["save_mean"][0].double() - 0.7).abs()) <= 1e-5


def test_batch_norm_parameter_gradients_accumulate_and_the_rest_is_overwritten():
    a = Abi("multi_split", 1)
    r = a.all()
    gw, gb = r["grad_weight"], r["grad_bias"]
    gw1, gb1 = gw.clone(), gb.clone()
    a.backward(r["save_mean"], r["save_invstd"], None, gw, gb, scale=0.5)
    torch.cuda.synchronize()
    # fl(g + fl(0.5 s)) against 1.5 g with g = fl(s): two roundings of fp32
    for got, one in ((gw, gw1), (gb, gb1)):
        assert float((got - 1.5 * one).abs().max()) <= 4 * 2.0 ** -24 * float(one.abs().max())
    # output and grad_input over NaN-filled buffers: finite, and equal between two calls
    r2 = a.all()
    for name in ("output", "grad_input"):
        assert bool(torch.isfinite(r2[name]).all()), name
        assert torch.equal(r[name].view(torch.int32), r2[name].view(torch.int32)), name
    # a NULL grad_input, or a NULL parameter pair, leaves the other result the same
    gw3, gb3 = torch.zeros_like(a.w), torch.zeros_like(a.w)
    a.backward(r["save_mean"], r["save_invstd"], None, gw3, gb3)
    gi3 = torch.full_like(a.x, float("nan"))
    a.backward(r["save_mean"], r["save_invstd"], gi3, None, None)
    torch.cuda.synchronize()
    assert torch.equal(gw3.view(torch.int32), gw1.view(torch.int32)) and torch.equal(gb3.view(torch.int32), gb1.view(torch.int32))
    assert torch.equal(gi3.view(torch.int32), r["grad_input"].view(torch.int32))
    _check("multi_split accumulate", a.ref, {"grad_weight": gw1, "grad_bias": gb1})


@pytest.mark.parametrize("case", ["multi_split", "offset_mean_split"])
def test_batch_norm_is_bitwise_reproducible(case):
    a = Abi(case, 1)
    first = a.all()
    Abi("conv7_like", 1).all()            # other work on the device in between must not change the arithmetic
    second = a.all()
    for name in NAMES:
        assert torch.equal(first[name].view(torch.int32), second[name].view(torch.int32)), name


SENTINEL = 0x7FBADBAD
GUARD = 4096


class Guarded(object):
    """`nbytes` of device memory that start `offset` bytes behind a 256-byte boundary, between two guard bands of a NaN pattern no
    kernel computes (the pattern of test_gpu_conv_grad.py)"""

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


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", ["tiny_odd", "conv7_like", "one_wide_plane"])
def test_batch_norm_writes_only_the_callers_buffers(case, relu):
    a = Abi(case, relu)
    want = a.all()
    ws = Guarded(nbytes=a.nb)                      # exactly the queried size
    a.ws = ws.t
    assert ws.t.data_ptr() % 256 == 0
    x, go = Guarded(a.x.shape, offset=4, init=a.x), Guarded(a.x.shape, offset=4, init=a.go)
    a.x, a.go = x.t, go.t
    g = {"output": Guarded(a.x.shape, offset=4), "save_mean": Guarded(a.w.shape, offset=4), "save_invstd": Guarded(a.w.shape, offset=4),
         "running_mean": Guarded(a.w.shape, offset=4, init=a.rm0), "running_var": Guarded(a.w.shape, offset=4, init=a.rv0),
         "grad_input": Guarded(a.x.shape, offset=4), "grad_weight": Guarded(a.w.shape, offset=4, init=torch.zeros_like(a.w)),
         "grad_bias": Guarded(a.w.shape, offset=4, init=torch.zeros_like(a.w))}
    assert all(v.t.data_ptr() % 256 == 4 for v in g.values()) and a.x.data_ptr() % 256 == 4
    a.forward(g["output"].t, g["save_mean"].t, g["save_invstd"].t, g["running_mean"].t, g["running_var"].t)
    a.backward(g["save_mean"].t, g["save_invstd"].t, g["grad_input"].t, g["grad_weight"].t, g["grad_bias"].t)
    for name in NAMES:
        g[name].check("%s relu=%d %s" % (case, relu, name))
        assert torch.equal(g[name].t.contiguous().view(torch.int32), want[name].view(torch.int32)), name
    ws.check("%s workspace" % case, full=False)
    x.check("%s input" % case)
    go.check("%s grad_output" % case)


def test_batch_norm_autograd_plumbing():
    case = "tiny_odd"
    N, C, H, W, _, _ = CASES[case]
    x0, w0, b0, _, rm0, rv0 = (t.to(DEV) for t in _inputs(case))
    for need in ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        x, w, b = (t.clone().requires_grad_(n) for t, n in zip((x0, w0, b0), need))
        y = networks.batch_norm(x, rm0.clone(), rv0.clone(), w, b, True, relu=True)
        assert y.requires_grad
        y.sum().backward()                           # a stride-0 grad_output
        for t, n in zip((x, w, b), need):
            assert (t.grad is not None) == n
    with torch.no_grad():
        assert networks.batch_norm(x0.clone().requires_grad_(True), rm0.clone(), rv0.clone(), w0, b0, True).grad_fn is None
    assert networks.batch_norm(x0, rm0.clone(), rv0.clone(), w0, b0, True).grad_fn is None
    # the gradient of sum(y) against float64, without running buffers
    x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
    y = networks.batch_norm(x, None, None, w, b, True, relu=False)
    y.sum().backward()
    xr, wr, br = (t.cpu().double().requires_grad_(True) for t in (x0, w0, b0))
    yr = F.batch_norm(xr, None, None, wr, br, True, MOMENTUM, EPS)
    yr.sum().backward()
    for got, ref in ((y, yr), (x.grad, xr.grad), (w.grad, wr.grad), (b.grad, br.grad)):
        assert float((got.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-4 * max(1.0, float(ref.detach().abs().max()))
    with pytest.raises(ValueError):
        networks.batch_norm(x0[0], rm0, rv0, w0, b0, True)                                   # 3-D
    with pytest.raises(ValueError):
        networks.batch_norm(x0[:1, :, :1, :1].contiguous(), rm0, rv0, w0, b0, True)          # one value per channel in training
    assert networks.batch_norm(x0[:1, :, :1, :1].contiguous(), rm0, rv0, w0, b0, False).shape == (1, C, 1, 1)
    with pytest.raises(ValueError):
        networks.batch_norm(x0, None, None, w0, b0, False)                                   # eval mode needs the running buffers
    # a module left on the CPU: its parameters must not reach the library as host pointers
    m = networks.BatchNorm2d(C, relu=True)
    with pytest.raises(NotImplementedError):
        m(x0)
    assert int(m.num_batches_tracked) == 0
    m = m.to(DEV)
    m(x0).mean().backward()
    assert m.weight.grad is not None and m.bias.grad is not None and int(m.num_batches_tracked) == 1


def test_batch_norm_short_training_run_follows_float64():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 10, 10, generator=gen)
    target = torch.randn(2, 8, 10, 10, generator=gen)
    torch.manual_seed(5)
    ref = torch.nn.Sequential(torch.nn.Conv2d(16, 32, 3, padding=1), torch.nn.BatchNorm2d(32), torch.nn.ReLU(),
                              torch.nn.Conv2d(32, 8, 1))
    with torch.no_grad():
        ref[1].weight.copy_(0.5 + torch.rand(32, generator=gen))
        ref[1].bias.copy_(0.2 * torch.randn(32, generator=gen))
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    ref = ref.double()

    tch = torch.nn.Sequential(torch.nn.Conv2d(16, 32, 3, padding=1), torch.nn.BatchNorm2d(32), torch.nn.ReLU(), torch.nn.Conv2d(32, 8, 1))
    tch.load_state_dict(state)
    tch = tch.to(DEV)

    class Ours(torch.nn.Module):
        def __init__(self):
            super(Ours, self).__init__()
            self.c1, self.bn, self.c2 = networks.Conv2d(16, 32, 3, padding=1), networks.BatchNorm2d(32, relu=True), networks.Conv2d(32, 8, 1)

        def forward(self, v):
            return self.c2(self.bn(self.c1(v)))
    ours = Ours()
    names = {"0": "c1", "1": "bn", "3": "c2"}
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
    for l in (l_ours, l_tch, l_ref):
        assert l[0] > l[1] > l[2], l
    assert int(ours.bn.num_batches_tracked) == 3
    so, st, sr = ours.state_dict(), tch.state_dict(), ref.state_dict()
    for ko, kr in zip(so, sr):
        if kr.endswith("num_batches_tracked"):
            continue
        r = sr[kr]
        d_ours = float((so[ko].cpu().double() - r).abs().max())
        d_torch = float((st[kr].cpu().double() - r).abs().max())
        bound = max(4 * d_torch, 1e-5 * max(1.0, float(r.abs().max())))
        print("training run %-22s ours %.3e  torch-GPU %.3e  bound %.3e" % (kr, d_ours, d_torch, bound))
        assert d_ours <= bound, (kr, d_ours, d_torch, bound)
