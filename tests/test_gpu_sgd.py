"""tdrn_amd.optim.SGD on the card against the numpy fp32 restatement of tdrn_hip.h section (i-j) (tests/_sgd_ref.py), bit for bit:
p and the momentum buffer are compared as int32 views after every step.

Sizes sit around the kernel's paths: below one 16-byte vector, a vector and its numel % 4 tail, one wave, a chunk
(_lib.SGD_CHUNK elements, the unit a workgroup takes) minus / plus one, several chunks; lists around the number of tensors one
launch carries (_lib.SGD_TENSORS_PER_LAUNCH)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _sgd_ref as R
from tdrn_amd import _lib
from tdrn_amd.optim import SGD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK, K = _lib.SGD_CHUNK, _lib.SGD_TENSORS_PER_LAUNCH
SIZES = [1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
MODES = {"no_momentum": dict(momentum=0.0), "momentum": dict(momentum=0.9), "nesterov": dict(momentum=0.9, nesterov=True)}


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).reshape(-1).view(np.int32)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, what
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d" % (what, bad.size, g.size, bad[0])


def _randn(n, seed, scale=1.0):
    return (scale * torch.randn(n, generator=torch.Generator().manual_seed(seed))).float()


@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("mode", list(MODES))
def test_three_steps_at_every_size(mode, wd):
    hp = dict(lr=4e-3, weight_decay=wd, **MODES[mode])
    params = [torch.nn.Parameter(_randn(n, 100 + i).to(DEV)) for i, n in enumerate(SIZES)]
    ref_p = [p.detach().cpu().numpy().copy() for p in params]
    ref_b = [np.zeros_like(a) for a in ref_p]
    opt = SGD(params, **hp)
    for step in range(3):
        for i, p in enumerate(params):
            g = _randn(p.numel(), 1000 * step + i)
            p.grad = g.to(DEV)
            ref_p[i], ref_b[i] = R.sgd_step(ref_p[i], g.numpy(), ref_b[i], **hp)
        assert opt.step() is None
        for i, p in enumerate(params):
            _same(p, ref_p[i], "%s wd %g: p of numel %d after step %d" % (mode, wd, p.numel(), step))
            _same(opt.state[p]["momentum_buffer"], ref_b[i], "%s wd %g: b of numel %d after step %d" % (mode, wd, p.numel(), step))
    assert opt.step(lambda: 1.5) == 1.5                       # the closure's value comes back, as torch's step gives it


@pytest.mark.parametrize("off", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 0, 0)], ids=lambda o: "p%d_g%d_b%d" % o)
def test_views_four_bytes_into_a_buffer_and_their_guard_bands(off):
    """p, g and b each start 64 (+ 1) floats into a larger buffer: a tensor with any of the three off the 16-byte grid takes the
    scalar path.  64 floats on either side of each must keep their bits."""
    n, guard = CHUNK + 5, 64
    hp = dict(lr=0.05, momentum=0.9, weight_decay=5e-4, nesterov=True)
    sentinel = float(np.array([0x4B1234AB], np.int32).view(np.float32)[0])
    bufs, views = [], []
    for o in off:
        buf = torch.full((guard + o + n + guard,), sentinel, device=DEV)
        bufs.append(buf)
        views.append(buf[guard + o:guard + o + n])
    p0, g0, b0 = _randn(n, 1), _randn(n, 2), _randn(n, 3)
    for v, src in zip(views, (p0, g0, b0)):
        v.copy_(src.to(DEV))
    assert [v.data_ptr() % 16 for v in views] == [4 * o for o in off]
    p = torch.nn.Parameter(views[0])
    assert p.data_ptr() == views[0].data_ptr()
    p.grad = views[1]
    opt = SGD([p], **hp)
    opt.state[p]["momentum_buffer"] = views[2]
    opt.step()
    rp, rb = R.sgd_step(p0.numpy(), g0.numpy(), b0.numpy(), **hp)
    _same(views[0], rp, "p")
    _same(views[2], rb, "b")
    _same(views[1], g0, "g")
    for name, buf, o in zip("pgb", bufs, off):
        inside = torch.zeros(buf.numel(), dtype=torch.bool)
        inside[guard + o:guard + o + n] = True
        band = buf.cpu()[~inside]
        assert band.numel() == 2 * guard + o
        assert bool((band.view(torch.int32) == 0x4B1234AB).all()), "the guard band of %s was written" % name


@pytest.mark.parametrize("count", [1, K, K + 1, 2 * K + 3])
def test_lists_split_into_launches_two_groups_interleaved(count):
    sizes = [(1, 2, 3, 4, 5, 7, 8, 13, 64, 67, 130, 257)[(5 * i) % 12] for i in range(count)]
    hps = [dict(lr=4e-3, momentum=0.9, weight_decay=5e-4, nesterov=False), dict(lr=0.05, momentum=0.0, weight_decay=0.0, nesterov=False)]
    if count > 1:
        hps[1] = dict(lr=0.05, momentum=0.5, weight_decay=1e-2, nesterov=True)
    params = [torch.nn.Parameter(_randn(n, 10 + i).to(DEV)) for i, n in enumerate(sizes)]
    no_grad = torch.nn.Parameter(_randn(9, 5).to(DEV))
    empty = torch.nn.Parameter(torch.zeros(0, device=DEV))
    empty.grad = torch.zeros(0, device=DEV)
    groups = [{"params": params[0::2], **hps[0]}, {"params": params[1::2] + [no_grad], **hps[1]}]
    groups[0]["params"] = groups[0]["params"][:1] + [empty] + groups[0]["params"][1:]
    opt = SGD(groups, lr=1.0)
    keep = no_grad.detach().clone()
    grads = [_randn(n, 500 + i) for i, n in enumerate(sizes)]
    for p, g in zip(params, grads):
        p.grad = g.to(DEV)
    want = [R.sgd_step(p.detach().cpu().numpy(), g.numpy(), np.zeros(n, np.float32), **hps[i % 2])
            for i, (p, g, n) in enumerate(zip(params, grads, sizes))]
    opt.step()
    for i, (p, (rp, rb)) in enumerate(zip(params, want)):
        _same(p, rp, "p of tensor %d of %d (numel %d, group %d)" % (i, count, sizes[i], i % 2))
        _same(opt.state[p]["momentum_buffer"], rb, "b of tensor %d of %d" % (i, count))
    _same(no_grad, keep, "the parameter without a gradient")
    assert no_grad.grad is None and "momentum_buffer" not in opt.state[no_grad]
    assert empty.numel() == 0 and empty.grad.numel() == 0


@pytest.mark.parametrize("count", [1, K, K + 1, 2 * K + 3])
def test_one_call_with_the_groups_interleaved_record_by_record(count):
    """tdrn_sgd_step itself: record i belongs to group i % 2; one record in the middle has a null grad, one has numel 0"""
    sizes = [(1, 2, 3, 4, 5, 7, 8, 13, 64, 67, 130, 257)[(7 * i) % 12] for i in range(count)]
    hps = [dict(lr=4e-3, momentum=0.9, weight_decay=5e-4, nesterov=False), dict(lr=0.05, momentum=0.5, weight_decay=1e-2, nesterov=True)]
    hyper = torch.tensor([[h["lr"], h["momentum"], h["weight_decay"], float(h["nesterov"])] for h in hps], device=DEV)
    p0, g0, b0 = ([_randn(n, s + i) for i, n in enumerate(sizes)] for s in (0, 300, 600))
    p, g, b = ([t.to(DEV) for t in ts] for ts in (p0, g0, b0))
    skipped = {count // 2: "null grad", count // 3: "numel 0"} if count > 2 else {}
    recs = (_lib.SgdTensor * count)()
    for i, r in enumerate(recs):
        r.param, r.grad, r.momentum_buf, r.numel, r.group = p[i].data_ptr(), g[i].data_ptr(), b[i].data_ptr(), sizes[i], i % 2
        if skipped.get(i) == "null grad":
            r.grad = None
        elif skipped.get(i) == "numel 0":
            r.numel = 0
    _lib.check(_lib.lib().tdrn_sgd_step(ctypes.cast(recs, ctypes.c_void_p), count, _lib.ptr(hyper), 2, 0, _lib.current_stream(DEV)))
    torch.cuda.synchronize()
    for i in range(count):
        rp, rb = (p0[i].numpy(), b0[i].numpy()) if i in skipped else R.sgd_step(p0[i].numpy(), g0[i].numpy(), b0[i].numpy(), **hps[i % 2])
        _same(p[i], rp, "p of record %d of %d (%s)" % (i, count, skipped.get(i, "numel %d" % sizes[i])))
        _same(b[i], rb, "b of record %d of %d" % (i, count))
        _same(g[i], g0[i], "g of record %d of %d" % (i, count))


def test_zero_grads_leaves_plus_zero_in_place_and_off_leaves_the_grads_alone():
    sizes = [5, 64, CHUNK + 1, 2 * CHUNK + 7]
    for zero in (True, False):
        params = [torch.nn.Parameter(_randn(n, i).to(DEV)) for i, n in enumerate(sizes)]
        grads = [-_randn(n, 50 + i).abs() for i, n in enumerate(sizes)]        # all negative: a zero that kept its sign would show
        for p, g in zip(params, grads):
            p.grad = g.to(DEV)
        odd = torch.full((CHUNK + 6,), 7.0, device=DEV)                          # one gradient on the scalar path
        params[2].grad = odd[1:CHUNK + 2].copy_(grads[2].to(DEV))
        ptrs = [p.grad.data_ptr() for p in params]
        opt = SGD(params, lr=4e-3, momentum=0.9, zero_grads=zero)
        opt.step()
        for i, (p, g, n) in enumerate(zip(params, grads, sizes)):
            rp, _ = R.sgd_step(_randn(n, i).numpy(), g.numpy(), np.zeros(n, np.float32), lr=4e-3, momentum=0.9)
            _same(p, rp, "p (zero_grads=%s)" % zero)
            if zero:
                assert not _bits(p.grad).any(), "zero_grads=True must leave +0 (all bits clear) in every gradient element"
            else:
                _same(p.grad, g, "the gradient with zero_grads=False")
        opt.zero_grad()
        if zero:
            assert [p.grad.data_ptr() for p in params] == ptrs           # still allocated, still there
            assert float(odd[0]) == 7.0 and bool((odd[CHUNK + 2:] == 7.0).all())
        else:
            assert all(p.grad is None for p in params)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_gradient_element_reaches_only_its_own_element(bad):
    n, at = CHUNK + 9, [0, 5, CHUNK - 1, CHUNK + 8]
    hp = dict(lr=4e-3, momentum=0.9, weight_decay=5e-4)
    p0, g0 = _randn(n, 1), _randn(n, 2)
    g0[at] = bad
    p = torch.nn.Parameter(p0.to(DEV))
    p.grad = g0.to(DEV)
    opt = SGD([p], **hp)
    opt.step()
    rp, rb = R.sgd_step(p0.numpy(), g0.numpy(), np.zeros(n, np.float32), **hp)
    finite_p, finite_b = torch.isfinite(p.detach().cpu()), torch.isfinite(opt.state[p]["momentum_buffer"].cpu())
    hit = torch.zeros(n, dtype=torch.bool)
    hit[at] = True
    assert torch.equal(~finite_p, hit) and torch.equal(~finite_b, hit)
    ok = (~hit).numpy()
    _same(p.detach().cpu().numpy()[ok], rp[ok], "p away from the bad elements")
    _same(opt.state[p]["momentum_buffer"].cpu().numpy()[ok], rb[ok], "b away from the bad elements")
    assert np.array_equal(p.detach().cpu().numpy()[~ok], rp[~ok], equal_nan=True)      # (a NaN's payload is not compared)


MODELS = [("dualrefinedet_vggbn", dict(multihead=True)), ("dualrefinedet_mobilenet", {}), ("ssd4scale_vgg", {}),
          ("ssd4scale_mobile", {}), ("refinedet_vgg", {})]


@pytest.mark.parametrize("model,kw", MODELS, ids=[m for m, _ in MODELS])
def test_two_steps_on_a_real_parameter_set(model, kw):
    """every parameter of build_net('train', 320, 21), random gradients, the reference's hyper-parameters; no forward is run"""
    hp = dict(lr=4e-3, momentum=0.9, weight_decay=5e-4)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        net = importlib.import_module("tdrn_amd.model." + model).build_net("train", 320, 21, **kw)
    host = [p.detach().numpy().copy() for p in net.parameters()]
    net = net.to(DEV)
    params = list(net.parameters())
    opt = SGD(params, **hp)
    gen = torch.Generator().manual_seed(17)
    bufs = [np.zeros_like(a) for a in host]
    for step in range(2):
        for i, p in enumerate(params):
            g = torch.randn(p.shape, generator=gen)
            p.grad = g.to(DEV)
            host[i], bufs[i] = R.sgd_step(host[i], g.numpy(), bufs[i], **hp)
        opt.step()
    torch.cuda.synchronize()
    bad = [i for i, p in enumerate(params)
           if not (np.array_equal(_bits(p), _bits(host[i])) and np.array_equal(_bits(opt.state[p]["momentum_buffer"]), _bits(bufs[i])))]
    assert not bad, "%s: tensors %r of %d differ from the restatement" % (model, bad[:10], len(params))


def test_step_on_a_side_stream_gives_the_same_bits():
    sizes = [3, 65, CHUNK + 1, 2 * CHUNK + 7] * 30             # two launches
    hp = dict(lr=4e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    outs = []
    for how in ("default", "side"):
        params = [torch.nn.Parameter(_randn(n, i).to(DEV)) for i, n in enumerate(sizes)]
        opt = SGD(params, **hp)
        side = torch.cuda.Stream(DEV)
        for step in range(2):
            for i, p in enumerate(params):
                p.grad = _randn(p.numel(), 1000 * step + i).to(DEV)
            torch.cuda.synchronize()
            if how == "side":
                a = torch.ones(2048, 2048, device=DEV)
                for _ in range(8):
                    a = (a @ a) * 2.0 ** -11                   # unrelated work on the default stream that nothing waits for
                with torch.cuda.stream(side):
                    opt.step()
                side.synchronize()
                assert bool(torch.isfinite(a).all())
            else:
                opt.step()
        torch.cuda.synchronize()
        outs.append([(p.detach().clone(), opt.state[p]["momentum_buffer"].clone()) for p in params])
    for i, ((p0, b0), (p1, b1)) in enumerate(zip(*outs)):
        _same(p1, p0, "p of tensor %d" % i)
        _same(b1, b0, "b of tensor %d" % i)
    first = outs[0][0][0].cpu()
    assert not torch.equal(first, _randn(sizes[0], 0))         # the steps moved something
