"""tdrn_amd.optim without a GPU: the constructor, the state dict and the schedules behave like torch.optim.SGD's and the
reference's, and the numpy restatement the GPU tests compare with (tests/_sgd_ref.py) is torch.optim.SGD's step up to rounding.

The bound of the last test, per element:
    |dp| <= 2^-22 (|p| + 2 lr (|g| + wd |p| + c mom |b| + [nesterov] mom (|g| + wd |p|))),   c = 2 with nesterov, else 1
A rounding bound: one ulp of the result at a binade edge plus the roundings of the update's own operations, which torch's
add(alpha=) contracts and the restatement does not.  It does not come from the outcome; the worst measured ratio to it is 0.53.
The momentum buffer's own bound is 2^-22 (mom |b| + |g| + wd |p|): its two roundings and the one inside d."""
import numpy as np
import pytest
import torch

import _sgd_ref as R
from tdrn_amd import optim


def _params(shapes=((3, 4), (5,), (2, 3, 2, 2)), seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-4),
                                dict(lr=0.1, nesterov=True), dict(lr=0.1, nesterov=True, momentum=0.0)])
def test_constructor_refuses_what_torch_refuses(kw):
    with pytest.raises(ValueError):
        torch.optim.SGD(_params(), **kw)
    with pytest.raises(ValueError):
        optim.SGD(_params(), **kw)


def test_constructor_refuses_what_the_kernel_does_not_cover():
    with pytest.raises(ValueError, match="lr, momentum, weight_decay and nesterov"):
        optim.SGD(_params(), lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match="lr, momentum, weight_decay and nesterov"):
        optim.SGD(_params(), lr=0.1, maximize=True)
    with pytest.raises(ValueError, match="dampening"):
        optim.SGD([{"params": _params()[:1]}, {"params": _params()[1:], "dampening": 0.5}], lr=0.1, momentum=0.9)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError):
            optim.SGD([torch.nn.Parameter(torch.zeros(4, dtype=dt))], lr=0.1)
    with pytest.raises(ValueError, match="contiguous"):
        optim.SGD([torch.nn.Parameter(torch.zeros(4, 6).t())], lr=0.1)
    with pytest.raises(ValueError):
        optim.SGD([], lr=0.1)                                   # torch: "optimizer got an empty parameter list"


@pytest.mark.parametrize("kw", [dict(), dict(lr=0.05), dict(lr=4e-3, momentum=0.9, weight_decay=5e-4),
                                dict(lr=0.1, momentum=0.5, nesterov=True)])
def test_defaults_and_group_keys_equal_torchs(kw):
    ours, theirs = optim.SGD(_params(), **kw), torch.optim.SGD(_params(), **kw)
    assert ours.defaults == theirs.defaults
    assert isinstance(ours, torch.optim.Optimizer)
    for a, b in zip(ours.param_groups, theirs.param_groups):
        assert list(a) == list(b)
        assert {k: v for k, v in a.items() if k != "params"} == {k: v for k, v in b.items() if k != "params"}
    two = optim.SGD([{"params": _params()[:1], "lr": 0.5}, {"params": _params()[1:], "weight_decay": 1e-2}], lr=0.1, momentum=0.9)
    assert [g["lr"] for g in two.param_groups] == [0.5, 0.1] and [g["weight_decay"] for g in two.param_groups] == [0, 1e-2]


def test_step_refuses_cpu_parameters_and_state_dict_works_there():
    ps = _params()
    opt = optim.SGD(ps, lr=0.1, momentum=0.9)
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(NotImplementedError):
        opt.step()
    with pytest.raises(NotImplementedError):
        opt.sync_hyper()
    assert all(torch.equal(a, p) for a, p in zip(before, ps))   # no CPU fall-back moved anything
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["lr"] == 0.1
    opt.zero_grad()
    assert all(p.grad is None for p in ps)                      # zero_grads=False: torch's zero_grad
    held = optim.SGD(ps, lr=0.1, zero_grads=True)
    for p in ps:
        p.grad = torch.ones_like(p)
    held.zero_grad()
    assert all(p.grad is not None for p in ps)                  # zero_grads=True: the step does it, zero_grad() does nothing


def test_state_dict_goes_to_torch_and_back():
    kw = dict(lr=4e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    # torch -> ours: after a torch step, with real buffers
    tp = _params()
    theirs = torch.optim.SGD(tp, foreach=False, **kw)
    for p in tp:
        p.grad = torch.randn_like(p)
    theirs.step()
    sd = theirs.state_dict()
    op = _params()
    ours = optim.SGD(op, lr=1.0)
    ours.load_state_dict(sd)
    assert {k: v for k, v in ours.param_groups[0].items() if k != "params"} == \
        {k: v for k, v in theirs.param_groups[0].items() if k != "params"}
    for a, b in zip(op, tp):
        assert torch.equal(ours.state[a]["momentum_buffer"], theirs.state[b]["momentum_buffer"])
    # ours -> torch
    back = torch.optim.SGD(_params(), lr=1.0)
    back.load_state_dict(ours.state_dict())
    assert back.state_dict()["param_groups"] == sd["param_groups"]
    for k, st in sd["state"].items():
        assert torch.equal(back.state_dict()["state"][k]["momentum_buffer"], st["momentum_buffer"])
    # ours -> ours
    again = optim.SGD(_params(), lr=1.0)
    again.load_state_dict(ours.state_dict())
    assert again.state_dict()["param_groups"] == ours.state_dict()["param_groups"]
    # a buffer of None (torch's state before a momentum step) loads as zeros
    sd_none = {"state": {k: {"momentum_buffer": None} for k in sd["state"]}, "param_groups": sd["param_groups"]}
    fresh_p = _params()
    fresh = optim.SGD(fresh_p, lr=1.0)
    fresh.load_state_dict(sd_none)
    for p in fresh_p:
        b = fresh.state[p]["momentum_buffer"]
        assert b.shape == p.shape and b.dtype == torch.float32 and not bool(b.any())
    # what the kernel does not cover is refused on loading too
    bad = {"state": {}, "param_groups": [dict(sd["param_groups"][0], dampening=0.5, nesterov=False)]}
    with pytest.raises(ValueError, match="dampening"):
        optim.SGD(_params(), lr=1.0).load_state_dict(bad)


def test_schedules_restate_the_reference():
    base, gamma, epoch_size, warm = 4e-3, 0.1, 517, 5
    for epoch in (0, 1, 4, 5, 6, 40):
        for it in (0, 1, epoch * epoch_size, epoch * epoch_size + 516):
            for si in (0, 1, 3):
                got = optim.warmup_step_lr(base, gamma, epoch, si, it, epoch_size, warm)
                assert got == R.warmup_step_lr(base, gamma, epoch, si, it, epoch_size, warm)
    # the boundary: epoch == warm_epoch is still warm-up (train.py:323, `<=`), the next epoch is the step schedule
    it = warm * epoch_size
    assert optim.warmup_step_lr(base, gamma, warm, 2, it, epoch_size, warm) == 1e-6 + (base - 1e-6) * it / (epoch_size * warm)
    assert optim.warmup_step_lr(base, gamma, warm + 1, 2, it, epoch_size, warm) == base * gamma ** 2
    assert optim.warmup_step_lr(base, gamma, 0, 0, 0, epoch_size, warm) == 1e-6
    for si in range(5):
        assert optim.step_lr(base, gamma, si) == R.step_lr(base, gamma, si) == base * (gamma ** si)


HYPER_SETS = [dict(lr=4e-3, momentum=0.9, weight_decay=5e-4, nesterov=False),
              dict(lr=1e-6, momentum=0.9, weight_decay=5e-4, nesterov=True),
              dict(lr=0.05, momentum=0.0, weight_decay=0.0, nesterov=False),
              dict(lr=1.0, momentum=0.5, weight_decay=1e-2, nesterov=True),
              dict(lr=4e-3, momentum=0.0, weight_decay=1e-2, nesterov=False),
              dict(lr=0.05, momentum=0.5, weight_decay=0.0, nesterov=False)]


@pytest.mark.parametrize("scale", [1e-3, 1.0, 30.0])
@pytest.mark.parametrize("hp", HYPER_SETS)
def test_restatement_equals_torch_sgd_up_to_rounding(hp, scale):
    n = 200003
    gen = torch.Generator().manual_seed(11)
    p0, g, b0 = (scale * torch.randn(n, generator=gen) for _ in range(3))
    p = torch.nn.Parameter(p0.clone())
    p.grad = g.clone()
    opt = torch.optim.SGD([p], foreach=False, **hp)
    if hp["momentum"] != 0:
        opt.state[p]["momentum_buffer"] = b0.clone()
    opt.step()
    rp, rb = R.sgd_step(p0.numpy(), g.numpy(), b0.numpy(), **hp)
    lr, mom, wd = hp["lr"], hp["momentum"], hp["weight_decay"]
    ap, ag, ab = (t.double().abs().numpy() for t in (p0, g, b0))
    d = ag + wd * ap
    bound = 2.0 ** -22 * (ap + 2 * lr * (d + (2 if hp["nesterov"] else 1) * mom * ab + (mom * d if hp["nesterov"] else 0)))
    err = np.abs(p.detach().double().numpy() - rp.astype(np.float64))
    ratio = float((err / bound).max())
    print("hyper %r scale %g: %d of %d elements differ, worst ratio to the bound %.3f" % (hp, scale, int((err > 0).sum()), n, ratio))
    assert ratio <= 1.0
    if mom != 0:
        berr = np.abs(opt.state[p]["momentum_buffer"].double().numpy() - rb.astype(np.float64))
        assert float((berr / (2.0 ** -22 * (mom * ab + d))).max()) <= 1.0
