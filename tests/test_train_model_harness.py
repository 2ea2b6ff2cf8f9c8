"""tests/_train_model_harness.py's checks proved on the CPU (no GPU) before they judge forward_train: each passes a correct input and
fails a doctored one.  Synthetic tensors only."""
import copy

import numpy as np
import pytest
import torch

import _train_model_harness as H

YARD = 2.0 ** -7            # the synthetic float32 yardstick's relative distance, exact in binary: bound = 10 * YARD = 0.078125


def _gradients():
    """-> (ours, the float64 log entry, [two float32 log entries]): three one-element tensors, so that every relative L2 distance is a
    ratio the test sets exactly; z.bias cancels in front of the BatchNorm bn"""
    ref = {"grads": {"a.weight": torch.tensor([4.0], dtype=torch.float64), "b.weight": torch.tensor([-2.0], dtype=torch.float64),
                     "bn.bias": torch.tensor([8.0, -16.0], dtype=torch.float64), "z.bias": torch.tensor([1e-17, 0.0], dtype=torch.float64)},
           "abs_go": {"z.bias": torch.tensor([3.0, 5.0], dtype=torch.float64)}}
    scaled = lambda f, z: {"grads": {n: ((g * f).float() if n != "z.bias" else torch.full((2,), z)) for n, g in ref["grads"].items()}}
    yards = [scaled(1 + YARD, 1e-7), scaled(1 - YARD / 2, 0.0)]              # the larger of the two is the yardstick
    ours = scaled(1 + 4 * YARD, 1e-6)["grads"]                               # inside 10 x, and |z.bias| inside both bias rules
    return ours, ref, yards


def _check(ours, ref, yards, cap=0.1, inclusive=True, rule="abs_go", extra=()):
    rule = H.AbsGoRule(["z.bias"], each=False) if rule == "abs_go" else H.BnBiasRule({"z.bias": "bn"})
    H.gradient_check("synthetic", ours, ref, yards, extra, cap, inclusive, rule)


@pytest.mark.parametrize("rule", ["abs_go", "bn_bias"])
def test_gradient_check_passes_correct_gradients(rule, capsys):
    ours, ref, yards = _gradients()
    r = torch.tensor([2.0], dtype=torch.float64)
    _check(ours, ref, yards, rule=rule, extra=[("leaf", torch.tensor([2.0 + 9 * YARD]), r, [r.float() * (1 + YARD / 4)])])
    out = capsys.readouterr().out
    assert "float32 yardstick worst 7.812e-03 (a.weight), bound 7.812e-02" in out and "ours worst 3.516e-02 (leaf)" in out


def test_gradient_check_fails_a_tensor_beyond_ten_yardsticks():
    ours, ref, yards = _gradients()
    ours["b.weight"] = ours["b.weight"] * (1 + 11 * YARD) / (1 + 4 * YARD)
    with pytest.raises(AssertionError, match="b.weight"):
        _check(ours, ref, yards)
    ours, ref, yards = _gradients()
    r = torch.tensor([2.0], dtype=torch.float64)
    with pytest.raises(AssertionError, match="leaf"):            # an extra tensor is held to the same bound
        _check(ours, ref, yards, extra=[("leaf", torch.tensor([2.0 + 22 * YARD]), r, [r.float()])])


def test_gradient_check_fails_a_yardstick_over_the_cap():
    ours, ref, yards = _gradients()
    _check(ours, ref, yards, cap=10 * YARD, inclusive=True)      # a bound AT the cap: the inclusive cap takes it,
    with pytest.raises(AssertionError, match="uninformative"):
        _check(ours, ref, yards, cap=10 * YARD, inclusive=False)  # the strict one does not
    for inclusive in (True, False):
        with pytest.raises(AssertionError, match="uninformative"):
            _check(ours, ref, yards, cap=9.99 * YARD, inclusive=inclusive)


def test_gradient_check_fails_a_cancelling_bias_over_its_bound():
    ours, ref, yards = _gradients()
    ours["z.bias"] = torch.tensor([1e-6, 2e-6 * 5.0 * 1.01])     # channel 1 over 2e-6 sum|grad_output|
    with pytest.raises(AssertionError, match="z.bias"):
        _check(ours, ref, yards, rule="abs_go")
    _check(ours, ref, yards, rule="bn_bias")                     # 1e-5 is inside 1e-4 max(1, 16)
    ours["z.bias"] = torch.tensor([1e-6, 1e-4 * 16.0 * 1.01])
    with pytest.raises(AssertionError, match="z.bias"):
        _check(ours, ref, yards, rule="bn_bias")
    ours, ref, yards = _gradients()
    ref["grads"]["z.bias"][0] = 1e-11                            # the abs_go rule holds only where float64 itself cancels
    with pytest.raises(AssertionError, match="z.bias"):
        _check(ours, ref, yards, rule="abs_go")


def test_gradient_check_fails_a_missing_gradient():
    for how in ("none", "absent", "nan"):
        ours, ref, yards = _gradients()
        if how == "absent":
            del ours["a.weight"]
        else:
            ours["a.weight"] = None if how == "none" else torch.tensor([float("nan")])
        with pytest.raises(AssertionError, match="a.weight"):
            _check(ours, ref, yards)


def test_rows_off():
    ref = torch.zeros(1, 40, 4, dtype=torch.float64)
    got = ref.float().clone()
    got[0, 3, 1], got[0, 7, 0], got[0, 9, 2] = 5e-3, 0.5, 9e-4
    allowed = np.zeros(40, bool)
    assert H.rows_off(got, ref, allowed, 1e-3) == (2, pytest.approx(9e-4))       # both bad rows are on no discontinuity
    allowed[7] = True
    assert H.rows_off(got, ref, allowed, 1e-3) == (1, pytest.approx(9e-4))       # row 3 still counts
    allowed[:30] = True
    assert H.rows_off(got, ref, allowed, 1e-3)[0] == 0                           # 30 rows on a discontinuity: the most it takes
    allowed[30] = True
    with pytest.raises(AssertionError, match="31 rows"):
        H.rows_off(got, ref, allowed, 1e-3)
    assert H.train_atol(torch.tensor([0.5, -0.25])) == 1e-4 and H.train_atol(torch.tensor([3.0, -50.0])) == pytest.approx(5e-3)


def test_running_statistics_check(capsys):
    ref = {"bn.running_mean": torch.tensor([0.5, -20.0], dtype=torch.float64), "bn.running_var": torch.tensor([0.9, 1.1], dtype=torch.float64),
           "bn.num_batches_tracked": torch.tensor(1)}
    got = {k: (v.float() if v.is_floating_point() else v.clone()) for k, v in ref.items()}
    got["bn.running_mean"][1] += 1e-3                            # inside 1e-4 max(1, 20)
    H.running_statistics_check("synthetic", got, ref)
    assert "train synthetic: running statistics, worst |d| / bound" in capsys.readouterr().out
    moved = copy.deepcopy(got)
    moved["bn.running_var"][0] += 2e-4
    with pytest.raises(AssertionError, match="running_var"):
        H.running_statistics_check("synthetic", moved, ref)
    for ours, theirs in ((2, 1), (0, 1), (1, 2)):
        with pytest.raises(AssertionError, match="num_batches_tracked"):
            H.running_statistics_check("synthetic", dict(got, **{"bn.num_batches_tracked": torch.tensor(ours)}),
                                       dict(ref, **{"bn.num_batches_tracked": torch.tensor(theirs)}))


def test_short_run_check():
    want, yard = [3.0, 2.0, 1.5], [3.0, 2.001, 1.498]
    H.short_run_check([3.00002, 2.009, 1.49], want, yard, 3)     # step 0 on the floor 1e-5 max(1, 3); steps 1 and 2 inside 10 x
    with pytest.raises(AssertionError):
        H.short_run_check([3.0, 2.0, 2.0], want, yard, 3)        # ours does not fall
    with pytest.raises(AssertionError):
        H.short_run_check([3.0, 2.0, 1.5], [3.0, 2.0, 2.0], [3.0, 2.0, 2.0], 3)      # float64 does not fall
    with pytest.raises(AssertionError):
        H.short_run_check([3.0, 2.011, 1.5], want, yard, 3)      # step 1 beyond 10 x |yardstick - float64|
    with pytest.raises(AssertionError):
        H.short_run_check([3.0001, 2.0, 1.5], want, yard, 3)     # step 0 beyond the floor
    with pytest.raises(AssertionError):
        H.short_run_check([3.0, 2.0], want, yard, 3)             # a step missing


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv, self.bn, self.unused = torch.nn.Conv2d(1, 1, 1), torch.nn.BatchNorm2d(1), torch.nn.Conv2d(1, 1, 1)


def test_plumbing():
    def net(filled, tracked=1):
        n = _Net()
        for name, p in n.named_parameters():
            if name.split(".")[0] in filled:
                p.grad = torch.zeros_like(p)
        n.bn.num_batches_tracked += tracked
        return n

    out = (torch.zeros(1, 6, 4), None, torch.zeros(1, 6, 4), torch.zeros(1, 6, 21))
    like = net(("conv", "bn"))
    H.plumbing(net(("conv", "bn")), out, like, 6, counters=True, exact=True)
    H.plumbing(net(("conv", "bn", "unused")), out, like, 6, counters=True, exact=False)
    with pytest.raises(AssertionError, match="unused"):
        H.plumbing(net(("conv", "bn", "unused")), out, like, 6, counters=True, exact=True)
    with pytest.raises(AssertionError, match="bn"):
        H.plumbing(net(("conv",)), out, like, 6, counters=False, exact=False)
    H.plumbing(net(("conv", "bn"), 2), out, like, 6, counters=False, exact=True)
    with pytest.raises(AssertionError, match="num_batches_tracked"):
        H.plumbing(net(("conv", "bn"), 2), out, like, 6, counters=True, exact=True)
    with pytest.raises(AssertionError):
        H.plumbing(net(("conv", "bn")), out[:1] + (torch.zeros(1),) + out[2:], like, 6, counters=True, exact=True)
    with pytest.raises(AssertionError):
        H.plumbing(net(("conv", "bn")), (out[0], None, out[2], torch.full((1, 6, 21), float("inf"))), like, 6, counters=True, exact=True)
