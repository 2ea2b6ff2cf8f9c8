"""BatchNorm2d with a fused ReLU on resident tensors (tdrn_hip.h section i-k: tdrn_batch_norm_nhwc_*) against float64 on the CPU.

Inputs (x, grad_output) are exact 16-bit values; gamma, beta and the running buffers are fp32.  Bounds (u, tiny: tests/_nhwc_harness.py):
output and grad_input u |ref| + 1e-4 max(1, max|ref|) + tiny (the fp32 NCHW op's bound and one rounding of the result); grad_weight and
grad_bias 1e-4 max(1, max|ref|); save_mean and running_mean 1e-5 max(1, |ref|); save_invstd and running_var 1e-5 relative
(tests/test_gpu_batch_norm.py's bounds).

ReLU kink, by that file's rule: an element whose float64 pre-activation lies within tau = 1e-4 max(1, max|y_ref|) of zero may fall on
either side; grad_output is set to exactly 0 there for the op and the reference alike, the reference alone decides which elements
those are, and they are at most 1 % of a case.

Shapes are C x M with M = N H W pixel rows: one row short of, at and one past the 32 rows a workgroup covers per pass; three channel
blocks; 25 splits; 1024 channels with two splits; a channel whose mean is about 1000 times its standard deviation and a constant channel.  Every
shape runs in training and in eval mode (eval also with one value per channel), with and without the ReLU, in both types."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _conv_train_harness import DEV
from _nhwc_harness import TINY, TYPES, U, GuardedResident, bn_backward, bn_forward, exact, nchw64, raw_equal, resident

pytestmark = pytest.mark.gpu
EPS, MOMENTUM = 1e-5, 0.1
MODES = ("bf16", "fp16")

# N, C, H, W
CASES = {"m2": (1, 64, 1, 2), "rows31": (1, 64, 31, 1), "rows32": (1, 64, 32, 1), "rows33": (1, 64, 33, 1), "blocks3": (2, 192, 5, 5),
         "splits25": (1, 128, 80, 80), "wide": (3, 1024, 10, 10), "special": (2, 64, 9, 9)}
TRAIN_CASES = sorted(CASES)
CASES["one_value"] = (1, 64, 1, 1)          # eval mode only
EVAL_CASES = TRAIN_CASES + ["one_value"]


@functools.lru_cache(maxsize=None)
def inputs(case, mode):
    N, C, H, W = CASES[case]
    gen = torch.Generator().manual_seed(sorted(CASES).index(case) * 2 + MODES.index(mode) + 41)
    x = torch.randn(N, C, H, W, generator=gen)
    if case == "special":
        # mean about 950 standard deviations, exact in both types (bf16's spacing at 1024 is 8): 1024 everywhere but 1032 at 3 of the
        # 162 pixels, which land in different rows of the sweep
        c3 = torch.full((N * H * W,), 1024.0)
        c3[[5, 70, 140]] = 1032.0
        x[:, 3] = c3.view(N, H, W)
        x[:, 5] = 0.75                                                                                 # a constant channel
    x = exact(x, mode)
    w = 0.5 + torch.rand(C, generator=gen)
    b = 0.2 * torch.randn(C, generator=gen) + 0.05
    go = exact(torch.randn(N, C, H, W, generator=gen), mode)
    rm = 0.5 * torch.randn(C, generator=gen)
    rv = 0.5 + torch.rand(C, generator=gen)
    if case == "special":
        rm[3], rv[3] = 1024.0, 1.0          # running statistics that have followed the channel (eval mode normalises with them)
    return x, w, b, go, rm, rv


@functools.lru_cache(maxsize=None)
def reference(case, mode, relu, training):
    """float64 on the CPU, written out (F.batch_norm's arithmetic) -> dict of references and the grad_output both sides use"""
    x, w, b, go, rm, rv = (t.double() for t in inputs(case, mode))
    M = x.numel() // x.shape[1]
    dims = (0, 2, 3)
    sh = (1, -1, 1, 1)
    if training:
        mean, var = x.mean(dims), x.var(dims, unbiased=False)
    else:
        mean, var = rm, rv
    invstd = (var + EPS).rsqrt()
    xhat = (x - mean.view(sh)) * invstd.view(sh)
    z = xhat * w.view(sh) + b.view(sh)
    y = z.clamp_min(0) if relu else z
    go_used = go.clone()
    if relu:
        tau = 1e-4 * max(1.0, float(y.abs().max()))
        near = z.abs() <= tau
        share = float(near.double().mean())
        assert share <= 0.01, "%s %s: %.2f %% of the elements sit on the ReLU kink: change the seed" % (case, mode, 100 * share)
        go_used[near] = 0.0
    dy = go_used * (z > 0) if relu else go_used
    gb, gw = dy.sum(dims), (dy * xhat).sum(dims)
    a = (w * invstd).view(sh)
    gx = a * (dy - (gb.view(sh) + xhat * gw.view(sh)) / M) if training else a * dy
    ref = {"output": y, "grad_input": gx, "grad_weight": gw, "grad_bias": gb, "go": go_used.float(), "save_mean": mean, "save_invstd": invstd}
    if training:
        ref.update(running_mean=(1 - MOMENTUM) * rm + MOMENTUM * mean, running_var=(1 - MOMENTUM) * rv + MOMENTUM * var * M / (M - 1))
    else:
        ref.update(running_mean=rm, running_var=rv)
    return ref


def test_reference_kink_shares_hold_for_every_case():
    """(no device work) the seeds keep the kink elements below 1 % in every case this file runs, and the `special` case's channel 3
    has a mean of 700 to 1500 standard deviations"""
    for mode in MODES:
        c = inputs("special", mode)[0][:, 3].double()
        assert 700 <= float(c.mean() / c.std(unbiased=False)) <= 1500, float(c.mean() / c.std(unbiased=False))
    for mode in MODES:
        for case in TRAIN_CASES:
            reference(case, mode, True, True)
        for case in EVAL_CASES:
            reference(case, mode, True, False)


def check(tag, mode, ref, got):
    for name, g in got.items():
        r = ref[name]
        g = nchw64(g) if g.dim() == 4 else g.detach().cpu().double()
        d = (g - r).abs()
        assert torch.isfinite(g).all(), "%s %s: non-finite values" % (tag, name)
        top = 1e-4 * max(1.0, float(r.abs().max()))
        if name in ("output", "grad_input"):
            bound = U[mode] * r.abs() + top + TINY[mode]
        elif name in ("grad_weight", "grad_bias"):
            bound = torch.full_like(r, top)
        elif name in ("save_mean", "running_mean"):
            bound = 1e-5 * r.abs().clamp_min(1.0)
        else:
            bound = 1e-5 * r.abs()
        ratio = float((d / bound).max())
        print("%s %-12s max|d| %.3e  worst ratio to the bound %.4f" % (tag, name, float(d.max()), ratio))
        assert ratio <= 1.0, (tag, name, float(d.max()), ratio)


def run(case, mode, relu, training, guarded=False, want=("gi", "gp")):
    x, w, b, _, rm, rv = inputs(case, mode)
    ref = reference(case, mode, relu, training)
    xr, gor = resident(x, mode), resident(ref["go"], mode)
    wd, bd = w.to(DEV), b.to(DEV)
    nan = float("nan")
    r = {"save_mean": torch.full_like(wd, nan), "save_invstd": torch.full_like(wd, nan), "running_mean": rm.to(DEV).clone(),
         "running_var": rv.to(DEV).clone(), "grad_weight": torch.zeros_like(wd), "grad_bias": torch.zeros_like(wd)}
    guards = []
    if guarded:
        guards = [GuardedResident(x.shape, mode), GuardedResident(x.shape, mode)]
        r["output"], r["grad_input"] = guards[0].t, guards[1].t
    else:
        r["output"], r["grad_input"] = torch.full_like(xr, nan), torch.full_like(xr, nan)
    bn_forward(xr, wd, bd, r["running_mean"], r["running_var"], r["output"], r["save_mean"], r["save_invstd"], training, MOMENTUM, EPS, relu, mode)
    gi = r["grad_input"] if "gi" in want else None
    gw, gb = (r["grad_weight"], r["grad_bias"]) if "gp" in want else (None, None)
    bn_backward(xr, gor, wd, bd, r["save_mean"], r["save_invstd"], gi, gw, gb, training, relu, 1.0, mode)
    torch.cuda.synchronize()
    for g, what in zip(guards, ("output", "grad_input")):
        g.check("%s %s %s" % (case, mode, what))
    return r, ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", TRAIN_CASES)
def test_training_against_float64(case, relu, mode):
    r, ref = run(case, mode, relu, True, guarded=True)
    check("%s %s relu=%d train" % (case, mode, relu), mode, ref, r)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", EVAL_CASES)
def test_eval_against_float64(case, relu, mode):
    r, ref = run(case, mode, relu, False, guarded=True)
    check("%s %s relu=%d eval" % (case, mode, relu), mode, ref, r)
    _, _, _, _, rm, rv = inputs(case, mode)
    assert torch.equal(r["running_mean"].cpu(), rm) and torch.equal(r["running_var"].cpu(), rv)        # read, not moved


@pytest.mark.parametrize("case", ["splits25", "wide", "rows33"])
def test_bitwise_reproducible_and_null_arguments(case):
    a, _ = run(case, "bf16", True, True)
    b, _ = run(case, "bf16", True, True)
    for k in a:
        assert (raw_equal(a[k], b[k]) if a[k].dim() == 4 else torch.equal(a[k], b[k])), k
    # a NULL grad_input or a NULL parameter pair drops kernels and changes no bit of the rest
    only_p, _ = run(case, "bf16", True, True, want=("gp",))
    only_i, _ = run(case, "bf16", True, True, want=("gi",))
    assert torch.equal(only_p["grad_weight"], a["grad_weight"]) and torch.equal(only_p["grad_bias"], a["grad_bias"])
    assert raw_equal(only_i["grad_input"], a["grad_input"])
    assert bool(torch.isnan(only_p["grad_input"].float()).all()) and not bool(only_i["grad_weight"].any())


def test_running_buffers_may_be_null_in_training():
    case, mode = "blocks3", "fp16"
    a, _ = run(case, mode, False, True)
    x, w, b, _, _, _ = inputs(case, mode)
    xr, wd, bd = resident(x, mode), w.to(DEV), b.to(DEV)
    out, sm, si = torch.empty_like(xr), torch.empty_like(wd), torch.empty_like(wd)
    bn_forward(xr, wd, bd, None, None, out, sm, si, True, MOMENTUM, EPS, False, mode)
    torch.cuda.synchronize()
    assert raw_equal(out, a["output"]) and torch.equal(sm, a["save_mean"]) and torch.equal(si, a["save_invstd"])


@pytest.mark.parametrize("mode", MODES)
def test_nan_stays_nan_through_the_relu(mode):
    x, w, b, _, rm, rv = inputs("rows33", mode)
    x = x.clone()
    x[0, 7, 4, 0] = float("nan")
    xr, wd, bd = resident(x, mode), w.to(DEV), b.to(DEV)
    out, sm, si = torch.empty_like(xr), torch.empty_like(wd), torch.empty_like(wd)
    bn_forward(xr, wd, bd, rm.to(DEV), rv.to(DEV), out, sm, si, False, MOMENTUM, EPS, True, mode)
    torch.cuda.synchronize()
    nan = torch.isnan(out.float())
    assert bool(nan[0, 7, 4, 0]) and int(nan.sum()) == 1 and out.dtype == TYPES[mode]
