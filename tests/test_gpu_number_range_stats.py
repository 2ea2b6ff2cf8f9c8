"""BatchNorm in training mode (fp32 NCHW: tdrn_batch_norm_*; resident 16-bit NHWC: tdrn_batch_norm_nhwc_*) and L2Norm (tdrn_l2norm_*)
over the whole number range, against float64 on the same inputs.

Draws, references and bounds: tests/_number_range_stats.py (its docstrings derive every constant; test_number_range_stats_ref.py checks
them on the CPU).  Every bound is a derived rounding bound, cast_interval around one, bit equality or same_class; none has a floor.
Each test prints the worst share of every bound it asserts.
"""
import numpy as np
import pytest
import torch

import _number_range_stats as S
from _number_range import TYPES, all16, cast_interval, inside, same_class, to_bits, worst_share
from tdrn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BN_NAMES = ("output", "save_mean", "save_invstd", "running_mean", "running_var", "grad_input", "grad_weight", "grad_bias")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- BatchNorm, fp32 NCHW ------------------------------------------------------------------------------------------------------------
def bn_run(inputs, go, eps, relu):
    """the two C entries on plain device buffers, outputs NaN-prefilled -> {name: tensor}"""
    lib = _lib.lib()
    x, w, b, _, rm, rv = (t.to(DEV) for t in inputs)
    go = go.to(DEV)
    dims = tuple(x.shape)
    nb = lib.tdrn_batch_norm_workspace_bytes(*dims)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = _lib.current_stream(DEV)
    nan = float("nan")
    r = {"output": torch.full_like(x, nan), "save_mean": torch.full_like(w, nan), "save_invstd": torch.full_like(w, nan),
         "running_mean": rm.clone(), "running_var": rv.clone(), "grad_input": torch.full_like(x, nan),
         "grad_weight": torch.zeros_like(w), "grad_bias": torch.zeros_like(w)}
    _lib.check(lib.tdrn_batch_norm_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(r["running_mean"]), _lib.ptr(r["running_var"]),
                                           _lib.ptr(r["output"]), _lib.ptr(r["save_mean"]), _lib.ptr(r["save_invstd"]), *dims, 1,
                                           S.BN_MOMENTUM, eps, int(relu), _lib.ptr(ws), nb, st))
    _lib.check(lib.tdrn_batch_norm_backward(_lib.ptr(x), _lib.ptr(go), _lib.ptr(w), _lib.ptr(b), _lib.ptr(r["save_mean"]),
                                            _lib.ptr(r["save_invstd"]), _lib.ptr(r["grad_input"]), _lib.ptr(r["grad_weight"]),
                                            _lib.ptr(r["grad_bias"]), *dims, 1, int(relu), 1.0, _lib.ptr(ws), nb, st))
    torch.cuda.synchronize()
    return r


def bn_splits_of(dims):
    """from the query: 12 C splits + 8 C bytes (tdrn_hip.h)"""
    nb, C = _lib.lib().tdrn_batch_norm_workspace_bytes(*dims), dims[1]
    assert (nb - 8 * C) % (12 * C) == 0
    return (nb - 8 * C) // (12 * C)


def bn_check(tag, ref, got):
    return {name: S.share_of_interval("%s %-12s" % (tag, name), got[name], *ref[name]) for name in BN_NAMES}


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("eps", S.BN_EPS)
@pytest.mark.parametrize("draw", S.BN_DRAWS)
@pytest.mark.parametrize("case", list(S.BN_SHAPES))
def test_batch_norm_training_at_every_scale_and_conditioning(case, draw, eps, relu):
    inputs = S.bn_inputs(case, draw)
    ref = S.bn_reference(case, draw, eps, bool(relu))
    assert ref["kink_share"] <= 0.01
    assert bn_splits_of(S.BN_SHAPES[case]) == ref["plan"][2] and (ref["plan"][2] > 1) == (case == "multi_split")
    got = bn_run(inputs, ref["go"], eps, relu)
    print("%s/%d eps %g relu=%d: channels (kappa, k, weight) %r, kink share %.4f" % (case, draw, eps, relu, S.bn_channel_plan(case, draw),
                                                                                   ref["kink_share"]))
    bn_check("%s/%d eps %g relu=%d" % (case, draw, eps, relu), ref, got)
    again = bn_run(inputs, ref["go"], eps, relu)                    # bitwise reproducible at every scale
    for name in BN_NAMES:
        assert torch.equal(_bits(got[name]), _bits(again[name])), name


def _probe_inputs(mean_exp, sigma_exp, seed=3):
    """offset_mean's shape with channel 1 = (2^mean_exp + 2^sigma_exp randn) beside three ordinary channels"""
    x, w, b, go, rm, rv = (t.clone() for t in S.bn_inputs("offset_mean", 0))
    gen = torch.Generator().manual_seed(seed)
    r = torch.randn(x[:, 1].shape, generator=gen, dtype=torch.float64)
    x[:, 1] = ((2.0 ** (mean_exp - sigma_exp) if mean_exp is not None else 0.0) + r).float() * 2.0 ** sigma_exp
    w[1], b[1] = 1.5, 0.25
    return x, w, b, go, rm, rv


def test_batch_norm_a_mean_past_2_64_beside_ordinary_channels():
    """mean 2^67, sigma 2^49: d * d overflows in a Chan merge against an empty record (inf * 0 = NaN) unless that merge returns the
    other record; M2 = 3069 * 2^98 is far inside fp32.  All eight tensors must meet the bounds of every other case."""
    inputs = _probe_inputs(67, 49)
    for relu in (0, 1):
        ref = S.bn_reference_of(inputs, 1e-5, bool(relu))
        got = bn_run(inputs, ref["go"], 1e-5, relu)
        bn_check("mean 2^67 sigma 2^49 relu=%d" % relu, ref, got)


def test_batch_norm_statistics_just_inside_their_range():
    """the header's range: M (max x - min x)^2 < 2^128.  sigma = 2^55 in 3069 values: (max - min)^2 M is about 2^127."""
    inputs = _probe_inputs(None, 55)
    c = inputs[0][:, 1].double()
    assert 2.0 ** 125 < float((c.max() - c.min()) ** 2 * c.numel()) < 2.0 ** 128
    ref = S.bn_reference_of(inputs, 1e-5, False)
    bn_check("sigma 2^55", ref, bn_run(inputs, ref["go"], 1e-5, 0))


@pytest.mark.parametrize("relu", [0, 1])
def test_batch_norm_statistics_past_their_range_have_the_documented_class(relu):
    """sigma = 2^62: M2 is about 2^136 and overflows to +inf.  The header's rule: variance inf -> save_invstd = 0 -> output = bias
    (clipped by the ReLU), grad_input = 0 and grad_weight = 0 for that channel, running_var = +inf; save_mean stays right, and the other
    channels are untouched."""
    inputs = _probe_inputs(None, 62)
    x, w, b, go, rm, rv = inputs
    fine = _probe_inputs(None, 0)
    ref = S.bn_reference_of(fine, 1e-5, bool(relu))
    got = bn_run(inputs, ref["go"], 1e-5, relu)
    got_fine = bn_run(fine, ref["go"], 1e-5, relu)
    c = 1
    beta = b[c].clamp_min(0) if relu else b[c]
    want = {"save_invstd": torch.zeros(()), "running_var": torch.tensor(float("inf")), "grad_weight": torch.zeros(()),
            "output": torch.full_like(x[:, c], float(beta)), "grad_input": torch.zeros_like(x[:, c])}
    for name, wv in want.items():
        g = got[name].cpu()[:, c] if got[name].dim() == 4 else got[name].cpu()[c]
        same_class(g, wv, name)
        assert torch.equal(g.double(), wv.double()), name
    N, C, H, W = x.shape
    mean64, _, e_mean, _ = S.bn_stat_bounds(x.double(), *S.bn_depth(N, H * W, *S.bn_splits(N, C, H * W)))
    assert abs(float(got["save_mean"][c]) - float(mean64[c])) <= float(e_mean[c])
    dy = (ref["go"][:, c].double() * (1.0 if float(beta) > 0 or not relu else 0.0))
    assert abs(float(got["grad_bias"][c]) - float(dy.sum())) <= float(S.acc_bound("fp32", dy.abs().sum(), dy.numel()))
    for name in BN_NAMES:                                             # the other channels: the bits of a run without the wide channel
        g, f = got[name].cpu(), got_fine[name].cpu()
        keep = [0, 2, 3]
        assert torch.equal(_bits(g[:, keep] if g.dim() == 4 else g[keep]), _bits(f[:, keep] if f.dim() == 4 else f[keep])), name


@pytest.mark.parametrize("k", [-20, 20])
@pytest.mark.parametrize("case,draw", [("offset_mean", 0), ("multi_split", 0)])
def test_batch_norm_statistics_are_homogeneous_bit_for_bit(case, draw, k):
    """inputs * 2^k with eps * 2^2k give save_mean * 2^k and save_invstd * 2^-k bit for bit: nothing in the scheme under- or overflows
    at these scales (the channels are at 2^-30 and 2^0), and every operation of it commutes with a power of two"""
    inputs = S.bn_inputs(case, draw)
    eps = float(np.float32(1e-5))
    go = inputs[3]
    base = bn_run(inputs, go, eps, 0)
    scaled = bn_run((inputs[0] * 2.0 ** k,) + tuple(inputs[1:]), go, eps * 2.0 ** (2 * k), 0)
    assert torch.equal(_bits(scaled["save_mean"]), _bits(base["save_mean"] * 2.0 ** k))
    assert torch.equal(_bits(scaled["save_invstd"]), _bits(base["save_invstd"] * 2.0 ** -k))
    assert bool((base["save_invstd"] > 0).all()) and bool(torch.isfinite(scaled["save_invstd"]).all())


# ---- BatchNorm, resident 16-bit NHWC ----------------------------------------------------------------------------------------------------
def nhwc_run(inputs, go, eps, relu, T):
    from _nhwc_harness import bn_backward, bn_forward, resident
    x, w, b, _, rm, rv = inputs
    xr, gor = resident(x, T), resident(go, T)
    wd, bd = w.to(DEV), b.to(DEV)
    nan = float("nan")
    r = {"save_mean": torch.full_like(wd, nan), "save_invstd": torch.full_like(wd, nan), "running_mean": rm.to(DEV).clone(),
         "running_var": rv.to(DEV).clone(), "grad_weight": torch.zeros_like(wd), "grad_bias": torch.zeros_like(wd),
         "output": torch.full_like(xr, nan), "grad_input": torch.full_like(xr, nan)}
    bn_forward(xr, wd, bd, r["running_mean"], r["running_var"], r["output"], r["save_mean"], r["save_invstd"], True, S.BN_MOMENTUM, eps, relu, T)
    bn_backward(xr, gor, wd, bd, r["save_mean"], r["save_invstd"], r["grad_input"], r["grad_weight"], r["grad_bias"], True, relu, 1.0, T)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("eps", S.BN_EPS)
@pytest.mark.parametrize("T", list(TYPES))
@pytest.mark.parametrize("case", list(S.NHWC_SHAPES))
def test_resident_batch_norm_on_every_finite_pattern_of_the_type(case, T, eps, relu):
    """Channels inside the header's range (M (max - min)^2 < 2^128): the fp32 statistics and parameter gradients under the bounds of the
    fp32 NCHW op, the 16-bit output and grad_input inside cast_interval around those bounds (an interval of one value is bit equality;
    an interval at +-inf is an output that overflows the type).  Channels whose M2 is certainly past 2^128 (bf16 only): the documented
    class.  The few channels in between must meet one or the other."""
    from _nhwc_harness import nchw64
    inputs = S.nhwc_inputs(case, T)
    ref, (ok, past, wild), splits = S.nhwc_reference(case, T, eps, bool(relu))
    x = inputs[0]
    if case == "wide":
        assert splits == 2
        seen = set(to_bits(x.to(TYPES[T])).reshape(-1).tolist())
        finite = torch.isfinite(all16(T)[1])
        assert seen == set(torch.arange(65536)[finite].tolist()), "not every finite pattern of %s is among the inputs" % T
    assert ref["kink_share"] <= 0.01
    got = nhwc_run(inputs, ref["go"], eps, relu, T)
    tag = "%s %s eps %g relu=%d" % (case, T, eps, relu)
    print("%s: %d channels inside the range, %d certainly past it, %d with |x| >= 2^123, %d in between" % (
        tag, int(ok.sum()), int(past.sum()), int(wild.sum()), int((~ok & ~past & ~wild).sum())))
    if T == "fp16":
        assert bool(ok.all())
    invstd = got["save_invstd"].cpu()
    fell = (invstd == 0) & ~ok                                    # the channels that took the documented class
    assert bool(fell[past].all()), "a channel whose M2 is past 2^128 kept a non-zero save_invstd"
    use = ok | (~past & ~wild & ~fell)                            # checked against the bounds
    for name in ("save_mean", "save_invstd", "running_mean", "running_var", "grad_weight", "grad_bias"):
        r, lo, hi = ref[name]
        S.share_of_interval("%s %-12s" % (tag, name), got[name].cpu()[use], r[use], lo[use], hi[use])
    for name in ("output", "grad_input"):
        r, lo, hi = ref[name]
        lo16, hi16 = cast_interval(T, lo[:, use], hi[:, use])
        g = nchw64(got[name])[:, use]
        same_class(g, torch.where(lo16 == hi16, lo16, g), "%s %s" % (tag, name))         # an interval at +-inf admits that infinity only
        single = lo16 == hi16
        print("%s %-12s %d of %d intervals hold one value (bit equality there), %d of them infinite" % (
            tag, name, int(single.sum()), single.numel(), int((single & torch.isinf(lo16)).sum())))
        assert not bool(torch.isnan(g).any()), name
        bad = ~inside(g, lo16, hi16)
        assert not bool(bad.any()), "%s %s: %d elements outside their interval" % (tag, name, int(bad.sum()))
    # the documented class past the range: save_invstd = 0 -> output = bias (clipped, rounded once), grad_input = +-0, grad_weight = 0
    if bool(fell.any()):
        from _number_range import rne
        beta = inputs[2].clamp_min(0) if relu else inputs[2]
        y = nchw64(got["output"])[:, fell]
        assert torch.equal(y, rne(T, beta[fell]).double().view(1, -1, 1, 1).expand_as(y))
        assert bool((nchw64(got["grad_input"])[:, fell] == 0).all()) and bool((got["grad_weight"].cpu()[fell] == 0).all())
        assert bool((got["running_var"].cpu()[fell] == float("inf")).all())
    again = nhwc_run(inputs, ref["go"], eps, relu, T)
    for name in BN_NAMES:
        a, b = got[name], again[name]
        keep = ~wild.to(a.device)
        a, b = (t[:, keep] if t.dim() == 4 else t[keep] for t in (a, b))
        assert torch.equal(a.contiguous().view(torch.int16 if a.dtype != torch.float32 else torch.int32),
                           b.contiguous().view(torch.int16 if b.dtype != torch.float32 else torch.int32)), name


# ---- L2Norm ----------------------------------------------------------------------------------------------------------------------------
L2_NAMES =("norm", "output", "grad_input", "grad_weight")


def l2_run(x, w, go, eps):
    lib = _lib.lib()
    x, w, go = (t.to(DEV) for t in (x, w, go))
    N, C, H, W = dims = tuple(x.shape)
    nb = lib.tdrn_l2norm_workspace_bytes(*dims)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = _lib.current_stream(DEV)
    nan = float("nan")
    r = {"output": torch.full_like(x, nan), "norm": torch.full((N, H, W), nan, device=DEV), "grad_input": torch.full_like(x, nan),
         "grad_weight": torch.zeros_like(w)}
    _lib.check(lib.tdrn_l2norm_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(r["output"]), _lib.ptr(r["norm"]), *dims, eps, st))
    _lib.check(lib.tdrn_l2norm_backward(_lib.ptr(x), _lib.ptr(go), _lib.ptr(w), _lib.ptr(r["norm"]), _lib.ptr(r["grad_input"]),
                                        _lib.ptr(r["grad_weight"]), *dims, eps, 1.0, _lib.ptr(ws), nb, st))
    torch.cuda.synchronize()
    return r


def l2_check(tag, ref, got, names=L2_NAMES):
    return {name: worst_share("%s %-11s" % (tag, name), got[name], *ref[name]) for name in names}


@pytest.mark.parametrize("eps", S.L2_EPS)
@pytest.mark.parametrize("case", list(S.L2_SHAPES))
def test_l2norm_with_every_pixel_scale_in_one_tile(case, eps):
    x, w, go = S.l2_inputs(case)
    got = l2_run(x, w, go, eps)
    l2_check("%s eps %g" % (case, eps), S.l2_case_reference(case, eps), got)
    again = l2_run(x, w, go, eps)                                   # bitwise reproducible at every scale
    for name in L2_NAMES:
        assert torch.equal(_bits(got[name]), _bits(again[name])), name


def _l2_probe(top):
    """tiny_odd's draw at unit weights with pixel (0, 3, 4) = +-top in every channel: sum x^2 = 5 top^2"""
    x, w, go = (t.clone() for t in S.l2_inputs("tiny_odd"))
    w = torch.where(w > 0, 1.0, -1.0)
    x[0, :, 3, 4] = torch.tensor([top, -top, top, top, -top])
    return x, w, go


def test_l2norm_a_sum_of_squares_just_inside_2_128():
    x, w, go = _l2_probe(2.0 ** 62.5)
    assert 2.0 ** 127 < float((x[0, :, 3, 4].double() ** 2).sum()) < 2.0 ** 128
    got = l2_run(x, w, go, 1e-10)
    l2_check("sum x^2 = 2^127.3", S.l2_reference(x, w, go, 1e-10), got)
    assert bool(torch.isfinite(got["norm"]).all()) and float(got["output"][0, 0, 3, 4]) != 0.0


def test_l2norm_a_sum_of_squares_past_2_128_has_the_documented_class():
    """the header: norm = inf and output = 0 there, as the fp32 formula gives; the backward gives 0 at that pixel (1 / inf = 0) and no
    NaN; every other pixel is untouched"""
    x, w, go = _l2_probe(2.0 ** 64)
    got = l2_run(x, w, go, 1e-10)
    want = S.l2_formula32(x, w, go, 1e-10)
    for name in L2_NAMES:
        same_class(got[name], want[name], name)
    assert float(got["norm"][0, 3, 4]) == float("inf")
    assert bool((got["output"][0, :, 3, 4] == 0).all()) and bool((got["grad_input"][0, :, 3, 4] == 0).all())
    ref = S.l2_reference(x, w, go, 1e-10)
    keep = torch.ones(x.shape, dtype=torch.bool)
    keep[0, :, 3, 4] = False
    for name in ("output", "grad_input"):
        r, e = ref[name]
        worst_share("past 2^128, the other pixels %s" % name, got[name].cpu()[keep], r[keep], e[keep])


def test_l2norm_zero_and_subnormal_pixels_follow_the_rule_for_r_0():
    """a pixel of +-0 (a -0 among them) and a pixel of subnormals only: the squares vanish, norm = eps exactly, r = 0; the output is
    weight x / eps and the gradient weight go / eps (the second term taken as 0), inside the bounds of every other pixel"""
    x, w, go = (t.clone() for t in S.l2_inputs("tiny_odd"))
    x[1, :, 3, 4] = torch.tensor([0.0, -0.0, 0.0, -0.0, 0.0])
    sub = torch.tensor([1, 0x7FFFFF, 0x400000, 3, 0x2AAAAA], dtype=torch.int32).view(torch.float32)
    x[1, :, 2, 5] = sub * torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0])
    for eps in S.L2_EPS:
        got = l2_run(x, w, go, eps)
        l2_check("zero and subnormal pixels eps %g" % eps, S.l2_reference(x, w, go, eps), got)
        e32 = torch.tensor(eps, dtype=torch.float32)
        for (h, q) in ((3, 4), (2, 5)):
            assert float(got["norm"][1, h, q]) == float(e32)
            want = (w * go[1, :, h, q]) * (1.0 / e32)                         # the kernel's (w go - x 0) (1 / norm), in fp32
            assert torch.equal(_bits(got["grad_input"][1, :, h, q].cpu()), _bits(want)), (eps, h, q)
        assert bool((got["output"][1, :, 3, 4] == 0).all())
