"""The depthwise 3x3 conv (tdrn_dwconv2d_*) and SGD (tdrn_sgd_step through tdrn_amd.optim.SGD) over the whole number range.

Depthwise forward and backward_input: bit for bit against the header's sentence -- nine fmaf in tap order from the bias or +0, a tap
in the padding skipped -- restated exactly (tests/_number_range_stats.py: float64 products, which are exact, and a round-to-odd sum; the
CPU test checks that fmaf against integer arithmetic).  That pins the order, the fusion and the denormal mode at once.  NaN meets NaN
(a NaN's sign and payload are not compared); every other value, the sign of a zero included, is compared as bits.
backward_parameters: acc_bound("fp32", S, K = N Ho Wo) against float64, no floor.
SGD: bit for bit against tests/_sgd_ref.py on the cross product of f32_edges().
"""
import numpy as np
import pytest
import torch

import _number_range_stats as S
import _sgd_ref as R
import test_dwconv_abi as A
from _conv_train_harness import Abi as _Abi
from _number_range import F32_MIN_SUB, acc_bound, same_class, worst_share
from tdrn_amd.optim import SGD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DW_SHAPES = {"odd": (2, 3, 9, 7), "one_pixel": (1, 2, 1, 1)}
# (input kind, weight kind): "edges" = f32_edges(), an int k = randn 2^k.  Subnormal inputs (-140), products that are subnormal
# (-140, 0), that vanish (-100, -100), that overflow (100, 100: inf and inf - inf = NaN follow the restatement)
DW_VALUES = [("edges", "edges"), ("edges", 0), (0, 0), (-140, 0), (0, -140), (-100, 0), (-100, -100), (100, 0), (100, 100)]


def _dims(N, C, H, W, s):
    return (N, C, H, W, 3, 3, s, s, 1, 1, 1, 1)


def _abi(x, w, b, go, s):
    N, C, H, W = x.shape
    return _Abi("tdrn_dwconv2d", _dims(N, C, H, W, s), tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in (x, w, b, go)), "fp32")


def _same_bits(what, got, want):
    """bit for bit; NaN by NaN-ness"""
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN in other places than the restatement (%d against %d)" % (what, gn.sum(), wn.sum())
    g, w = got.view(np.int32)[~gn], want.view(np.int32)[~wn]
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, "%s: %d of %d elements differ from the restatement, first %r against %r" % (
        what, bad.size, g.size, got[~gn][bad[0]], want[~wn][bad[0]])
    return int(gn.sum())


def _dw_inputs(shape, s, kinds, seed):
    N, C, H, W = shape
    Ho, Wo = S.dw_out_hw(H, W, s)
    x, w = S.dw_values(shape, kinds[0], seed), S.dw_values((C, 1, 3, 3), kinds[1], seed + 1)
    # the bias at the scale of the products it joins (a finite one: 2^100 at the most)
    b = S.dw_values((C,), kinds[1] if kinds[0] == "edges" or kinds[1] == "edges" else min(kinds[0] + kinds[1], 100), seed + 2)
    go = S.dw_values((N, C, Ho, Wo), kinds[0], seed + 3)
    return x, w, b, go


@pytest.mark.parametrize("kinds", DW_VALUES, ids=lambda k: "x%s_w%s" % k)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", list(DW_SHAPES))
def test_dwconv_forward_and_backward_input_are_the_nine_fmaf_bit_for_bit(shape, stride, kinds):
    x, w, b, go = _dw_inputs(DW_SHAPES[shape], stride, kinds, 10 * DW_VALUES.index(kinds))
    a = _abi(x, w, b, go, stride)
    nan = float("nan")
    with_b = a.forward(torch.full_like(a.go, nan), bias=True).clone()
    no_b = a.forward(torch.full_like(a.go, nan), bias=False).clone()
    gi = a.backward_input(torch.full_like(a.x, nan))
    torch.cuda.synchronize()
    tag = "%s s%d x %s w %s" % (shape, stride, kinds[0], kinds[1])
    n1 = _same_bits(tag + " forward", with_b, S.dw_forward_exact(x, w, b, stride))
    n2 = _same_bits(tag + " forward, no bias", no_b, S.dw_forward_exact(x, w, None, stride))
    n3 = _same_bits(tag + " backward_input", gi, S.dw_backward_input_exact(go, w, x.shape[2], x.shape[3], stride))
    want = S.dw_forward_exact(x, w, b, stride)
    sub = int(((np.abs(want) < 2.0 ** -126) & (want != 0)).sum())
    print("%s: %d outputs, %d subnormal, %d infinite, NaN %d / %d / %d: all equal to the restatement" % (
        tag, want.size, sub, int(np.isinf(want).sum()), n1, n2, n3))


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv_a_non_finite_weight_on_a_padding_tap_and_a_non_finite_input(stride, bad):
    """weight (0,0) of channel 1 is not finite: the output pixels of the first row and the first column, for which that tap lies in the
    padding, stay finite (the tap is skipped, not multiplied by 0); the others follow the restatement.  Then a non-finite input
    element: NaN exactly where the restatement has it."""
    N, C, H, W = DW_SHAPES["odd"]
    x, w, b, go = _dw_inputs((N, C, H, W), stride, (0, 0), 77)
    w[1, 0, 0, 0] = bad
    a = _abi(x, w, b, go, stride)
    y = a.forward(torch.full_like(a.go, float("nan"))).clone()
    gi = a.backward_input(torch.full_like(a.x, float("nan"))).clone()
    torch.cuda.synchronize()
    want = S.dw_forward_exact(x, w, b, stride)
    same_class(y, torch.from_numpy(want), "forward")
    _same_bits("forward", y, want)
    _same_bits("backward_input", gi, S.dw_backward_input_exact(go, w, H, W, stride))
    yc = y.cpu()
    assert bool(torch.isfinite(yc[:, 1, 0, :]).all()) and bool(torch.isfinite(yc[:, 1, :, 0]).all())
    assert not bool(torch.isfinite(yc[:, 1, 1:, 1:]).any())
    assert bool(torch.isfinite(yc[:, 0]).all()) and bool(torch.isfinite(yc[:, 2]).all())
    w[1, 0, 0, 0] = 0.5
    x[1, 2, 4, 3] = bad
    a = _abi(x, w, b, go, stride)
    y = a.forward(torch.full_like(a.go, float("nan")))
    torch.cuda.synchronize()
    want = S.dw_forward_exact(x, w, b, stride)
    same_class(y, torch.from_numpy(want), "forward, a non-finite input")
    _same_bits("forward, a non-finite input", y, want)
    assert 0 < int((~np.isfinite(want)).sum()) <= 9


PARAM_SCALES = [(0, 0), (-140, 0), (-100, 0), (0, -100), (100, 0)]              # the exponents of (input, grad_output)


@pytest.mark.parametrize("scales", PARAM_SCALES, ids=lambda s: "x%d_go%d" % s)
@pytest.mark.parametrize("shape,stride", [((2, 3, 9, 7), 1), ((2, 3, 9, 7), 2), ((2, 3, 24, 23), 1)], ids=["odd_s1", "odd_s2", "two_ranges"])
def test_dwconv_backward_parameters_within_acc_bound_at_every_scale(shape, stride, scales):
    N, C, H, W = shape
    Ho, Wo = S.dw_out_hw(H, W, stride)
    K = N * Ho * Wo
    splits = A.wgrad_splits(N, C, H, W, stride)[0]
    assert (splits > 1) == (shape == (2, 3, 24, 23)), splits                   # the header's formula: K = 1104 is cut into two ranges
    x, go = S.dw_values(shape, scales[0], 41), S.dw_values((N, C, Ho, Wo), scales[1], 42)
    a = _abi(x, np.zeros((C, 1, 3, 3), np.float32), np.zeros(C, np.float32), go, stride)
    gw, gb = a.backward_parameters(torch.zeros_like(a.w), torch.zeros_like(a.b))
    torch.cuda.synchronize()
    rw, sw, rb, sb = S.dw_params_reference(x, go, stride)
    tag = "%r s%d x 2^%d go 2^%d" % (shape, stride, scales[0], scales[1])
    worst_share(tag + " grad_weight", gw, rw, acc_bound("fp32", sw, K))
    worst_share(tag + " grad_bias", gb, rb, acc_bound("fp32", sb, K))
    if scales == (-140, 0):
        # grad_weight is about sqrt(K) 2^-140: thousands of subnormal spacings, and the bound is (K + 3) of them -- a flush to zero fails
        assert int((gw != 0).sum()) == gw.numel() and float(gw.abs().max()) < 2.0 ** -126
    # += scale * into a non-zero buffer at the same scale: fl(old + 0.5 s), one fma more
    k = scales[0] + scales[1]
    old_w = torch.from_numpy(S.dw_values((C, 1, 3, 3), k + 3, 43)).to(DEV)
    old_b = torch.from_numpy(S.dw_values((C,), scales[1] + 3, 44)).to(DEV)
    gw2, gb2 = a.backward_parameters(old_w.clone(), old_b.clone(), scale=0.5)
    torch.cuda.synchronize()
    for name, got, old, r, s in (("grad_weight", gw2, old_w, rw, sw), ("grad_bias", gb2, old_b, rb, sb)):
        ref = old.cpu().double() + 0.5 * r
        bound = 0.5 * acc_bound("fp32", s, K) + 1.001 * S.U32 * ref.abs() + F32_MIN_SUB
        worst_share(tag + " += 0.5 * " + name, got, ref, bound)


# ---- SGD -------------------------------------------------------------------------------------------------------------------------------
def _sgd_same(what, got, want):
    got = got.detach().cpu().numpy().reshape(-1)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN in other places than the restatement" % what
    g, w = got.view(np.int32)[~gn], want.view(np.int32)[~wn]
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, "%s: %d of %d elements differ, first %r against %r" % (what, bad.size, g.size, got[~gn][bad[0]], want[~wn][bad[0]])


@pytest.mark.parametrize("lr", list(S.SGD_LRS))
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("mode", list(S.SGD_MODES))
def test_sgd_three_steps_on_the_cross_product_of_the_edge_values(mode, wd, lr):
    """numel 5 (a 16-byte vector and its tail) and numel 67 as views 4 bytes into their buffers (the scalar path); p, g and the
    momentum buffer from f32_edges() x f32_edges() x f32_edges(); the third step's gradient also holds +inf, -inf and NaN"""
    hp = dict(lr=S.SGD_LRS[lr], weight_decay=wd, **S.SGD_MODES[mode])
    params, views, refs = [], [], []
    for n in S.SGD_SIZES:
        off = 1 if n == 67 else 0
        p0, _, b0 = S.sgd_triples(n, 0)
        bufs = [torch.zeros(n + 8, device=DEV) for _ in range(3)]
        pv, gv, bv = (t[off:off + n] for t in bufs)
        pv.copy_(torch.from_numpy(p0))
        bv.copy_(torch.from_numpy(b0))
        assert pv.data_ptr() % 16 == 4 * off
        p = torch.nn.Parameter(pv)
        assert p.data_ptr() == pv.data_ptr()
        params.append(p)
        views.append((pv, gv, bv))
        refs.append([p0.copy(), b0.copy()])
    opt = SGD(params, **hp)
    for p, (_, _, bv) in zip(params, views):
        opt.state[p]["momentum_buffer"] = bv
    for step in range(3):
        for i, (n, p) in enumerate(zip(S.SGD_SIZES, params)):
            g = S.sgd_triples(n, step)[1]
            if step == 2:
                g[[0, n // 2, n - 1]] = [np.inf, -np.inf, np.nan]
            views[i][1].copy_(torch.from_numpy(g))
            p.grad = views[i][1]
            refs[i][0], refs[i][1] = R.sgd_step(refs[i][0], g, refs[i][1], **hp)
        opt.step()
        torch.cuda.synchronize()
        for i, (n, p) in enumerate(zip(S.SGD_SIZES, params)):
            tag = "%s wd %g lr %s numel %d step %d" % (mode, wd, lr, n, step)
            _sgd_same(tag + " p", p, refs[i][0])
            _sgd_same(tag + " b", opt.state[p]["momentum_buffer"], refs[i][1])
            assert opt.state[p]["momentum_buffer"].data_ptr() == views[i][2].data_ptr()
    last = np.concatenate([r[0] for r in refs])
    print("%s wd %g lr %s: after three steps %d of %d values of p are subnormal, %d are +-0, %d infinite, %d NaN" % (
        mode, wd, lr, int(((np.abs(last) < 2.0 ** -126) & (last != 0)).sum()), last.size, int((last == 0).sum()), int(np.isinf(last).sum()),
        int(np.isnan(last).sum())))
