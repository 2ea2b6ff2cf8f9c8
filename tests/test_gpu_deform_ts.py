"""The transform-domain deformable conv (tdrn_hip.h section i-l) on the GPU: the C entries and the Python op
against the float64 oracle of tests/_deform_grad_ref.py.  The entries' wrapper, the inputs, the references and the bound are those of
tests/_deform_ts_harness.py (shared with test_gpu_deform_ts_scope.py, which leaves the square stride-1 geometry of the cases here).

Inputs are exact by construction, so the bound is derived, not tuned: X, W and grad_output are exactly representable in the compute
type; offsets are fp32 multiples of 2^-6 with |offset| <= 16, so coordinates, fractions, the four bilinear weights and b * gO are exact
in fp32, and integer coordinates (offset 0 included), the [H-1, H) band and rejections are ordinary cases.

Bound, elementwise, nothing exempted:  |got - ref| <= (U + 2 C_ACC) S + TINY.
  * each result passes through exactly one 16-bit rounding of an inexact intermediate (Y for output and grad_offset, Z for grad_input
    and grad_weight); U is a whole last-place unit, twice the rounding's half unit;
  * each result passes through two fp32 summation stages (GEMM, then blend / scatter / reduction), one C_ACC S each;
  * S is the same quantity on absolute values in float64: for output, grad_input and grad_weight the oracle run on |X|, |W|, |gO| (the
    bilinear weights are non-negative); for grad_offset it is restated here, sum_co |gO| sum_corners |db/dpos| Ybar with
    Ybar = sum_c |W| |X| (offset_S), zero along an axis inside its clamp band, where the derivative is zero.
The worst share of the bound is printed per result.

The link to the gather op (conv_offset2d on the same inputs) allows the sum of both ops' bounds; the gather op's is the same
expression: it rounds the sampled column once (U) and has the blend and the GEMM as its two fp32 stages.  The gather op keeps the
reference's "input image is smaller than kernel" rule, so the 1 x 1 case has no such link (it raises there)."""
import pytest
import torch

from tdrn_amd.model import networks

from _conv_train_harness import DEV, Guarded
from _deform_ts_harness import MODES, NAMES, REGIMES, bound, same_bits, square, within
from _deform_ts_harness import Ts as _Ts, problem as _problem

pytestmark = pytest.mark.gpu

# (N, Cin, H, W, Cout, k): stride 1, pad k // 2, dilation 1
CASES = [(1, 64, 1, 1, 12, 3),          # one pixel; every neighbour tap rejected or clamped
         (2, 64, 3, 3, 63, 3),          # smallest pyramid level; two images: a scatter must not cross images
         (1, 128, 5, 7, 75, 3),         # M = 35, not a multiple of any tile; two channel chunks; paired width
         (2, 256, 6, 5, 12, 5),         # 25 taps
         (1, 64, 9, 8, 105, 3),         # past 64, 80 and 96 columns
         (1, 1024, 3, 3, 63, 3),        # K = 1024
         (3, 64, 24, 24, 75, 3)]        # several workgroups
ids = lambda c: "x".join(str(v) for v in c)


def problem(case, mode, regime):
    """inputs (CPU fp32), float64 references and absolute-value sums, computed once and left unchanged (the harness caches them)"""
    return _problem(square(*case), mode, regime, 1000 * CASES.index(case) + 10 * REGIMES.index(regime) + MODES.index(mode))


def Ts(case, mode):
    """the entries on plain device buffers"""
    return _Ts(square(*case), mode)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_entries_match_the_oracle(case, mode, regime):
    p = problem(case, mode, regime)
    ts = Ts(case, mode)
    what = "%s %s %s" % (ids(case), mode, regime)
    first = ts.all(p)
    for name, got in zip(NAMES, first):
        within(what, mode, name, got, p)
    # two runs: equal bits for output, Y and grad_offset; y_saved null: Y is recomputed to the same bits
    again = ts.all(p, y_given=False)
    for i in (0, 2, 4):
        assert same_bits(first[i], again[i]), (what, (NAMES + ("Y",))[i])
    for i in (1, 3):
        within(what + " (run 2)", mode, NAMES[i], again[i], p)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_subsets_of_gradients(case, mode):
    """each subset of null gradient pointers gives, for the outputs that remain, what the full call gives"""
    p = problem(case, mode, "half")
    ts = Ts(case, mode)
    what = "%s %s subsets" % (ids(case), mode)
    full = ts.all(p)
    x, w, off, go = ts.inputs(p)
    for y in (full[4], None):
        for mask in range(1, 7):
            want = [bool(mask & 1), bool(mask & 2), bool(mask & 4)]             # grad_input, grad_offset, grad_weight
            ts.ws.fill_(0xFF)
            bufs = [torch.full_like(t, float("nan")) if on else None for t, on in zip((x, off, w), want)]
            ts.backward(x, w, off, go, y, *bufs)
            torch.cuda.synchronize()
            if want[1]:
                assert same_bits(bufs[1], full[2]), (what, mask, y is None)
            if want[0]:
                within("%s mask %d" % (what, mask), mode, "grad_input", bufs[0], p)
            if want[2]:
                within("%s mask %d" % (what, mask), mode, "grad_weight", bufs[2], p)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_caller_memory(case, mode):
    """caller buffers 16 bytes behind a 256-byte boundary between NaN guard bands; a workspace of exactly the queried size, filled
    with NaN bytes"""
    p = problem(case, mode, "wide")
    ts = Ts(case, mode)
    what = "%s %s guarded" % (ids(case), mode)
    full = ts.all(p)
    gx, gw_, goff_, ggo = (Guarded(p[n].shape, offset=16, init=p[n].to(DEV)) for n in ("x", "w", "off", "go"))
    out, gi, goff, gw = (Guarded(p[n].shape, offset=16) for n in ("go", "x", "off", "w"))
    y = Guarded(nbytes=ts.yb, offset=16)
    ws = Guarded(nbytes=ts.nb, offset=16)
    ws.t.fill_(0xFF)
    ts.forward(gx.t, gw_.t, goff_.t, out.t, y.t, ws=ws.t)
    ws.check(what + " forward workspace", full=False)
    ws.t.fill_(0xFF)
    ts.backward(gx.t, gw_.t, goff_.t, ggo.t, y.t, gi.t, goff.t, gw.t, ws=ws.t)
    for name, g in (("output", out), ("grad_input", gi), ("grad_offset", goff), ("grad_weight", gw), ("Y", y), ("workspace", ws)):
        g.check("%s %s" % (what, name), full=name != "workspace")
    for name, g in (("x", gx), ("w", gw_), ("off", goff_), ("go", ggo)):
        g.check("%s %s" % (what, name))
        assert torch.equal(g.t.cpu(), p[name]), (what, name, "an input was written")
    assert same_bits(out.t, full[0]) and same_bits(goff.t, full[2]) and same_bits(y.t, full[4]), what
    within(what, mode, "grad_input", gi.t, p)
    within(what, mode, "grad_weight", gw.t, p)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_python_op_equals_the_entries(case, mode):
    N, Cin, H, W, Cout, k = case
    p = problem(case, mode, "half")
    what = "%s %s python" % (ids(case), mode)
    full = Ts(case, mode).all(p)
    for save_y in (True, False):
        x, w, off = (p[n].to(DEV).requires_grad_(True) for n in ("x", "w", "off"))
        networks.ConvOffset2dTsFunction.save_y = save_y
        try:
            out = networks.conv_offset2d_ts(x, off, w, 1, k // 2, 1, mode)
            out.backward(p["go"].to(DEV))
        finally:
            networks.ConvOffset2dTsFunction.save_y = True
        assert same_bits(out.detach(), full[0]) and same_bits(off.grad, full[2]), (what, save_y)
        within(what, mode, "grad_input", x.grad, p)
        within(what, mode, "grad_weight", w.grad, p)
    # the dispatch rule of conv_offset2d: no grad_fn when nothing upstream requires grad; only the gradients asked for
    x, w, off = (p[n].to(DEV) for n in ("x", "w", "off"))
    plain = networks.conv_offset2d_ts(x, off, w.requires_grad_(True), 1, k // 2, 1, mode)
    assert plain.grad_fn is None and same_bits(plain, full[0])
    off = off.requires_grad_(True)
    out = networks.conv_offset2d_ts(x, off, w.detach(), 1, k // 2, 1, mode)
    out.backward(p["go"].to(DEV))
    assert same_bits(off.grad, full[2]), what


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case,regime", [(CASES[2], "half"), (CASES[6], "converging")], ids=["5x7", "24x24-converging"])
def test_side_stream_and_graph_replay(case, regime, mode):
    p = problem(case, mode, regime)
    ts = Ts(case, mode)
    what = "%s %s %s graph" % (ids(case), mode, regime)
    want = ts.all(p)
    x, w, off, go = ts.inputs(p)
    out, gi, goff, gw, y = torch.empty_like(go), torch.empty_like(x), torch.empty_like(off), torch.empty_like(w), ts.new_y()

    def work():
        ts.forward(x, w, off, out, y)
        ts.backward(x, w, off, go, y, gi, goff, gw)

    def check(tag):
        assert same_bits(out, want[0]) and same_bits(goff, want[2]) and same_bits(y, want[4]), (what, tag)
        within("%s %s" % (what, tag), mode, "grad_input", gi, p)
        within("%s %s" % (what, tag), mode, "grad_weight", gw, p)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()                                     # warm-up on the side stream: lazy initialisation happens outside the capture
    side.synchronize()
    check("side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        work()
    for k in range(2):
        for t in (out, gi, goff, gw):
            t.fill_(float("nan"))
        y.fill_(0xFF)
        ts.ws.fill_(0x4B)                          # the entries zero what they need on every replay
        graph.replay()
        torch.cuda.synchronize()
        check("replay %d" % k)
    del graph


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in CASES if c[2] >= c[5] and c[3] >= c[5]], ids=ids)
def test_output_against_the_gather_op(case, mode):
    """a sanity link to conv_offset2d on the same inputs: within the sum of both ops' bounds (the module docstring)"""
    N, Cin, H, W, Cout, k = case
    for regime in REGIMES:
        p = problem(case, mode, regime)
        x, w, off, _ = Ts(case, mode).inputs(p)
        a = networks.conv_offset2d_ts(x, off, w, 1, k // 2, 1, mode)
        b = networks.conv_offset2d(x, off, w, 1, k // 2, 1, 1, mode)
        d = (a.double() - b.double()).abs().cpu()
        bd = 2 * bound(mode, p["S"]["output"])
        print("%s %s %s transform vs gather: max|d| %.3e  worst share of the summed bounds %.3e"
              % (ids(case), mode, regime, float(d.max()), float((d / bd).max())))
        assert bool((d <= bd).all())
