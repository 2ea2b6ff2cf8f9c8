"""The transform-domain deformable conv (tdrn_hip.h section i-l) across its declared scope, on the GPU: what
test_gpu_deform_ts.py's square stride-1 cases with Cout <= 105 do not reach.
  a. a fuzz over non-square kernels, strides, paddings and dilations drawn per axis (Ho x Wo outputs over an H x W map), every
     number of columns per lane (Cout 1 ... 256), M that is no multiple of the four waves of a workgroup, maps smaller than the kernel;
  b. the edges of `lane + 64 j < Cout` and of Cp = Cout rounded up to 8 on one geometry, and rows with no and with 56 of 64 columns
     of padding;
  c. the paired loc + conf heads at 81 classes (255 columns, 3 x 3 and 5 x 5), eagerly, on a side stream and replayed from a graph;
  d. offsets far outside the map, infinite and NaN: rejected samples, a finite zero contribution and a zero grad_offset.
Shapes, inputs, references and the derived bound |got - ref| <= (U + 2 C_ACC) S + TINY (elementwise, nothing exempted) are those of
tests/_deform_ts_harness.py; tests/test_deform_ts_ref.py shows on the CPU that these shapes tell a wrong kernel from a right one.
Every case is tiny; the float64 oracle of a case is computed once per process."""
import pytest
import torch

from tdrn_amd.model import networks

from _conv_train_harness import DEV, Guarded
from _deform_ts_harness import (EDGES, FAR_GEOMS, GRAPH_FUZZ_SEED, HEAD_REGIMES, HEADS, MODES, NAMES, NON_FINITE, TS_FUZZ_SEEDS, Ts, bits,
                                bound, edge_problem, far_problem, far_seed, fuzz_problem, head_problem, make_far, same_bits, within)

pytestmark = pytest.mark.gpu

RESULTS = NAMES + ("Y",)


def entries(what, g, mode, p, group):
    """the four results against the oracle; a second run with y_saved null: Y is recomputed to the same bits -> (Ts, the first run)"""
    ts = Ts(g, mode)
    first = ts.all(p)
    assert tuple(first[0].shape) == (g.N, g.Cout, g.Ho, g.Wo) and tuple(first[2].shape) == (g.N, 2 * g.taps, g.Ho, g.Wo)
    for name, got in zip(NAMES, first):
        within(what, mode, name, got, p, group=group)
    again = ts.all(p, y_given=False)
    for i in (0, 2, 4):
        assert same_bits(first[i], again[i]), (what, RESULTS[i])
    for i in (1, 3):
        within(what + " (run 2)", mode, NAMES[i], again[i], p, group=group)
    return ts, first


def python_op(what, g, mode, p, full, group):
    """conv_offset2d_ts with tuple stride, padding and dilation gives the entries' bits: _deform_geometry's reordering"""
    for save_y in (True, False):
        x, w, off = (p[n].to(DEV).requires_grad_(True) for n in ("x", "w", "off"))
        networks.ConvOffset2dTsFunction.save_y = save_y
        try:
            out = networks.conv_offset2d_ts(x, off, w, g.stride, g.padding, g.dilation, mode)
            out.backward(p["go"].to(DEV))
        finally:
            networks.ConvOffset2dTsFunction.save_y = True
        assert same_bits(out.detach(), full[0]) and same_bits(off.grad, full[2]), (what, save_y)
        within(what + " python", mode, "grad_input", x.grad, p, group=group)
        within(what + " python", mode, "grad_weight", w.grad, p, group=group)


def gather_link(what, g, mode, p, full):
    """conv_offset2d(compute=mode) on the same inputs: within the sum of both ops' bounds.  The gather op refuses a map smaller than
    the kernel (the reference's rule): no link there."""
    if g.smaller_than_kernel:
        with pytest.raises(RuntimeError):
            networks.conv_offset2d(p["x"].to(DEV), p["off"].to(DEV), p["w"].to(DEV), g.stride, g.padding, g.dilation, 1, mode)
        return
    b = networks.conv_offset2d(p["x"].to(DEV), p["off"].to(DEV), p["w"].to(DEV), g.stride, g.padding, g.dilation, 1, mode)
    d = (full[0].double() - b.double()).abs().cpu()
    bd = 2 * bound(mode, p["S"]["output"])
    print("%s transform vs gather: max|d| %.3e  worst share of the summed bounds %.3e" % (what, float(d.max()), float((d / bd).max())))
    assert bool((d <= bd).all()), what


def comparison(what, g, mode, p, group):
    ts, full = entries(what, g, mode, p, group)
    python_op(what, g, mode, p, full, group)
    gather_link(what, g, mode, p, full)
    return ts, full


def caller_memory(what, g, mode, p):
    """caller buffers 16 bytes behind a 256-byte boundary between NaN guard bands; a workspace of exactly the queried size, filled
    with 0xFF bytes; inputs unwritten"""
    ts = Ts(g, mode)
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
    for name, b in (("output", out), ("grad_input", gi), ("grad_offset", goff), ("grad_weight", gw), ("Y", y), ("workspace", ws)):
        b.check("%s %s" % (what, name), full=name != "workspace")
    for name, b in (("x", gx), ("w", gw_), ("off", goff_), ("go", ggo)):
        b.check("%s %s" % (what, name))
        assert torch.equal(b.t.cpu(), p[name]), (what, name, "an input was written")
    assert same_bits(out.t, full[0]) and same_bits(goff.t, full[2]) and same_bits(y.t, full[4]), what
    within(what, mode, "grad_input", gi.t, p)
    within(what, mode, "grad_weight", gw.t, p)


# ---- a. fuzz -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", TS_FUZZ_SEEDS)
def test_fuzz_matches_the_oracle(seed, mode):
    g, p = fuzz_problem(seed, mode)
    comparison("fuzz %d %s %s" % (seed, g.name, mode), g, mode, p, "fuzz")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", TS_FUZZ_SEEDS)
def test_fuzz_caller_memory(seed, mode):
    g, p = fuzz_problem(seed, mode)
    caller_memory("fuzz %d %s %s guarded" % (seed, g.name, mode), g, mode, p)


# ---- b. column edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("g", EDGES, ids=lambda g: g.name)
def test_column_edges(g, mode):
    p = edge_problem(g, mode)
    what = "edge %s %s" % (g.name, mode)
    ts, full = comparison(what, g, mode, p, "edges")
    # grad_input and grad_weight from calls that ask for them alone: they read no Y (the workspace holds none: 0xFF bytes)
    x, w, off, go = ts.inputs(p)
    for i, name in ((0, "grad_input"), (2, "grad_weight")):
        ts.ws.fill_(0xFF)
        bufs = [None, None, None]
        bufs[i] = torch.full_like((x, off, w)[i], float("nan"))
        ts.backward(x, w, off, go, None, *bufs)
        torch.cuda.synchronize()
        within(what + " alone", mode, name, bufs[i], p, group="edges")


# ---- c. the 81-class heads ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("regime", HEAD_REGIMES)
@pytest.mark.parametrize("g", HEADS, ids=lambda g: g.name)
def test_heads_81_classes(g, regime, mode):
    comparison("heads %s %s %s" % (g.name, mode, regime), g, mode, head_problem(g, mode, regime), "heads")


def _graph_cases():
    yield pytest.param(lambda mode: (HEADS[0], head_problem(HEADS[0], mode, "half")), id="heads-" + HEADS[0].name)
    yield pytest.param(lambda mode: fuzz_problem(GRAPH_FUZZ_SEED, mode), id="fuzz-%d-stride-2" % GRAPH_FUZZ_SEED)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _graph_cases())
def test_side_stream_and_graph_replay(case, mode):
    g, p = case(mode)
    ts = Ts(g, mode)
    what = "%s %s graph" % (g.name, mode)
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


# ---- d. rejected and non-finite offsets --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("g", FAR_GEOMS, ids=lambda g: g.name)
def test_far_and_non_finite_offsets(g, mode):
    p = far_problem(g, mode)
    what = "far %s %s" % (g.name, mode)
    ts = Ts(g, mode)
    far = ts.all(p)
    for name, got in zip(NAMES, far):
        within(what, mode, name, got, p, group="far")
    # a rejected sample: grad_offset is +0 or -0, bit for bit, on both axes of the sample
    rejected = (~p["kinds"]["accepted"]).repeat_interleave(2, dim=1)
    assert bool(rejected[p["far"]].all()) and 0.1 < float(rejected.double().mean()) < 0.9, what
    assert bool(((bits(far[2]).cpu()[rejected] & 0x7FFFFFFF) == 0).all()), what
    # +-Inf and NaN on the same entries: rejected by the same comparison
    off, mask = make_far(p["near"], NON_FINITE, far_seed(g))
    assert torch.equal(mask, p["far"]) and not bool(torch.isfinite(off[mask]).any()) and bool(torch.isnan(off).any())
    wild = ts.all(p, off=off)
    for i in (0, 2, 4):
        assert same_bits(far[i], wild[i]), (what, RESULTS[i])
    for i in (1, 3):
        within(what + " non-finite", mode, NAMES[i], wild[i], p, group="far")       # (within asserts finiteness)
    again = ts.all(p, y_given=False, off=off)
    for i in (0, 2, 4):
        assert same_bits(far[i], again[i]), (what, RESULTS[i], "Y recomputed")
