"""The training kernels' rounding over the whole number range (tdrn_hip.h sections i-c, i-f, i-g, i-i and the layout boundary of i-k):
ties, subnormals, the overflow boundary and values that become +-inf in the type.  Helpers and bounds: tests/_number_range.py.

1. Layout boundary: tdrn_nhwc16_from_nchw / tdrn_nchw_from_nhwc16 (and networks.to_nhwc / from_nhwc) bit for bit on every tie and every
   16-bit pattern.
2. Operand rounding, bit for bit.  A 0/1 selector in the other operand makes every output element ONE product value * 1 plus exact zeros,
   so the fp32 result IS the operand as the kernel rounded it: expected rne_bits(value).  The probe values sit in the input (forward,
   backward_parameters), in grad_output (backward_input, backward_parameters) or in the weight (forward, backward_input: the repack
   kernels).  Which element of the carrier an output element reads is found by running the float64 restatement on the carrier's own
   element numbers, so no index map is written twice.  The expectation is the float64 restatement below on the rounded inputs, with
   explicit zero padding: a value that rounds to +-inf meets the zeros of its neighbours' taps, and inf * 0 = NaN is predicted there, not
   excused (those values go in a run of their own, spread so that each inf also survives at its own element; non-finite weights sit
   on corner and edge taps too, where they meet the padding's zeros: the training entries form every tap, KOFF_TAP_SKIP).  Finite results are
   compared bit for bit, the sign of a zero sum (+0: the accumulators start at +0) included; the rest class by class.
3. A scale sweep against float64 with no floor: |got - ref| <= acc_bound elementwise on all four outputs with the inputs multiplied by
   powers of two that put them, or the results, at the ends of fp32's and of the 16-bit type's range; and homogeneity: scaling by 2^+-40
   changes no mantissa bit (fp32 and bf16 compute).
"""
import functools

import pytest
import torch

import _number_range as nr
from _conv_train_harness import DEV, Abi
from tdrn_amd import _lib
from tdrn_amd.model import networks

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

TS = ("bf16", "fp16")
MODES = ("fp32", "bf16", "fp16")


# ---- 1. the layout boundary ---------------------------------------------------------------------------------------------------------------
def _as_image(values, C=64, W=61):
    """a flat fp32 tensor -> (1, C, H, W), zero-filled behind its end"""
    H = -(-values.numel() // (C * W))
    t = torch.zeros(C * H * W)
    t[:values.numel()] = values
    return t.view(1, C, H, W)


def _assert_bits16(what, got16, want_bits_nchw):
    """a resident tensor against bit patterns given in NCHW order; NaN by NaN-ness"""
    assert got16.is_contiguous(memory_format=torch.channels_last), what
    got = nr.to_bits(got16.detach().cpu().contiguous())
    want = want_bits_nchw.reshape(got.shape)
    T = {torch.bfloat16: "bf16", torch.float16: "fp16"}[got16.dtype]
    gn, wn = torch.isnan(nr.decode64(T, got)), torch.isnan(nr.decode64(T, want))
    assert torch.equal(gn, wn), "%s: NaN in other places" % what
    bad = (got != want) & ~wn
    assert not bool(bad.any()), "%s: %d of %d differ, first got %#06x want %#06x" % (
        what, int(bad.sum()), bad.numel(), int(got[bad][0]), int(want[bad][0]))


@pytest.mark.parametrize("T", TS)
def test_from_nchw_rounds_every_tie_and_pattern_to_nearest_even(T):
    x = _as_image(torch.cat([nr.ties(T).reshape(-1), nr.all16(T)[1]]))
    want = nr.rne_bits(T, x)                      # (= x.to(T) on the CPU bit for bit: test_number_range_ref.py)
    xd = x.to(DEV)
    out = torch.zeros(x.shape, dtype=nr.TYPES[T], device=DEV).contiguous(memory_format=torch.channels_last)
    _lib.check(_lib.lib().tdrn_nhwc16_from_nchw(_lib.ptr(xd), _lib.ptr(out), *x.shape, _lib.DTYPES[T], _lib.current_stream(DEV)))
    torch.cuda.synchronize()
    _assert_bits16("tdrn_nhwc16_from_nchw %s" % T, out, want)
    _assert_bits16("to_nhwc %s" % T, networks.to_nhwc(xd, nr.TYPES[T]), want)


@pytest.mark.parametrize("T", TS)
def test_from_nhwc16_is_exact_on_every_pattern(T):
    t16, f32 = nr.all16(T)
    x16 = t16.view(1, 64, 32, 32).to(DEV).contiguous(memory_format=torch.channels_last)
    want = f32.view(1, 64, 32, 32)
    for what, got in (("tdrn_nchw_from_nhwc16", None), ("from_nhwc", networks.from_nhwc(x16))):
        if got is None:
            got = torch.zeros(want.shape, device=DEV)
            _lib.check(_lib.lib().tdrn_nchw_from_nhwc16(_lib.ptr(x16), _lib.ptr(got), *want.shape, _lib.DTYPES[T], _lib.current_stream(DEV)))
            torch.cuda.synchronize()
        got = got.cpu()
        assert got.is_contiguous() and torch.equal(torch.isnan(got), torch.isnan(want)), what
        keep = ~torch.isnan(want)
        assert torch.equal(nr.f32_bits(got)[keep], nr.f32_bits(want)[keep]), what


# ---- 2. operand rounding through selector operands ---------------------------------------------------------------------------------------
# geometry -> (entry prefix, k, stride, pad, transposed)
GEOS = {"conv2d_k1": ("tdrn_conv2d", 1, 1, 0, False), "conv2d_k3": ("tdrn_conv2d", 3, 1, 1, False),
        "conv2d_strided": ("tdrn_conv2d_strided", 3, 2, 1, False), "conv5x5": ("tdrn_conv5x5", 5, 1, 2, False),
        "conv_transpose2d": ("tdrn_conv_transpose2d", 2, 2, 0, True)}


def _dims(geo, N, Ci, H, W, Co):
    prefix, k, s, p, tr = GEOS[geo]
    return (N, Ci, H, W, Co, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1) if tr else (N, Ci, H, W, Co, k, k, s, s, p, p, 1, 1)


# The float64 restatement.  A base conv takes `big` (N, Cb, Hb, Wb) to `small` (N, Cs, Hs, Ws) with a weight (Cs, Cb, k, k), stride s and
# explicit zero padding p.  Every product the kernels form is formed here, elementwise (so inf * 0 = NaN appears where a kernel makes
# it), and every sum starts at +0.  exact=False contracts by matmul instead (finite values only: one product per element is exact in
# any order).
def _contract(a, w, exact):
    """a (N, Ca, H, W), w (Co, Ca) -> (N, Co, H, W)"""
    if exact:
        return (a[:, None] * w[None, :, :, None, None]).sum(2)
    return torch.einsum("nahw,oa->nohw", a, w)


def _fwd(big, w, s, p, exact=True):
    k = w.shape[2]
    bp = torch.nn.functional.pad(big, (p, p, p, p))
    Hs, Ws = (bp.shape[2] - k) // s + 1, (bp.shape[3] - k) // s + 1
    out = torch.zeros(big.shape[0], w.shape[0], Hs, Ws, dtype=torch.float64)
    for i in range(k):
        for j in range(k):
            out = out + _contract(bp[:, :, i:i + s * (Hs - 1) + 1:s, j:j + s * (Ws - 1) + 1:s], w[:, :, i, j], exact)
    return out


def _dgrad_gather(small, w, s, p, big_hw, exact=True):
    """the input gradient as the dense families compute it: a stride-1 conv with the rotated, transposed kernel and pad' = k - 1 - p over
    grad_output, zero-inserted for s = 2 (conv_strided.hip): the inserted and the padding zeros meet every tap"""
    k = w.shape[2]
    Hd, Wd = big_hw[0] + 2 * p - k + 1, big_hw[1] + 2 * p - k + 1
    d = torch.zeros(small.shape[0], small.shape[1], Hd, Wd, dtype=torch.float64)
    d[:, :, ::s, ::s] = small
    out = _fwd(d, w.flip(2, 3).transpose(0, 1), 1, k - 1 - p, exact)
    assert tuple(out.shape[2:]) == tuple(big_hw)
    return out


def _dgrad_scatter(small, w, s, exact=True):
    """k = s, p = 0 (ConvTranspose2d's forward): every tap writes a phase of its own, no product crosses phases"""
    k = w.shape[2]
    out = torch.zeros(small.shape[0], w.shape[1], s * small.shape[2], s * small.shape[3], dtype=torch.float64)
    for i in range(k):
        for j in range(k):
            out[:, :, i::s, j::s] = _contract(small, w[:, :, i, j].t(), exact)
    return out


def _wgrad(big, small, k, s, p, exact=True):
    bp = torch.nn.functional.pad(big, (p, p, p, p))
    Hs, Ws = small.shape[2:]
    gw = torch.zeros(small.shape[1], big.shape[1], k, k, dtype=torch.float64)
    for i in range(k):
        for j in range(k):
            v = bp[:, :, i:i + s * (Hs - 1) + 1:s, j:j + s * (Ws - 1) + 1:s]
            if exact:
                gw[:, :, i, j] = (small[:, :, None] * v[:, None]).sum((0, 3, 4))
            else:
                gw[:, :, i, j] = torch.einsum("nshw,nbhw->sb", small, v)
    return gw


def restate(geo, entry, x, w, go, exact=True):
    """one entry of the family in float64 (bias zero; backward_parameters -> grad_weight)"""
    _, k, s, p, tr = GEOS[geo]
    if not tr:
        if entry == "forward":
            return _fwd(x, w, s, p, exact)
        if entry == "backward_input":
            return _dgrad_gather(go, w, s, p, x.shape[2:], exact)
        return _wgrad(x, go, k, s, p, exact)
    if entry == "forward":
        return _dgrad_scatter(x, w, s, exact)
    if entry == "backward_input":
        return _fwd(go, w, s, p, exact)
    return _wgrad(go, x, k, s, p, exact)


def _shapes(geo, Ci, Co, Hx, Wx):
    _, k, s, p, tr = GEOS[geo]
    wshape = (Ci, Co, k, k) if tr else (Co, Ci, k, k)
    Ho, Wo = (s * Hx, s * Wx) if tr else ((Hx + 2 * p - k) // s + 1, (Wx + 2 * p - k) // s + 1)
    return (1, Ci, Hx, Wx), wshape, (1, Co, Ho, Wo)


def _selector_tap(geo):
    k = GEOS[geo][1]
    return (1, 0) if GEOS[geo][4] else (k // 2, k // 2)          # the centre tap; ConvTranspose2d: a tap off the first phase


def _pixel_selector(geo, shape, which):
    """a 0/1 tensor with one pixel per channel, the pixels six columns apart (twelve in ConvTranspose2d's grad_output, three in the
    strided conv's) so that the windows they select do not meet"""
    _, k, s, p, tr = GEOS[geo]
    t = torch.zeros(shape, dtype=torch.float64)
    for c in range(shape[1]):
        if which == "x":
            r, q = (4, 4 + 6 * c) if s == 2 and not tr else (3, 3 + 6 * c)
        elif tr:
            r, q = 7, 6 + 12 * c
        elif s == 2:
            r, q = 2, 2 + 3 * c
        else:
            r, q = 3, 3 + 6 * c
        t[0, c, r, q] = 1.0
    return t


@functools.lru_cache(maxsize=None)
def _build(geo, entry, holder, n, spread):
    """the three operands in float64 with the holder numbered 1 .. numel -> (x, w, go, shapes, slots): slots = the flat indices of
    n holder elements that an output element reads, which take the probe values.
    Image kind (input or grad_output through a one-tap weight): one channel, 53 (106) columns.  Channel kind (a weight, or the two
    operands of backward_parameters): C x C channels, the other operand selects one pixel per channel; C grows until n elements are read.
    spread (the run of values that become inf): image kind: slots far apart; channel kind: one slot per channel, and for a weight on
    the diagonal cout = cin, so that no row or column of the product meets two non-finite values"""
    _, k, s, p, tr = GEOS[geo]
    channel_kind = holder == "w" or entry == "backward_parameters"
    C = n + 1 if spread else max(2, int((n / (k * k)) ** 0.5))
    while True:
        if channel_kind:
            xs, ws, gs = _shapes(geo, C, C, 7, 6 * C + 6)
        else:
            m = 2 if s == 2 and not tr else 1
            xs, ws, gs = _shapes(geo, 1, 1, m * max(7, -(-n // 53)), m * 53)
        shapes = {"x": xs, "w": ws, "go": gs}
        ops = {}
        for name in ("x", "w", "go"):
            if name == holder:
                ops[name] = torch.arange(1, torch.Size(shapes[name]).numel() + 1, dtype=torch.float64).view(shapes[name])
            elif name == "w":
                ops[name] = torch.zeros(ws, dtype=torch.float64)
                ops[name][:, :, _selector_tap(geo)[0], _selector_tap(geo)[1]] = 1.0
            elif (entry == "forward" and name == "go") or (entry == "backward_input" and name == "x"):
                ops[name] = torch.zeros(shapes[name], dtype=torch.float64)          # not read by the entry
            else:
                ops[name] = _pixel_selector(geo, shapes[name], name)
        read = restate(geo, entry, ops["x"], ops["w"], ops["go"], exact=False)
        ones = dict(ops)
        ones[holder] = torch.ones(shapes[holder], dtype=torch.float64)
        assert float(restate(geo, entry, ones["x"], ones["w"], ones["go"], exact=False).max()) == 1.0, "more than one product per element"
        slots = torch.unique(read[read > 0]).long() - 1
        if spread and channel_kind:
            hs = shapes[holder]
            per = torch.Size(hs[2:]).numel()
            c0, c1 = (slots // (per * hs[1]), (slots // per) % hs[1]) if holder == "w" else ((slots // per) % hs[1],) * 2
            # channel c takes the c-th of its read elements: for a weight that walks the taps from the first corner on, so non-finite
            # weights meet the padding's zeros at the border (inf * 0 = NaN there is predicted like everywhere else)
            own = [slots[(c0 == c) & (c1 == c)] for c in range(n)]
            slots = torch.stack([s[c % s.numel()] for c, s in enumerate(own)])
        elif spread:
            assert slots.numel() >= 53 * n                             # the read elements form rows of 53: one value a row, five columns on
            slots = slots[torch.arange(n) * 58]
        if slots.numel() >= n:
            return ops["x"], ops["w"], ops["go"], shapes, slots[:n]
        assert channel_kind and not spread
        C += max(1, C // 8)


def _run_entry(geo, entry, mode, x, w, go):
    prefix = GEOS[geo][0]
    N, Ci, H, W = x.shape
    Co = go.shape[1]
    a = Abi(prefix, _dims(geo, N, Ci, H, W, Co), (x, w, torch.zeros(Co), go), mode)
    nan = float("nan")
    if entry == "forward":
        got = a.forward(torch.full_like(a.go, nan))
    elif entry == "backward_input":
        got = a.backward_input(torch.full_like(a.x, nan))
    else:
        got, _ = a.backward_parameters(torch.zeros_like(a.w), torch.zeros_like(a.b))
    torch.cuda.synchronize()
    return got.cpu()


def _probe(geo, entry, holder, mode, values, spread=False, want_inf=False):
    """place `values` (fp32) in the holder, run the entry and compare with the restatement on the rounded operands"""
    what = "%s %s values in %s, %s compute" % (geo, entry, holder, mode)
    x, w, go, shapes, slots = _build(geo, entry, holder, values.numel(), spread)
    carrier = torch.zeros(torch.Size(shapes[holder]).numel())
    carrier[slots] = values
    ops = {"x": x.float(), "w": w.float(), "go": go.float()}
    ops[holder] = carrier.view(shapes[holder])
    got = _run_entry(geo, entry, mode, ops["x"], ops["w"], ops["go"])
    r = {n: nr.rounded(t, mode).double() for n, t in ops.items()}
    want64 = restate(geo, entry, r["x"], r["w"], r["go"], exact=spread or (holder != "w" and entry != "backward_parameters"))
    want = want64.float()
    assert torch.equal(want.double(), want64) or bool(torch.isnan(want64).any())                 # one product: fp32 holds it
    # every probe value is met: its rounding (where that is not zero) is among the expected elements
    rv = nr.rounded(values, mode)
    have = set(nr.f32_bits(want.reshape(-1)).tolist())
    missing = [float(v) for v, b in zip(rv.tolist(), nr.f32_bits(rv).tolist()) if v != 0 and v == v and abs(v) != float("inf") and b not in have]
    assert not missing, (what, "probe values no element reads", missing[:5])
    if want_inf:
        assert bool((want == float("inf")).any()) and bool((want == float("-inf")).any()) and bool(torch.isnan(want).any()), what
    mask = nr.same_class(got, want, what)
    gb, wb = nr.f32_bits(got)[mask], nr.f32_bits(want)[mask]
    bad = gb != wb
    print("%s: %d elements, %d finite, %d differ" % (what, got.numel(), int(mask.sum()), int(bad.sum())))
    if bool(bad.any()):
        g, e = got[mask][bad], want[mask][bad]
        shown = ", ".join("got %r (%#010x) want %r (%#010x)" % (float(a), int(nr.f32_bits(a.reshape(1))), float(b), int(nr.f32_bits(b.reshape(1))))
                          for a, b in list(zip(g, e))[:6])
        flushed = int(((g == 0) & (e != 0)).sum())
        raise AssertionError("%s: %d of %d finite elements differ (%d of them zero where a nonzero value is due): %s" % (
            what, int(bad.sum()), int(mask.sum()), flushed, shown))


@functools.lru_cache(maxsize=None)
def _values(mode, overflow):
    """the probe values of a compute mode: edges(T), split into those that stay finite in the type and those that become +-inf (with
    +-inf and NaN themselves); fp32 compute takes both types' edges and fp32's own subnormals and ends"""
    if mode == "fp32":
        fin = torch.cat([nr.edges("fp16"), nr.edges("bf16"), nr.f32_edges()])
        return torch.tensor([float("inf"), float("-inf"), float("nan"), 3.0e38, -3.0e38]) if overflow else fin
    e = nr.edges(mode)
    over = torch.isinf(nr.rne(mode, e))
    extra = torch.tensor([float("inf"), float("-inf"), float("nan")])
    return torch.cat([e[over], extra]) if overflow else e[~over]


# (entry, the tensor that carries the probe values): section 2b rounds input and grad_output, section 2c the weight
PROBES = [("forward", "x"), ("backward_input", "go"), ("backward_parameters", "x"), ("backward_parameters", "go"),
          ("forward", "w"), ("backward_input", "w")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry,holder", PROBES)
@pytest.mark.parametrize("geo", list(GEOS))
def test_operands_are_rounded_once_to_nearest_even(geo, entry, holder, mode):
    _probe(geo, entry, holder, mode, _values(mode, False))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry,holder", PROBES)
@pytest.mark.parametrize("geo", list(GEOS))
def test_values_past_the_largest_finite_become_inf_and_nan_is_predicted(geo, entry, holder, mode):
    _probe(geo, entry, holder, mode, _values(mode, True), spread=True, want_inf=True)


# ---- 3. the scale sweep and homogeneity ----------------------------------------------------------------------------------------------------
def _abi(family, case, mode, inputs):
    return Abi(nr.FAMILIES[family][0], nr.FAMILIES[family][2](*nr.SHAPES[case]), inputs, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family,case", nr.SWEEP_CASES)
def test_scale_sweep_against_float64_without_a_floor(family, case, mode):
    for scale, exps in nr.SCALES[mode].items():
        x, w, b, go = nr.scaled_inputs(family, case, exps)
        if mode == "fp16":
            for t, a in ((x, exps[0]), (go, exps[2])):
                r = nr.rne("fp16", t)
                if a == -20:
                    assert bool((r.abs() < 2.0 ** -14).all()) and float((r != 0).double().mean()) >= 0.9
                if a == 13:
                    assert bool(torch.isfinite(r).all())
        ref, S, bound = nr.sweep_reference(family, case, mode, scale)
        got = _abi(family, case, mode, (x, w, b, go)).all()
        failed = []
        for name, g, r, bd in zip(nr.NAMES, got, ref, bound):
            try:
                nr.worst_share("%s %s %s %s %s" % (family, case, mode, scale, name), g, r, bd)
            except AssertionError as e:
                failed.append(str(e))
        assert not failed, failed


@pytest.mark.parametrize("a", [40, -40])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("family,case", nr.SWEEP_CASES)
def test_scaling_by_a_power_of_two_changes_no_mantissa_bit(family, case, mode, a):
    x, w, b, go = nr.unit_inputs(family, case)
    f = 2.0 ** a
    y0, gx0, gw0, gb0 = (t.cpu() for t in _abi(family, case, mode, (x, w, b, go)).all())
    y1, _, gw1, gb1 = (t.cpu() for t in _abi(family, case, mode, (x * f, w, b * f, go)).all())
    _, gx2, gw2, gb2 = (t.cpu() for t in _abi(family, case, mode, (x, w, b, go * f)).all())
    for name, scaled, unit in (("output", y1, y0), ("grad_weight of x", gw1, gw0), ("grad_bias of x", gb1, gb0), ("grad_input", gx2, gx0),
                               ("grad_weight of grad_output", gw2, gw0), ("grad_bias of grad_output", gb2, gb0)):
        if name == "grad_bias of x":
            want = unit                                                 # (grad_bias does not read x)
        else:
            want = unit * f
        assert bool(torch.isfinite(want).all()) and bool((want.abs() >= 2.0 ** -126).logical_or(want == 0).all())
        bad = nr.f32_bits(scaled) != nr.f32_bits(want)
        assert not bool(bad.any()), "%s %s %s 2^%d %s: %d of %d elements differ from 2^a times the unit-scale result" % (
            family, case, mode, a, name, int(bad.sum()), bad.numel())
