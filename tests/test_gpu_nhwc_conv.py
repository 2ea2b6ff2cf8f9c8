"""The resident conv (tdrn_hip.h section i-k: tdrn_conv2d_nhwc_*, networks.conv2d_nhwc) on the GPU.

Inputs are exact 16-bit values, references float64 autograd on the CPU.  Bounds (u, tiny, c, S: tests/_nhwc_harness.py):
output and grad_input |got - ref| <= c S + u (|ref| + c S) + tiny (fp32 accumulation, one rounding of the result); grad_weight and
grad_bias c S (fp32 results).  No element is exempted.

conv_route.hip sends a 3x3 / pad 1 / dilation 1 layer to the direct-conv kernels from 400 pixels a map, so the conv3x3_patch cases are
the smallest maps of that size with each tile mode: 16 x 32 (W % 32 == 0, H % 8 == 0), 32 x 16 (16 x 16 tiles) and 21 x 20 (flat).
kernels.h states that every route but head3x3 gives the same output bits.  On these entries that holds only for a launch with one
64-channel chunk and no bias (measured: DESIGN 22): conv3x3_patch / conv3x3_pp start their accumulators at the bias and walk the taps
inside a channel chunk, conv_igemm adds the bias last and walks the chunks inside a tap.  So the patch cases are compared bit for bit
with the same entry under TDRN_CONV_NHWC_IGEMM_ONLY where the orders agree and held to the float64 bound on both routes elsewhere,
and the conv3x3_pp case (conv3_2 at batch 8: 200 items, 29 GMAC) is gated on a float64 reference of 64 sampled pixels.
Split-K of launch_conv, by igemm_splitk_choice: fewer than 160 blocks of 128 pixels x the cout tile and nk = taps Cin / 64 >= 8 steps
give min(ceil(384 / blocks), nk / 4, 16) slices: 9 for `splitk` (1 block, nk = 36), 2 for the 64-channel 3x3 cases, none for `k1`
(nk = 2).  Weight-gradient K splits, by conv_wgrad_splits: min(ceil(512 / tiles), ceil(M / 256)): 2 for the 512-pixel cases, 1 below
257 pixels.

The direct-conv cases here run one image (conv3x3_patch: 64-cout items, at most one per workgroup, no tail split) or one item per
workgroup (conv3x3_pp: 16 x 16 tiles, bf16, one cout tile), and Cout = Npad throughout.  test_gpu_nhwc_direct.py holds the variants
they do not reach: 128-cout items, the tail split, several items per workgroup, two cout tiles, flat and 8 x 32 tiles on
conv3x3_pp, fp16 there, and Cout < Npad on every direct route."""
import pytest
import torch
import torch.nn.functional as F

from tdrn_amd import _lib
from tdrn_amd.model import networks

from _conv_train_harness import C_ACC, DEV
from _nhwc_harness import TYPES, ConvAbi, GuardedResident, assert_within, bound16, exact, nchw64, raw_equal, resident

pytestmark = pytest.mark.gpu

# (forward split-K slices, input-gradient slices, weight-gradient K splits) the library reports for a case: what the docstring derives
SPLITS = {"tile": (2, 2, 1), "ragged": (2, 4, 1), "k1": (1, 1, 1), "dil6": (2, 2, 1), "fullpad": (2, 2, 1), "valid": (2, 2, 1),
          "splitk": (9, 2, 1), "patch32": (1, 1, 2), "patch16": (1, 1, 2), "flat": (1, 1, 2)}

#        name       N  Cin  H   W  Cout k pad dil  forward / input-gradient kernel
CASES = {"tile":   (1, 64,  8,  8,  64, 3, 1, 1, "igemm"),
         "ragged": (2, 64,  9,  7, 128, 3, 1, 1, "igemm"),
         "k1":     (2, 128, 7,  5,  64, 1, 0, 1, "igemm"),
         "dil6":   (1, 64,  7,  7,  64, 3, 6, 6, "igemm"),
         "fullpad": (1, 64, 6,  5,  64, 3, 2, 1, "igemm"),
         "valid":  (1, 64,  9,  8,  64, 3, 0, 1, "igemm"),
         "splitk": (1, 256, 5,  5,  64, 3, 1, 1, "igemm"),
         "patch32": (1, 64, 16, 32, 64, 3, 1, 1, "patch"),
         "patch16": (1, 64, 32, 16, 64, 3, 1, 1, "patch"),
         "flat":   (1, 64, 21, 20, 128, 3, 1, 1, "patch")}
PATCH = ("patch32", "patch16", "flat")
MODES = ("bf16", "fp16")


def splits_of(case, mode="bf16"):
    import ctypes
    f, d, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().tdrn_conv2d_nhwc_splits(*dims_of(case), _lib.DTYPES[mode], 0, ctypes.byref(f), ctypes.byref(d), ctypes.byref(w)) == 0
    return f.value, d.value, w.value


def test_cases_split_as_the_docstring_says():
    """the cases that are here FOR a split keep it: launch_conv's split-K (`splitk`: 9 slices forward; the small 3x3 cases 2) and more
    than one K split of the weight gradient (the 400-pixel-and-up cases)"""
    for case, want in SPLITS.items():
        for mode in MODES:
            assert splits_of(case, mode) == want, (case, mode, splits_of(case, mode))
    assert SPLITS["splitk"][0] > 1 and SPLITS["ragged"][1] > 1 and SPLITS["flat"][2] > 1


def dims_of(case):
    N, Cin, H, W, Cout, k, pad, dil, _ = CASES[case]
    return (N, Cin, H, W, Cout, k, k, 1, 1, pad, pad, dil, dil)


def inputs(case, mode):
    N, Cin, H, W, Cout, k, pad, dil, _ = CASES[case]
    g = torch.Generator().manual_seed(sorted(CASES).index(case) * 7 + MODES.index(mode))
    Ho = H + 2 * pad - dil * (k - 1)
    Wo = W + 2 * pad - dil * (k - 1)
    x = exact(torch.randn(N, Cin, H, W, generator=g), mode)
    w = exact(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5, mode)
    b = exact(torch.randn(Cout, generator=g), mode)
    go = exact(torch.randn(N, Cout, Ho, Wo, generator=g), mode)
    return x, w, b, go


_REF = {}


def reference(case, mode):
    """((y, gx, gw, gb), (Sy, Sgx, Sgw, Sgb)) in float64, computed once"""
    if (case, mode) not in _REF:
        _, _, _, _, _, _, pad, dil, _ = CASES[case]
        out = []
        for absolute in (False, True):
            x, w, b, go = (t.double().abs() if absolute else t.double() for t in inputs(case, mode))
            x.requires_grad_(True); w.requires_grad_(True); b.requires_grad_(True)
            y = F.conv2d(x, w, b, 1, pad, dil)
            y.backward(go)
            out.append((y.detach(), x.grad, w.grad, b.grad))
        _REF[(case, mode)] = tuple(out)
    return _REF[(case, mode)]


def run_abi(case, mode, flags=0, guarded=False):
    """the three entries -> (y, gx, gw, gb) on the device, and the guarded buffers"""
    x, w, b, go = inputs(case, mode)
    abi = ConvAbi(dims_of(case), mode, flags)
    xr, gor, wd, bd = resident(x, mode), resident(go, mode), w.to(DEV), b.to(DEV)
    nan = float("nan")
    if guarded:
        y, gx = GuardedResident(go.shape, mode), GuardedResident(x.shape, mode)
        yt, gxt = y.t, gx.t
    else:
        y = gx = None
        yt, gxt = torch.full_like(gor, nan), torch.full_like(xr, nan)
    abi.forward(xr, wd, bd, yt)
    abi.backward_input(gor, wd, gxt)
    gw, gb = abi.backward_parameters(xr, gor, torch.zeros_like(wd), torch.zeros_like(bd))
    torch.cuda.synchronize()
    return (yt, gxt, gw, gb), (y, gx), abi


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_entries_against_float64(case, mode):
    (y, gx, gw, gb), guards, abi = run_abi(case, mode, guarded=True)
    assert abi.route(0) == CASES[case][-1] and abi.route(1) == CASES[case][-1], (abi.route(0), abi.route(1))
    for g, what in zip(guards, ("output", "grad_input")):
        g.check("%s %s %s" % (case, mode, what))                # guard bands intact, every element written
    ref, S = reference(case, mode)
    assert_within("%s %s output" % (case, mode), nchw64(y), ref[0], bound16(mode, ref[0], S[0]))
    assert_within("%s %s grad_input" % (case, mode), nchw64(gx), ref[1], bound16(mode, ref[1], S[1]))
    assert_within("%s %s grad_weight" % (case, mode), gw.cpu().double(), ref[2], C_ACC[mode] * S[2])
    assert_within("%s %s grad_bias" % (case, mode), gb.cpu().double(), ref[3], C_ACC[mode] * S[3])


def run_pair(case, mode, bias):
    """forward (with or without a bias) and input gradient of one case on the default route and under TDRN_CONV_NHWC_IGEMM_ONLY"""
    x, w, b, go = inputs(case, mode)
    xr, gor, wd, bd = resident(x, mode), resident(go, mode), w.to(DEV), (b.to(DEV) if bias else None)
    out = []
    for flags in (0, _lib.CONV_NHWC_IGEMM_ONLY):
        abi = ConvAbi(dims_of(case), mode, flags)
        out.append((abi.forward(xr, wd, bd, torch.full_like(gor, float("nan"))), abi.backward_input(gor, wd, torch.full_like(xr, float("nan"))),
                    abi.route(0), abi.route(1)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", PATCH)
def test_patch_against_igemm(case, mode):
    """Bit for bit where the two kernels sum in the same fp32 order: a launch with ONE 64-channel chunk (conv3x3_patch walks the taps
    inside a channel chunk, conv_igemm the channel chunks inside a tap) and no bias (conv3x3_patch starts its accumulators at the
    bias, conv_igemm adds it behind the sum).  That is the forward without a bias of all three cases and the input gradient of the two
    64 -> 64 ones; `flat`'s input gradient convolves 128 channels.  Everything else is held to the float64 bound on BOTH routes."""
    d, i = run_pair(case, mode, False)
    assert (d[2], d[3], i[2], i[3]) == ("patch", "patch", "igemm", "igemm")
    assert raw_equal(d[0], i[0]), "conv3x3_patch and conv_igemm differ in a forward without bias"
    ref, S = reference(case, mode)
    if CASES[case][4] == 64:
        assert raw_equal(d[1], i[1]), "conv3x3_patch and conv_igemm differ in the input gradient"
    for got, what in ((d[1], "patch"), (i[1], "igemm")):
        assert_within("%s %s grad_input on %s" % (case, mode, what), nchw64(got), ref[1], bound16(mode, ref[1], S[1]))
    d, i = run_pair(case, mode, True)
    for got, what in ((d[0], "patch"), (i[0], "igemm")):
        assert_within("%s %s forward with bias on %s" % (case, mode, what), nchw64(got), ref[0], bound16(mode, ref[0], S[0]))


def test_pp_against_sampled_float64():
    """conv3_2 at batch 8: 200 items of 256 pixels x 256 couts, Cin = 256: four channel chunks, so conv3x3_pp and conv_igemm sum in
    different fp32 orders and are not bit-equal.  Forward (with a bias) and input gradient of both routes against float64
    on 64 sampled pixels, all 256 channels of each"""
    dims, mode = (8, 256, 80, 80, 256, 3, 3, 1, 1, 1, 1, 1, 1), "bf16"
    g = torch.Generator().manual_seed(5)
    xc = exact(torch.randn(8, 256, 80, 80, generator=g), mode)
    goc = exact(torch.randn(8, 256, 80, 80, generator=g), mode)
    wc = exact(torch.randn(256, 256, 3, 3, generator=g) / 48, mode)
    bc = torch.randn(256, generator=g)
    x, go, w, b = resident(xc, mode), resident(goc, mode), wc.to(DEV), bc.to(DEV)
    # sampled pixels: corners, edges and the inside of several images and tiles
    pix = [(0, 0, 0), (0, 0, 79), (7, 79, 0), (7, 79, 79), (3, 0, 40), (4, 41, 79), (2, 15, 16), (5, 16, 15)]
    pix += [(int(n), int(h), int(w_)) for n, h, w_ in zip(torch.randint(0, 8, (56,), generator=g), torch.randint(0, 80, (56,), generator=g),
                                                          torch.randint(0, 80, (56,), generator=g))]

    def sampled(t, weight, bias):
        """float64 conv of the 3x3 neighbourhoods of the sampled pixels of t with weight (out, in, 3, 3) -> (reference, S)"""
        tp = F.pad(t, (1, 1, 1, 1)).double()
        patches = torch.stack([tp[n, :, h:h + 3, w_:w_ + 3] for n, h, w_ in pix])
        ref = torch.einsum("pcij,ocij->po", patches, weight) + bias
        return ref, torch.einsum("pcij,ocij->po", patches.abs(), weight.abs()) + bias.abs()
    ref_y, S_y = sampled(xc, wc.double(), bc.double())
    ref_gx, S_gx = sampled(goc, wc.double().flip(2, 3).transpose(0, 1), torch.zeros(256, dtype=torch.float64))
    pick = lambda t: torch.stack([t[n, :, h, w_] for n, h, w_ in pix]).float().cpu().double()
    for flags, want in ((0, "pp"), (_lib.CONV_NHWC_IGEMM_ONLY, "igemm")):
        abi = ConvAbi(dims, mode, flags)
        assert (abi.route(0), abi.route(1)) == (want, want)
        y = abi.forward(x, w, b, torch.full_like(go, float("nan")))
        gx = abi.backward_input(go, w, torch.full_like(x, float("nan")))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(gx.float()).all())
        assert_within("%s forward with bias, 64 sampled pixels" % want, pick(y), ref_y, bound16(mode, ref_y, S_y))
        assert_within("%s input gradient, 64 sampled pixels" % want, pick(gx), ref_gx, bound16(mode, ref_gx, S_gx))


@pytest.mark.parametrize("case", ["ragged", "splitk", "patch16", "flat"])
def test_bitwise_reproducible(case):
    a, _, _ = run_abi(case, "bf16")
    b, _, _ = run_abi(case, "bf16")
    assert raw_equal(a[0], b[0]) and raw_equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_grad_weight_accumulates_with_scale():
    case, mode = "ragged", "fp16"
    x, w, b, go = inputs(case, mode)
    abi = ConvAbi(dims_of(case), mode)
    xr, gor = resident(x, mode), resident(go, mode)
    gw1, gb1 = abi.backward_parameters(xr, gor, torch.zeros_like(w, device=DEV), torch.zeros_like(b, device=DEV))
    g = torch.Generator().manual_seed(9)
    gw0, gb0 = torch.randn(w.shape, generator=g).to(DEV), torch.randn(b.shape, generator=g).to(DEV)
    gw, gb = abi.backward_parameters(xr, gor, gw0.clone(), gb0.clone(), scale=-0.5)
    torch.cuda.synchronize()
    # the sums are the same floats; += scale * sum is one fma per element
    assert torch.equal(gw, torch.addcmul(gw0.double(), gw1.double(), torch.tensor(-0.5, dtype=torch.float64, device=DEV)).float())
    assert torch.equal(gb, torch.addcmul(gb0.double(), gb1.double(), torch.tensor(-0.5, dtype=torch.float64, device=DEV)).float())
    # without a bias gradient: grad_weight alone, the same bits
    gw2, _ = abi.backward_parameters(xr, gor, torch.zeros_like(gw1), None)
    torch.cuda.synchronize()
    assert torch.equal(gw2, gw1)


def test_python_op_equals_the_entries_and_autograd_plumbing():
    case, mode = "flat", "bf16"
    x, w, b, go = inputs(case, mode)
    _, _, _, _, _, _, pad, dil, _ = CASES[case]
    (y, gx, gw, gb), _, _ = run_abi(case, mode)
    xr = resident(x, mode).requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = networks.conv2d_nhwc(xr, wd, bd, pad, dil)
    assert out.dtype == TYPES[mode] and out.is_contiguous(memory_format=torch.channels_last) and out.grad_fn is not None
    # a grad_output that is neither resident nor of the type: fp32 NCHW
    out.backward(go.to(DEV))
    assert raw_equal(out.detach(), y) and raw_equal(xr.grad, gx) and torch.equal(wd.grad, gw) and torch.equal(bd.grad, gb)
    assert xr.grad.dtype == TYPES[mode] and wd.grad.dtype == torch.float32
    # needs_input_grad subsets
    for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        xs = resident(x, mode).requires_grad_(need[0])
        ws, bs = w.to(DEV).requires_grad_(need[1]), b.to(DEV).requires_grad_(need[2])
        networks.conv2d_nhwc(xs, ws, bs, pad, dil).backward(resident(go, mode))
        for t, n, want in ((xs, need[0], gx), (ws, need[1], gw), (bs, need[2], gb)):
            assert (t.grad is not None) == n
            if n:
                assert raw_equal(t.grad, want) if t is xs else torch.equal(t.grad, want)
    # nothing requires grad / no_grad: the forward alone
    assert networks.conv2d_nhwc(resident(x, mode), w.to(DEV), b.to(DEV), pad, dil).grad_fn is None
    with torch.no_grad():
        o = networks.conv2d_nhwc(xr, wd, bd, pad, dil)
    assert o.grad_fn is None and raw_equal(o, y)
    # a misaligned storage is cloned, an NCHW-contiguous 16-bit tensor is made resident
    flat = torch.empty(xr.numel() + 1, dtype=TYPES[mode], device=DEV)
    off = flat[1:].view(x.shape[0], x.shape[2], x.shape[3], x.shape[1]).permute(0, 3, 1, 2)
    off.copy_(xr.detach())
    assert off.data_ptr() % 16 != 0
    assert raw_equal(networks.conv2d_nhwc(off, w.to(DEV), b.to(DEV), pad, dil), y)
    assert raw_equal(networks.conv2d_nhwc(xr.detach().contiguous(), w.to(DEV), b.to(DEV), pad, dil), y)


def test_python_op_refusals():
    x = torch.zeros(1, 64, 8, 8, dtype=torch.bfloat16, device=DEV).contiguous(memory_format=torch.channels_last)
    w = torch.zeros(64, 64, 3, 3, device=DEV)
    with pytest.raises(NotImplementedError):
        networks.conv2d_nhwc(x.cpu(), w.cpu())
    with pytest.raises(ValueError):
        networks.conv2d_nhwc(x.float(), w)                                  # fp32 is conv2d's
    with pytest.raises(RuntimeError):
        networks.conv2d_nhwc(x, torch.zeros(64, 64, 5, 5, device=DEV), None, 2)      # k = 5
    with pytest.raises(RuntimeError):
        networks.conv2d_nhwc(x, torch.zeros(70, 64, 3, 3, device=DEV), None, 1)      # Cout % 64
    with pytest.raises(RuntimeError):
        networks.conv2d_nhwc(x[:, :32], torch.zeros(64, 32, 3, 3, device=DEV), None, 1)
    # conv2d given a bf16 tensor converts it to fp32, as before
    y = networks.conv2d(x, w, None, 1, 1, "bf16")
    assert y.dtype == torch.float32 and y.is_contiguous()
