"""The resident conv's direct-conv kernels (conv3x3_patch, conv3x3_pp behind tdrn_conv2d_nhwc_*) at the variants a training step at
batch 32 runs and test_gpu_nhwc_conv.py does not reach: 128-cout patch items with and without the tail split, several items in a
workgroup, conv3x3_pp's item-to-item path, two cout tiles (n_major), flat and 8 x 32 tiles, fp16, an odd chunk count, and Cout < Npad
on every direct route.  tests/_nhwc_direct_cases.py holds the cases, the launch each reaches (LAUNCHES, checked without a GPU by
test_nhwc_direct_ref.py), the period-3 replica inputs and the float64 references; DESIGN.md section 22 the measured shares.

Per case and type the three entries run once on guarded resident buffers (module-scoped fixture `ran`); then
  * the routes are the table's, the guard bands intact, every element written;
  * every element of every replica is within the float64 bounds (bound16 for output and grad_input, c S for grad_weight / grad_bias);
  * output and grad_input of every replica are bit-equal to the first period's: conv3x3_patch.hip and conv3x3_pp.hip state that an
    element's fp32 order does not depend on where its tile or item falls, and the tail split's half items rest on it.
patch_bn128_32 (one 64-channel chunk) is also bit-equal to conv_igemm without a bias, the condition of DESIGN 22 on 128-cout items.

Splits: every forward and input gradient here is a direct-conv launch, which is never split (conv_splitk_choice).  Weight-gradient K
splits by conv_wgrad_splits, S = min(ceil(512 / tiles), ceil(M / 256)) with tiles = (Cin / 64) (Cout / 64), per_split = ceil(M / S)
rounded up to 64, splits = ceil(M / per_split): pp_flat 32 tiles, M 36000: S 16, per 2304 -> 16; pp_32 28 tiles, M 50688: S 19, per
2688 -> 19; pp_16 16 tiles, M 76032: S 32, per 2432 -> 32; patch_flat_chunks 9 tiles, M 1260: S 5, per 256 -> 5; patch_bn128_32 3
tiles, M 24576: S 96, per 256 -> 96; patch_tail_16 8 tiles, M 36864: S 64, per 576 -> 64."""
import ctypes

import pytest
import torch

import _nhwc_direct_cases as D
from tdrn_amd import _lib

from _conv_train_harness import DEV
from _nhwc_harness import ConvAbi, GuardedResident, raw_equal, resident

pytestmark = pytest.mark.gpu

# (forward split-K slices, input-gradient slices, weight-gradient K splits) the library reports: what the docstring derives
SPLITS = {"pp_flat": (1, 1, 16), "pp_32": (1, 1, 19), "pp_16": (1, 1, 32), "patch_flat_chunks": (1, 1, 5), "patch_bn128_32": (1, 1, 96),
          "patch_tail_16": (1, 1, 64)}
PARAMS = [(case, mode) for case in D.CASES for mode in D.MODES]


def device_batch(t, case, mode):
    """the resident batch of a base: uploaded once, repeated on the device"""
    return resident(t.to(DEV).repeat(D.replicas(case), 1, 1, 1), mode)


@pytest.fixture(scope="module", params=PARAMS, ids=["%s-%s" % p for p in PARAMS])
def ran(request):
    """the three entries of one case and type, once: guarded outputs, parameter gradients and the ConvAbi"""
    case, mode = request.param
    x, w, b, go = D.base_inputs(case, mode)
    abi = ConvAbi(D.dims_of(case), mode)
    xr, gor, wd, bd = device_batch(x, case, mode), device_batch(go, case, mode), w.to(DEV), b.to(DEV)
    y, gx = GuardedResident(gor.shape, mode), GuardedResident(xr.shape, mode)
    abi.forward(xr, wd, bd, y.t)
    abi.backward_input(gor, wd, gx.t)
    gw, gb = abi.backward_parameters(xr, gor, torch.zeros_like(wd), torch.zeros_like(bd))
    torch.cuda.synchronize()
    yield case, mode, abi, y, gx, gw, gb


def test_entries_against_float64(ran):
    case, mode, abi, y, gx, gw, gb = ran
    assert (abi.route(0), abi.route(1)) == tuple(l.kernel for l in D.LAUNCHES[case]), (abi.route(0), abi.route(1))
    for g, what in ((y, "output"), (gx, "grad_input")):
        g.check("%s %s %s" % (case, mode, what))                # guard bands intact, every element written
    ref, S = D.reference(case, mode)
    D.assert_replicas_within("%s %s output" % (case, mode), mode, y.t, ref[0], S[0])
    D.assert_replicas_within("%s %s grad_input" % (case, mode), mode, gx.t, ref[1], S[1])
    D.assert_sum_within("%s %s grad_weight" % (case, mode), mode, gw, ref[2], S[2])
    D.assert_sum_within("%s %s grad_bias" % (case, mode), mode, gb, ref[3], S[3])


def test_replicas_are_bit_equal(ran):
    """an element's bits do not depend on the tile, item, workgroup or XCD its replica falls into (whole item or tail-split half)"""
    case, mode, abi, y, gx, gw, gb = ran
    for g, what in ((y, "output"), (gx, "grad_input")):
        n = D.replica_bits_differ(g.t)
        assert n == 0, "%s %s %s: %d elements of the later replicas differ from the first period's" % (case, mode, what, n)


@pytest.mark.parametrize("mode", D.MODES)
def test_patch_128_cout_items_against_igemm(mode):
    """one 64-channel chunk and no bias: conv3x3_patch and conv_igemm sum in the same fp32 order, here on 128-cout items
    with the last one half masked"""
    case = "patch_bn128_32"
    assert D.LAUNCHES[case][0][:3] == ("patch", 32, 128) and D.LAUNCHES[case][0].chunks == 1
    x, w, b, go = D.base_inputs(case, mode)
    xr, wd = device_batch(x, case, mode), w.to(DEV)
    nan = resident(torch.full((xr.shape[0],) + tuple(go.shape[1:]), float("nan"), device=DEV), mode)
    out = []
    for flags, want in ((0, "patch"), (_lib.CONV_NHWC_IGEMM_ONLY, "igemm")):
        abi = ConvAbi(D.dims_of(case), mode, flags)
        assert abi.route(0) == want
        out.append(abi.forward(xr, wd, None, nan.clone()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0]).all())
    assert raw_equal(out[0], out[1]), "conv3x3_patch (128-cout items) and conv_igemm differ in a forward without bias"


def test_cases_split_as_the_docstring_says():
    lib = _lib.lib()
    f, d, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for case, want in SPLITS.items():
        for mode in D.MODES:
            assert lib.tdrn_conv2d_nhwc_splits(*D.dims_of(case), _lib.DTYPES[mode], 0, ctypes.byref(f), ctypes.byref(d), ctypes.byref(w)) == 0
            assert (f.value, d.value, w.value) == want, (case, mode, (f.value, d.value, w.value))
    assert set(SPLITS) == set(D.CASES) and all(s[:2] == (1, 1) for s in SPLITS.values())        # a direct route reports 1 slice
