"""What test_gpu_train_large.py's construction relies on (tests/_train_large_cases.py), asserted without a GPU: the sizes, the
period condition, and the conditions only the float64 reference can decide (the share of elements on the ReLU kink, the smallest
pixel norm, and for the conv families of sections i-f to i-i that a wrapped offset lands on a value that differs).  For those four
families the file also asserts, host only, that the API admits each shape and that every limit the header lists lies below 2^31."""
import pytest
import torch

import _train_large_cases as L
from tdrn_amd import _lib

NEW = [c for f in L.NEW_FAMILIES for c in L.FAMILIES[f][1]]
NEW_MODES = [(c, m) for f in L.NEW_FAMILIES for c in L.FAMILIES[f][1] for m in L.FAMILIES[f][2]]
C_ACC_BF16 = 2e-6                               # _conv_train_harness.C_ACC["bf16"]
ALL = list(L.BN_CASES) + list(L.POOL_CASES) + list(L.L2_CASES) + list(L.CONV_CASES) + NEW


@pytest.mark.parametrize("case", ALL)
def test_big_tensor_lies_between_2_30_and_2_31_elements(case):
    n = L.big_elements(case)
    assert 2 ** 30 < n < 2 ** 31, (case, n)
    assert 4 * n > 2 ** 32 and 2 * n > 2 ** 31            # fp32 past 4 GiB; the 16-bit staging past 2 GiB


@pytest.mark.parametrize("case", ALL)
def test_no_period_divides_a_wrap_distance(case):
    for period in L.periods(case):
        for k in (29, 30, 31):
            assert 2 ** k % period != 0, (case, period, k)
    if case in L.CONV_CASES or (case in NEW and case not in L.DW_CASES):
        assert len(L.periods(case)) >= 2                   # the NCHW tensors and the channel-padded NHWC staging


def test_conv_cases_are_the_big_output_and_the_big_input_gradient():
    Cin, H, W, Cout, k, pad, dil = L.CONV_CASES["conv_big_output"]
    assert L.R * Cout * H * W > 2 ** 30 and L.R * L.cpad(Cin) * H * W > 2 ** 30 > L.R * Cin * H * W
    Cin, H, W, Cout, k, pad, dil = L.CONV_CASES["conv_big_grad_input"]
    assert L.R * Cin * H * W > 2 ** 30 > L.R * Cout * H * W
    assert set(L.CONV_MODES) == {"fp32", "bf16"}


def test_batch_norm_cases_take_both_sweeps():
    assert (500 * 500) % 4 == 0 and (501 * 501) % 4 != 0      # the 16-byte sweep and the per-plane sweep
    assert [c[3] for c in L.BN_CASES.values()] == [1, 0]


def test_relu_kink_share_is_decided_by_the_reference_and_small():
    ref = L.bn_reference("bn_500_relu")
    print("bn_500_relu: %.4f %% of the elements lie on the ReLU kink" % (100 * ref["kink_share"]))
    assert 0 < ref["kink_share"] <= 0.01
    zeroed = float((ref["go"] == 0).double().mean())
    assert abs(zeroed - ref["kink_share"]) < 1e-6
    assert L.bn_reference("bn_501")["kink_share"] == 0.0


def test_l2norm_base_has_no_small_pixel_norm():
    smallest = float(L.l2_reference("l2_500")["norm"].min())
    print("smallest pixel norm of the base: %.4f" % smallest)
    assert smallest > 0.02


def test_pool_cases_cover_the_three_geometries_on_both_maps():
    geos = {(c[1], c[3]) for c in L.POOL_CASES.values()}
    assert geos == {(500, L.FLOOR), (501, L.FLOOR), (501, L.CEIL), (500, L.K3), (501, L.K3)}


# ---------------------------------------------------------------------------------------------
# sections i-f to i-i: conv_transpose2d, conv2d at stride 2, depthwise conv2d, conv5x5
# ---------------------------------------------------------------------------------------------
def test_the_new_families_keep_the_earlier_cases_inputs():
    # _gen numbers the first four families' names as it always did
    assert [L._gen(c).initial_seed() for c in ("bn_500_relu", "conv_big_output", "l2_500", "pool_501_k3")] == [101, 104, 105, 110]
    assert len({L._gen(c).initial_seed() for c in ALL}) == len(ALL)
    assert set(L.DW_MODES) == {"fp32"} and all(set(L.FAMILIES[f][2]) == {"fp32", "bf16"} for f in ("convt", "s2", "k5"))


@pytest.mark.parametrize("case,mode", NEW_MODES)
def test_the_api_admits_the_case(case, mode):
    prefix = L.FAMILIES[L.family(case)][0]
    query = getattr(_lib.lib(), prefix + "_workspace_bytes")
    nb = query(*L.op_dims(case), _lib.DTYPES[mode])
    print("%s %s: workspace %.2f GiB" % (case, mode, nb / 2.0 ** 30))
    assert nb > 0
    assert query(*L.op_dims(case, 2 * L.R), _lib.DTYPES[mode]) == 0            # twice the batch is past the limit: the case sits in its last octave


def test_every_limit_of_the_header_is_met_and_which_tensor_is_big():
    R, lo, hi = L.R, 2 ** 30, 2 ** 31
    assert R == 80
    # i-f: N*H*W*Cin_pad, N*H*W*4*Cout_pad and N*4*H*W*Cout below 2^31
    Cin, H, W, Cout = L.CONVT_CASES["convt_big_output"]
    assert (Cin, H, W, Cout) == (3, 250, 250, 64) and W % 2 == 0
    assert R * H * W * 64 == 320000000 < lo                                     # Cin_pad = 64: the x staging is small
    assert lo < R * H * W * 4 * 64 == R * 4 * H * W * Cout == 1280000000 < hi   # the s2d image and the output
    Cin, H, W, Cout = L.CONVT_CASES["convt_big_grad_input"]
    assert (Cin, H, W, Cout) == (256, 251, 251, 3) and W % 2 == 1
    assert lo < R * H * W * 256 == R * H * W * 4 * 64 == 1290260480 < hi        # x, grad_input, both stagings
    assert R * 4 * H * W * Cout == 60480960 < lo
    # i-g: N*H*W*Cin_pad, N*Ho*Wo*Cout_pad and N*(H + 2 pad - 2)*(W + 2 pad - 2)*Cout_pad below 2^31
    Cin, H, W, Cout, pad = L.S2_CASES["s2_big_grad_input"]
    assert (Cin, H, W, Cout, pad) == (64, 506, 506, 3, 0) and (H - 3) // 2 + 1 == 252 and 252 % 4 == 0
    assert lo < R * H * W * 64 == 1310904320 < hi                               # x, grad_input, the x staging
    assert lo < R * (H - 2) * (W - 2) * 64 == 1300561920 < hi                   # D
    assert R * 252 * 252 * 64 == 325140480 < lo
    assert L.untouched("s2_big_grad_input") == ([505], [505])
    Cin, H, W, Cout, pad = L.S2_CASES["s2_big_dilated"]
    assert (Cin, H, W, Cout, pad) == (3, 501, 501, 64, 1) and (H + 2 - 3) // 2 + 1 == 251 and H + 2 * pad - 2 == 2 * 251 - 1
    assert lo < R * H * W * 64 == R * (H + 2 * pad - 2) * (W + 2 * pad - 2) * 64 == 1285125120 < hi    # the x staging and D
    assert R * 251 * 251 * 64 == 322565120 < lo and R * H * W * Cin < lo        # no caller tensor is big: the stagings alone
    assert L.untouched("s2_big_dilated") == ([], [])
    # i-h: N*C*H*W below 2^31
    assert L.DW_CASES == {"dw_500_s1": (64, 500, 500, 1), "dw_501_s2": (64, 501, 501, 2)}
    assert lo < R * 64 * 500 * 500 == 1280000000 < hi and lo < R * 64 * 501 * 501 == 1285125120 < hi
    assert R * 64 * 251 * 251 < lo                                              # at stride 2 the output side is small
    # i-i: N*H*W*Cin_pad and N*H*W*Cout_pad below 2^31
    assert L.K5_CASES == {"k5_big_output": (3, 500, 500, 64), "k5_big_grad_input": (64, 500, 500, 3)}
    assert lo < R * 500 * 500 * 64 == 1280000000 < hi                           # both paddings are 64
    assert R * 3 * 500 * 500 < lo


def test_untouched_row_and_column_of_the_stride_2_input_gradient_are_zero_in_the_reference():
    for mode in L.CONV_MODES:
        gx = L.op_reference("s2_big_grad_input", mode)[0][1][0]                 # (Cin, H, W)
        rows, cols = gx.abs().amax((0, 2)), gx.abs().amax((0, 1))
        assert (rows == 0).nonzero().flatten().tolist() == [505] and (cols == 0).nonzero().flatten().tolist() == [505]
        assert bool((gx[:, 505, :] == 0).all()) and bool((gx[:, :, 505] == 0).all())


def _big_results(case):
    """(name, index in the reference) of the caller-visible results of more than 2^30 elements"""
    xs, _, ys, _ = L.op_shapes(case)
    numel = lambda shape: shape[1] * shape[2] * shape[3]
    return [(n, i) for n, i, shape in (("output", 0, ys), ("grad_input", 1, xs)) if L.R * numel(shape) > 2 ** 30]


def test_which_results_are_big():
    big = {case: [n for n, _ in _big_results(case)] for case in NEW}
    assert big == {"convt_big_output": ["output"], "convt_big_grad_input": ["grad_input"], "s2_big_grad_input": ["grad_input"],
                   "s2_big_dilated": [],                    # (its big tensors are stagings; the limits test states their sizes)
                   "dw_500_s1": ["output", "grad_input"], "dw_501_s2": ["grad_input"],
                   "k5_big_output": ["output"], "k5_big_grad_input": ["grad_input"]}


@pytest.mark.parametrize("case,mode", NEW_MODES)
def test_a_wrapped_offset_lands_on_a_value_that_differs(case, mode):
    """A condition on the inputs, not a measurement.  For each big result and each k in (29, 30, 31): 10^5 random flat offsets o of
    the replicated NCHW tensor, the reference at o's position in the base against the reference at (o - 2^k)'s.  o is drawn from
    [2^k, R * period) where the tensor has more than 2^k elements; it has fewer than 2^31, so for k = 31 o is drawn from the whole
    tensor and o - 2^31 is taken modulo the period, as if the replicas went on in front of the tensor.  At most 1 % of the pairs may
    agree within the GPU test's own bound (fp32: 1e-4 max(1, max|ref|); bf16: 2e-6 S at o).  In s2_big_grad_input the untouched row
    and column 505 are exactly 0 by construction, so pairs are drawn from touched positions only: a pair with either end in that row
    or column is drawn again."""
    ref, S = L.op_reference(case, mode)
    rows, cols = L.untouched(case)
    gen = torch.Generator().manual_seed(29)
    for name, i in _big_results(case):
        r, s = ref[i][0], S[i][0]
        C, H, W = r.shape
        period, total = C * H * W, L.R * C * H * W
        touched = torch.ones(H, W, dtype=torch.bool)
        if name == "grad_input":
            touched[rows, :] = False
            touched[:, cols] = False
        touched = touched.expand(C, H, W).reshape(-1)
        r, s = r.reshape(-1), s.reshape(-1)
        for k in (29, 30, 31):
            lo = 2 ** k if total > 2 ** k else 0
            o = lo + (torch.rand(400000, generator=gen, dtype=torch.float64) * (total - lo)).long().clamp_(max=total - lo - 1)
            p, q = o % period, (o - 2 ** k) % period
            keep = (touched[p] & touched[q]).nonzero().flatten()[:100000]
            assert keep.numel() == 100000
            p, q = p[keep], q[keep]
            d = (r[p] - r[q]).abs()
            bound = 1e-4 * max(1.0, float(r.abs().max())) if mode == "fp32" else C_ACC_BF16 * s[p]
            share = float((d <= bound).double().mean())
            print("%s %s %-10s wrap at 2^%d: %.5f %% of 100000 pairs agree within the bound" % (case, mode, name, k, 100 * share))
            assert share <= 0.01, (case, mode, name, k, share)
