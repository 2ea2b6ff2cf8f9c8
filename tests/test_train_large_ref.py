"""What test_gpu_train_large.py's construction relies on (tests/_train_large_cases.py), asserted without a GPU: the sizes, the
period condition, and the two conditions only the float64 reference can decide (the share of elements on the ReLU kink, the
smallest pixel norm)."""
import pytest

import _train_large_cases as L

ALL = list(L.BN_CASES) + list(L.POOL_CASES) + list(L.L2_CASES) + list(L.CONV_CASES)


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
    if case in L.CONV_CASES:
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
