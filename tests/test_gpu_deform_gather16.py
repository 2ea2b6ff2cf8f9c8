"""deform_gemm_kernel<bf16_t | f16_t> (csrc/deform.hip) pinned from its own inputs through the public op,
conv_offset2d(..., compute="bf16" | "fp16") / tdrn_deform_conv_forward.

The op rounds its fp32 input and weight once to the type, so the kernel's operands x16 = round16(x), w16 = round16(w) are known here;
offsets stay fp32; the output is fp32.  tests/_deform_gather_ref.py restates the kernel's arithmetic exactly (fp32 sampling decisions
and bilinear weights, the fp32 fma chain of the blend, one nearest-even rounding of the blend to the type, exact products), so every
output must satisfy

        |got - ref| <= C_ACC * S + extra,      S = sum |blend16| |w16|,   C_ACC = 2e-6 (bf16) / 4e-5 (fp16)

(tests/test_gpu_pin16.py: fp32 accumulation noise of the matrix cores; no output rounding: out16=False) on every output pixel that is
not `near` the discontinuity of the rejection test.  tests/test_deform_gather_ref.py shows on the CPU that the restatement agrees
with the oracle, that a swapped corner weight, a late weight latch, a wrong group base, a dropped tap and a truncating rounding
each leave this tolerance, and that `near` is empty on these seeds.

The cases (tests/_deform_gather_ref.py CASES) are the smallest that reach each path of the kernel: a ragged single tile, M = 128
exactly, a 4-row second tile, NTL = 1 ... 4, one and two K-steps per tap, group-padded channels (8 -> 64, 96 -> 128), 25 taps, two
column chunks, offsets that leave the map on every side, every per-axis parameter different.
"""
import numpy as np
import pytest
import torch

from tdrn_amd.model.networks import conv_offset2d

import _deform_gather_ref as R
import test_gpu_pin16 as pin

pytestmark = pytest.mark.gpu
DEV = pin.DEV


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_gather_kernel_from_its_own_inputs(i, dtype):
    N, Cin, H, W, Cout, k, st, pad, dil, G, sigma = R.CASES[i]
    x, w, off = R.case_inputs(R.CASES[i], R.SEEDS[i])
    ref, S, extra, near = R.gather_ref(R.round16(x, dtype), off, R.round16(w, dtype), st, pad, dil, G, dtype)
    got = conv_offset2d(*(torch.from_numpy(a).to(DEV) for a in (x, off, w)), st, pad, dil, G, compute=dtype).cpu().double()
    assert tuple(got.shape) == ref.shape
    keep = torch.from_numpy(~near)                                       # (N, Ho, Wo)
    sel = lambda a: torch.as_tensor(a).permute(0, 2, 3, 1)[keep]         # (kept pixels, Cout)
    report = []
    try:
        pin._assert_stage(R.CASE_IDS[i], sel(got), sel(ref), sel(S), dtype, out16=False, extra=sel(extra), report=report)
    finally:
        print("\n%s %s: worst error / tolerance %.3f (max |err| %.3g at max |ref| %.3g), near %d of %d pixels" % (
            R.CASE_IDS[i], dtype, report[0][1], report[0][2], report[0][3], int(near.sum()), near.size))
    assert near.sum() * 10 <= near.size
