"""Pins the deformable-conv gradient oracle (tests/_deform_grad_ref.py) on the CPU: its forward is the oracle's forward,
its weight gradient is grad_out . im2col^T, its three gradients match central finite differences away from the
measure-zero points, and hand-computed answers on a 4x4 map hold the border rules of the reference's backward
(deform_conv_cuda_kernel.cu:53-154)."""
import numpy as np
import pytest
import torch

import _deform_grad_ref as gref
from oracle import oracle as orc

# the shape classes of tests/test_gpu_ops.py DEFORM_CASES (copied, not imported)
DEFORM_CASES = [
    # N, Cin, H, W, Cout, k, stride, pad, dil, G, offset scale
    (2, 6, 9, 7, 4, 3, 1, 1, 1, 1, 0.0),
    (1, 6, 9, 7, 4, 3, 1, 1, 1, 1, 1.0),
    (2, 32, 10, 10, 12, 3, 1, 1, 1, 1, 1.5),
    (1, 64, 20, 20, 75, 3, 1, 1, 1, 1, 1.0),
    (1, 64, 12, 11, 63, 5, 1, 2, 1, 1, 2.0),
    (2, 64, 8, 8, 12, 3, 1, 1, 1, 8, 1.0),
    (1, 24, 13, 9, 10, 3, 2, 1, 1, 2, 1.0),
    (1, 16, 9, 9, 8, 3, 1, 2, 2, 1, 1.0),
    (1, 8, 6, 6, 140, 1, 1, 0, 1, 1, 0.7),
    (3, 256, 5, 5, 75, 3, 1, 1, 1, 1, 3.0),
    (2, 16, 11, 13, 9, (3, 5), 1, (1, 2), 1, 1, 1.0),
    (1, 32, 14, 9, 12, (1, 3), (2, 1), (0, 1), 1, 2, 1.5),
]


def _pr(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _rand(shape, seed, scale=1.0):
    return (scale * np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)).astype(np.float32)


def _case(case):
    N, Cin, H, W, Cout, k, st, pad, dil, G, osc = case
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pr(k), _pr(st), _pr(pad), _pr(dil)
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    x, w = _rand((N, Cin, H, W), 1), _rand((Cout, Cin, kh, kw), 2, (Cin * kh * kw) ** -0.5)
    off = _rand((N, G * 2 * kh * kw, Ho, Wo), 3, osc)
    return x, off, w, st, pad, dil, G, (N, Cout, Ho, Wo)


@pytest.mark.parametrize("case", DEFORM_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_oracle_forward_equals_reference_forward(case):
    x, off, w, st, pad, dil, G, _ = _case(case)
    ref = orc.deform_conv_forward(x, off, w, st, pad, dil, G)
    got = gref.deform_conv(torch.from_numpy(x).double(), torch.from_numpy(off).double(), torch.from_numpy(w).double(),
                           st, pad, dil, G).numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("case", [c for c in DEFORM_CASES if isinstance(c[5], int) and isinstance(c[6], int)
                                  and isinstance(c[7], int)], ids=lambda c: "x".join(str(v) for v in c))
def test_oracle_grad_weight_is_grad_out_times_columns(case):
    x, off, w, st, pad, dil, G, oshape = _case(case)
    N, Cout, Ho, Wo = oshape
    gout = _rand(oshape, 4)
    _, _, _, gw = gref.grads(x, off, w, gout, st, pad, dil, G)
    k = w.shape[2]
    ref = np.zeros((Cout, w.shape[1] * k * k), np.float64)
    for n in range(N):
        col = orc.deform_im2col(x[n], off[n], k, k, pad, st, dil, G).astype(np.float64)     # (Cin*k*k, Ho*Wo)
        ref += gout[n].reshape(Cout, -1).astype(np.float64) @ col.T
    np.testing.assert_allclose(gw.numpy().reshape(Cout, -1), ref, rtol=1e-5, atol=1e-5)


FD_CASES = [
    (1, 4, 6, 5, 3, 3, 1, 1, 1, 1),
    (1, 4, 7, 6, 2, 3, 2, 1, 1, 2),
    (2, 2, 5, 5, 2, (3, 2), 1, (1, 0), (1, 2), 1),
]


@pytest.mark.parametrize("case", FD_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_oracle_gradients_match_finite_differences(case):
    N, Cin, H, W, Cout, k, st, pad, dil, G = case
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pr(k), _pr(st), _pr(pad), _pr(dil)
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    rng = np.random.Generator(np.random.PCG64(11))
    x = torch.from_numpy(rng.standard_normal((N, Cin, H, W)))
    w = torch.from_numpy(rng.standard_normal((Cout, Cin, kh, kw)))
    # offsets with fractional parts in [0.1, 0.9]: every sample coordinate stays >= 1e-3 from an integer, hence from the
    # borders 0, H-1, H (W-1, W) as well; whole parts -1..1 reach the rejected region and the clamp band
    off = torch.from_numpy(rng.integers(-1, 2, (N, G * 2 * kh * kw, Ho, Wo)) + rng.uniform(0.1, 0.9, (N, G * 2 * kh * kw, Ho, Wo)))
    _, hs, ws = gref.deform_conv(x, off, w, st, pad, dil, G, with_coords=True)
    frac = lambda c: (c.double() - torch.round(c.double())).abs()
    assert float(torch.minimum(frac(hs), frac(ws)).min()) > 1e-3
    gout = torch.from_numpy(rng.standard_normal((N, Cout, Ho, Wo)))
    _, gx, go, gw = gref.grads(x, off, w, gout, st, pad, dil, G)
    loss = lambda xx, oo, ww: float((gref.deform_conv(xx, oo, ww, st, pad, dil, G) * gout).sum())
    eps = 1e-6
    for name, t, g in (("input", x, gx), ("offset", off, go), ("weight", w, gw)):
        flat = t.reshape(-1)
        for i in np.random.Generator(np.random.PCG64(5)).choice(flat.numel(), min(40, flat.numel()), replace=False):
            args = [x.clone(), off.clone(), w.clone()]
            idx = {"input": 0, "offset": 1, "weight": 2}[name]
            a = args[idx].reshape(-1)
            a[i] += eps
            lp = loss(*args)
            a[i] -= 2 * eps
            lm = loss(*args)
            fd = (lp - lm) / (2 * eps)
            assert abs(fd - float(g.reshape(-1)[i])) <= 1e-6 * max(1.0, abs(fd)), (name, int(i), fd, float(g.reshape(-1)[i]))


def _probe(h, wq, dh, dw):
    """one 1x1 tap on a 4x4 map of x = 1..16, weight 1, grad_out = 1 at (h, wq) only"""
    H = W = 4
    x = np.arange(16, dtype=np.float32).reshape(1, 1, H, W) + 1.0
    w = np.ones((1, 1, 1, 1), np.float32)
    off = np.zeros((1, 2, H, W), np.float32)
    off[0, 0, h, wq], off[0, 1, h, wq] = dh, dw
    gout = np.zeros((1, 1, H, W), np.float32)
    gout[0, 0, h, wq] = 1.0
    _, gx, go, gw = gref.grads(x, off, w, gout)
    return gx.numpy()[0, 0], go.numpy()[0, :, h, wq], float(gw.numpy().ravel()[0])


@pytest.mark.parametrize("h,wq,dh,dw", [(0, 0, -0.25, 0.0), (0, 0, 0.0, -0.5), (3, 1, 1.0, 0.0), (1, 3, 0.0, 1.25)])
def test_known_answer_rejected_coordinates_have_zero_gradients(h, wq, dh, dw):
    gx, go, gw = _probe(h, wq, dh, dw)
    assert not gx.any() and not go.any() and gw == 0.0


def test_known_answer_clamp_band():
    # h = 3.75 in [H-1, H): all of the weight on row 3, zero offset gradient along h; w = 1.5 splits between columns 1, 2
    gx, go, gw = _probe(3, 1, 0.75, 0.5)
    want = np.zeros((4, 4))
    want[3, 1] = want[3, 2] = 0.5
    np.testing.assert_allclose(gx, want, atol=1e-12)
    assert go[0] == 0.0
    np.testing.assert_allclose(go[1], 1.0, atol=1e-12)           # v(3,2) - v(3,1)
    np.testing.assert_allclose(gw, 14.5, atol=1e-12)             # the sample itself: 0.5 * v(3,1) + 0.5 * v(3,2)
    # and the same along w: w = 3.5 -> column 3, zero offset gradient along w
    gx, go, _ = _probe(1, 3, 0.5, 0.5)
    want = np.zeros((4, 4))
    want[1, 3] = want[2, 3] = 0.5
    np.testing.assert_allclose(gx, want, atol=1e-12)
    assert go[1] == 0.0
    np.testing.assert_allclose(go[0], 4.0, atol=1e-12)           # v(2,3) - v(1,3)


def test_known_answer_exact_integer_is_one_sided():
    # h = 1 + 1.0 = 2 exactly: lh = 0, all of the weight on row 2, d/dh = v(3,1) - v(2,1) = 4; w = 1.5 at (1,1): 0.5 / 0.5
    gx, go, _ = _probe(1, 1, 1.0, 0.5)
    want = np.zeros((4, 4))
    want[2, 1] = want[2, 2] = 0.5
    np.testing.assert_allclose(gx, want, atol=1e-12)
    np.testing.assert_allclose(go, [4.0, 1.0], atol=1e-12)
    # exact integer along w: w = 2 at (2,1): d/dw = v(2,3) - v(2,2) = 1
    gx, go, _ = _probe(2, 1, 0.0, 1.0)
    want = np.zeros((4, 4))
    want[2, 2] = 1.0
    np.testing.assert_allclose(gx, want, atol=1e-12)
    np.testing.assert_allclose(go, [4.0, 1.0], atol=1e-12)


def test_backward_fuzz_shapes_reach_the_kernels_branches():
    """The shapes of test_gpu_train_fuzz.test_deform_backward_fuzz_matches_oracle: every channels-per-group and Cout value,
    every offset scale, pixel counts M below the 128 of one weight split and above it with a ragged last 32-pixel step."""
    S = [gref.fuzz_shape(seed) for seed in gref.FUZZ_SEEDS]
    assert {s["cpg"] for s in S} == set(gref.FUZZ_CPG) and {s["Cout"] for s in S} == set(gref.FUZZ_COUT)
    assert {s["osc"] for s in S} == set(gref.FUZZ_OFFSET_SCALE) and {s["G"] for s in S} == {1, 2, 4, 8}
    assert all(s["Cin"] == s["G"] * s["cpg"] <= 520 and s["Ho"] >= 1 and s["Wo"] >= 1 for s in S)
    assert sum(s["M"] < 128 for s in S) >= 4 and sum(s["M"] > 128 and s["M"] % 32 != 0 for s in S) >= 4
    assert any(s["M"] % 16 != 0 for s in S)                          # a ragged last pixel tile of the data kernel
    assert any(s["cpg"] > 64 and s["G"] > 1 for s in S)              # several groups of more than one chunk each
    assert max(s["N"] * s["Cin"] * s["k"][0] * s["k"][1] * s["Ho"] * s["Wo"] for s in S) <= 4_000_000    # the oracle's column tensor
