"""Exact restatement of the fused gather kernel's arithmetic in its 16-bit modes (test helper; product code never imports it).

deform_gemm_kernel<bf16_t | f16_t> (csrc/deform.hip) is fully specified:

  sampling  csrc/deform_sampler.h, fp32: h_im = (float)(h_in + ti*dil) + off for the rejection test, h = (float)(ti*dil) + off for
            the floor, the height - 1 clamp with fraction 0, corner rows clamped into the map, the four weights hh*hw, hh*lw, lh*hw,
            lh*lw with hh = 1 - lh: one fp32 product each.  Followed here line by line in np.float32.
  blend     fmaf(w4, v4, fmaf(w3, v3, fmaf(w2, v2, w1 * v1))) in fp32 on the 16-bit corner values.  Emulated EXACTLY: a product of an
            fp32 and a 16-bit value is exact in float64; the sum with the fp32 addend is formed in float64 together with its rounding
            error (TwoSum), and where the float64 sum sits exactly half way between two fp32 values the sign of that error decides
            the fp32 rounding -- so the float64 detour never rounds differently from one fused multiply-add.
  rounding  once, nearest-even, to the 16-bit type (torch's cast; fp16 subnormals kept).
  product   exact products with fp32 accumulation on the matrix cores: ref = sum blend16 * w16 in float64, S = sum |blend16| |w16|;
            the accumulation noise is what the caller's C_ACC * S allows.

`extra`: the blend is also computed in plain float64; where that value lies within 2^-22 (relative) of the midpoint between two
adjacent 16-bit values the rounding is not trusted and ulp16(value) * |w16| is added to `extra` of every output that element feeds.
`near`: output pixels with a (tap, group) whose h_im or w_im lies within 1e-4 of 0 or of H (W) and is not an exact integer (the
rejection test is discontinuous there; an exact integer is unambiguous in fp32: with zero offsets nothing is near).

`mutate` applies ONE deliberate error to the restatement (tests/test_deform_gather_ref.py shows that each leaves the tolerance):
  "swap23"      corner weights 2 and 3 swapped
  "next_tap"    tap t blended with tap t+1's weights (the weights latched one step late)
  "prev_group"  group g's channels read from group g-1
  "drop_last"   the last tap dropped
  "trunc"       the blend rounded toward zero instead of to nearest
"""
import numpy as np
import torch

TORCH16 = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": (7, -126), "fp16": (10, -14)}       # stored mantissa bits, exponent of the smallest normal
MUTATIONS = ("swap23", "next_tap", "prev_group", "drop_last", "trunc")
F32 = np.float32


def _pr(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def round16(a, dtype):
    """fp64 / fp32 array -> nearest-even 16-bit value, as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TORCH16[dtype]).double().numpy()


def ulp16(a, dtype):
    """spacing of the 16-bit type at magnitude a (float64 array >= 0; the subnormal spacing below the smallest normal)"""
    mant, emin = MANT[dtype]
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return np.exp2(np.maximum(e, emin) - mant)


def _trunc16(v32, dtype):
    """fp32 array -> the 16-bit value toward zero, as float64 (the "trunc" mutation)"""
    if dtype == "bf16":
        return (np.ascontiguousarray(v32, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32).astype(np.float64)
    r = v32.astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(v32.astype(np.float64))
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float64)


def _fma32(w, v, a):
    """fp32(w * v + a) with ONE rounding: w fp32, v 16-bit, a fp32, all held in float64 (w * v is exact there)"""
    p = w * v
    s = p + a
    bb = s - p
    e = (p - (s - bb)) + (a - bb)                    # TwoSum: p + a == s + e exactly
    r = s.astype(F32)
    d = r.astype(np.float64) - s                     # (exact: r and s are neighbours)
    other = np.where(d > 0, np.nextafter(r, F32(-np.inf)), np.nextafter(r, F32(np.inf))).astype(F32)
    tie = (d != 0) & (np.abs(other.astype(np.float64) - s) == np.abs(d)) & (e != 0)
    if tie.any():
        hi, lo = np.maximum(r, other), np.minimum(r, other)
        r = np.where(tie, np.where(e > 0, hi, lo), r).astype(F32)
    return r.astype(np.float64)


def sample(H, W, h_in, w_in, ti_dil, tj_dil, dh, dw):
    """deform_sampler.h in np.float32 for arrays of output pixels: ok, the clamped corner rows / columns, the four fp32 weights
    (zero where the tap is rejected) and the rejection coordinates h_im, w_im."""
    dh, dw = dh.astype(F32), dw.astype(F32)
    h_im = (h_in + ti_dil).astype(F32) + dh
    w_im = (w_in + tj_dil).astype(F32) + dw
    ok = (h_im >= 0) & (w_im >= 0) & (h_im < F32(H)) & (w_im < F32(W))
    h = F32(ti_dil) + dh
    w = F32(tj_dil) + dw
    height, width = H - h_in, W - w_in
    h_low, w_low = np.floor(h).astype(np.int64), np.floor(w).astype(np.int64)
    ch, cw = h_low >= height - 1, w_low >= width - 1
    h_low, w_low = np.where(ch, height - 1, h_low), np.where(cw, width - 1, w_low)
    h_high, w_high = np.where(ch, h_low, h_low + 1), np.where(cw, w_low, w_low + 1)
    h = np.where(ch, h_low.astype(F32), h).astype(F32)
    w = np.where(cw, w_low.astype(F32), w).astype(F32)
    lh, lw = (h - h_low.astype(F32)).astype(F32), (w - w_low.astype(F32)).astype(F32)
    hh, hw = F32(1) - lh, F32(1) - lw
    wg = [np.where(ok, v, F32(0)).astype(F32) for v in (hh * hw, hh * lw, lh * hw, lh * lw)]
    r0, r1 = np.clip(h_in + h_low, 0, H - 1), np.clip(h_in + h_high, 0, H - 1)
    q0, q1 = np.clip(w_in + w_low, 0, W - 1), np.clip(w_in + w_high, 0, W - 1)
    return ok, (r0 * W + q0, r0 * W + q1, r1 * W + q0, r1 * W + q1), wg, h_im, w_im


def out_size(H, W, kh, kw, stride, padding, dilation):
    (sh, sw), (ph, pw), (dh, dw) = _pr(stride), _pr(padding), _pr(dilation)
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def gather_ref(x16, off, w16, stride, padding, dilation, G, dtype, second=None, round_blend=True, mutate=None):
    """x16 (N, Cin, H, W): the kernel's input values, 16-bit representable; off (N, G*2*kh*kw, Ho, Wo) fp32 (channel of group g, tap t:
    g*2*kh*kw + 2*t + {0, 1}); w16 (Cout, Cin, kh, kw) rounded weights; stride / padding / dilation: int or (h, w).
    second: dict(off=, w16=, stride=, padding=, dilation=, G=) of a second branch over the same x16 whose result is added.
    round_blend=False leaves the blend in float64 (no fp32 chain, no 16-bit rounding): the comparison with the CPU oracle.
    Returns ref, S, extra (N, Cout, Ho, Wo) float64 and near (N, Ho, Wo) bool."""
    assert mutate is None or mutate in MUTATIONS
    x16 = np.asarray(x16, dtype=np.float64)
    N, Cin, H, W = x16.shape
    xf = x16.reshape(N, Cin, H * W)
    branches = [dict(off=off, w16=w16, stride=stride, padding=padding, dilation=dilation, G=G)]
    if second is not None:
        branches.append(second)
    ref = S = extra = near = None
    for br in branches:
        wb = np.asarray(br["w16"], dtype=np.float64)
        ob = np.asarray(br["off"], dtype=F32)
        Cout, cw_, kh, kw = wb.shape
        Gb = br["G"]
        assert cw_ == Cin and Cin % Gb == 0
        (sh, sw), (ph, pw), (dlh, dlw) = _pr(br["stride"]), _pr(br["padding"]), _pr(br["dilation"])
        Ho, Wo = out_size(H, W, kh, kw, br["stride"], br["padding"], br["dilation"])
        taps, cpg, P = kh * kw, Cin // Gb, Ho * Wo
        assert ob.shape == (N, Gb * 2 * taps, Ho, Wo), (ob.shape, (N, Gb * 2 * taps, Ho, Wo))
        if ref is None:
            ref, S, extra = (np.zeros((N, Cout, P)) for _ in range(3))
            near = np.zeros((N, P), bool)
        assert ref.shape == (N, Cout, P)
        ho, wo = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
        h_in, w_in = ho.reshape(-1) * sh - ph, wo.reshape(-1) * sw - pw
        for n in range(N):
            for t in range(taps - 1 if mutate == "drop_last" else taps):
                ti, tj = divmod(t, kw)
                for g in range(Gb):
                    c0 = g * 2 * taps
                    ok, idx, wg, h_im, w_im = sample(H, W, h_in, w_in, ti * dlh, tj * dlw, ob[n, c0 + 2 * t].reshape(-1),
                                                     ob[n, c0 + 2 * t + 1].reshape(-1))
                    for c, lim in ((h_im, H), (w_im, W)):
                        c = c.astype(np.float64)
                        near[n] |= ((np.abs(c) < 1e-4) | (np.abs(c - lim) < 1e-4)) & (c != np.round(c))
                    if mutate == "next_tap":
                        t2 = (t + 1) % taps
                        wg = sample(H, W, h_in, w_in, (t2 // kw) * dlh, (t2 % kw) * dlw, ob[n, c0 + 2 * t2].reshape(-1),
                                    ob[n, c0 + 2 * t2 + 1].reshape(-1))[2]
                    if mutate == "swap23":
                        wg = [wg[0], wg[2], wg[1], wg[3]]
                    gs = (g - 1) % Gb if mutate == "prev_group" else g
                    xg = xf[n, gs * cpg:(gs + 1) * cpg]                                    # (cpg, H W)
                    v = [xg[:, q] for q in idx]                                            # four (cpg, P) corner values
                    w64 = [a.astype(np.float64)[None, :] for a in wg]
                    plain = w64[0] * v[0] + w64[1] * v[1] + w64[2] * v[2] + w64[3] * v[3]
                    if round_blend:
                        b32 = (w64[0] * v[0]).astype(F32).astype(np.float64)
                        for k in (1, 2, 3):
                            b32 = _fma32(w64[k], v[k], b32)
                        b16 = _trunc16(b32.astype(F32), dtype) if mutate == "trunc" else round16(b32, dtype)
                        a = np.abs(plain)
                        u = ulp16(a, dtype)
                        frac = a / u - np.floor(a / u)
                        amb = np.where(np.abs(frac - 0.5) * u <= 2.0 ** -22 * a, u, 0.0)
                        amb[a == 0] = 0.0
                    else:
                        b16, amb = plain, None
                    wt = wb[:, g * cpg:(g + 1) * cpg, ti, tj]                              # (Cout, cpg)
                    ref[n] += wt @ b16
                    S[n] += np.abs(wt) @ np.abs(b16)
                    if amb is not None and amb.any():
                        extra[n] += np.abs(wt) @ amb
    shape = (N, ref.shape[1], Ho, Wo)
    return ref.reshape(shape), S.reshape(shape), extra.reshape(shape), near.reshape(N, Ho, Wo)


# The stand-alone cases of tests/test_gpu_deform_gather16.py and tests/test_deform_gather_ref.py: the smallest that reach each code
# path of deform_gemm_kernel.  N, Cin, H, W, Cout, k, stride, pad, dil, G, offset sigma
CASES = [
    (2, 64, 9, 7, 12, 3, 1, 1, 1, 1, 0.0),         # M = 126: one ragged tile, NTL = 1, every border tap rejected exactly
    (2, 64, 8, 8, 12, 3, 1, 1, 1, 8, 1.0),         # M = 128 exactly; 8 groups of 8 channels, each padded to 64
    (1, 128, 12, 11, 75, 3, 1, 1, 1, 1, 1.0),      # M = 132: second tile holds 4 rows; NTL = 3; two K-steps per tap
    (1, 192, 13, 9, 33, 3, 2, 1, 1, 2, 1.0),       # stride 2; 96 channels per group padded to 128; NTL = 2 with ragged columns
    (1, 64, 12, 11, 128, 5, 1, 2, 1, 1, 2.0),      # 25 taps; NTL = 4 full
    (1, 8, 6, 6, 140, 1, 1, 0, 1, 1, 0.7),         # two column chunks (128 + 12); Cin padded 8 -> 64
    (3, 256, 5, 5, 75, 3, 1, 1, 1, 1, 3.0),        # smallest pyramid level; offsets leave the map on every side
    (1, 72, 14, 13, 9, (3, 5), (2, 1), (1, 2), (2, 1), 1, 1.5),     # every per-axis parameter different
]
CASE_IDS = ["x".join(str(v).replace(" ", "") for v in c) for c in CASES]
SEEDS = [11, 12, 13, 14, 15, 16, 17, 18]           # one per case (chosen so that `near` marks at most 10 % of the output pixels)


def case_inputs(case, seed):
    """fp32 x (standard normal), w (scaled by (Cin kh kw)^-0.5, as tests/test_gpu_ops.py does) and offsets (sigma) of a case"""
    N, Cin, H, W, Cout, k, st, pad, dil, G, sigma = case
    kh, kw = _pr(k)
    Ho, Wo = out_size(H, W, kh, kw, st, pad, dil)
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((N, Cin, H, W)).astype(F32)
    w = ((Cin * kh * kw) ** -0.5 * rng.standard_normal((Cout, Cin, kh, kw))).astype(F32)
    off = (sigma * rng.standard_normal((N, G * 2 * kh * kw, Ho, Wo))).astype(F32)
    return x, w, off
