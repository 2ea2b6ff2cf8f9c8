"""Draws, float64 references, derived bounds and fp32 restatements for the tests that pin BatchNorm's training statistics, L2Norm, the
depthwise conv and SGD over the whole number range (test_number_range_stats_ref.py, test_gpu_number_range_stats.py,
test_gpu_number_range_pointwise.py).  A sibling of _number_range.py, whose value sets and comparators it builds on.  CPU only: nothing
here touches the library.

Every bound is bit equality, a rounding bound derived from the op's formula and its term count, cast_interval around such a bound, or
same_class.  None has an absolute floor; the only absolute terms are multiples of 2^-149, the spacing of fp32's subnormals, one per
rounding that can leave the normal range.  u = 2^-24 throughout; 1.001 covers the second-order terms of a first-order rounding bound
(the places where a second-order term is not small are written out).
"""
import functools
import math

import numpy as np
import torch

from _number_range import F32_MIN_SUB, acc_bound, f32_edges

U32 = 2.0 ** -24
ONE = 1.001


# =====================================================================================================================================
# BatchNorm in training mode
# =====================================================================================================================================
BN_SHAPES = {"tiny_odd": (2, 5, 7, 9), "m2": (2, 3, 1, 1), "offset_mean": (3, 4, 33, 31), "multi_split": (4, 3, 40, 40)}
KAPPAS = (0.0, 120.0, 2.0 ** 12, 2.0 ** 20)
EXPS = (-100, -60, -30, 0, 30, 55)
BN_WEIGHTS = (2.0 ** -20, 1.0, 2.0 ** 20)
BN_EPS = (1e-5, 1e-30)
BN_DRAWS = (0, 1)                        # the 15 channels of the four shapes, twice: all 24 (kappa, k) pairs are met
BN_MOMENTUM = 0.1
COMBOS = [(ka, k) for k in EXPS for ka in KAPPAS]
BN_CHUNK, BN_THREADS, BN_MIN_SPLIT, BN_GROUPS = 16, 256, 4096, 2048     # batch_norm.hip: kLoads quads, kT, kMinSplit, kGroups


def bn_splits(N, C, HW):
    """batch_norm_splits restated -> (splits, per_split)"""
    M = N * HW
    S = max(1, min(BN_GROUPS // max(C, 1), (M + BN_MIN_SPLIT - 1) // BN_MIN_SPLIT))
    per = ((M + S - 1) // S + 3) // 4 * 4
    return (M + per - 1) // per, per


def bn_channel_plan(case, draw):
    """per channel of the case: (kappa, k, weight) -- channel g of the 15 (30 with the second draw) takes pair g mod 24"""
    first = sum(BN_SHAPES[c][1] for c in list(BN_SHAPES)[:list(BN_SHAPES).index(case)]) + 15 * draw
    C = BN_SHAPES[case][1]
    return [COMBOS[(first + c) % len(COMBOS)] + (BN_WEIGHTS[(first + c + draw) % 3],) for c in range(C)]


@functools.lru_cache(maxsize=None)
def bn_inputs(case, draw):
    """x, weight, bias, grad_output, running_mean, running_var (CPU, fp32).  A channel is (mean + randn) 2^k with mean = +-kappa.
    The bias of a channel is 0.2 randn |weight|, but +-6 |weight| where kappa = 2^20: there the mean is 2^20 sigma and fp32 holds it
    to sigma / 16 per rounding at best, so elements would sit on the ReLU kink by the dozen; with that bias none does (the channel is
    then all positive or all clipped), and the ReLU is exercised by the other channels."""
    N, C, H, W = BN_SHAPES[case]
    gen = torch.Generator().manual_seed(2500 + 10 * list(BN_SHAPES).index(case) + draw)
    plan = bn_channel_plan(case, draw)
    x = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    w, b = torch.empty(C), torch.empty(C)
    r = torch.randn(C, generator=gen)
    for c, (ka, k, wt) in enumerate(plan):
        sign = 1.0 if c % 2 == 0 else -1.0
        x[:, c] = ((sign * ka + x[:, c]).float().double()) * 2.0 ** k
        w[c] = wt * sign
        b[c] = (6.0 * sign if ka == 2.0 ** 20 else 0.2 * float(r[c])) * wt
    x = x.float()
    go = torch.randn(N, C, H, W, generator=gen)
    rm = 0.5 * torch.randn(C, generator=gen)
    rv = 0.5 + torch.rand(C, generator=gen)
    return x, w, b, go, rm, rv


def bn_depth(N, HW, splits, per):
    """-> (L, K): an upper count L of the fp32 roundings of a record's mean on its way through the merges of bn_stats_kernel, and the
    chunk length K.  A thread folds at most ceil(q / 256) quad chunks per plane part of q quads (one flat part when H W is a multiple
    of 4) and one single element per part; then 6 shuffle steps, 3 wave merges, and the final cast of the float64 finalize.  A merge
    with an empty record is exact, so the count of non-empty lanes caps the tree's depth."""
    if HW % 4 == 0:
        parts, quads = 1, per // 4
    else:
        parts, quads = min(N, (per + HW - 1) // HW + 1), min(per, HW) // 4
    chain = parts * ((quads + BN_THREADS - 1) // BN_THREADS + (1 if HW % 4 else 0))
    lanes = max(1, min(BN_THREADS, max(quads, 3 if HW % 4 else 1)))
    tree = math.ceil(math.log2(min(64, lanes))) if lanes > 1 else 0
    waves = (lanes + 63) // 64 - 1
    return max(chain - 1, 0) + tree + waves + 1, BN_CHUNK


def bn_depth_nhwc(M, splits, per):
    """the same count for bn_nhwc_stats_kernel: a thread's rows lo + (t >> 3) + 32 j in chunks of 4 rows or single rows, 3 shuffle
    steps, 3 wave merges, the finalize's cast"""
    rows = (per + 31) // 32
    lanes = min(32, per)
    return max(rows - 1, 0) + (math.ceil(math.log2(min(8, lanes))) if lanes > 1 else 0) + ((lanes + 7) // 8 - 1) + 1, 4


def bn_stat_bounds(x64, L, K):
    """x64 (N, C, H, W) float64 -> per channel: mean, M2, e_mean (the bound of save_mean) and (m2_lo, m2_hi).

    Scheme (bn_prims.h): a chunk of K values is differenced against its first value v0; mu = sum (v_i - v0) / K; the chunk's mean is
    fl(v0 + mu) and its M2 is sum ((v_i - v0) - mu)^2 by fmaf; records merge by Chan's formula, mean = a.mean + d w with
    d = b.mean - a.mean; the splits merge in float64.  With A = max|x| and D = max|x - mean| of the channel (differences inside a chunk
    are at most 2 D):
      a chunk's mean:  u A (the one rounding at the size of the values) + (2 K + 2) u D (K - 1 differences and K - 1 adds of partial
                       sums up to 2 (K - 1) D, the product with 1 / K);
      a merge:         the merged error is a weighted mean of the two records' errors, plus u A for fl(a.mean + d w) and 6 u D for
                       d, w and d w;
      so e_mean = (L + 1) u A + (2 K + 2 + 6 L) u D -- the c1 u max|x| of the issue with c1 = L + 1 + (2 K + 2 + 6 L) D / A.
      M2 inside the chunks: each d_i carries at most 6 u D, the centre's own error enters in second order only (sum d_i = 0 about the
                       true centre), the K fmaf roundings K u; summed over the chunks with Cauchy-Schwarz: 12 u (D / sigma) + K u.
      M2 across merges: the rounding of a record's mean moves, exactly, every value under that record by one common amount and leaves
                       their M2 alone, so the computed M2 is the exact M2 of the values x_i + s_i with |s_i| <= e_mean (the roundings
                       on the value's path): M2 + 2 sum (x_i - mean) s_i + sum (s_i - mean(s))^2, a change of at most
                       2 e_mean sqrt(M M2) + M e_mean^2: relative 2 eps + eps^2 with eps = e_mean / sigma -- written out in full,
                       not to first order, because eps is not small at kappa = 2^20 (there fp32 holds the mean to sigma / 16 per
                       rounding, and for L + 1 > 6 roundings the lower end of M2 is 0: the bound then says nothing about
                       save_invstd, and so nothing about the output, of that channel).  The merge terms' own roundings: 6 u per
                       term, 2 L u for the adds.
      That is relative c2 u (1 + kappa): eps is linear in A / sigma <= (D / sigma) (1 + kappa), never quadratic.
      Products below the normal range lose at most 2^-150 each, weighted by a count of at most M in a merge: 4 M 2^-149 in all."""
    M = x64.numel() // x64.shape[1]
    dims = (0, 2, 3)
    mean = x64.mean(dims)
    dev = x64 - mean.view(1, -1, 1, 1)
    m2 = (dev * dev).sum(dims)
    A, D = x64.abs().amax(dims), dev.abs().amax(dims)
    sigma = (m2 / M).sqrt()
    e_mean = ONE * ((L + 1) * U32 * A + (2 * K + 2 + 6 * L) * U32 * D) + (L + K) * F32_MIN_SUB
    eps = e_mean / sigma
    rel = ONE * (12 * (D / sigma) + K + 2 * L + 6) * U32 + 2 * eps + eps * eps
    d = rel * m2 + 4 * M * F32_MIN_SUB
    return mean, m2, e_mean, ((m2 - d).clamp_min(0.0), m2 + d)


@functools.lru_cache(maxsize=None)
def bn_reference(case, draw, eps, relu):
    """the reference of a drawn case; computed once, never changed"""
    return bn_reference_of(bn_inputs(case, draw), eps, relu)


def bn_reference_of(inputs, eps, relu, depth=None):
    """float64 on the fp32 inputs -> dict name -> (reference, lo, hi), the grad_output both sides use ("go") and the kink share.
    eps is the fp32 value the entry receives.  depth: (L, K) of another kernel (the resident one).

    ReLU kink: an element whose float64 z lies within its own output bound of 0 gets grad_output = 0 on both sides.  The share is
    counted over the channels with |mean| < 2^19 sigma.  In a channel of kappa = 2^20 the a-priori bound of z is larger than |z| for
    every element (see bn_stat_bounds), so by the rule the whole channel's grad_output is 0: its gradients are then checked to be
    exactly the zeros and the sums the other terms give."""
    x, w, b, go, rm, rv = (t.double() for t in inputs)
    N, C, H, W = x.shape
    M = N * H * W
    S, per = bn_splits(N, C, H * W)
    L, K = depth if depth is not None else bn_depth(N, H * W, S, per)
    eps = float(np.float32(eps))
    mo = float(np.float32(BN_MOMENTUM))
    sh = (1, -1, 1, 1)
    mean, m2, e_mean, (m2_lo, m2_hi) = bn_stat_bounds(x, L, K)
    out = {}
    out["save_mean"] = (mean, mean - e_mean, mean + e_mean)
    inv = lambda q: (q / M + eps).rsqrt()
    invstd = inv(m2)
    out["save_invstd"] = (invstd, inv(m2_hi) * (1 - ONE * U32), inv(m2_lo) * (1 + ONE * U32))
    rmn = (1 - mo) * rm + mo * mean
    e = mo * e_mean + ONE * U32 * rmn.abs() + F32_MIN_SUB
    out["running_mean"] = (rmn, rmn - e, rmn + e)
    rvn = lambda q: (1 - mo) * rv + mo * q / (M - 1)
    out["running_var"] = (rvn(m2), rvn(m2_lo) * (1 - ONE * U32), rvn(m2_hi) * (1 + ONE * U32))
    # the relative error of invstd, both sides
    rho = torch.maximum(out["save_invstd"][2] / invstd - 1, 1 - out["save_invstd"][1] / invstd)
    a = (w * invstd)
    dev = x - mean.view(sh)
    za = dev.abs() * a.abs().view(sh)
    z = dev * a.view(sh) + b.view(sh)
    # z = fmaf(fl(x - mean), fl(w invstd), beta): three roundings, then the statistics' own errors
    bz = (ONE * U32 * (2 * za + z.abs()) + F32_MIN_SUB + (a.abs() * e_mean * (1 + rho)).view(sh) + za * rho.view(sh))
    y = z.clamp_min(0) if relu else z
    out["output"] = (y, y - bz, y + bz)
    go_used = go.clone()
    share = 0.0
    if relu:
        near = z.abs() <= bz
        counted = mean.abs() < 2.0 ** 19 * (m2 / M).sqrt()
        share = float(near[:, counted].double().mean()) if bool(counted.any()) else 0.0
        go_used[near] = 0.0
    dy = go_used * (z > 0) if relu else go_used
    xhat = dev * invstd.view(sh)
    ex = 2 * ONE * U32 * xhat.abs() + (invstd * e_mean * (1 + rho)).view(sh) + xhat.abs() * rho.view(sh)      # the error of xhat
    s1, s2 = dy.sum((0, 2, 3)), (dy * xhat).sum((0, 2, 3))
    a1, a2 = dy.abs().sum((0, 2, 3)), (dy * xhat).abs().sum((0, 2, 3))
    e1 = acc_bound("fp32", a1, M)
    e2 = acc_bound("fp32", a2, M + 2) + (dy.abs() * ex).sum((0, 2, 3))
    out["grad_bias"] = (s1, s1 - e1, s1 + e1)
    out["grad_weight"] = (s2, s2 - e2, s2 + e2)
    k1, k2 = s1 / M, s2 / M
    ek1, ek2 = e1 / M + ONE * U32 * k1.abs(), e2 / M + ONE * U32 * k2.abs()
    gx = a.view(sh) * (dy - (k1.view(sh) + xhat * k2.view(sh)))
    mag = dy.abs() + k1.abs().view(sh) + xhat.abs() * k2.abs().view(sh)
    # a (dy - fmaf(xhat, k2, k1)): five roundings on the magnitudes, the relative error of a, then the errors of k1, k2 and xhat
    egx = a.abs().view(sh) * ((5 * ONE * U32 + (rho + 2 * U32).view(sh)) * mag + ek1.view(sh) + xhat.abs() * ek2.view(sh)
                              + (k2.abs() + ek2).view(sh) * ex) + F32_MIN_SUB
    out["grad_input"] = (gx, gx - egx, gx + egx)
    out["go"] = go_used.float()
    out["kink_share"] = share
    out["plan"] = (L, K, S)
    return out


def share_of_interval(what, got, ref, lo, hi):
    """print the worst share of the one-sided bounds, then assert lo <= got <= hi elementwise (an infinite end admits anything finite
    on its side; non-finite values never pass) -> the share"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % what
    d = got - ref
    room = torch.where(d >= 0, hi - ref, ref - lo)
    share = torch.where(d == 0, torch.zeros_like(d), d.abs() / room)
    worst = float(share.max())
    print("%s: max|d| %.3e  worst share of the bound %.3e" % (what, float(d.abs().max()), worst))
    ok = (got >= lo) & (got <= hi)
    assert bool(ok.all()), (what, worst, int((~ok).sum()))
    return worst


# ---- the resident 16-bit NHWC BatchNorm: every finite pattern of the type over the channels of one case ---------------------------------
NHWC_SHAPES = {"wide": (3, 1024, 10, 10), "m2": (1, 64, 1, 2)}      # test_gpu_nhwc_batch_norm.py's smallest case with two splits, and its smallest
NHWC_GROUPS, NHWC_MIN_ROWS = 2048, 256


def nhwc_splits(N, C, HW):
    """batch_norm_nhwc_splits restated (tdrn_hip.h section i-k) -> (splits, per_split)"""
    M = N * HW
    S = max(1, min(NHWC_GROUPS // (C // 64), (M + NHWC_MIN_ROWS - 1) // NHWC_MIN_ROWS))
    per = ((M + S - 1) // S + 31) // 32 * 32
    return (M + per - 1) // per, per


@functools.lru_cache(maxsize=None)
def nhwc_inputs(case, T):
    """x, weight, bias, grad_output, running_mean, running_var (CPU, fp32; x and grad_output exact in T).
    wide: the finite non-negative patterns of T in order are cut into 1024 blocks; channel c holds every pattern of block c once with
    each sign (so all finite patterns of the type, +-0 and the subnormals among them, are met), and its other rows repeat patterns of
    the block with a sign that is + three times in four (a mean away from 0).  Every eighth channel fills those rows from the whole
    range of the type instead: in fp16 values near 65504 beside subnormals in one channel.
    m2: two random finite patterns per channel."""
    from _number_range import decode64, inf_bits
    N, C, H, W = NHWC_SHAPES[case]
    M = N * H * W
    gen = torch.Generator().manual_seed(2800 + list(NHWC_SHAPES).index(case) + (7 if T == "fp16" else 0))
    top = inf_bits(T)                                      # the finite non-negative patterns are 0 .. top - 1
    if case == "m2":
        pat = torch.randint(0, top, (M, C), generator=gen)
        sign = torch.randint(0, 2, (M, C), generator=gen)
    else:
        edge = (torch.arange(C + 1) * top) // C
        pat, sign = torch.empty(M, C, dtype=torch.int64), torch.empty(M, C, dtype=torch.int64)
        for c in range(C):
            block = torch.arange(int(edge[c]), int(edge[c + 1]))
            n = block.numel()
            assert 2 * n <= M
            src = torch.arange(top) if c % 8 == 7 else block
            rest = src[torch.randint(0, src.numel(), (M - 2 * n,), generator=gen)]
            col = torch.cat([block, block, rest])
            sg = torch.cat([torch.zeros(n, dtype=torch.int64), torch.ones(n, dtype=torch.int64),
                            (torch.randint(0, 4, (M - 2 * n,), generator=gen) == 0).to(torch.int64)])
            order = torch.randperm(M, generator=gen)
            pat[:, c], sign[:, c] = col[order], sg[order]
    bits = pat | (sign << (15))
    x = decode64(T, bits).float().view(N, H, W, C).permute(0, 3, 1, 2).contiguous()
    c = torch.arange(C)
    w = torch.tensor(BN_WEIGHTS)[c % 3] * torch.where((c // 3) % 2 == 0, 1.0, -1.0)
    b = 0.2 * torch.randn(C, generator=gen) * w.abs()
    go = torch.randn(N, C, H, W, generator=gen).to({"bf16": torch.bfloat16, "fp16": torch.float16}[T]).float()
    rm = 0.5 * torch.randn(C, generator=gen)
    rv = 0.5 + torch.rand(C, generator=gen)
    return x, w.float(), b.float(), go, rm, rv


def bn_range_classes(x64):
    """per channel -> (inside, past): inside = M (max - min)^2 < 2^128 (the header's range); past = the true M2 is 2^129 or more, so
    the fp32 M2 is certainly +inf; unspecified = max|x| >= 2^123, where the differences themselves can overflow"""
    M = x64.numel() // x64.shape[1]
    dims = (0, 2, 3)
    rng = x64.amax(dims) - x64.amin(dims)
    dev = x64 - x64.mean(dims).view(1, -1, 1, 1)
    m2 = (dev * dev).sum(dims)
    wild = x64.abs().amax(dims) >= 2.0 ** 123
    return (M * rng * rng < 2.0 ** 128) & ~wild, (m2 >= 2.0 ** 129) & ~wild, wild


@functools.lru_cache(maxsize=None)
def nhwc_reference(case, T, eps, relu):
    """-> (bn_reference_of's dict at the resident kernel's depth, bn_range_classes, splits); computed once, never changed"""
    x = nhwc_inputs(case, T)[0]
    N, C, H, W = x.shape
    splits, per = nhwc_splits(N, C, H * W)
    ref = bn_reference_of(nhwc_inputs(case, T), eps, relu, depth=bn_depth_nhwc(N * H * W, splits, per))
    return ref, bn_range_classes(x.double()), splits


# ---- fp32 restatements of the statistics, numpy --------------------------------------------------------------------------------------
def _f(v):
    return np.asarray(v, dtype=np.float32)


def welford_merge32(a, b, fixed=True):
    """welford_merge on arrays of records (n, mean, m2), every operation rounded to fp32.  fixed: a merge with an empty record
    returns the other record (bn_prims.h)."""
    with np.errstate(all="ignore"):
        n = a[0] + b[0]
        w = np.where(n > 0, b[0] / np.where(n > 0, n, _f(1)), _f(0)).astype(np.float32)
        d = b[1] - a[1]
        mean = a[1] + d * w
        m2 = a[2] + b[2] + d * d * a[0] * w
    if fixed:
        ea, eb = a[0] == 0, b[0] == 0
        mean = np.where(ea, b[1], np.where(eb, a[1], mean))
        m2 = np.where(ea, b[2], np.where(eb, a[2], m2))
    return n.astype(np.float32), mean.astype(np.float32), m2.astype(np.float32)


def welford_chunks32(v):
    """welford_chunk on rows of K fp32 values -> records; the fmaf as one float64 product (exact) and one float64 add"""
    K = v.shape[1]
    with np.errstate(all="ignore"):
        s = np.zeros(v.shape[0], np.float32)
        for i in range(1, K):
            s = s + (v[:, i] - v[:, 0])
        mu = s * np.float32(1.0 / K)
        m2 = np.zeros(v.shape[0], np.float32)
        for i in range(K):
            d = (v[:, i] - v[:, 0]) - mu
            m2 = (d.astype(np.float64) * d.astype(np.float64) + m2.astype(np.float64)).astype(np.float32)
        return np.full(v.shape[0], K, np.float32), v[:, 0] + mu, m2


def welford_channel32(v, chunk=BN_CHUNK, lanes=BN_THREADS, fixed=True, wave=64):
    """one channel's values in linear order -> (mean, m2) in fp32: chunks of `chunk` values (then quads, then single values) dealt to
    `lanes` lanes in turn and folded in order into a record that starts empty, the lanes of each `wave` merged by the shuffle tree,
    the waves in order -- the kernel's chunk length in a fixed merge order (the resident kernel: chunk 4, 32 row-lanes, 8 per wave)"""
    v = _f(v).reshape(-1)
    recs = []
    at = 0
    for K in (chunk, 4, 1):
        if K > chunk:
            continue
        n = (len(v) - at) // K
        if n:
            recs.append(welford_chunks32(v[at:at + n * K].reshape(n, K)) if K > 1 else
                        (np.ones(n, np.float32), v[at:at + n].copy(), np.zeros(n, np.float32)))
            at += n * K
    rec = tuple(np.concatenate([r[i] for r in recs]) for i in range(3))
    cnt = len(rec[0])
    rounds = (cnt + lanes - 1) // lanes
    pad = rounds * lanes - cnt
    rec = tuple(np.concatenate([r, np.zeros(pad, np.float32)]).reshape(rounds, lanes) for r in rec)
    w = tuple(np.zeros(lanes, np.float32) for _ in range(3))
    for j in range(rounds):
        w = welford_merge32(w, tuple(r[j] for r in rec), fixed)
    w = tuple(r.reshape(-1, wave) for r in w)
    o = wave // 2
    while o:
        b = tuple(np.concatenate([r[:, o:], np.zeros((r.shape[0], o), np.float32)], 1) for r in w)      # shfl_down by o
        w = welford_merge32(w, b, fixed)
        o //= 2
    a = tuple(r[0, 0:1] for r in w)
    for i in range(1, w[0].shape[0]):
        a = welford_merge32(a, tuple(r[i, 0:1] for r in w), fixed)
    return float(a[1][0]), float(a[2][0])


def sums_channel32(v, lanes=BN_THREADS):
    """the doctored scheme: per-lane fp32 sums of x and x^2 in order, lanes added in order, M2 = sum x^2 - (sum x)^2 / M"""
    v = _f(v).reshape(-1)
    pad = (-len(v)) % lanes
    t = np.concatenate([v, np.zeros(pad, np.float32)]).reshape(-1, lanes)
    with np.errstate(all="ignore"):
        s, q = np.zeros(lanes, np.float32), np.zeros(lanes, np.float32)
        for row in t:
            s, q = s + row, q + row * row
        s1, s2 = np.float32(0), np.float32(0)
        for i in range(lanes):
            s1, s2 = s1 + s[i], s2 + q[i]
        n = np.float32(len(v))
        mean = s1 / n
        return float(mean), float(s2 - mean * mean * n)


def two_pass_channel32(v):
    """a different algorithm of the kappa-linear class: the mean (float64 sum, rounded ONCE to fp32), then fp32 deviations from it"""
    v = _f(v).reshape(-1)
    mean = np.float32(v.astype(np.float64).mean())
    with np.errstate(all="ignore"):
        d = v - mean
        return float(mean), float((d.astype(np.float64) ** 2).sum().astype(np.float32))


# =====================================================================================================================================
# L2Norm
# =====================================================================================================================================
L2_SHAPES = {"tiny_odd": (2, 5, 7, 9), "conv4_3_like": (2, 512, 10, 10), "ragged_c": (1, 1030, 4, 6)}
L2_EXPS = (-100, -70, -50, -40, -33, -30, -20, 0, 30, 55)
L2_WEIGHTS = (2.0 ** -20, 1.0, 10.0, 2.0 ** 20)
L2_EPS = (1e-10, 1e-30)


@functools.lru_cache(maxsize=None)
def l2_inputs(case):
    """x, weight, grad_output (CPU, fp32): pixel p of an image is randn 2^k with k = L2_EXPS[p mod 10], so the neighbours in a 64-pixel
    tile span all ten scales; channel c has weight L2_WEIGHTS[c mod 4] (signs alternate every fourth channel)"""
    N, C, H, W = L2_SHAPES[case]
    gen = torch.Generator().manual_seed(2600 + list(L2_SHAPES).index(case))
    x = torch.randn(N, C, H, W, generator=gen)
    k = torch.tensor(L2_EXPS, dtype=torch.float64)[torch.arange(H * W) % len(L2_EXPS)].view(1, 1, H, W)
    x = (x.double() * 2.0 ** k).float()
    c = torch.arange(C)
    w = torch.tensor(L2_WEIGHTS)[c % 4] * torch.where((c // 4) % 2 == 0, 1.0, -1.0)
    go = torch.randn(N, C, H, W, generator=gen)
    return x, w.float(), go


def f32_ulp(t64):
    """the spacing of fp32 at |t| (float64 in and out), 2^-149 below the normal range"""
    e = torch.floor(torch.log2(t64.abs().clamp_min(2.0 ** -126)))
    return 2.0 ** (e - 23)


def l2_reference(x, w, go, eps):
    """float64 on the fp32 inputs -> dict name -> (reference, bound).  eps: the fp32 value the entry receives.

    norm = fl(fl(sqrt(T)) + eps), T the fp32 sum of C squares (four waves of C / 4, four accumulators each: far fewer than C / 2
    sequential adds).  Relative (C / 2 + 3) u.  A square below the normal range loses at most min(x^2, 2^-150); the root of the lost
    sum, uf <= sqrt(C 2^-149), is the absolute underflow term.
    So e_norm = (C / 2 + 3) u norm + uf, and 1 / norm is off by at most ri = e_norm / (norm - e_norm) relatively (written out, not
    to first order: where every square is lost, uf = r and norm_f = eps exactly).
    output = fl(w fl(x fl(1 / norm))): three more roundings: (ri + 3 u) |ref| -- to first order the (C / 2 + 6) u |ref| + |ref| uf /
    norm of the issue (+ 2^-149 (1 + |w|) for a product that is subnormal).
    grad_input = (w go - x t) / norm, t = s / (norm r), r = norm - eps, s = sum w go x:
      first term:  (ri + 3 u) |w go| / norm;
      second term T2 = x s / (norm^2 r): s is off by (C / 2 + 3) u sum|w go x|; 1 / norm enters twice; six roundings; and r itself:
                   fl(sqrt(T)) is relatively right, but the add of eps rounds it to the grid of norm and the lost squares move it:
                   |r_f - r| <= g = (C / 2 + 3) u r + ulp(norm) / 2 + uf.  For r > g the term is off by the ratio
                   r / (r - g) (1 + ri)^2 (1 + 6 u) at most -- to first order the |T2| ulp(norm) / (2 r) of the issue.  For r <= g
                   the kernel may see r = 0 and drop T2 (the header's rule: the error is |T2|) or see a positive r_f, which is at
                   least q = ulp(eps) / 2, the smallest positive norm_f - eps.
      the last subtraction and product: u |ref|.
    grad_weight[c] = sum_pixels go x / norm: acc_bound with K = N H W on absolute values, plus each term's share of its norm's error.
    Where the reference's norm^2 r is 0 (an all-zero pixel) the second term is 0 by the header's rule."""
    x, w, go = x.double(), w.double(), go.double()
    N, C, H, W = x.shape
    eps = float(np.float32(eps))
    wv = w.view(1, -1, 1, 1)
    sq = x * x
    r = sq.sum(1, keepdim=True).sqrt()
    norm = r + eps
    lost = torch.where(sq < 2.0 ** -126, sq.clamp_max(2.0 ** -150), torch.zeros_like(sq))
    uf = lost.sum(1, keepdim=True).sqrt()
    c_norm = ONE * (C / 2 + 3) * U32
    e_norm = c_norm * norm + uf
    ri = e_norm / (norm - e_norm)                  # the relative error of 1 / norm (norm - e_norm >= eps (1 - c u) > 0: uf <= r)
    y = wv * x / norm
    e_y = (ri + 3 * ONE * U32 * (1 + ri)) * y.abs() + F32_MIN_SUB * (1 + wv.abs())
    wgx = wv * go * x
    s, sa = wgx.sum(1, keepdim=True), wgx.abs().sum(1, keepdim=True)
    zero = r == 0
    safe = torch.where(zero, torch.ones_like(r), r)
    t2 = torch.where(zero, torch.zeros_like(s), x * s / (norm * norm * safe))
    t2a = torch.where(zero, torch.zeros_like(s), x.abs() * sa / (norm * norm * safe))
    gx = wv * go / norm - t2
    g = c_norm * r + f32_ulp(norm) / 2 + uf                                 # |r_f - r|
    q = f32_ulp(torch.tensor(eps, dtype=torch.float64)) / 2                 # the smallest positive norm_f - eps
    drop = r - g <= 0                                                       # the kernel may see r = 0 and take the term as 0
    r_lo = torch.where(drop, torch.full_like(r, float(q)), r - g)
    ratio = r / r_lo * (1 + ri) ** 2 * (1 + 6 * ONE * U32)
    e_t2 = t2.abs() * torch.maximum(ratio - 1, drop.double()) + ONE * (C / 2 + 3) * U32 * t2a * ratio
    e_gx = (ri + 3 * ONE * U32 * (1 + ri)) * (wv * go).abs() / norm + e_t2 + ONE * U32 * gx.abs() + F32_MIN_SUB
    term = go * x / norm
    gw, ga = term.sum((0, 2, 3)), term.abs().sum((0, 2, 3))
    e_gw = acc_bound("fp32", ga, N * H * W) + (term.abs() * (ri + 2 * ONE * U32 * (1 + ri))).sum((0, 2, 3))
    return {"norm": (norm[:, 0], e_norm[:, 0]), "output": (y, e_y), "grad_input": (gx, e_gx), "grad_weight": (gw, e_gw)}


@functools.lru_cache(maxsize=None)
def l2_case_reference(case, eps):
    return l2_reference(*l2_inputs(case), eps)


def l2_formula32(x, w, go, eps, doctor=None):
    """the module's formula and the header's gradient in torch's fp32 on the CPU, every operation rounded on its own -> the four
    tensors.  (Not torch's autograd: its division's gradient forms norm^2, which is 0 in fp32 for norm = 1e-30.)
    doctor: "eps_inside" puts eps under the root, "no_xt" drops the x t term of the gradient."""
    eps = torch.tensor(eps, dtype=torch.float32)
    wv = w.view(1, -1, 1, 1)
    ss = x.pow(2).sum(1, keepdim=True)
    norm = (ss + eps).sqrt() if doctor == "eps_inside" else ss.sqrt() + eps
    y = wv * (x / norm)
    r = norm - eps
    s = (wv * go * x).sum(1, keepdim=True)
    t = torch.where(r > 0, s / norm / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(r))
    if doctor == "no_xt":
        t = torch.zeros_like(t)
    gx = (wv * go - x * t) / norm
    gw = (go * x / norm).sum((0, 2, 3))
    return {"norm": norm[:, 0], "output": y, "grad_input": gx, "grad_weight": gw}


# =====================================================================================================================================
# the depthwise 3x3 conv: an exact restatement of nine fmaf in tap order
# =====================================================================================================================================
def fmaf32(a, b, c):
    """fl32(a b + c) with ONE rounding, on float32 numpy arrays.  The product of two fp32 values is exact in float64 (48 bits, an
    exponent within +-300).  The float64 sum p + c rounds; TwoSum gives its exact error e, and where e != 0 the sum is moved to the
    neighbour with an odd last bit (round to odd).  A round-to-odd value with 53 >= 24 + 2 bits rounds to fp32 (subnormals included,
    which need fewer bits still) as the exact sum does: no double rounding.  test_number_range_stats_ref.py checks it against integer
    arithmetic."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def dw_out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def dw_forward_exact(x, w, b, s):
    """x (N, C, H, W), w (C, 1, 3, 3), b (C) or None, fp32 numpy -> the header's sentence: nine fmaf in the order (0,0) .. (2,2) from
    the bias or +0, a tap in the padding skipped"""
    N, C, H, W = x.shape
    Ho, Wo = dw_out_hw(H, W, s)
    acc = np.zeros((N, C, Ho, Wo), np.float32) if b is None else np.broadcast_to(b.reshape(1, C, 1, 1), (N, C, Ho, Wo)).astype(np.float32)
    ho, wo = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    for i in range(3):
        for j in range(3):
            h, q = s * ho - 1 + i, s * wo - 1 + j
            ok = (h >= 0) & (h < H) & (q >= 0) & (q < W)
            v = x[:, :, np.clip(h, 0, H - 1), np.clip(q, 0, W - 1)]
            wt = np.broadcast_to(w[:, 0, i, j].reshape(1, C, 1, 1), v.shape)
            acc = np.where(ok[None, None], fmaf32(v, wt, acc), acc)
    return acc


def dw_backward_input_exact(go, w, H, W, s):
    """grad_input by the header's sentence: the taps in the same order from +0, a tap whose output pixel does not exist skipped"""
    N, C, Ho, Wo = go.shape
    acc = np.zeros((N, C, H, W), np.float32)
    h, q = np.arange(H)[:, None], np.arange(W)[None, :]
    for i in range(3):
        for j in range(3):
            a, c = h + 1 - i, q + 1 - j
            ok = (a % s == 0) & (c % s == 0) & (a // s >= 0) & (a // s < Ho) & (c // s >= 0) & (c // s < Wo) & (a >= 0) & (c >= 0)
            v = go[:, :, np.clip(a // s, 0, Ho - 1), np.clip(c // s, 0, Wo - 1)]
            wt = np.broadcast_to(w[:, 0, i, j].reshape(1, C, 1, 1), v.shape)
            acc = np.where(ok[None, None], fmaf32(v, wt, acc), acc)
    return acc


def dw_params_reference(x, go, s):
    """float64 -> (grad_weight, S_w, grad_bias, S_b): the sums and the same sums on absolute values"""
    x, go = torch.as_tensor(x).double(), torch.as_tensor(go).double()
    N, C, H, W = x.shape
    Ho, Wo = go.shape[2:]
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    gw, sw = torch.zeros(C, 1, 3, 3, dtype=torch.float64), torch.zeros(C, 1, 3, 3, dtype=torch.float64)
    for i in range(3):
        for j in range(3):
            v = xp[:, :, i:i + s * (Ho - 1) + 1:s, j:j + s * (Wo - 1) + 1:s]
            gw[:, 0, i, j] = (go * v).sum((0, 2, 3))
            sw[:, 0, i, j] = (go * v).abs().sum((0, 2, 3))
    return gw, sw, go.sum((0, 2, 3)), go.abs().sum((0, 2, 3))


def dw_values(shape, kind, seed):
    """fp32 values of `shape`: "edges" cycles f32_edges() from a seed-dependent start, an int k gives randn 2^k"""
    n = int(np.prod(shape))
    if kind == "edges":
        e = f32_edges()
        return e[(torch.arange(n) * 7 + 3 * seed) % e.numel()].reshape(shape).numpy().copy()
    gen = torch.Generator().manual_seed(2700 + seed)
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * 2.0 ** kind).float().numpy()


def f32_from_fraction(fr):
    """an exact rational (fractions.Fraction) -> the fp32 nearest to it, ties to even, subnormals kept, overflow to inf: integer
    arithmetic only (the independent evaluation fmaf32 is checked against)"""
    if fr == 0:
        return 0.0
    sign = -1.0 if fr < 0 else 1.0
    fr = abs(fr)
    n, d = fr.numerator, fr.denominator
    e = n.bit_length() - d.bit_length()
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1                                                      # 2^e <= fr < 2^(e + 1)
    q = max(e, -126) - 23                                           # the spacing is 2^q
    num, den = (n << max(-q, 0)), (d << max(q, 0))
    k, rem = divmod(num, den)
    if 2 * rem > den or (2 * rem == den and k & 1):
        k += 1
    if q > 104 or (q >= 0 and (k << q) >= (1 << 128)):
        return sign * float("inf")
    return sign * math.ldexp(float(k), q)


# =====================================================================================================================================
# SGD
# =====================================================================================================================================
SGD_MODES = {"no_momentum": dict(momentum=0.0), "momentum": dict(momentum=0.9), "nesterov": dict(momentum=0.9, nesterov=True)}
SGD_LRS = {"4e-3": 4e-3, "2^-140": 2.0 ** -140, "2^100": 2.0 ** 100}
SGD_SIZES = (5, 67)


def sgd_triples(n, step):
    """(p, g, b) of numel n from the cross product of f32_edges() with itself three times, truncated to the tensor: element t of
    step `step` takes the triple of index 997 t + 131 step + 17 (a stride coprime to 38^3, so every value of every factor turns up)"""
    e = f32_edges()
    m = e.numel()
    idx = (torch.arange(n) * 997 + 131 * step + 17) % (m ** 3)
    return e[idx // (m * m)].numpy().copy(), e[(idx // m) % m].numpy().copy(), e[idx % m].numpy().copy()
