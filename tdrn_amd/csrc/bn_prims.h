// bn_prims.h -- the arithmetic both BatchNorm files share (batch_norm.hip: fp32 NCHW; batch_norm_nhwc.hip: 16-bit NHWC): the
// pre-activation and the (count, mean, M2) records of the statistics with their merge.
#pragma once
#include "common.h"

namespace tdrn {

// the pre-activation, in forward and backward alike: the centred form keeps the bits of x - mean that x * a + (beta - mean * a) loses
__device__ __forceinline__ float bn_z(float x, float mean, float a, float beta) { return __builtin_fmaf(x - mean, a, beta); }

// ---- statistics: (count, mean, M2) records merged with Chan's formula ---------------------------------------------------------------
struct Welford { float n, mean, m2; };

// A merge with an empty record (a sweep's starting value, an idle lane of the shuffle tree) returns the other record: the formula
// gives the same bits there (0 + b.mean * 1, b.m2 + 0) unless d * d overflows -- a mean past 2^64 -- and inf * 0 makes M2 NaN.
// Between two records that hold values, d * d * a.n stays finite while n (max x - min x)^2 < 2^128 (tdrn_hip.h section i-d).
// The rule is one select on the difference that enters the M2 term (q = 0 for an empty side: the term is then 0, and the mean's
// a.mean + d * w is already exact with w = 0 or 1).  The formula itself keeps its shape, so the compiler contracts it into the same
// fma as before the rule existed and a merge of two records that hold values keeps its bits.
__device__ __forceinline__ Welford welford_merge(Welford a, Welford b)
{
    const float n = a.n + b.n;
    const float w = n > 0.f ? b.n / n : 0.f;
    const float d = b.mean - a.mean;
    const float q = (a.n == 0.f || b.n == 0.f) ? 0.f : d;
    return Welford{n, a.mean + d * w, a.m2 + b.m2 + q * q * a.n * w};
}

// K values held in registers: mean and M2 about the mean in two passes, differences taken against the first value
template <int K> __device__ __forceinline__ Welford welford_chunk(const float *v)
{
    float s = 0.f;
#pragma unroll
    for (int i = 1; i < K; ++i) s += v[i] - v[0];
    const float mu = s * (1.f / K);
    float m2 = 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float d = (v[i] - v[0]) - mu;
        m2 = __builtin_fmaf(d, d, m2);
    }
    return Welford{(float)K, v[0] + mu, m2};
}

}  // namespace tdrn
