// bn_prims.h -- the arithmetic both BatchNorm files share (batch_norm.hip: fp32 NCHW; batch_norm_nhwc.hip: 16-bit NHWC): the
// pre-activation and the (count, mean, M2) records of the statistics with their merge.
#pragma once
#include "common.h"

namespace tdrn {

// the pre-activation, in forward and backward alike: the centred form keeps the bits of x - mean that x * a + (beta - mean * a) loses
__device__ __forceinline__ float bn_z(float x, float mean, float a, float beta) { return __builtin_fmaf(x - mean, a, beta); }

// ---- statistics: (count, mean, M2) records merged with Chan's formula ---------------------------------------------------------------
struct Welford { float n, mean, m2; };

__device__ __forceinline__ Welford welford_merge(Welford a, Welford b)
{
    const float n = a.n + b.n;
    const float w = n > 0.f ? b.n / n : 0.f;
    const float d = b.mean - a.mean;
    return Welford{n, a.mean + d * w, a.m2 + b.m2 + d * d * a.n * w};
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
