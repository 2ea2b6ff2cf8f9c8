// batch_norm.hip -- BatchNorm2d with an optional fused ReLU, forward and backward, fp32 NCHW (tdrn_hip.h section i-d).
//
// A channel's M = N*H*W values are N planes of H*W contiguous floats.  Every pass cuts the channel's LINEAR index range [0, M) into
// `splits` equal pieces (batch_norm_splits: a pure function of N, C, H*W); workgroup (split s, channel c) sweeps its piece with 16-byte
// loads and stores.  The reducing passes write one record per (channel, split) into the workspace; a finalize kernel merges a channel's
// records in split order.  No float atomics: every output is bitwise reproducible.
//
// Which elements a thread takes is decided by the logical index alone, never by an address: the quads of a piece start at the piece's
// own first element (of a plane's part of it, when H*W is no multiple of 4), so a caller's buffer on any 4-byte boundary gives the
// same summation order, and the same bits, as an aligned one.  On a 16-byte-aligned plane segment the quads are aligned 16-byte
// accesses; elsewhere the same instructions run on a 4-byte boundary, which global loads and stores of a dword or more allow.
#include <type_traits>

#include "bn_prims.h"
#include "kernels.h"

namespace tdrn {

namespace {

constexpr int kT = 256;                 // threads per workgroup
constexpr int kLoads = 4;               // independent 16-byte loads a thread keeps in flight (over all tensors it reads)
constexpr unsigned kMinSplit = 4096;    // a split is worth a workgroup from 16 elements per thread
constexpr unsigned kGroups = 2048;      // 256 CUs x 8 workgroups

struct BnGeom { unsigned C, HW, M, S, per; };

typedef f32x4 f32x4_u __attribute__((aligned(4)));
__device__ __forceinline__ f32x4 ld4(const float *p) { return *(const f32x4_u *)p; }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *(f32x4_u *)p = v; }

// Workgroup (s, c)'s piece [lo, hi) of channel c: use(off[K], v[K], K) for K = U or 1 quads loaded by load(off), one(off) for the
// up to three elements behind a plane segment's last whole quad.  `off` is the element's offset in the NCHW tensor (< 2^31).
template <int U, typename Load, typename Use, typename One>
__device__ __forceinline__ void bn_sweep(const BnGeom &g, unsigned c, unsigned lo, unsigned hi, Load load, Use use, One one)
{
    const unsigned tid = threadIdx.x;
    auto quads = [&](unsigned nq, auto off_of) {
        unsigned q = tid;
        for (; q + (U - 1) * kT < nq; q += U * kT) {
            unsigned off[U];
            decltype(load(0u)) v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                off[u] = off_of(q + u * kT);
                v[u] = load(off[u]);
            }
            use(off, v, std::integral_constant<int, U>());
        }
        for (; q < nq; q += kT) {
            const unsigned off = off_of(q);
            const auto v = load(off);
            use(&off, &v, std::integral_constant<int, 1>());
        }
    };
    if (g.HW % 4 == 0) {
        // no quad of the linear index straddles two planes (lo and hi are multiples of 4): one flat loop, whatever the plane size
        const unsigned q0 = lo / 4;
        quads((hi - lo) / 4, [&](unsigned q) {
            const unsigned i = (q0 + q) * 4, n = i / g.HW;
            return (n * g.C + c) * g.HW + (i - n * g.HW);
        });
        return;
    }
    for (unsigned n = lo / g.HW; n * g.HW < hi; ++n) {      // the part of plane n inside the piece
        const unsigned p0 = n * g.HW, a = (lo > p0 ? lo : p0) - p0, b = (hi < p0 + g.HW ? hi : p0 + g.HW) - p0;
        const unsigned first = (n * g.C + c) * g.HW + a, nq = (b - a) / 4;
        quads(nq, [&](unsigned q) { return first + 4 * q; });
        if (tid < b - a - 4 * nq) one(first + 4 * nq + tid);
    }
}

__device__ __forceinline__ void bn_piece(const BnGeom &g, unsigned &c, unsigned &s, unsigned &lo, unsigned &hi)
{
    c = blockIdx.x / g.S;
    s = blockIdx.x - c * g.S;
    lo = s * g.per;
    hi = g.M - lo < g.per ? g.M : lo + g.per;
}

// (the pre-activation bn_z and the (count, mean, M2) records with their merge: bn_prims.h, shared with batch_norm_nhwc.hip)

__global__ __launch_bounds__(kT) void bn_stats_kernel(const float *__restrict__ x, float *__restrict__ rec, BnGeom g)
{
    unsigned c, s, lo, hi;
    bn_piece(g, c, s, lo, hi);
    Welford w{0.f, 0.f, 0.f};
    bn_sweep<kLoads>(
        g, c, lo, hi, [&](unsigned off) { return ld4(x + off); },
        [&](const unsigned *, const f32x4 *v, auto kc) {
            constexpr int K = decltype(kc)::value;
            float e[4 * K];
#pragma unroll
            for (int u = 0; u < K; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i) e[4 * u + i] = v[u][i];
            w = welford_merge(w, welford_chunk<4 * K>(e));
        },
        [&](unsigned off) { w = welford_merge(w, Welford{1.f, x[off], 0.f}); });
    // lanes of a wave, then the four waves, always in the same order
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const Welford b{__shfl_down(w.n, o), __shfl_down(w.mean, o), __shfl_down(w.m2, o)};
        w = welford_merge(w, b);
    }
    __shared__ float sh[kT / 64][3];
    const unsigned tid = threadIdx.x;
    if ((tid & 63) == 0) { sh[tid >> 6][0] = w.n; sh[tid >> 6][1] = w.mean; sh[tid >> 6][2] = w.m2; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kT / 64; ++i) w = welford_merge(w, Welford{sh[i][0], sh[i][1], sh[i][2]});
        float *r = rec + ((size_t)c * g.S + s) * 3;
        r[0] = w.n; r[1] = w.mean; r[2] = w.m2;
    }
}

// one thread per channel: the records in split order (training), or the running buffers (eval) -> save_mean, save_invstd; the
// running statistics move once
__global__ __launch_bounds__(kT) void bn_stats_finalize_kernel(const float *__restrict__ rec, float *running_mean, float *running_var,
                                                                float *__restrict__ save_mean, float *__restrict__ save_invstd, BnGeom g,
                                                                int training, float momentum, float eps)
{
    const unsigned c = blockIdx.x * kT + threadIdx.x;
    if (c >= g.C) return;
    if (!training) {
        save_mean[c] = running_mean[c];
        save_invstd[c] = (float)(1.0 / sqrt((double)running_var[c] + (double)eps));
        return;
    }
    double n = 0.0, mean = 0.0, m2 = 0.0;
    const float *r = rec + (size_t)c * g.S * 3;
    for (unsigned s = 0; s < g.S; ++s, r += 3) {
        const double nb = r[0], d = (double)r[1] - mean, nn = n + nb, w = nb / nn;     // nb >= 1: no split is empty
        mean += d * w;
        m2 += (double)r[2] + d * d * n * w;
        n = nn;
    }
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)(1.0 / sqrt(m2 / (double)g.M + (double)eps));
    if (running_mean) {
        const double mo = momentum;
        running_mean[c] = (float)((1.0 - mo) * (double)running_mean[c] + mo * mean);
        running_var[c] = (float)((1.0 - mo) * (double)running_var[c] + mo * (m2 / ((double)g.M - 1.0)));
    }
}

// ---- forward apply --------------------------------------------------------------------------------------------------------------------
template <bool RELU> __device__ __forceinline__ float bn_act(float z) { return RELU ? (z < 0.f ? 0.f : z) : z; }

template <bool RELU>
__global__ __launch_bounds__(kT) void bn_apply_kernel(const float *__restrict__ x, const float *__restrict__ weight, const float *__restrict__ bias,
                                                       const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                       float *__restrict__ y, BnGeom g)
{
    unsigned c, s, lo, hi;
    bn_piece(g, c, s, lo, hi);
    const float mean = save_mean[c], a = weight[c] * save_invstd[c], beta = bias[c];
    bn_sweep<kLoads>(
        g, c, lo, hi, [&](unsigned off) { return ld4(x + off); },
        [&](const unsigned *off, const f32x4 *v, auto kc) {
#pragma unroll
            for (int u = 0; u < decltype(kc)::value; ++u) {
                f32x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = bn_act<RELU>(bn_z(v[u][i], mean, a, beta));
                st4(y + off[u], o);
            }
        },
        [&](unsigned off) { y[off] = bn_act<RELU>(bn_z(x[off], mean, a, beta)); });
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------
struct XG { f32x4 x, g; };

// dy' = dy [z > 0] (z recomputed from x as the forward computed it; without ReLU dy' = dy)
template <bool RELU> __device__ __forceinline__ float bn_dy(float x, float dy, float mean, float a, float beta)
{
    return RELU ? (bn_z(x, mean, a, beta) > 0.f ? dy : 0.f) : dy;
}

// per (channel, split): sum dy' and sum dy' xhat
template <bool RELU>
__global__ __launch_bounds__(kT) void bn_bwd_reduce_kernel(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ weight,
                                                            const float *__restrict__ bias, const float *__restrict__ save_mean,
                                                            const float *__restrict__ save_invstd, float *__restrict__ rec, BnGeom g)
{
    unsigned c, s, lo, hi;
    bn_piece(g, c, s, lo, hi);
    const float mean = save_mean[c], invstd = save_invstd[c], a = weight[c] * invstd, beta = bias[c];
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    bn_sweep<kLoads / 2>(
        g, c, lo, hi, [&](unsigned off) { return XG{ld4(x + off), ld4(dy + off)}; },
        [&](const unsigned *, const XG *v, auto kc) {
#pragma unroll
            for (int u = 0; u < decltype(kc)::value; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float d = bn_dy<RELU>(v[u].x[i], v[u].g[i], mean, a, beta);
                    s1[i] += d;
                    s2[i] = __builtin_fmaf(d, (v[u].x[i] - mean) * invstd, s2[i]);
                }
        },
        [&](unsigned off) {
            const float d = bn_dy<RELU>(x[off], dy[off], mean, a, beta);
            s1[0] += d;
            s2[0] = __builtin_fmaf(d, (x[off] - mean) * invstd, s2[0]);
        });
    float t1 = (s1[0] + s1[1]) + (s1[2] + s1[3]), t2 = (s2[0] + s2[1]) + (s2[2] + s2[3]);
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        t1 += __shfl_down(t1, o);
        t2 += __shfl_down(t2, o);
    }
    __shared__ float sh[kT / 64][2];
    const unsigned tid = threadIdx.x;
    if ((tid & 63) == 0) { sh[tid >> 6][0] = t1; sh[tid >> 6][1] = t2; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kT / 64; ++i) { t1 += sh[i][0]; t2 += sh[i][1]; }
        float *r = rec + ((size_t)c * g.S + s) * 2;
        r[0] = t1; r[1] = t2;
    }
}

// one thread per channel: the records in split order -> sums[c] = (sum dy' / M, sum dy' xhat / M) for the apply pass,
// grad_weight += scale sum dy' xhat, grad_bias += scale sum dy'
__global__ __launch_bounds__(kT) void bn_bwd_finalize_kernel(const float *__restrict__ rec, float *__restrict__ sums, float *grad_weight,
                                                              float *grad_bias, BnGeom g, float scale)
{
    const unsigned c = blockIdx.x * kT + threadIdx.x;
    if (c >= g.C) return;
    double t1 = 0.0, t2 = 0.0;
    const float *r = rec + (size_t)c * g.S * 2;
    for (unsigned s = 0; s < g.S; ++s, r += 2) { t1 += (double)r[0]; t2 += (double)r[1]; }
    sums[2 * (size_t)c] = (float)(t1 / (double)g.M);
    sums[2 * (size_t)c + 1] = (float)(t2 / (double)g.M);
    if (grad_weight) {
        grad_weight[c] += scale * (float)t2;
        grad_bias[c] += scale * (float)t1;
    }
}

// dx = a (dy' - (sum dy' + xhat sum dy' xhat) / M) with batch statistics, a dy' with the running ones
template <bool RELU, bool TRAIN>
__global__ __launch_bounds__(kT) void bn_bwd_apply_kernel(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ weight,
                                                           const float *__restrict__ bias, const float *__restrict__ save_mean,
                                                           const float *__restrict__ save_invstd, const float *__restrict__ sums,
                                                           float *__restrict__ dx, BnGeom g)
{
    unsigned c, s, lo, hi;
    bn_piece(g, c, s, lo, hi);
    const float mean = save_mean[c], invstd = save_invstd[c], a = weight[c] * invstd, beta = bias[c];
    const float k1 = TRAIN ? sums[2 * (size_t)c] : 0.f, k2 = TRAIN ? sums[2 * (size_t)c + 1] : 0.f;
    auto grad = [&](float xv, float dv) {
        const float d = bn_dy<RELU>(xv, dv, mean, a, beta);
        return TRAIN ? a * (d - __builtin_fmaf((xv - mean) * invstd, k2, k1)) : a * d;
    };
    bn_sweep<kLoads / 2>(
        g, c, lo, hi, [&](unsigned off) { return XG{ld4(x + off), ld4(dy + off)}; },
        [&](const unsigned *off, const XG *v, auto kc) {
#pragma unroll
            for (int u = 0; u < decltype(kc)::value; ++u) {
                f32x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = grad(v[u].x[i], v[u].g[i]);
                st4(dx + off[u], o);
            }
        },
        [&](unsigned off) { dx[off] = grad(x[off], dy[off]); });
}

BnGeom bn_geom(int N, int C, int HW)
{
    int S, per;
    batch_norm_splits(N, C, HW, S, per);
    return BnGeom{(unsigned)C, (unsigned)HW, (unsigned)((long long)N * HW), (unsigned)S, (unsigned)per};
}

// records of the reducing passes [C][S][3] fp32, then the backward's per-channel sums [C][2]
size_t bn_rec_bytes(const BnGeom &g) { return (size_t)g.C * g.S * 3 * 4; }

}  // namespace

// S = clamp(floor(2048 / C), 1, ceil(M / 4096)) pieces of per_split = ceil(M / S) rounded up to 4 elements
void batch_norm_splits(int N, int C, int HW, int &splits, int &per_split)
{
    const long long M = (long long)N * HW;
    long long S = kGroups / (unsigned)(C < 1 ? 1 : C);
    const long long most = (M + kMinSplit - 1) / kMinSplit;
    if (S > most) S = most;
    if (S < 1) S = 1;
    const long long per = ((M + S - 1) / S + 3) / 4 * 4;
    per_split = (int)per;
    splits = (int)((M + per - 1) / per);
}

size_t batch_norm_workspace_bytes(int N, int C, int HW)
{
    const BnGeom g = bn_geom(N, C, HW);
    return bn_rec_bytes(g) + (size_t)g.C * 2 * 4;
}

// the two per-channel finalize kernels for a caller with its own sweeps (batch_norm_nhwc.hip): records [C][S][3] / [C][S][2]
int launch_bn_stats_finalize(const float *rec, float *running_mean, float *running_var, float *save_mean, float *save_invstd, int C,
                             long long M, int S, int training, float momentum, float eps, hipStream_t s)
{
    const BnGeom g{(unsigned)C, 0u, (unsigned)M, (unsigned)S, 0u};
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((g.C + kT - 1) / kT), dim3(kT), 0, s, rec, running_mean, running_var, save_mean,
                       save_invstd, g, training, momentum, eps);
    return hip_status(hipGetLastError());
}

int launch_bn_bwd_finalize(const float *rec, float *sums, float *grad_weight, float *grad_bias, int C, long long M, int S, float scale,
                           hipStream_t s)
{
    const BnGeom g{(unsigned)C, 0u, (unsigned)M, (unsigned)S, 0u};
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((g.C + kT - 1) / kT), dim3(kT), 0, s, rec, sums, grad_weight, grad_bias, g, scale);
    return hip_status(hipGetLastError());
}

int launch_batch_norm_forward(const float *input, const float *weight, const float *bias, float *running_mean, float *running_var,
                              float *output, float *save_mean, float *save_invstd, int N, int C, int HW, int training, float momentum,
                              float eps, int relu, void *ws, hipStream_t s)
{
    const BnGeom g = bn_geom(N, C, HW);
    float *rec = (float *)ws;
    const unsigned groups = g.C * g.S, cblocks = (g.C + kT - 1) / kT;
    if (training) hipLaunchKernelGGL(bn_stats_kernel, dim3(groups), dim3(kT), 0, s, input, rec, g);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(cblocks), dim3(kT), 0, s, rec, running_mean, running_var, save_mean, save_invstd, g,
                       training, momentum, eps);
    if (relu)
        hipLaunchKernelGGL(bn_apply_kernel<true>, dim3(groups), dim3(kT), 0, s, input, weight, bias, save_mean, save_invstd, output, g);
    else
        hipLaunchKernelGGL(bn_apply_kernel<false>, dim3(groups), dim3(kT), 0, s, input, weight, bias, save_mean, save_invstd, output, g);
    return hip_status(hipGetLastError());
}

int launch_batch_norm_backward(const float *input, const float *grad_output, const float *weight, const float *bias, const float *save_mean,
                               const float *save_invstd, float *grad_input, float *grad_weight, float *grad_bias, int N, int C, int HW,
                               int training, int relu, float scale, void *ws, hipStream_t s)
{
    const BnGeom g = bn_geom(N, C, HW);
    float *rec = (float *)ws, *sums = (float *)((char *)ws + bn_rec_bytes(g));
    const unsigned groups = g.C * g.S, cblocks = (g.C + kT - 1) / kT;
    // the sums serve the parameter gradients and, with batch statistics, the input gradient
    if (grad_weight || (grad_input && training)) {
        if (relu)
            hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, dim3(groups), dim3(kT), 0, s, input, grad_output, weight, bias, save_mean,
                               save_invstd, rec, g);
        else
            hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, dim3(groups), dim3(kT), 0, s, input, grad_output, weight, bias, save_mean,
                               save_invstd, rec, g);
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cblocks), dim3(kT), 0, s, rec, sums, grad_weight, grad_bias, g, scale);
    }
    if (grad_input) {
        auto k = relu ? (training ? bn_bwd_apply_kernel<true, true> : bn_bwd_apply_kernel<true, false>)
                      : (training ? bn_bwd_apply_kernel<false, true> : bn_bwd_apply_kernel<false, false>);
        hipLaunchKernelGGL(k, dim3(groups), dim3(kT), 0, s, input, grad_output, weight, bias, save_mean, save_invstd, sums, grad_input, g);
    }
    return hip_status(hipGetLastError());
}

}  // namespace tdrn
