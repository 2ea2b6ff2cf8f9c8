// batch_norm_nhwc.hip -- BatchNorm2d with an optional fused ReLU, forward and backward, on resident tensors: 16-bit NHWC activations
// and activation gradients, fp32 parameters and statistics (tdrn_hip.h section i-k).
//
// The tensor is a matrix [M][C], M = N*H*W pixel rows of C contiguous channels (C a multiple of 64), and every reduction runs DOWN the
// pixel axis.  A workgroup owns a block of 64 channels and one of `splits` pixel ranges (batch_norm_nhwc_splits: a pure function of
// N, C, H*W).  Thread t takes the 8 channels 8 (t & 7) .. of the block -- one 16-byte access per pixel -- and the pixel rows
// lo + (t >> 3) + 32 j of the range: the 8 threads of a row read 128 contiguous bytes, a wave 8 rows.  Four rows are in flight per
// thread in the statistics and apply sweeps, two of each tensor in the backward sweeps.
//
// Statistics are (count, mean, M2) records per channel (bn_prims.h), never sums of squares: a thread folds chunks of four rows
// (welford_chunk: differences against the chunk's first value) into its running record, then the records merge with Chan's formula
// in a fixed order: the thread's chunks in row order; the 8 lanes of a wave that hold the same channels (shuffles by 32, 16, 8); the
// four waves in wave order through LDS; the splits in split order, in float64, in batch_norm.hip's finalize kernels, whose record
// layout [C][S][3] (and [C][S][2] for the backward's two sums) these kernels write.  No float atomics: every output is bitwise
// reproducible.  The pre-activation is bn_z, the one of the fp32 NCHW kernels; the ReLU acts on it in fp32 before the one rounding of
// the output, and the backward recomputes the mask z > 0 from the saved 16-bit input.
#include <type_traits>

#include "bn_prims.h"
#include "kernels.h"

namespace tdrn {

namespace {

constexpr int kT = 256;                 // threads per workgroup
constexpr int kCB = 64;                 // channels per workgroup (= kChanPad: C holds whole blocks)
constexpr int kCT = 8;                  // channels per thread: 16 bytes of a 16-bit type
constexpr int kRows = kT / (kCB / kCT); // pixel rows a workgroup covers per pass: 32
constexpr int kU = 4;                   // rows a thread keeps in flight
constexpr int kMinRows = 256;           // a split is worth a workgroup from 8 rows per thread
constexpr int kGroups = 2048;           // 256 CUs x 8 workgroups
static_assert(kCB == kChanPad && kRows == 32, "whole channel blocks; the lane merge below assumes 8 rows of 8 threads per wave");

struct BnNhwcGeom { unsigned C, M, S, per; };

// workgroup -> (channel block, split); thread -> its first channel and its first row; [lo, hi) = the split's rows
struct Piece { unsigned c0, s, lo, hi, row; };
__device__ __forceinline__ Piece bn_nhwc_piece(const BnNhwcGeom &g)
{
    const unsigned cb = blockIdx.x / g.S, s = blockIdx.x - cb * g.S, lo = s * g.per;
    return Piece{cb * kCB + (threadIdx.x & 7) * kCT, s, lo, g.M - lo < g.per ? g.M : lo + g.per, lo + (threadIdx.x >> 3)};
}

__device__ __forceinline__ u32x4 ld16(const char *p, unsigned row, unsigned C, unsigned c0) { return *(const u32x4 *)(p + ((size_t)row * C + c0) * 2); }
__device__ __forceinline__ void st16(char *p, unsigned row, unsigned C, unsigned c0, u32x4 v) { *(u32x4 *)(p + ((size_t)row * C + c0) * 2) = v; }

// rows row, row + 32, ... < hi of a thread: use(rows[K], raw[K], K) for K = U whole groups, then K = 1
template <int U, typename Load, typename Use> __device__ __forceinline__ void bn_nhwc_sweep(unsigned row, unsigned hi, Load load, Use use)
{
    for (; row + (U - 1) * kRows < hi; row += U * kRows) {
        unsigned rows[U];
        decltype(load(0u)) v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            rows[u] = row + u * kRows;
            v[u] = load(rows[u]);
        }
        use(rows, v, std::integral_constant<int, U>());
    }
    for (; row < hi; row += kRows) {
        const auto v = load(row);
        use(&row, &v, std::integral_constant<int, 1>());
    }
}

// the 8 lanes of a wave that hold the same channels are lanes l, l + 8, ..., l + 56: after the three steps lanes 0..7 hold the wave's value
template <typename T, typename Merge> __device__ __forceinline__ void lane_merge(T &v, Merge merge)
{
#pragma unroll
    for (int o = 32; o >= 8; o >>= 1) merge(v, o);
}

// ---- statistics -----------------------------------------------------------------------------------------------------------------------
template <typename DT>
__global__ __launch_bounds__(kT) void bn_nhwc_stats_kernel(const char *__restrict__ x, float *__restrict__ rec, BnNhwcGeom g)
{
    const Piece pc = bn_nhwc_piece(g);
    Welford w[kCT];
#pragma unroll
    for (int c = 0; c < kCT; ++c) w[c] = Welford{0.f, 0.f, 0.f};
    bn_nhwc_sweep<kU>(
        pc.row, pc.hi, [&](unsigned row) { return ld16(x, row, g.C, pc.c0); },
        [&](const unsigned *, const u32x4 *raw, auto kc) {
            constexpr int K = decltype(kc)::value;
            float v[K][kCT];
#pragma unroll
            for (int u = 0; u < K; ++u) unpack16<DT>(raw[u], v[u]);
#pragma unroll
            for (int c = 0; c < kCT; ++c) {
                if constexpr (K == 1) {
                    w[c] = welford_merge(w[c], Welford{1.f, v[0][c], 0.f});
                } else {
                    float e[K];
#pragma unroll
                    for (int u = 0; u < K; ++u) e[u] = v[u][c];
                    w[c] = welford_merge(w[c], welford_chunk<K>(e));
                }
            }
        });
#pragma unroll
    for (int c = 0; c < kCT; ++c)
        lane_merge(w[c], [](Welford &a, int o) {
            const Welford b{__shfl_down(a.n, o), __shfl_down(a.mean, o), __shfl_down(a.m2, o)};
            a = welford_merge(a, b);
        });
    __shared__ float sh[kT / 64][kCB][3];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane < 8) {
#pragma unroll
        for (int c = 0; c < kCT; ++c) {
            float *d = sh[wave][lane * kCT + c];
            d[0] = w[c].n; d[1] = w[c].mean; d[2] = w[c].m2;
        }
    }
    __syncthreads();
    if (tid < kCB) {
        Welford a{sh[0][tid][0], sh[0][tid][1], sh[0][tid][2]};
        for (int i = 1; i < kT / 64; ++i) a = welford_merge(a, Welford{sh[i][tid][0], sh[i][tid][1], sh[i][tid][2]});
        float *r = rec + ((size_t)(pc.c0 - (tid & 7) * kCT + tid) * g.S + pc.s) * 3;
        r[0] = a.n; r[1] = a.mean; r[2] = a.m2;
    }
}

// ---- forward apply --------------------------------------------------------------------------------------------------------------------
struct ChanCoef { float mean[kCT], invstd[kCT], a[kCT], beta[kCT]; };
__device__ __forceinline__ ChanCoef chan_coef(const float *weight, const float *bias, const float *save_mean, const float *save_invstd, unsigned c0)
{
    ChanCoef k;
#pragma unroll
    for (int c = 0; c < kCT; ++c) {
        k.mean[c] = save_mean[c0 + c];
        k.invstd[c] = save_invstd[c0 + c];
        k.a[c] = weight[c0 + c] * k.invstd[c];
        k.beta[c] = bias[c0 + c];
    }
    return k;
}

template <typename DT, bool RELU>
__global__ __launch_bounds__(kT) void bn_nhwc_apply_kernel(const char *__restrict__ x, const float *__restrict__ weight,
                                                            const float *__restrict__ bias, const float *__restrict__ save_mean,
                                                            const float *__restrict__ save_invstd, char *__restrict__ y, BnNhwcGeom g)
{
    const Piece pc = bn_nhwc_piece(g);
    const ChanCoef k = chan_coef(weight, bias, save_mean, save_invstd, pc.c0);
    bn_nhwc_sweep<kU>(
        pc.row, pc.hi, [&](unsigned row) { return ld16(x, row, g.C, pc.c0); },
        [&](const unsigned *rows, const u32x4 *raw, auto kc) {
#pragma unroll
            for (int u = 0; u < decltype(kc)::value; ++u) {
                float v[kCT];
                unpack16<DT>(raw[u], v);
#pragma unroll
                for (int c = 0; c < kCT; ++c) {
                    const float z = bn_z(v[c], k.mean[c], k.a[c], k.beta[c]);
                    v[c] = RELU ? (z < 0.f ? 0.f : z) : z;           // (a NaN stays a NaN)
                }
                st16(y, rows[u], g.C, pc.c0, pack16<DT>(v));
            }
        });
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------
struct XG16 { u32x4 x, g; };

// dy' = dy [z > 0] (z recomputed from x as the forward computed it; without ReLU dy' = dy)
template <bool RELU> __device__ __forceinline__ float bn_nhwc_dy(float x, float dy, const ChanCoef &k, int c)
{
    return RELU ? (bn_z(x, k.mean[c], k.a[c], k.beta[c]) > 0.f ? dy : 0.f) : dy;
}

// per (channel, split): sum dy' and sum dy' xhat
template <typename DT, bool RELU>
__global__ __launch_bounds__(kT) void bn_nhwc_bwd_reduce_kernel(const char *__restrict__ x, const char *__restrict__ dy,
                                                                 const float *__restrict__ weight, const float *__restrict__ bias,
                                                                 const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                                 float *__restrict__ rec, BnNhwcGeom g)
{
    const Piece pc = bn_nhwc_piece(g);
    const ChanCoef k = chan_coef(weight, bias, save_mean, save_invstd, pc.c0);
    float s1[kCT], s2[kCT];
#pragma unroll
    for (int c = 0; c < kCT; ++c) s1[c] = s2[c] = 0.f;
    bn_nhwc_sweep<kU / 2>(
        pc.row, pc.hi, [&](unsigned row) { return XG16{ld16(x, row, g.C, pc.c0), ld16(dy, row, g.C, pc.c0)}; },
        [&](const unsigned *, const XG16 *v, auto kc) {
#pragma unroll
            for (int u = 0; u < decltype(kc)::value; ++u) {
                float xv[kCT], gv[kCT];
                unpack16<DT>(v[u].x, xv);
                unpack16<DT>(v[u].g, gv);
#pragma unroll
                for (int c = 0; c < kCT; ++c) {
                    const float d = bn_nhwc_dy<RELU>(xv[c], gv[c], k, c);
                    s1[c] += d;
                    s2[c] = __builtin_fmaf(d, (xv[c] - k.mean[c]) * k.invstd[c], s2[c]);
                }
            }
        });
#pragma unroll
    for (int c = 0; c < kCT; ++c) {
        lane_merge(s1[c], [](float &a, int o) { a += __shfl_down(a, o); });
        lane_merge(s2[c], [](float &a, int o) { a += __shfl_down(a, o); });
    }
    __shared__ float sh[kT / 64][kCB][2];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane < 8) {
#pragma unroll
        for (int c = 0; c < kCT; ++c) {
            sh[wave][lane * kCT + c][0] = s1[c];
            sh[wave][lane * kCT + c][1] = s2[c];
        }
    }
    __syncthreads();
    if (tid < kCB) {
        float t1 = sh[0][tid][0], t2 = sh[0][tid][1];
        for (int i = 1; i < kT / 64; ++i) { t1 += sh[i][tid][0]; t2 += sh[i][tid][1]; }
        float *r = rec + ((size_t)(pc.c0 - (tid & 7) * kCT + tid) * g.S + pc.s) * 2;
        r[0] = t1; r[1] = t2;
    }
}

// dx = a (dy' - (sum dy' + xhat sum dy' xhat) / M) with batch statistics, a dy' with the running ones
template <typename DT, bool RELU, bool TRAIN>
__global__ __launch_bounds__(kT) void bn_nhwc_bwd_apply_kernel(const char *__restrict__ x, const char *__restrict__ dy,
                                                                const float *__restrict__ weight, const float *__restrict__ bias,
                                                                const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                                const float *__restrict__ sums, char *__restrict__ dx, BnNhwcGeom g)
{
    const Piece pc = bn_nhwc_piece(g);
    const ChanCoef k = chan_coef(weight, bias, save_mean, save_invstd, pc.c0);
    float k1[kCT], k2[kCT];
#pragma unroll
    for (int c = 0; c < kCT; ++c) {
        k1[c] = TRAIN ? sums[2 * (size_t)(pc.c0 + c)] : 0.f;
        k2[c] = TRAIN ? sums[2 * (size_t)(pc.c0 + c) + 1] : 0.f;
    }
    bn_nhwc_sweep<kU / 2>(
        pc.row, pc.hi, [&](unsigned row) { return XG16{ld16(x, row, g.C, pc.c0), ld16(dy, row, g.C, pc.c0)}; },
        [&](const unsigned *rows, const XG16 *v, auto kc) {
#pragma unroll
            for (int u = 0; u < decltype(kc)::value; ++u) {
                float xv[kCT], gv[kCT];
                unpack16<DT>(v[u].x, xv);
                unpack16<DT>(v[u].g, gv);
#pragma unroll
                for (int c = 0; c < kCT; ++c) {
                    const float d = bn_nhwc_dy<RELU>(xv[c], gv[c], k, c);
                    gv[c] = TRAIN ? k.a[c] * (d - __builtin_fmaf((xv[c] - k.mean[c]) * k.invstd[c], k2[c], k1[c])) : k.a[c] * d;
                }
                st16(dx, rows[u], g.C, pc.c0, pack16<DT>(gv));
            }
        });
}

BnNhwcGeom bn_nhwc_geom(int N, int C, int HW)
{
    int S, per;
    batch_norm_nhwc_splits(N, C, HW, S, per);
    return BnNhwcGeom{(unsigned)C, (unsigned)((long long)N * HW), (unsigned)S, (unsigned)per};
}

size_t bn_nhwc_rec_bytes(const BnNhwcGeom &g) { return (size_t)g.C * g.S * 3 * 4; }

}  // namespace

// S = clamp(floor(2048 / (C / 64)), 1, ceil(M / 256)) ranges of per_split = ceil(M / S) rounded up to 32 rows
void batch_norm_nhwc_splits(int N, int C, int HW, int &splits, int &per_split)
{
    const long long M = (long long)N * HW, blocks = C / kCB < 1 ? 1 : C / kCB;
    long long S = kGroups / blocks;
    const long long most = (M + kMinRows - 1) / kMinRows;
    if (S > most) S = most;
    if (S < 1) S = 1;
    const long long per = ((M + S - 1) / S + kRows - 1) / kRows * kRows;
    per_split = (int)per;
    splits = (int)((M + per - 1) / per);
}

// the per-(channel, split) records [C][S][3] fp32, then the backward's per-channel sums [C][2]
size_t batch_norm_nhwc_workspace_bytes(int N, int C, int HW)
{
    const BnNhwcGeom g = bn_nhwc_geom(N, C, HW);
    return bn_nhwc_rec_bytes(g) + (size_t)g.C * 2 * 4;
}

int launch_batch_norm_nhwc_forward(const void *input, const float *weight, const float *bias, float *running_mean, float *running_var,
                                   void *output, float *save_mean, float *save_invstd, int N, int C, int HW, int training, float momentum,
                                   float eps, int relu, int dtype, void *ws, hipStream_t s)
{
    if (C % kCB) return TDRN_E_UNSUPPORTED;
    const BnNhwcGeom g = bn_nhwc_geom(N, C, HW);
    float *rec = (float *)ws;
    const dim3 grid(g.C / kCB * g.S), block(kT);
    const char *x = (const char *)input;
    return dispatch_dtype16(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        if (training) {
            hipLaunchKernelGGL(bn_nhwc_stats_kernel<DT>, grid, block, 0, s, x, rec, g);
            TDRN_HIP_TRY(hipGetLastError());
        }
        TDRN_TRY(launch_bn_stats_finalize(rec, running_mean, running_var, save_mean, save_invstd, C, g.M, (int)g.S, training, momentum, eps, s));
        hipLaunchKernelGGL((relu ? bn_nhwc_apply_kernel<DT, true> : bn_nhwc_apply_kernel<DT, false>), grid, block, 0, s, x, weight, bias,
                           save_mean, save_invstd, (char *)output, g);
        return hip_status(hipGetLastError());
    });
}

namespace {

template <typename DT>
int bn_nhwc_backward_dt(const BnNhwcGeom &g, const char *x, const char *dy, const float *weight, const float *bias, const float *save_mean,
                        const float *save_invstd, char *dx, float *grad_weight, float *grad_bias, int training, int relu, float scale,
                        void *ws, hipStream_t s)
{
    float *rec = (float *)ws, *sums = (float *)((char *)ws + bn_nhwc_rec_bytes(g));
    const dim3 grid(g.C / kCB * g.S), block(kT);
    // the sums serve the parameter gradients and, with batch statistics, the input gradient
    if (grad_weight || (dx && training)) {
        hipLaunchKernelGGL((relu ? bn_nhwc_bwd_reduce_kernel<DT, true> : bn_nhwc_bwd_reduce_kernel<DT, false>), grid, block, 0, s, x, dy, weight,
                           bias, save_mean, save_invstd, rec, g);
        TDRN_HIP_TRY(hipGetLastError());
        TDRN_TRY(launch_bn_bwd_finalize(rec, sums, grad_weight, grad_bias, (int)g.C, g.M, (int)g.S, scale, s));
    }
    if (dx) {
        auto k = relu ? (training ? bn_nhwc_bwd_apply_kernel<DT, true, true> : bn_nhwc_bwd_apply_kernel<DT, true, false>)
                      : (training ? bn_nhwc_bwd_apply_kernel<DT, false, true> : bn_nhwc_bwd_apply_kernel<DT, false, false>);
        hipLaunchKernelGGL(k, grid, block, 0, s, x, dy, weight, bias, save_mean, save_invstd, sums, dx, g);
    }
    return hip_status(hipGetLastError());
}

}  // namespace

int launch_batch_norm_nhwc_backward(const void *input, const void *grad_output, const float *weight, const float *bias,
                                    const float *save_mean, const float *save_invstd, void *grad_input, float *grad_weight,
                                    float *grad_bias, int N, int C, int HW, int training, int relu, float scale, int dtype, void *ws,
                                    hipStream_t s)
{
    if (C % kCB) return TDRN_E_UNSUPPORTED;
    const BnNhwcGeom g = bn_nhwc_geom(N, C, HW);
    const char *x = (const char *)input, *dy = (const char *)grad_output;
    char *dx = (char *)grad_input;
    return dispatch_dtype16(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        return bn_nhwc_backward_dt<DT>(g, x, dy, weight, bias, save_mean, save_invstd, dx, grad_weight, grad_bias, training, relu, scale, ws, s);
    });
}

}  // namespace tdrn
