// dwconv_train.hip -- the depthwise 3x3 conv of conv_dw (model/networks.py:736-745 of the reference: nn.Conv2d(c, c, 3, s, 1, groups=c)) with
// gradients, stride 1 and 2, pad 1 (tdrn_hip.h section i-h).  fp32 NCHW in, fp32 NCHW out: every (n, c) plane is independent and
// contiguous, so there is no layout conversion, no repacked weight and, for the forward and the input gradient, no workspace.
//   y[n][c][ho][wo]  = b[c] + sum_{i,j} x[n][c][s ho - 1 + i][s wo - 1 + j] w[c][i][j]
//   gx[n][c][h][w]   = sum_{i,j} go[n][c][(h + 1 - i) / s][(w + 1 - j) / s] w[c][i][j]     over the taps whose quotient is whole and in range
//   gw[c][i][j]     += scale sum_{n,ho,wo} go[n][c][ho][wo] x[n][c][s ho - 1 + i][s wo - 1 + j],   gb[c] += scale sum go
// Mapping.  Forward and input gradient: one thread per result element, the flat NCHW index cut into 256-thread workgroups, so the 64
// lanes of a wave read and write consecutive columns of a row (or, on the small maps, of consecutive rows and planes): every access is
// a run of consecutive dwords.  The 9-fold reuse of the source is left to the caches, not staged in LDS: the planes go from 160 x 160
// down to 3 x 3, a tile with its halo would be mostly halo on the lower half of them, and the three source rows an output row needs
// (<= 1.9 KiB at 160 columns) stay in the CU's 32-KiB L1 from one tap row to the next.  The nine weights of a plane are wave-uniform
// on the large maps and come from the same cache.  Nine fmaf in the fixed order (0,0) (0,1) ... (2,2), starting from the bias or
// +0; a tap in the padding (or, in the gradient, of the wrong parity) is skipped, so it contributes nothing and an input row or
// column that no output touches gets exactly 0.
// Weight gradient: ten sums per channel over K = N Ho Wo.  Workgroup (c, split) takes the K range [split per_split, ...) of channel c,
// thread t its elements t, t + 256, ... in that order; the 256 threads are summed by __shfl_down inside each wave (a fixed tree) and
// over the four waves in wave order; partial[c][split][10] goes to the workspace and dwconv_wgrad_reduce_kernel adds the splits in split
// order.  splits and per_split come from (N, C, Ho, Wo) alone (dwconv_wgrad_splits).  No float atomics; nothing depends on an
// address: bitwise reproducible, and the same bits for a caller's buffer on any 4-byte boundary.
#include "kernels.h"

namespace tdrn {

namespace {

constexpr int kDwThreads = 256;
constexpr int kDwGroups = 2048;        // 256 CUs x 8 workgroups: what the (channel, split) grid of the weight gradient aims at
constexpr int kDwMinPerSplit = 1024;   // a split is worth a workgroup from four elements a thread

// STRIDE in {1, 2}; total = planes * Ho * Wo
template <int STRIDE>
__global__ __launch_bounds__(kDwThreads) void dwconv_forward_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                    const float *__restrict__ bias, float *__restrict__ y, int C, int H, int W,
                                                                    int Ho, int Wo, long long total)
{
    const long long e = (long long)blockIdx.x * kDwThreads + threadIdx.x;
    if (e >= total) return;
    const int wo = (int)(e % Wo);
    const long long r = e / Wo;
    const int ho = (int)(r % Ho);
    const long long plane = r / Ho;
    const int c = (int)(plane % C);
    const float *xp = x + plane * ((long long)H * W), *wp = w + (long long)c * 9;
    const int h0 = ho * STRIDE - 1, w0 = wo * STRIDE - 1;
    float acc = bias ? bias[c] : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int h = h0 + i;
        if (h < 0 || h >= H) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int q = w0 + j;
            if (q < 0 || q >= W) continue;
            acc = fmaf(xp[(long long)h * W + q], wp[i * 3 + j], acc);
        }
    }
    y[e] = acc;
}

// the gather form over the rotated kernel; at stride 2 a tap takes part only where both quotients are whole.  total = planes * H * W
template <int STRIDE>
__global__ __launch_bounds__(kDwThreads) void dwconv_dgrad_kernel(const float *__restrict__ go, const float *__restrict__ w,
                                                                  float *__restrict__ gx, int C, int H, int W, int Ho, int Wo, long long total)
{
    const long long e = (long long)blockIdx.x * kDwThreads + threadIdx.x;
    if (e >= total) return;
    const int q = (int)(e % W);
    const long long r = e / W;
    const int h = (int)(r % H);
    const long long plane = r / H;
    const int c = (int)(plane % C);
    const float *gp = go + plane * ((long long)Ho * Wo), *wp = w + (long long)c * 9;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = h + 1 - i;
        if (a < 0 || (STRIDE == 2 && (a & 1))) continue;
        const int ho = a / STRIDE;
        if (ho >= Ho) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int b = q + 1 - j;
            if (b < 0 || (STRIDE == 2 && (b & 1))) continue;
            const int wo = b / STRIDE;
            if (wo >= Wo) continue;
            acc = fmaf(gp[(long long)ho * Wo + wo], wp[i * 3 + j], acc);
        }
    }
    gx[e] = acc;
}

// workgroup blockIdx.x = c * S + split -> partial[c][split][0..8] = sum go x(tap), [9] = sum go over K elements [k0, k1) of channel c
template <int STRIDE>
__global__ __launch_bounds__(kDwThreads) void dwconv_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ go,
                                                                  float *__restrict__ partial, int C, int H, int W, int Ho, int Wo, int S,
                                                                  long long per_split, long long K)
{
    __shared__ float red[kDwThreads / 64][10];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int c = (int)(blockIdx.x / (unsigned)S), split = (int)(blockIdx.x % (unsigned)S);
    const long long k0 = split * per_split, k1 = k0 + per_split < K ? k0 + per_split : K;
    const long long HoWo = (long long)Ho * Wo, HW = (long long)H * W;
    float acc[10];
#pragma unroll
    for (int z = 0; z < 10; ++z) acc[z] = 0.f;
    for (long long k = k0 + t; k < k1; k += kDwThreads) {
        const long long n = k / HoWo;
        const int p = (int)(k - n * HoWo), ho = p / Wo, wo = p - ho * Wo;
        const long long plane = n * C + c;
        const float g = go[plane * HoWo + p];
        const float *xp = x + plane * HW;
        const int h0 = ho * STRIDE - 1, w0 = wo * STRIDE - 1;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int h = h0 + i;
            if (h < 0 || h >= H) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int q = w0 + j;
                if (q < 0 || q >= W) continue;
                acc[i * 3 + j] = fmaf(g, xp[(long long)h * W + q], acc[i * 3 + j]);
            }
        }
        acc[9] += g;
    }
#pragma unroll
    for (int z = 0; z < 10; ++z) {
        float v = acc[z];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (lane == 0) red[wave][z] = v;
    }
    __syncthreads();
    if (t < 10) {
        float v = red[0][t];
#pragma unroll
        for (int k = 1; k < kDwThreads / 64; ++k) v += red[k][t];
        partial[(long long)blockIdx.x * 10 + t] = v;
    }
}

// grad_weight[c][z] += scale sum_split partial[c][split][z] (z < 9), grad_bias[c] (or null) += scale sum_split partial[c][split][9]
__global__ __launch_bounds__(kDwThreads) void dwconv_wgrad_reduce_kernel(const float *__restrict__ partial, float *__restrict__ gw,
                                                                         float *__restrict__ gb, long long C, int S, float scale)
{
    const long long total = C * 10;
    for (long long i = (long long)blockIdx.x * kDwThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kDwThreads) {
        const long long c = i / 10;
        const int z = (int)(i - c * 10);
        if (z == 9 && !gb) continue;
        const float *p = partial + c * S * 10 + z;
        float s = 0.f;
        for (int k = 0; k < S; ++k) s += p[(long long)k * 10];
        float *d = z == 9 ? gb + c : gw + c * 9 + z;
        *d = fmaf(scale, s, *d);
    }
}

unsigned flat_grid(long long total) { return (unsigned)((total + kDwThreads - 1) / kDwThreads); }

}  // namespace

void dwconv_wgrad_splits(int N, int C, int Ho, int Wo, int &splits, long long &per_split)
{
    const long long K = (long long)N * Ho * Wo;
    long long s = (kDwGroups + (long long)C - 1) / C;                       // enough (channel, split) workgroups to fill the chip ...
    const long long by_k = (K + kDwMinPerSplit - 1) / kDwMinPerSplit;       // ... of at least kDwMinPerSplit elements each
    if (s > by_k) s = by_k;
    if (s < 1) s = 1;
    per_split = (K + s - 1) / s;
    splits = (int)((K + per_split - 1) / per_split);                        // no empty split
}

size_t dwconv_workspace_bytes(int N, int C, int Ho, int Wo)
{
    int splits;
    long long per_split;
    dwconv_wgrad_splits(N, C, Ho, Wo, splits, per_split);
    return align_up((size_t)C * splits * 10 * 4, 256);
}

int launch_dwconv_forward(const float *x, const float *w, const float *bias, float *y, int N, int C, int H, int W, int stride, int Ho, int Wo,
                          hipStream_t s)
{
    const long long total = (long long)N * C * Ho * Wo;
    if (stride == 1) hipLaunchKernelGGL(dwconv_forward_kernel<1>, dim3(flat_grid(total)), dim3(kDwThreads), 0, s, x, w, bias, y, C, H, W, Ho, Wo, total);
    else hipLaunchKernelGGL(dwconv_forward_kernel<2>, dim3(flat_grid(total)), dim3(kDwThreads), 0, s, x, w, bias, y, C, H, W, Ho, Wo, total);
    return hip_status(hipGetLastError());
}

int launch_dwconv_backward_input(const float *go, const float *w, float *gx, int N, int C, int H, int W, int stride, int Ho, int Wo, hipStream_t s)
{
    const long long total = (long long)N * C * H * W;
    if (stride == 1) hipLaunchKernelGGL(dwconv_dgrad_kernel<1>, dim3(flat_grid(total)), dim3(kDwThreads), 0, s, go, w, gx, C, H, W, Ho, Wo, total);
    else hipLaunchKernelGGL(dwconv_dgrad_kernel<2>, dim3(flat_grid(total)), dim3(kDwThreads), 0, s, go, w, gx, C, H, W, Ho, Wo, total);
    return hip_status(hipGetLastError());
}

int launch_dwconv_backward_parameters(const float *x, const float *go, float *gw, float *gb, int N, int C, int H, int W, int stride, int Ho,
                                      int Wo, float scale, void *ws, hipStream_t s)
{
    int S;
    long long per_split;
    dwconv_wgrad_splits(N, C, Ho, Wo, S, per_split);
    const long long K = (long long)N * Ho * Wo;
    float *partial = (float *)ws;
    const dim3 grid((unsigned)((long long)C * S));
    if (stride == 1) hipLaunchKernelGGL(dwconv_wgrad_kernel<1>, grid, dim3(kDwThreads), 0, s, x, go, partial, C, H, W, Ho, Wo, S, per_split, K);
    else hipLaunchKernelGGL(dwconv_wgrad_kernel<2>, grid, dim3(kDwThreads), 0, s, x, go, partial, C, H, W, Ho, Wo, S, per_split, K);
    TDRN_HIP_TRY(hipGetLastError());
    const long long total = (long long)C * 10;
    const unsigned blocks = (unsigned)((total + kDwThreads - 1) / kDwThreads > kDwGroups ? kDwGroups : (total + kDwThreads - 1) / kDwThreads);
    hipLaunchKernelGGL(dwconv_wgrad_reduce_kernel, dim3(blocks), dim3(kDwThreads), 0, s, (const float *)partial, gw, gb, (long long)C, S, scale);
    return hip_status(hipGetLastError());
}

}  // namespace tdrn
