// deform_bwd.hip -- deformable convolution v1 backward (fp32), the gradients of the forward in deform.hip:
//   grad_input  += col2im of grad_col        utils/deformconv/deform_conv_cuda_kernel.cu:247-298 (deformable_col2im)
//   grad_offset  = sum_c grad_col * d sample  deform_conv_cuda_kernel.cu:337-400 (deformable_col2im_coord)
//   grad_weight += scale * grad_out * cols^T  deform_conv_cuda.c:327-409 (deform_conv_backward_parameters_cuda)
// where grad_col = W^T * grad_out (deform_conv_cuda.c:280-292).  The sampling rule (rejection, the [H-1, H) clamp, fp32
// coordinates) is the forward's own (deform_sampler.h), so away from its measure-zero points these are exactly the
// derivatives of what the forward computes.
//
// Layouts (workspace): the input as NHWC fp32 with every deformable group's channels padded to a multiple of 64
// (cpg64), so one wave's 64 lanes are 64 consecutive channels of one group; the grad_input accumulator in the same
// layout.  Kernels:
//   deform_bwd_data_kernel   one workgroup = PX consecutive output pixels x all taps x all channels.  Per tap and
//                            64-channel chunk a wave forms grad_col (K = Cout, fp32 FMA against an LDS tile of grad_out),
//                            re-gathers the forward's four corner rows, adds grad_col * w_k into the NHWC accumulator
//                            with one 256-byte float-atomic wave-instruction per corner, and reduces the offset
//                            derivative over its 64 channels in registers; the chunks of a group are summed in LDS in a
//                            fixed order and grad_offset is stored once (no atomics: bitwise reproducible).
//   deform_bwd_input_add     NHWC accumulator -> the caller's NCHW grad_input (+=), through a 32x32 LDS transpose.
//   deform_bwd_weight_kernel K split over pixel ranges: every split gathers its columns exactly as the forward does and
//                            writes an fp32 partial slab [split][tap][Cout][Cpad];
//   deform_bwd_weight_reduce sums the slabs in split order and applies += scale * into OIHW (bitwise reproducible).
#include <algorithm>

#include "deform_sampler.h"
#include "kernels.h"

namespace tdrn {

namespace {

struct BwdGeomK {
    int N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, G;
    int Ho, Wo, HoWo, M, taps, cpg, cpg64, Cpad, cpc, nchunks, offC;
};

BwdGeomK kgeom(const DeformBwdGeom &g)
{
    BwdGeomK k;
    k.N = g.N; k.Cin = g.Cin; k.H = g.H; k.W = g.W; k.Cout = g.Cout; k.kh = g.kh; k.kw = g.kw;
    k.sh = g.sh; k.sw = g.sw; k.ph = g.ph; k.pw = g.pw; k.dh = g.dh; k.dw = g.dw; k.G = g.G;
    k.Ho = g.Ho; k.Wo = g.Wo; k.HoWo = g.Ho * g.Wo; k.M = g.N * g.Ho * g.Wo; k.taps = g.kh * g.kw;
    k.cpg = g.Cin / g.G; k.cpg64 = deform_bwd_cpg64(g); k.Cpad = k.cpg64 * g.G; k.cpc = k.cpg64 / 64;
    k.nchunks = g.G * k.cpc; k.offC = g.G * 2 * k.taps;
    return k;
}

// NV (power of two <= 64) values per lane -> lane l holds the sum over all 64 lanes of value (l & (NV-1)).
// Butterfly over the lane bits >= NV, then recursive halving: 2 NV - 1 + (64 / NV - 1) NV shuffles, fixed order.
template <int NV> __device__ __forceinline__ float wave_reduce_scatter(float (&v)[NV], int lane)
{
#pragma unroll
    for (int s = 32; s >= NV; s >>= 1)
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] += __shfl_xor(v[i], s);
#pragma unroll
    for (int s = NV / 2; s >= 1; s >>= 1) {
        const bool upper = (lane & s) != 0;
#pragma unroll
        for (int i = 0; i < s; ++i) {
            const float keep = upper ? v[i + s] : v[i], send = upper ? v[i] : v[i + s];
            v[i] = keep + __shfl_xor(send, s);
        }
    }
    return v[0];
}

}  // namespace

int deform_bwd_cpg64(const DeformBwdGeom &g) { return (int)align_up((size_t)(g.Cin / g.G), 64); }

// ---------------------------------------------------------------------------------------------
// grad_input (into the NHWC accumulator) and grad_offset
// ---------------------------------------------------------------------------------------------
struct BwdCorner { int o[4]; };          // element offsets of the four corners' group-channel base; o[0] < 0: tap rejected

template <int PX>
__global__ __launch_bounds__(256) void deform_bwd_data_kernel(const float *__restrict__ in, const float *__restrict__ off,
                                                              const float *__restrict__ gout, const float *__restrict__ wr,
                                                              float *__restrict__ gin, float *__restrict__ goff, const BwdGeomK g)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *s_go = smem;                                             // [Cout][PX]  grad_out tile
    BwdCorner *s_cr = (BwdCorner *)(s_go + g.Cout * PX);            // [G][PX]     corners
    float2 *s_fr = (float2 *)(s_cr + g.G * PX);                     // [G][PX]     (lh, lw)
    float *s_part = (float *)(s_fr + g.G * PX);                     // [nchunks][2 PX]  per-chunk offset-gradient sums
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.x * PX;

    for (int i = t; i < g.Cout * PX; i += 256) {
        const int co = i / PX, p = i - co * PX, m = m0 + p;
        float v = 0.f;
        if (m < g.M) {
            const int n = m / g.HoWo, pix = m - n * g.HoWo;
            v = gout[((size_t)n * g.Cout + co) * g.HoWo + pix];
        }
        s_go[i] = v;
    }

    for (int tap = 0; tap < g.taps; ++tap) {
        const int ti = tap / g.kw, tj = tap - ti * g.kw;
        for (int i = t; i < g.G * PX; i += 256) {
            const int gg = i / PX, p = i - gg * PX, m = m0 + p;
            BwdCorner c;
            c.o[0] = c.o[1] = c.o[2] = c.o[3] = -1;
            float2 fr = make_float2(0.f, 0.f);
            if (m < g.M) {
                const int n = m / g.HoWo, pix = m - n * g.HoWo, ho = pix / g.Wo, wo = pix - ho * g.Wo;
                const float *op = off + ((size_t)n * g.offC + gg * 2 * g.taps + 2 * tap) * g.HoWo + pix;
                int r0, r1, q0, q1;
                float lh, lw;
                if (deform_sample(g.H, g.W, ho * g.sh - g.ph, wo * g.sw - g.pw, ti * g.dh, tj * g.dw, op[0], op[g.HoWo], r0, r1, q0,
                                  q1, lh, lw)) {
                    const int base = n * g.H * g.W, cb = gg * g.cpg64;
                    c.o[0] = (base + r0 * g.W + q0) * g.Cpad + cb;
                    c.o[1] = (base + r0 * g.W + q1) * g.Cpad + cb;
                    c.o[2] = (base + r1 * g.W + q0) * g.Cpad + cb;
                    c.o[3] = (base + r1 * g.W + q1) * g.Cpad + cb;
                    fr = make_float2(lh, lw);
                }
            }
            s_cr[i] = c;
            s_fr[i] = fr;
        }
        __syncthreads();

        for (int chunk = wave; chunk < g.nchunks; chunk += 4) {
            const int gg = chunk / g.cpc, cl = (chunk - gg * g.cpc) * 64 + lane;     // channel inside the group (padded)
            // grad_col[p] of channel gg*cpg64 + cl at this tap: sum_co W[co][tap][c] * grad_out[co][p]
            float acc[PX];
#pragma unroll
            for (int p = 0; p < PX; ++p) acc[p] = 0.f;
            const float *wp = wr + (size_t)tap * g.Cpad + gg * g.cpg64 + cl;
            const size_t wstride = (size_t)g.taps * g.Cpad;
            for (int co = 0; co < g.Cout; ++co) {
                const float wv = wp[co * wstride];
                const f32x4 *gp = (const f32x4 *)(s_go + co * PX);
#pragma unroll
                for (int q = 0; q < PX / 4; ++q) {
                    const f32x4 gq = gp[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * q + e] = fmaf(wv, gq[e], acc[4 * q + e]);
                }
            }
            float red[2 * PX];
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const BwdCorner c = s_cr[gg * PX + p];
                red[2 * p] = 0.f;
                red[2 * p + 1] = 0.f;
                if (c.o[0] >= 0) {                                          // (uniform across the wave)
                    const float2 fr = s_fr[gg * PX + p];
                    const float lh = fr.x, lw = fr.y, hh = 1.f - lh, hw = 1.f - lw;
                    const float v1 = in[c.o[0] + cl], v2 = in[c.o[1] + cl], v3 = in[c.o[2] + cl], v4 = in[c.o[3] + cl];
                    const float a = acc[p];
                    atomicAdd(gin + c.o[0] + cl, a * (hh * hw));
                    atomicAdd(gin + c.o[1] + cl, a * (hh * lw));
                    atomicAdd(gin + c.o[2] + cl, a * (lh * hw));
                    atomicAdd(gin + c.o[3] + cl, a * (lh * lw));
                    // d sample / d h, d sample / d w: zero inside the clamp band (the corners coincide there)
                    red[2 * p] = a * (hw * (v3 - v1) + lw * (v4 - v2));
                    red[2 * p + 1] = a * (hh * (v2 - v1) + lh * (v4 - v3));
                }
            }
            const float r = wave_reduce_scatter<2 * PX>(red, lane);
            if (lane < 2 * PX) s_part[chunk * 2 * PX + lane] = r;
        }
        __syncthreads();

        // grad_offset (NCHW, channel gg*2*taps + 2*tap + axis): the group's chunks in a fixed order, one store
        for (int i = t; i < g.G * 2 * PX; i += 256) {
            const int gg = i / (2 * PX), k = i - gg * 2 * PX, p = k >> 1, axis = k & 1, m = m0 + p;
            if (m < g.M) {
                float s = 0.f;
                for (int cc = 0; cc < g.cpc; ++cc) s += s_part[(gg * g.cpc + cc) * 2 * PX + k];
                const int n = m / g.HoWo, pix = m - n * g.HoWo;
                goff[((size_t)n * g.offC + gg * 2 * g.taps + 2 * tap + axis) * g.HoWo + pix] = s;
            }
        }
        __syncthreads();
    }
}

template <int PX> static size_t data_lds_bytes(const BwdGeomK &k)
{
    return (size_t)k.Cout * PX * 4 + (size_t)k.G * PX * (sizeof(BwdCorner) + sizeof(float2)) + (size_t)k.nchunks * 2 * PX * 4;
}
constexpr size_t kBwdMaxLds = 64 * 1024;

int deform_bwd_data_px(const DeformBwdGeom &g)
{
    const BwdGeomK k = kgeom(g);
    if ((long long)g.N * g.H * g.W * k.Cpad >= (1ll << 31)) return 0;           // 32-bit element offsets
    if (data_lds_bytes<16>(k) <= kBwdMaxLds) return 16;
    if (data_lds_bytes<8>(k) <= kBwdMaxLds) return 8;
    return 0;
}

int launch_deform_bwd_data(const DeformBwdGeom &g, const float *in_nhwc, const float *off, const float *gout, const float *wr,
                           float *gin_nhwc, float *goff, hipStream_t s)
{
    const BwdGeomK k = kgeom(g);
    const int px = deform_bwd_data_px(g);
    if (px == 0) return TDRN_E_UNSUPPORTED;
    const dim3 grid((unsigned)cdiv(k.M, px));
    if (px == 16)
        hipLaunchKernelGGL((deform_bwd_data_kernel<16>), grid, dim3(256), data_lds_bytes<16>(k), s, in_nhwc, off, gout, wr, gin_nhwc, goff, k);
    else
        hipLaunchKernelGGL((deform_bwd_data_kernel<8>), grid, dim3(256), data_lds_bytes<8>(k), s, in_nhwc, off, gout, wr, gin_nhwc, goff, k);
    return hip_status(hipGetLastError());
}

// NHWC (group-padded) accumulator -> NCHW grad_input, +=
__global__ __launch_bounds__(256) void deform_bwd_input_add_kernel(const float *__restrict__ gin, float *__restrict__ out, int Cin,
                                                                   int HW, int cpg, int cpg64, int Cpad)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int hw0 = blockIdx.x * 32, c0 = blockIdx.y * 32, n = blockIdx.z;
#pragma unroll
    for (int r = 0; r < 32; r += 8) {
        const int hw = hw0 + ty + r, c = c0 + tx;
        float v = 0.f;
        if (hw < HW && c < Cin) v = gin[((size_t)n * HW + hw) * Cpad + (c / cpg) * cpg64 + c % cpg];
        tile[ty + r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 32; r += 8) {
        const int c = c0 + ty + r, hw = hw0 + tx;
        if (hw < HW && c < Cin) out[((size_t)n * Cin + c) * HW + hw] += tile[tx][ty + r];
    }
}

int launch_deform_bwd_input_add(const DeformBwdGeom &g, const float *gin_nhwc, float *grad_input, hipStream_t s)
{
    const BwdGeomK k = kgeom(g);
    const int HW = g.H * g.W;
    const dim3 grid((unsigned)cdiv(HW, 32), (unsigned)cdiv(g.Cin, 32), (unsigned)g.N);
    hipLaunchKernelGGL(deform_bwd_input_add_kernel, grid, dim3(256), 0, s, gin_nhwc, grad_input, g.Cin, HW, k.cpg, k.cpg64, k.Cpad);
    return hip_status(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// grad_weight: split-K partial slabs, then a fixed-order sum
// ---------------------------------------------------------------------------------------------
// one workgroup = (pixel split, tap, 64-channel chunk, block of 4 NJ output channels); lane = channel, wave w owns
// output channels cob + w NJ + j.  Per step of 32 pixels: the grad_out tile [32][4 NJ] and the gathered column tile [32][64]
// (wave w samples pixels 8w .. 8w+7, the forward's blend order) go through LDS, then 32 x NJ FMAs per lane.
template <int NJ>
__global__ __launch_bounds__(256) void deform_bwd_weight_kernel(const float *__restrict__ in, const float *__restrict__ off,
                                                                const float *__restrict__ gout, float *__restrict__ slab, const BwdGeomK g,
                                                                int per_split)
{
    constexpr int PS = 32, COB = 4 * NJ;
    __shared__ __attribute__((aligned(16))) float s_col[PS][64];
    __shared__ __attribute__((aligned(16))) float s_go[PS][COB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int split = blockIdx.x, tap = blockIdx.y;
    const int chunk = (int)blockIdx.z % g.nchunks, cob = ((int)blockIdx.z / g.nchunks) * COB;
    const int gg = chunk / g.cpc, ch = gg * g.cpg64 + (chunk - gg * g.cpc) * 64 + lane;
    const int ti = tap / g.kw, tj = tap - ti * g.kw;
    const int mbeg = split * per_split, mend = min(g.M, mbeg + per_split);
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = 0.f;

    for (int mb = mbeg; mb < mend; mb += PS) {
        for (int i = t; i < PS * COB; i += 256) {
            const int c = i / PS, p = i - c * PS, m = mb + p, co = cob + c;
            float v = 0.f;
            if (m < mend && co < g.Cout) {
                const int n = m / g.HoWo, pix = m - n * g.HoWo;
                v = gout[((size_t)n * g.Cout + co) * g.HoWo + pix];
            }
            s_go[p][c] = v;
        }
#pragma unroll 2
        for (int q = 0; q < PS / 4; ++q) {
            const int p = wave * (PS / 4) + q, m = mb + p;
            float v = 0.f;
            if (m < mend) {
                const int n = m / g.HoWo, pix = m - n * g.HoWo, ho = pix / g.Wo, wo = pix - ho * g.Wo;
                const float *op = off + ((size_t)n * g.offC + gg * 2 * g.taps + 2 * tap) * g.HoWo + pix;
                int r0, r1, q0, q1;
                float lh, lw;
                if (deform_sample(g.H, g.W, ho * g.sh - g.ph, wo * g.sw - g.pw, ti * g.dh, tj * g.dw, op[0], op[g.HoWo], r0, r1, q0, q1,
                                  lh, lw)) {
                    const float hh = 1.f - lh, hw = 1.f - lw;
                    const float *b = in + (size_t)n * g.H * g.W * g.Cpad + ch;
                    const float v1 = b[(r0 * g.W + q0) * g.Cpad], v2 = b[(r0 * g.W + q1) * g.Cpad];
                    const float v3 = b[(r1 * g.W + q0) * g.Cpad], v4 = b[(r1 * g.W + q1) * g.Cpad];
                    v = fmaf(lh * lw, v4, fmaf(lh * hw, v3, fmaf(hh * lw, v2, (hh * hw) * v1)));
                }
            }
            s_col[p][lane] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int p = 0; p < PS; ++p) {
            const float cv = s_col[p][lane];
            const f32x4 *gp = (const f32x4 *)&s_go[p][wave * NJ];
#pragma unroll
            for (int q = 0; q < NJ / 4; ++q) {
                const f32x4 gq = gp[q];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * q + e] = fmaf(gq[e], cv, acc[4 * q + e]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int co = cob + wave * NJ + j;
        if (co < g.Cout) slab[(((size_t)split * g.taps + tap) * g.Cout + co) * g.Cpad + ch] = acc[j];
    }
}

// grad_weight[co][c][tap] += scale * sum_{split = 0..S-1} slab[split][tap][co][c]   (thread index: c fastest -> coalesced slab reads)
__global__ __launch_bounds__(256) void deform_bwd_weight_reduce_kernel(const float *__restrict__ slab, float *__restrict__ gw, const BwdGeomK g,
                                                                       int S, float scale)
{
    const long long total = (long long)g.taps * g.Cout * g.Cin;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % g.Cin);
        const long long r = i / g.Cin;
        const int co = (int)(r % g.Cout), tap = (int)(r / g.Cout);
        const size_t cp = (size_t)(c / g.cpg) * g.cpg64 + c % g.cpg;
        const size_t sstride = (size_t)g.taps * g.Cout * g.Cpad;
        const float *sp = slab + ((size_t)tap * g.Cout + co) * g.Cpad + cp;
        float s = 0.f;
        for (int k = 0; k < S; ++k) s += sp[k * sstride];
        float *d = gw + ((size_t)co * g.Cin + c) * g.taps + tap;
        *d = fmaf(scale, s, *d);
    }
}

static int weight_nj(const DeformBwdGeom &g) { return g.Cout <= 32 ? 8 : 32; }

void deform_bwd_weight_splits(const DeformBwdGeom &g, int &splits, int &per_split)
{
    const BwdGeomK k = kgeom(g);
    const int cob = 4 * weight_nj(g);
    const int per_split_wgs = k.taps * k.nchunks * cdiv(g.Cout, cob);
    int S = cdiv(2048, per_split_wgs);
    const int max_s = cdiv(k.M, 128);                 // at least four 32-pixel steps per split
    S = S < 1 ? 1 : (S > max_s ? max_s : S);
    per_split = (int)align_up((size_t)cdiv(k.M, S), 32);
    splits = cdiv(k.M, per_split);
}

int launch_deform_bwd_weight(const DeformBwdGeom &g, const float *in_nhwc, const float *off, const float *gout, float *slab, float *grad_weight,
                             float scale, hipStream_t s)
{
    const BwdGeomK k = kgeom(g);
    int S, per_split;
    deform_bwd_weight_splits(g, S, per_split);
    const int nj = weight_nj(g);
    const dim3 grid((unsigned)S, (unsigned)k.taps, (unsigned)(k.nchunks * cdiv(g.Cout, 4 * nj)));
    if (nj == 8)
        hipLaunchKernelGGL((deform_bwd_weight_kernel<8>), grid, dim3(256), 0, s, in_nhwc, off, gout, slab, k, per_split);
    else
        hipLaunchKernelGGL((deform_bwd_weight_kernel<32>), grid, dim3(256), 0, s, in_nhwc, off, gout, slab, k, per_split);
    TDRN_HIP_TRY(hipGetLastError());
    const long long total = (long long)k.taps * g.Cout * g.Cin;
    hipLaunchKernelGGL(deform_bwd_weight_reduce_kernel, stride_grid(total, 4096), dim3(256), 0, s, slab, grad_weight, k, S, scale);
    return hip_status(hipGetLastError());
}

}  // namespace tdrn
