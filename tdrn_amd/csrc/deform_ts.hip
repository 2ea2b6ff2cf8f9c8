// deform_ts.hip -- "transform, then sample": the second algorithm of the differentiable deformable conv v1 (tdrn_hip.h section i-l),
// one deformable group, 16-bit compute types.  A deformable conv is linear in the sampled values, so the 1x1 product with the weight
// of every tap can be formed on the UN-deformed pixels first and the bilinear sampling then works on rows of Cout values, not Cin:
//   Y_t[n,co,q]      = sum_c W[co,c,t] X[n,c,q]                       1x1 GEMM over input pixels (launch_conv, 16-bit result)
//   out[n,co,p]      = sum_t sum_q b(p,t,q) Y_t[n,co,q]               deform_ts_sample_kernel
//   grad_offset[p,t] = sum_co gO[n,co,p] d/dpos sum_q b(p,t,q) Y_t    deform_ts_backward_kernel (four Y corners)
//   Z_t[n,co,q]      = sum_p b(p,t,q) gO[n,co,p]                      deform_ts_backward_kernel (fp32 atomics), rounded once to 16 bit
//   grad_input       = sum_t sum_co W[co,c,t] Z_t[n,co,q]             1x1 GEMM, K = T Cout (launch_conv)
//   grad_weight      = sum_{n,q} Z_t[n,co,q] X[n,c,q]                 1x1 weight-gradient GEMM, K = N H W (launch_conv_wgrad_slabs)
// b(p,t,q): the bilinear coefficient of input pixel q for the sample of output pixel p at tap t, by deform_sample (deform_sampler.h):
// rejection, the [H-1, H) clamp band and the fp32 coordinates are the gather op's own.
//
// Layout.  Y and Z are pixel-major over INPUT pixels: row q = [tap][Cp] with Cp = Cout rounded up to 8 (16-byte pieces), the row padded
// with zeros to YC = a multiple of kChanPad columns, so launch_conv writes Y, and reads Z, as an NHWC tensor of YC channels and
// launch_conv_wgrad_slabs takes Z as its "grad_output".  Row indices are 64-bit.
// Kernels (one wave = one output pixel, lane l = columns l, l + 64, ... of a row: 64 lanes address consecutive columns):
//   deform_ts_sample_kernel    per tap the geometry once, four corner rows of Y blended with the fp32 weights (fmaf chain in corner
//                              order 1..4), taps summed in tap order in fp32; result [pixel][Cout] fp32.  No atomics.
//   deform_ts_backward_kernel  gO[p][.] loaded once; per tap the geometry once; grad_offset = two sums over the Cout columns (a lane's
//                              columns ascending, then a butterfly over the lanes: a fixed order), one-sided derivative at integers,
//                              zero inside the clamp band (the corners coincide there), stored once; Z[q][t][.] += b gO[p][.], one
//                              contiguous fp32 atomic wave-instruction per corner row with a non-zero coefficient.
//   deform_ts_round_kernel     Z fp32 -> 16 bit, one rounding to nearest even
//   TsRepackMap (pack_kernel)  OIHW fp32 -> the two 1x1 matrices: [t Cp + co][c] (Y) and [c][t Cp + co] (grad_input)
//   deform_ts_wgrad_reduce     grad_weight[co][c][t] = the slabs' rows t Cp + co summed in split order (overwrites): slab_reduce_kernel
#include "deform_sampler.h"
#include "kernels.h"

namespace tdrn {

namespace {

struct TsGeomK {
    int N, H, W, Cout, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, HoWo, M, taps, Cp, YC, offC;
};

TsGeomK ts_kgeom(const DeformBwdGeom &g)
{
    TsGeomK k;
    k.N = g.N; k.H = g.H; k.W = g.W; k.Cout = g.Cout; k.kw = g.kw; k.sh = g.sh; k.sw = g.sw; k.ph = g.ph; k.pw = g.pw;
    k.dh = g.dh; k.dw = g.dw; k.Ho = g.Ho; k.Wo = g.Wo; k.HoWo = g.Ho * g.Wo; k.M = g.N * g.Ho * g.Wo; k.taps = g.kh * g.kw;
    k.Cp = deform_ts_cp(g.Cout); k.YC = deform_ts_cols(g); k.offC = 2 * k.taps;
    return k;
}

// what a wave knows of its output pixel
struct TsPixel { int n, pix, h_in, w_in; };

__device__ __forceinline__ TsPixel ts_pixel(const TsGeomK &g, int m)
{
    TsPixel p;
    p.n = m / g.HoWo;
    p.pix = m - p.n * g.HoWo;
    const int ho = p.pix / g.Wo, wo = p.pix - ho * g.Wo;
    p.h_in = ho * g.sh - g.ph;
    p.w_in = wo * g.sw - g.pw;
    return p;
}

template <typename DT, int NJ>
__global__ __launch_bounds__(256) void deform_ts_sample_kernel(const DT *__restrict__ y, const float *__restrict__ off,
                                                               float *__restrict__ out, const TsGeomK g)
{
    const int lane = threadIdx.x & 63;
    const int m = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (m >= g.M) return;                                            // (wave-uniform; the kernel has no barrier)
    const TsPixel px = ts_pixel(g, m);
    const float *op = off + (size_t)px.n * g.offC * g.HoWo + px.pix;
    const DT *yb = y + (size_t)px.n * g.H * g.W * g.YC + lane;
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
    for (int t = 0; t < g.taps; ++t) {
        const int ti = t / g.kw, tj = t - ti * g.kw;
        int r0, r1, q0, q1;
        float lh, lw;
        if (!deform_sample(g.H, g.W, px.h_in, px.w_in, ti * g.dh, tj * g.dw, op[(size_t)(2 * t) * g.HoWo],
                           op[(size_t)(2 * t + 1) * g.HoWo], r0, r1, q0, q1, lh, lw))
            continue;
        const float hh = 1.f - lh, hw = 1.f - lw;
        const float b1 = hh * hw, b2 = hh * lw, b3 = lh * hw, b4 = lh * lw;
        const int tc = t * g.Cp;
        const DT *p1 = yb + (size_t)(r0 * g.W + q0) * g.YC + tc, *p2 = yb + (size_t)(r0 * g.W + q1) * g.YC + tc;
        const DT *p3 = yb + (size_t)(r1 * g.W + q0) * g.YC + tc, *p4 = yb + (size_t)(r1 * g.W + q1) * g.YC + tc;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (lane + 64 * j < g.Cout) {
                const float v1 = to_f32<DT>(p1[64 * j]), v2 = to_f32<DT>(p2[64 * j]), v3 = to_f32<DT>(p3[64 * j]), v4 = to_f32<DT>(p4[64 * j]);
                const float v = fmaf(b4, v4, fmaf(b3, v3, fmaf(b2, v2, b1 * v1)));
                acc[j] = acc[j] + v;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (lane + 64 * j < g.Cout) out[(size_t)m * g.Cout + lane + 64 * j] = acc[j];
}

// y == null: no grad_offset (goff is not written); z == null: no scatter
template <typename DT, int NJ>
__global__ __launch_bounds__(256) void deform_ts_backward_kernel(const DT *__restrict__ y, const float *__restrict__ off,
                                                                 const float *__restrict__ go, float *__restrict__ z,
                                                                 float *__restrict__ goff, const TsGeomK g)
{
    const int lane = threadIdx.x & 63;
    const int m = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (m >= g.M) return;                                            // (wave-uniform; the kernel has no barrier)
    const TsPixel px = ts_pixel(g, m);
    const float *op = off + (size_t)px.n * g.offC * g.HoWo + px.pix;
    const size_t img = (size_t)px.n * g.H * g.W * g.YC + lane;
    float gv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) gv[j] = lane + 64 * j < g.Cout ? go[(size_t)m * g.Cout + lane + 64 * j] : 0.f;
    for (int t = 0; t < g.taps; ++t) {
        const int ti = t / g.kw, tj = t - ti * g.kw;
        int r0, r1, q0, q1;
        float lh, lw;
        const bool ok = deform_sample(g.H, g.W, px.h_in, px.w_in, ti * g.dh, tj * g.dw, op[(size_t)(2 * t) * g.HoWo],
                                      op[(size_t)(2 * t + 1) * g.HoWo], r0, r1, q0, q1, lh, lw);
        float sum_h = 0.f, sum_w = 0.f;                               // a rejected tap has a zero offset gradient
        if (ok) {                                                     // (wave-uniform)
            const float hh = 1.f - lh, hw = 1.f - lw;
            const int tc = t * g.Cp;
            const size_t e1 = img + (size_t)(r0 * g.W + q0) * g.YC + tc, e2 = img + (size_t)(r0 * g.W + q1) * g.YC + tc;
            const size_t e3 = img + (size_t)(r1 * g.W + q0) * g.YC + tc, e4 = img + (size_t)(r1 * g.W + q1) * g.YC + tc;
            if (y) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    if (lane + 64 * j < g.Cout) {
                        const float v1 = to_f32<DT>(y[e1 + 64 * j]), v2 = to_f32<DT>(y[e2 + 64 * j]);
                        const float v3 = to_f32<DT>(y[e3 + 64 * j]), v4 = to_f32<DT>(y[e4 + 64 * j]);
                        // d sample / d h, d sample / d w: zero inside the clamp band (the corners coincide there)
                        sum_h += gv[j] * (hw * (v3 - v1) + lw * (v4 - v2));
                        sum_w += gv[j] * (hh * (v2 - v1) + lh * (v4 - v3));
                    }
                }
            }
            if (z) {
                const float b1 = hh * hw, b2 = hh * lw, b3 = lh * hw, b4 = lh * lw;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    if (lane + 64 * j < g.Cout) {
                        if (b1 != 0.f) atomicAdd(z + e1 + 64 * j, b1 * gv[j]);
                        if (b2 != 0.f) atomicAdd(z + e2 + 64 * j, b2 * gv[j]);
                        if (b3 != 0.f) atomicAdd(z + e3 + 64 * j, b3 * gv[j]);
                        if (b4 != 0.f) atomicAdd(z + e4 + 64 * j, b4 * gv[j]);
                    }
                }
            }
        }
        if (y) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                sum_h += __shfl_xor(sum_h, s);
                sum_w += __shfl_xor(sum_w, s);
            }
            if (lane == 0) {
                float *d = goff + ((size_t)px.n * g.offC + 2 * t) * g.HoWo + px.pix;
                d[0] = sum_h;
                d[g.HoWo] = sum_w;
            }
        }
    }
}

// 8 consecutive fp32 -> 16 bytes of DT; `groups` = elements / 8
template <typename DT>
__global__ __launch_bounds__(256) void deform_ts_round_kernel(const float *__restrict__ in, char *__restrict__ out, long long groups)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (long long)gridDim.x * blockDim.x) {
        const f32x4 a = *(const f32x4 *)(in + 8 * i), b = *(const f32x4 *)(in + 8 * i + 4);
        const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        *(u32x4 *)(out + 16 * i) = pack16<DT>(v);
    }
}

// OIHW fp32 -> DGRAD ? out[c][t Cp + co] ([Npad][YC]) : out[t Cp + co][c] ([Npad][Cin]); everything that is no weight is zero
template <bool DGRAD> struct TsRepackMap {
    const float *w;
    int Cout, Cin, taps, Cp, inner;      // inner = DGRAD ? YC : Cin
    __device__ float operator()(long long i) const
    {
        const int a = (int)(i % inner), r = (int)(i / inner);
        const int col = DGRAD ? a : r, c = DGRAD ? r : a;
        const int t = col / Cp, co = col - t * Cp;
        return (t < taps && co < Cout && c < Cin) ? w[((size_t)co * Cin + c) * taps + t] : 0.f;
    }
};

}  // namespace

int deform_ts_cp(int Cout) { return (int)align_up((size_t)Cout, 8); }

int deform_ts_cols(const DeformBwdGeom &g) { return (int)align_up((size_t)g.kh * g.kw * deform_ts_cp(g.Cout), kChanPad); }

int launch_deform_ts_sample(const DeformBwdGeom &g, const void *y, const float *off, float *out_nhwc, int dtype, hipStream_t s)
{
    if (g.G != 1 || g.Cout < 1 || g.Cout > 256 || !y || !off || !out_nhwc) return TDRN_E_UNSUPPORTED;
    const TsGeomK k = ts_kgeom(g);
    return dispatch_dtype16(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        return dispatch_1to4(cdiv(k.Cout, 64), [&](auto nj) {       // NJ: columns per lane
            hipLaunchKernelGGL((deform_ts_sample_kernel<DT, decltype(nj)::value>), dim3((unsigned)cdiv(k.M, 4)), dim3(256), 0, s, (const DT *)y, off,
                               out_nhwc, k);
            return hip_status(hipGetLastError());
        });
    });
}

int launch_deform_ts_backward(const DeformBwdGeom &g, const void *y, const float *off, const float *go_nhwc, float *z, float *goff,
                              int dtype, hipStream_t s)
{
    if (g.G != 1 || g.Cout < 1 || g.Cout > 256 || !off || !go_nhwc || (y == nullptr) != (goff == nullptr)) return TDRN_E_UNSUPPORTED;
    if (!y && !z) return TDRN_OK;
    const TsGeomK k = ts_kgeom(g);
    return dispatch_dtype16(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        return dispatch_1to4(cdiv(k.Cout, 64), [&](auto nj) {       // NJ: columns per lane
            hipLaunchKernelGGL((deform_ts_backward_kernel<DT, decltype(nj)::value>), dim3((unsigned)cdiv(k.M, 4)), dim3(256), 0, s, (const DT *)y,
                               off, go_nhwc, z, goff, k);
            return hip_status(hipGetLastError());
        });
    });
}

int launch_deform_ts_round(const float *in, void *out, long long elems, int dtype, hipStream_t s)
{
    if (elems % 8 || dtype == TDRN_F32) return TDRN_E_UNSUPPORTED;
    if (elems == 0) return TDRN_OK;
    return dispatch_dtype16(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        hipLaunchKernelGGL((deform_ts_round_kernel<DT>), stride_grid(elems / 8), dim3(256), 0, s, in, (char *)out, elems / 8);
        return hip_status(hipGetLastError());
    });
}

int launch_deform_ts_repack(const DeformBwdGeom &g, const float *w, void *out, int Npad, int dgrad, int dtype, hipStream_t s)
{
    if (dtype == TDRN_F32) return TDRN_E_UNSUPPORTED;       // (16-bit types only)
    const int taps = g.kh * g.kw, Cp = deform_ts_cp(g.Cout), YC = deform_ts_cols(g);
    if (dgrad) return launch_pack(dtype, out, (long long)Npad * YC, TsRepackMap<true>{w, g.Cout, g.Cin, taps, Cp, YC}, s);
    return launch_pack(dtype, out, (long long)Npad * g.Cin, TsRepackMap<false>{w, g.Cout, g.Cin, taps, Cp, g.Cin}, s);
}

int launch_deform_ts_wgrad_reduce(const DeformBwdGeom &g, const float *slab, float *grad_weight, int splits, hipStream_t s)
{
    const int taps = g.kh * g.kw;
    SlabReduce r;
    r.Cout = g.Cout; r.Cin = g.Cin; r.taps = taps;
    r.d_co = (long long)g.Cin * taps; r.d_ci = taps; r.d_t = 1;                 // OIHW
    r.pitch = deform_ts_cp(g.Cout); r.CiPad = g.Cin; r.sstride = (size_t)deform_ts_cols(g) * g.Cin;
    r.bias_rows = 0; r.accumulate = false;                                       // overwrites; grad_weight is not read
    return launch_slab_reduce(r, slab, nullptr, grad_weight, nullptr, splits, s);
}

}  // namespace tdrn
