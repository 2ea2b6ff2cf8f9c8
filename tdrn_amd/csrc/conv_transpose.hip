// conv_transpose.hip -- what ConvTranspose2d(kernel 2, stride 2, pad 0) with gradients (tdrn_hip.h section i-f) needs beyond the
// kernels of the dense conv.  With k = s = 2 the four kernel taps z = 2i + j write four disjoint output phases, so
//   y[n][co][2h+i][2w+j]  = b[co] + sum_ci x[n][ci][h][w] W[ci][co][i][j]          four 1x1 GEMMs: launch_conv with phases = 4
//   gx[n][ci][h][w]       = sum_{z, co} go[n][co][2h+i][2w+j] W[ci][co][i][j]      ONE 1x1 GEMM over the space-to-depth image of go
//   gW[ci][co][i][j]      = sum_{n, h, w} x[n][ci][h][w] go[n][co][2h+i][2w+j]     the one-tap wgrad GEMM over the same image
//   gb[co]                = sum go
// The space-to-depth image S[n][h][w][z * CoPad + co] = go[n][co][2h+i][2w+j] (4 CoPad channels, CoPad = Cout padded to 64) is
// written by the layout conversion fp32 NCHW -> DT NHWC that both gradients need anyway (nchw_to_nhwc_s2d_kernel): no extra pass.
//   * a workgroup converts 64 channels x 2 rows (2h, 2h + 1) x 32 columns (16 output pixels): whole row segments of 128 B are read
//     with 16-byte loads (W even) or dword loads (W odd: a row is no whole number of quads), scattered into an fp32 LDS image
//     [pixel][z][64 channels] and read back as runs of 64 channels per (pixel, z): 128-B (16-bit) or 256-B (fp32) stores of 16 B a lane.
//   * LDS image: pixel stride 260 dwords.  A 32-lane half of a quad load holds 8 column quads x 4 channels; its four ds_write_b32
//     hit banks 8 cq + c (2 * 260 = 8 mod 32): 2-way, which a ds_write_b32 hides.  The odd-W path writes 4-way (j and w alias).
//     The read-back is ds_read_b128 over 64 consecutive dwords per 16 lanes.
//   * which elements a thread takes depends on (n, h, tile, thread) alone, never on an address, and nothing is summed: a caller's
//     buffer on any 4-byte boundary gives the same bits (the 16-byte loads then run on a 4-byte boundary, which global loads allow).
// The packers are index maps of pack_kernel (kernels.h) and the reduce is slab_reduce_kernel (conv_bwd.hip) with the strides of
// the (Cin, Cout, 2, 2) weight layout.  No float atomics: every gradient is bitwise reproducible.
#include <algorithm>

#include "kernels.h"

namespace tdrn {

namespace {

constexpr int kS2dPx = 16;                 // output pixels (of one row h) per workgroup: 32 grad_output columns
constexpr int kS2dCh = 64;                 // channels per workgroup (= kChanPad: the padded image holds whole tiles)
constexpr int kS2dWs = 4 * kS2dCh + 4;     // dwords between pixels of the LDS image
static_assert(kS2dCh == kChanPad, "whole tiles");

typedef f32x4 f32x4_u __attribute__((aligned(4)));

// VEC: W is even, so a row of 2W floats is a whole number of quads and a quad lies inside the row or outside it
template <typename DT, bool VEC>
__global__ __launch_bounds__(256) void nchw_to_nhwc_s2d_kernel(const float *__restrict__ in, char *__restrict__ out, int Cout, int H, int W,
                                                               int CoPad, int wtiles, int ctiles)
{
    constexpr int ES = elem_traits<DT>::bytes, CH = elem_traits<DT>::per16, G = kS2dCh / CH;
    __shared__ __attribute__((aligned(16))) float tile[kS2dPx * kS2dWs];
    const int t = threadIdx.x;
    unsigned b = blockIdx.x;
    const int ct = (int)(b % ctiles); b /= ctiles;
    const int wt = (int)(b % wtiles); b /= wtiles;
    const int h = (int)(b % H), n = (int)(b / H);
    const int co0 = ct * kS2dCh, w0 = wt * kS2dPx, W2 = 2 * W, col0 = 2 * w0;
    const size_t plane = (size_t)2 * H * W2;

    if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = t + k * 256, cq = q & 7, cl = (q >> 3) & 63, i = q >> 9;
            const int co = co0 + cl, col = col0 + 4 * cq;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (co < Cout && col < W2) v = *(const f32x4_u *)(in + ((size_t)n * Cout + co) * plane + (size_t)(2 * h + i) * W2 + col);
            float *d = tile + (2 * cq) * kS2dWs + (2 * i) * kS2dCh + cl;      // columns 4cq .. 4cq+3 = pixels 2cq, 2cq + 1 x j = 0, 1
            d[0] = v[0]; d[kS2dCh] = v[1]; d[kS2dWs] = v[2]; d[kS2dWs + kS2dCh] = v[3];
        }
    } else {
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int e = t + k * 256, c = e & 31, cl = (e >> 5) & 63, i = e >> 11;
            const int co = co0 + cl, col = col0 + c;
            const float v = (co < Cout && col < W2) ? in[((size_t)n * Cout + co) * plane + (size_t)(2 * h + i) * W2 + col] : 0.f;
            tile[(c >> 1) * kS2dWs + (2 * i + (c & 1)) * kS2dCh + cl] = v;
        }
    }
    __syncthreads();

    const size_t C4 = (size_t)4 * CoPad;
    for (int it = t; it < kS2dPx * 4 * G; it += 256) {
        const int g = it % G, z = (it / G) & 3, wl = it / (4 * G);
        if (w0 + wl >= W) break;                       // (wl grows with it)
        const float *src = tile + wl * kS2dWs + z * kS2dCh + g * CH;
        float v[CH];
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {
            const f32x4 x = *(const f32x4 *)(src + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * q + j] = x[j];
        }
        const size_t eo = (((size_t)n * H + h) * W + w0 + wl) * C4 + (size_t)z * CoPad + co0 + g * CH;
        *(u32x4 *)(out + eo * ES) = pack16<DT>(v);
    }
}

// (Cin, Cout, 2, 2) fp32 -> out[z][co][ci] ([4][Npad][CiPad]): launch_conv's phases = 4 packing; rows >= Cout and channels >= Cin zero
struct RepackIohwPhasesMap {
    const float *w;
    int Cin, Cout, Npad, CiPad;
    __device__ float operator()(long long i) const
    {
        const int ci = (int)(i % CiPad);
        const long long r = i / CiPad;
        const int co = (int)(r % Npad), z = (int)(r / Npad);
        return (ci < Cin && co < Cout) ? w[((size_t)ci * Cout + co) * 4 + z] : 0.f;
    }
};

// (Cin, Cout, 2, 2) fp32 -> out[ci][z * CoPad + co] ([Npad][4 CoPad]): the 1x1 conv over the space-to-depth image; rows >= Cin and
// channels >= Cout of every phase zero
struct RepackIohwDgradMap {
    const float *w;
    int Cin, Cout, CoPad;
    __device__ float operator()(long long i) const
    {
        const int co = (int)(i % CoPad);
        const long long r = i / CoPad;
        const int z = (int)(r & 3), ci = (int)(r >> 2);
        return (ci < Cin && co < Cout) ? w[((size_t)ci * Cout + co) * 4 + z] : 0.f;
    }
};

}  // namespace

int launch_nchw_to_nhwc_s2d(const float *in, void *out, int N, int Cout, int H, int W, int dtype, hipStream_t s)
{
    if (N <= 0 || Cout <= 0 || H <= 0 || W <= 0) return TDRN_OK;
    // one workgroup per (image row, 16 pixels, 64 channels): the count stays below N H W 4 CoPad / 4096, which the caller keeps under 2^31
    const int CoPad = conv_bwd_cpad(Cout), wtiles = cdiv(W, kS2dPx), ctiles = CoPad / kS2dCh;
    if ((long long)N * H * wtiles * ctiles >= (1ll << 31)) return TDRN_E_UNSUPPORTED;
    const dim3 grid((unsigned)((long long)N * H * wtiles * ctiles));
    return dispatch_dtype(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        hipLaunchKernelGGL((W % 2 == 0 ? nchw_to_nhwc_s2d_kernel<DT, true> : nchw_to_nhwc_s2d_kernel<DT, false>), grid, dim3(256), 0, s, in,
                           (char *)out, Cout, H, W, CoPad, wtiles, ctiles);
        return hip_status(hipGetLastError());
    });
}

int launch_repack_iohw_phases(const float *w, void *out, int Cin, int Cout, int Npad, int dtype, hipStream_t s)
{
    const int CiPad = conv_bwd_cpad(Cin);
    return launch_pack(dtype, out, 4ll * Npad * CiPad, RepackIohwPhasesMap{w, Cin, Cout, Npad, CiPad}, s);
}

int launch_repack_iohw_dgrad(const float *w, void *out, int Cin, int Cout, int Npad, int dtype, hipStream_t s)
{
    const int CoPad = conv_bwd_cpad(Cout);
    return launch_pack(dtype, out, 4ll * Npad * CoPad, RepackIohwDgradMap{w, Cin, Cout, CoPad}, s);
}

int launch_convt_wgrad_reduce(const float *slab, const float *bias_slab, float *grad_weight, float *grad_bias, int Cin, int Cout, int splits,
                              float scale, hipStream_t s)
{
    const int CoPad = conv_bwd_cpad(Cout), CiPad = conv_bwd_cpad(Cin);
    SlabReduce r;
    r.Cout = Cout; r.Cin = Cin; r.taps = 4;
    r.d_co = 4; r.d_ci = 4ll * Cout; r.d_t = 1;                                 // (Cin, Cout, 2, 2)
    r.pitch = CoPad; r.CiPad = CiPad; r.sstride = (size_t)4 * CoPad * CiPad;
    r.bias_rows = 4; r.scale = scale; r.accumulate = true;
    return launch_slab_reduce(r, slab, bias_slab, grad_weight, grad_bias, splits, s);
}

}  // namespace tdrn
