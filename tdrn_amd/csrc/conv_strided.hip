// conv_strided.hip -- what the dense 3x3 stride-2 conv with gradients (tdrn_hip.h section i-g) needs beyond the kernels of the
// stride-1 family.  With Ho = (H + 2 pad - 3) / 2 + 1:
//   y[n][co][ho][wo]   = b[co] + sum_{ci,i,j} x[n][ci][2ho - pad + i][2wo - pad + j] W[co][ci][i][j]     launch_conv with stride = 2
//   gW[co][ci][i][j]   = sum_{n,ho,wo} go[n][co][ho][wo] x[n][ci][2ho - pad + i][2wo - pad + j]          conv_wgrad_kernel, pixel stepped by 2
//   gx[n][ci][h][w]    = sum_{co,i,j : h + pad - i = 2ho, w + pad - j = 2wo} go[n][co][ho][wo] W[co][ci][i][j]
// The last line is a stride-1 conv, with the kernel rotated and pad' = 2 - pad, over the zero-inserted image of grad_output
//   D[n][r][c][co],  r < Hd = H + 2 pad - 2,  c < Wd = W + 2 pad - 2:   D[2ho][2wo] = go[ho][wo], zero elsewhere,
// so the input gradient is section i-c's chain (launch_repack_oihw_dgrad, launch_conv) on (N, CoPad, Hd, Wd) -> (Cin, H, W).  Hd is
// 2 Ho - 1 or 2 Ho (H + 2 pad - 3 even or odd), so every row r of D belongs to exactly one ho = r >> 1 < Ho, and likewise every column.
// D is written by the layout conversion fp32 NCHW -> DT NHWC that the gradient needs anyway (nchw_to_nhwc_dilate2_kernel): no extra
// pass, no memset, and every element of D -- the zeros of the odd rows and columns and of the padded channels included -- is stored
// by the kernel on every call, so nothing depends on what the workspace held before.
//   * a workgroup converts 64 channels x 16 grad_output pixels of one row ho and writes the 2 x 32 pixels of D they own (rows 2ho and
//     2ho + 1, columns 2w and 2w + 1, clipped to Hd x Wd).  The 64 x 16 floats are read as row segments of 64 B: one 16-byte load a
//     lane when Wo % 4 == 0 (a quad then lies inside the row or outside it), one dword a lane otherwise; four (sixteen) consecutive
//     lanes cover one channel's segment.  They are transposed through an fp32 LDS image [pixel][64 channels] and read back as runs
//     of 64 channels per D pixel: 128-B (16-bit) or 256-B (fp32) stores of 16 B a lane.  Three of the four D pixels of every
//     grad_output pixel are stores of zeros that read nothing.
//   * LDS image: pixel stride 68 dwords (a multiple of 4: the read-back is ds_read_b128 on 16-byte addresses).  The bank rule relied
//     on: 32 banks of 4 bytes, a ds_write_b32 is served one 32-lane half at a time.  A half of the quad load holds 4 column quads x
//     8 channels; its store j hits banks (4 cq + j) 68 + c = 16 cq + 4 j + c mod 32: cq and cq + 2 alias, 2-way.  The dword path
//     holds 16 columns x 2 channels a half: banks 4 col + c mod 32, columns col and col + 8 alias, 2-way as well.  The read-back
//     reads 64 consecutive dwords per 16 (8) lanes: conflict-free.  This is the rule section 15 of DESIGN states for the
//     space-to-depth kernel, and like there it is NOT confirmed by counters.
//   * which elements a thread takes depends on (block, thread) alone, never on an address, and nothing is summed: a caller's buffer on
//     any 4-byte boundary gives the same bits (the 16-byte loads then run on a 4-byte boundary, which global loads allow).
#include "kernels.h"

namespace tdrn {

namespace {

constexpr int kDilPx = 16;                 // grad_output pixels (of one row ho) per workgroup: 32 columns of D
constexpr int kDilCh = 64;                 // channels per workgroup (= kChanPad: the padded image holds whole tiles)
constexpr int kDilWs = kDilCh + 4;         // dwords between pixels of the LDS image
static_assert(kDilCh == kChanPad, "whole tiles");

typedef f32x4 f32x4_u __attribute__((aligned(4)));

// VEC: Wo % 4 == 0, so a row of Wo floats is a whole number of quads
template <typename DT, bool VEC>
__global__ __launch_bounds__(256) void nchw_to_nhwc_dilate2_kernel(const float *__restrict__ in, char *__restrict__ out, int Cout, int Ho,
                                                                   int Wo, int Hd, int Wd, int CoPad, int wtiles, int ctiles)
{
    constexpr int ES = elem_traits<DT>::bytes, CH = elem_traits<DT>::per16, G = kDilCh / CH;
    __shared__ __attribute__((aligned(16))) float tile[kDilPx * kDilWs];
    const int t = threadIdx.x;
    unsigned b = blockIdx.x;
    const int ct = (int)(b % ctiles); b /= ctiles;
    const int wt = (int)(b % wtiles); b /= wtiles;
    const int ho = (int)(b % Ho), n = (int)(b / Ho);
    const int co0 = ct * kDilCh, w0 = wt * kDilPx;
    const size_t plane = (size_t)Ho * Wo;

    if constexpr (VEC) {
        const int cq = t & 3, cl = t >> 2;
        const int co = co0 + cl, col = w0 + 4 * cq;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (co < Cout && col < Wo) v = *(const f32x4_u *)(in + ((size_t)n * Cout + co) * plane + (size_t)ho * Wo + col);
        float *d = tile + (4 * cq) * kDilWs + cl;
        d[0] = v[0]; d[kDilWs] = v[1]; d[2 * kDilWs] = v[2]; d[3 * kDilWs] = v[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = t + k * 256, c = e & 15, cl = e >> 4;
            const int co = co0 + cl, col = w0 + c;
            const float v = (co < Cout && col < Wo) ? in[((size_t)n * Cout + co) * plane + (size_t)ho * Wo + col] : 0.f;
            tile[c * kDilWs + cl] = v;
        }
    }
    __syncthreads();

    // item = (grad_output pixel wl, z = 2 i + j: row 2ho + i and column 2w + j of D, 16-byte piece g); only z = 0 holds data
    for (int it = t; it < kDilPx * 4 * G; it += 256) {
        const int g = it % G, z = (it / G) & 3, wl = it / (4 * G);
        if (w0 + wl >= Wo) break;                      // (wl grows with it)
        const int r = 2 * ho + (z >> 1), c = 2 * (w0 + wl) + (z & 1);
        if (r >= Hd || c >= Wd) continue;
        u32x4 o = {0u, 0u, 0u, 0u};
        if (z == 0) {
            const float *src = tile + wl * kDilWs + g * CH;
            float v[CH];
#pragma unroll
            for (int q = 0; q < CH / 4; ++q) {
                const f32x4 x = *(const f32x4 *)(src + 4 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[4 * q + j] = x[j];
            }
            o = pack16<DT>(v);
        }
        const size_t eo = (((size_t)n * Hd + r) * Wd + c) * CoPad + co0 + g * CH;
        *(u32x4 *)(out + eo * ES) = o;
    }
}

}  // namespace

int launch_nchw_to_nhwc_dilate2(const float *in, void *out, int N, int Cout, int Ho, int Wo, int Hd, int Wd, int dtype, hipStream_t s)
{
    if (N <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0) return TDRN_OK;
    // every row and column of D must belong to a grad_output pixel: the kernel writes rows 2ho, 2ho + 1 and columns 2wo, 2wo + 1 only
    if (Hd < 2 * Ho - 1 || Hd > 2 * Ho || Wd < 2 * Wo - 1 || Wd > 2 * Wo) return TDRN_E_UNSUPPORTED;
    // one workgroup per (grad_output row, 16 pixels, 64 channels): fewer than the N Hd Wd CoPad / 64 the caller keeps under 2^31
    const int CoPad = conv_bwd_cpad(Cout), wtiles = cdiv(Wo, kDilPx), ctiles = CoPad / kDilCh;
    if ((long long)N * Ho * wtiles * ctiles >= (1ll << 31)) return TDRN_E_UNSUPPORTED;
    const dim3 grid((unsigned)((long long)N * Ho * wtiles * ctiles));
    return dispatch_dtype(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        hipLaunchKernelGGL((Wo % 4 == 0 ? nchw_to_nhwc_dilate2_kernel<DT, true> : nchw_to_nhwc_dilate2_kernel<DT, false>), grid, dim3(256), 0, s,
                           in, (char *)out, Cout, Ho, Wo, Hd, Wd, CoPad, wtiles, ctiles);
        return hip_status(hipGetLastError());
    });
}

}  // namespace tdrn
