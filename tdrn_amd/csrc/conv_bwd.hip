// conv_bwd.hip -- the gradients of the dense convolution (tdrn_hip.h section i-c; with the output pixel stepped by ConvBwdGeom::stride
// also section i-g's weight gradient) that no inference kernel computes:
//   grad_weight[co][ci][i][j] += scale * sum_p GO[p][co] * X[p (+) tap][ci]      (wgrad: conv_wgrad_kernel + slab_reduce_kernel)
//   grad_bias[co]             += scale * sum_p GO[p][co]                         (the same two kernels)
// and the weight packing of the input gradient, which is launch_conv over grad_output with the kernel rotated by 180 degrees
// and its two channel axes exchanged (RepackOihwDgradMap).  slab_reduce_kernel also serves ConvTranspose2d's and deform_ts's slabs.
//
// wgrad is a GEMM whose contraction index is the PIXEL: K = N*Ho*Wo, the output is taps x Cout x Cin.  Both operands arrive NHWC
// (pixel rows of contiguous channels, in the compute type, channel-padded to kChanPad), so the contraction index is the row.
//   * one workgroup = (K split, 64 cin, 64 cout); its four waves own one 32 x 32 (cout x cin) tile each and keep the accumulator
//     tiles of ALL k*k taps in registers (9 x 16 VGPRs).  K runs in chunks of 64 output pixels.
//   * per chunk the grad_output tile [64 pixels][64 cout] is staged in LDS once as it comes from HBM; its MFMA fragments are read
//     once and serve all taps.  The input tile [64 pixels (+) tap][64 cin] is staged per tap into a two-slot ring (the loads of
//     tap t+1 are in flight under the MFMAs of tap t); a pixel whose tap lies in the padding -- or past the split's end --
//     loads the zero page instead (a pointer select, no branch).  The row of every pixel is decoded from (n, ho, wo), so a chunk
//     may cross image boundaries and the padding of one image never reads its neighbour's rows.  (One haloed patch per chunk
//     shared by all nine taps, without this prefetch, measured 3-9 % (bf16) and 14-22 % (fp32) slower: DESIGN 11.)
//   * 16-bit types: both operands of v_mfma_f32_32x32x16 are read with ds_read_b64_tr_b16 from the [pixel][channel] image (lane
//     4q+p of a 16-lane group addresses pixel row q, channels 4p..4p+3 and receives channel i of the 4 pixels).  EXEC is all
//     ones (no divergent branch around a read, 256 threads), every address is 8-byte aligned.  Rows are 128 B of data on a
//     192-byte stride: a 32-lane half reads 4 rows x 64 contiguous bytes, and 192 q mod 256 = 0, 192, 128, 64 puts the four
//     rows on four disjoint sets of 16 banks: conflict-free by the bank rule.
//   * fp32: v_mfma_f32_32x32x2_f32 takes one float per lane with k = lane >> 5: a ds_read_b32 of the [pixel][channel] image at
//     (pixel 2kk + (lane >> 5), channel lane & 31) is already the operand.  ds_read_b32 is served one 32-lane half per LDS cycle
//     (lanes l and l+32 never conflict) and a half reads 32 consecutive floats of one row: one per bank at any row stride.
//   * grad_bias rides along: the workgroups of cin tile 0 multiply the grad_output fragments with an all-ones operand.
//   * every split stores its fp32 slab [split][tap][CoutPad][CinPad] (+ [split][CoutPad] for the bias); the reduce kernel sums
//     them in split order and applies += scale * into OIHW.  No float atomics: bitwise reproducible, and the split count is a pure
//     function of the geometry (conv_wgrad_splits).
//   * k = 5 (tdrn_hip.h section i-i): 25 taps x 16 accumulators do not fit the register file, so the grid gains the kernel ROW: a
//     workgroup is (K split, kernel row r, 64 cin, 64 cout), holds the five tiles of taps 5r .. 5r+4, stages their input tiles
//     through the same ring (the last tap index of a pass is even, as at nine taps, so slot 0 is free at the chunk boundary) and
//     writes slab rows [split][5r + j]; it restages the grad_output tile of its chunks, and grad_bias rides along in row 0 only.
#include <algorithm>

#include "kernels.h"
#include "mfma_prims.h"

namespace tdrn {

namespace {

constexpr int kWgPx = 64;            // output pixels per chunk
constexpr int kWgTile = 64;          // cout x cin tile of a workgroup (= kChanPad: the padded tensors hold whole tiles)
static_assert(kWgTile == kChanPad, "whole tiles");

struct WgradParams {
    const char *x, *go, *zero;
    float *slab, *bslab;
    int M, H, W, Ho, Wo, HoWo, CiPad, CoPad, pad, dil, per_split;
    int stride = 1;        // input rows / columns per output pixel (2: tdrn_hip.h section i-g)
};

template <typename DT> struct WgLds {
    // bytes between pixel rows of an LDS tile: 16-bit 128 + 64 (see the header), fp32 256 + 16
    static constexpr int ROWB = elem_traits<DT>::bytes == 2 ? 192 : 272;
    static constexpr int V16 = elem_traits<DT>::bytes * 64 / 4 / 16;     // 16-byte pieces per thread (a quarter row)
};

typedef short v4s __attribute__((ext_vector_type(4)));

// the 8-element fragment (k = 8h + j of the 16-pixel step starting at row k0) of channel c0 + (lane & 31), for both operands of
// the 32x32x16 MFMA.  `a` = this lane's byte address for (row k0, channels c0 ..): tile + ((lane>>5)*8 + ((lane&15)>>2)) * ROWB +
// (c0 + 16*((lane>>4)&1) + 4*(lane&3)) * 2
template <int ROWB> __device__ __forceinline__ u32x4 tr_frag(const char *a)
{
    typedef __attribute__((address_space(3))) v4s *lds_v4s;
    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)a);
    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(a + 4 * ROWB));
    const i16x8 f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(u32x4, f);
}

template <typename DT> __device__ __forceinline__ unsigned ones2();
template <> __device__ __forceinline__ unsigned ones2<bf16_t>() { return 0x3f803f80u; }
template <> __device__ __forceinline__ unsigned ones2<f16_t>() { return 0x3c003c00u; }

// the accumulators of one wave -> its split's slab.  C/D map of the 32x32 MFMAs: column = lane & 31 (cin), row = (reg & 3) +
// 8 (reg >> 2) + 4 (lane >> 5) (cout)
// (NT accumulated taps of the split's ROWS * NT, starting at tap0)
template <int NT, int ROWS>
__device__ __forceinline__ void wgrad_store(const WgradParams &g, const f32x16 (&acc)[NT], const f32x16 &bacc, int split, int tap0, int ci0,
                                            int co0, int lane, int wm, int wn, bool with_bias)
{
    const int cil = ci0 + wn * 32 + (lane & 31);
#pragma unroll
    for (int tap = 0; tap < NT; ++tap) {
        float *sl = g.slab + ((size_t)split * (ROWS * NT) + tap0 + tap) * g.CoPad * g.CiPad;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            sl[(size_t)co * g.CiPad + cil] = acc[tap][r];
        }
    }
    if (with_bias && (lane & 31) == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            g.bslab[(size_t)split * g.CoPad + co] = bacc[r];
        }
    }
}

// NT = taps a workgroup accumulates, KK = kernel size: (9, 3) and (1, 1) are the whole kernel; (5, 5) is one kernel row, and
// blockIdx.x = split * 5 + row
template <typename DT, int NT, int KK>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradParams g)
{
    constexpr int ES = elem_traits<DT>::bytes, ROWB = WgLds<DT>::ROWB, V16 = WgLds<DT>::V16, ROWS = KK * KK / NT;
    static_assert(ROWS * NT == KK * KK && (NT & 1) == 1, "whole passes; an even last tap index leaves ring slot 0 to the next chunk");
    constexpr int TILEB = kWgPx * ROWB;
    __shared__ __attribute__((aligned(16))) char s_go[TILEB];
    __shared__ __attribute__((aligned(16))) char s_x[2][TILEB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
    const int split = blockIdx.x / ROWS, tap0 = (blockIdx.x % ROWS) * NT, ci0 = blockIdx.y * kWgTile, co0 = blockIdx.z * kWgTile;
    const int mbeg = split * g.per_split, mend = min(g.M, mbeg + g.per_split);
    const bool with_bias = blockIdx.y == 0 && wn == 0 && tap0 == 0;     // (wave-uniform)

    // staging: thread = a quarter (16 channels) of pixel row sp
    const int sp = t >> 2, sq = t & 3;
    const unsigned st_off = sp * ROWB + sq * (16 * V16);
    const char *zsrc = g.zero;                                           // (every piece of a masked row reads the zero page's first bytes)
    u32x4 rgo[V16], rx[V16];
    int pn = 0, pho = 0, pwo = 0;
    bool pvalid = false;

    auto decode = [&](int mb) {
        const int m = mb + sp;
        pvalid = m < mend;
        const int mm = pvalid ? m : mbeg;
        pn = mm / g.HoWo;
        const int pix = mm - pn * g.HoWo;
        pho = pix / g.Wo;
        pwo = pix - pho * g.Wo;
    };
    auto load_go = [&](int mb) {
        const char *src = pvalid ? g.go + ((size_t)(mb + sp) * g.CoPad + co0 + sq * 16) * ES : zsrc;
#pragma unroll
        for (int v = 0; v < V16; ++v) rgo[v] = *(const u32x4 *)(src + 16 * v);
    };
    auto load_x = [&](int tap) {
        const int kt = tap0 + tap;
        const int hi = pho * g.stride - g.pad + (kt / KK) * g.dil, wi = pwo * g.stride - g.pad + (kt % KK) * g.dil;
        const bool ok = pvalid && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
        const char *src = ok ? g.x + ((((size_t)pn * g.H + hi) * g.W + wi) * g.CiPad + ci0 + sq * 16) * ES : zsrc;
#pragma unroll
        for (int v = 0; v < V16; ++v) rx[v] = *(const u32x4 *)(src + 16 * v);
    };
    auto store = [&](char *tile, const u32x4 (&r)[V16]) {
#pragma unroll
        for (int v = 0; v < V16; ++v) *(u32x4 *)(tile + st_off + 16 * v) = r[v];
    };

    f32x16 acc[NT], bacc;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) bacc[r] = 0.f;

    // this lane's operand addresses inside a tile (row k0 = 0)
    unsigned a_off, b_off;
    if constexpr (ES == 2) {
        const unsigned row = (lane >> 5) * 8 + ((lane & 15) >> 2), col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        a_off = row * ROWB + (wm * 32 + col) * 2;
        b_off = row * ROWB + (wn * 32 + col) * 2;
    } else {
        a_off = (lane >> 5) * ROWB + (wm * 32 + (lane & 31)) * 4;
        b_off = (lane >> 5) * ROWB + (wn * 32 + (lane & 31)) * 4;
    }

    decode(mbeg);
    load_go(mbeg);
    load_x(0);
    for (int mb = mbeg; mb < mend; mb += kWgPx) {
        __syncthreads();                             // the previous chunk's reads of s_go and s_x[0] are done
        store(s_go, rgo);
        store(s_x[0], rx);
        [[maybe_unused]] u32x4 afrag[kWgPx / 16];
#pragma unroll
        for (int tap = 0; tap < NT; ++tap) {
            // loads of the next input tile (and, behind the last tap, of the next chunk) fly under this tap's MFMAs
            if (tap + 1 < NT) {
                load_x(tap + 1);
            } else if (mb + kWgPx < mend) {
                decode(mb + kWgPx);
                load_go(mb + kWgPx);
                load_x(0);
            }
            __syncthreads();                         // s_x[tap & 1] (and at tap 0 s_go) is complete
            const char *xt = s_x[tap & 1];
            if constexpr (ES == 2) {
                if (tap == 0) {
#pragma unroll
                    for (int ks = 0; ks < kWgPx / 16; ++ks) afrag[ks] = tr_frag<ROWB>(s_go + a_off + ks * 16 * ROWB);
                    if (with_bias) {
                        const unsigned o2 = ones2<DT>();
                        const u32x4 ones = {o2, o2, o2, o2};
#pragma unroll
                        for (int ks = 0; ks < kWgPx / 16; ++ks) Mma32<DT>::run(afrag[ks], ones, bacc);
                    }
                }
#pragma unroll
                for (int ks = 0; ks < kWgPx / 16; ++ks) {
                    const u32x4 bfrag = tr_frag<ROWB>(xt + b_off + ks * 16 * ROWB);
                    Mma32<DT>::run(afrag[ks], bfrag, acc[tap]);
                }
            } else {
#pragma unroll 8
                for (int kk = 0; kk < kWgPx / 2; ++kk) {
                    const float a = *(const float *)(s_go + a_off + kk * 2 * ROWB);
                    const float b = *(const float *)(xt + b_off + kk * 2 * ROWB);
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[tap], 0, 0, 0);
                    if (tap == 0 && with_bias) bacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, 1.f, bacc, 0, 0, 0);
                }
            }
            // s_x[(tap + 1) & 1] was last read at tap - 1: every wave is past the barrier above
            if (tap + 1 < NT) store(s_x[(tap + 1) & 1], rx);
        }
    }

    wgrad_store<NT, ROWS>(g, acc, bacc, split, tap0, ci0, co0, lane, wm, wn, with_bias);
}

// The one reduce of the split-K slabs [split][row(t, co) = t * pitch + co][CiPad] (SlabReduce, kernels.h; thread index: ci fastest ->
// coalesced slab reads): the sum over the S splits in split order, in fp32, lands at gw[co * d_co + ci * d_ci + t * d_t] as
// fmaf(scale, sum, *d) (accumulate) or as a plain store that never reads the destination.  Then, with gb:
// grad_bias[co] += scale * sum_s sum_{z < bias_rows} bslab[s][z * pitch + co], the split outer and the row inner.
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float *__restrict__ slab, const float *__restrict__ bslab,
                                                          float *__restrict__ gw, float *__restrict__ gb, const SlabReduce r, int S)
{
    const long long total = (long long)r.taps * r.Cout * r.Cin;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total + (gb ? r.Cout : 0); i += (long long)gridDim.x * blockDim.x) {
        if (i >= total) {
            const int co = (int)(i - total);
            float s = 0.f;
            for (int k = 0; k < S; ++k)
                for (int z = 0; z < r.bias_rows; ++z) s += bslab[((size_t)k * r.bias_rows + z) * r.pitch + co];
            gb[co] = fmaf(r.scale, s, gb[co]);
            continue;
        }
        const int c = (int)(i % r.Cin);
        const long long q = i / r.Cin;
        const int co = (int)(q % r.Cout), t = (int)(q / r.Cout);
        const float *sp = slab + ((size_t)t * r.pitch + co) * r.CiPad + c;
        float s = 0.f;
        for (int k = 0; k < S; ++k) s += sp[k * r.sstride];
        float *d = gw + (size_t)co * r.d_co + (size_t)c * r.d_ci + (size_t)t * r.d_t;
        if (r.accumulate) *d = fmaf(r.scale, s, *d);
        else *d = s;
    }
}

// OIHW fp32 -> the forward packing of the dgrad conv: out[ci][taps - 1 - tap][co] = w[co][ci][tap], rows >= Cin and channels >= Cout zero
struct RepackOihwDgradMap {
    const float *w;
    int Cout, Cin, taps, CoPad;
    __device__ float operator()(long long i) const
    {
        const int co = (int)(i % CoPad);
        const long long r = i / CoPad;
        const int tp = (int)(r % taps), ci = (int)(r / taps);
        return (ci < Cin && co < Cout) ? w[((size_t)co * Cin + ci) * taps + (taps - 1 - tp)] : 0.f;
    }
};

template <typename DT> int launch_wgrad_dt(const WgradParams &p, int taps, dim3 grid, hipStream_t s)
{
    if (taps == 25) hipLaunchKernelGGL((conv_wgrad_kernel<DT, 5, 5>), dim3(grid.x * 5, grid.y, grid.z), dim3(256), 0, s, p);
    else if (taps == 9) hipLaunchKernelGGL((conv_wgrad_kernel<DT, 9, 3>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((conv_wgrad_kernel<DT, 1, 1>), grid, dim3(256), 0, s, p);
    return hip_status(hipGetLastError());
}

}  // namespace

int conv_bwd_cpad(int c) { return (int)align_up((size_t)c, kChanPad); }

// K splits: enough workgroups for two per CU, at least four 64-pixel chunks each.  Geometry only.  k = 5 runs five workgroups (the
// kernel rows) per split and tile and counts them; the rule of k = 1 | 3 is untouched.
void conv_wgrad_splits(const ConvBwdGeom &g, int &splits, int &per_split)
{
    const int M = g.N * g.Ho * g.Wo;
    const int tiles = (conv_bwd_cpad(g.Cin) / kWgTile) * (conv_bwd_cpad(g.Cout) / kWgTile);
    int S = cdiv(512, g.k == 5 ? 5 * tiles : tiles);
    const int max_s = cdiv(M, 4 * kWgPx);
    S = S < 1 ? 1 : (S > max_s ? max_s : S);
    per_split = (int)align_up((size_t)cdiv(M, S), kWgPx);
    splits = cdiv(M, per_split);
}

size_t conv_wgrad_slab_bytes(const ConvBwdGeom &g)
{
    int S, per_split;
    conv_wgrad_splits(g, S, per_split);
    const size_t cop = conv_bwd_cpad(g.Cout), cip = conv_bwd_cpad(g.Cin);
    return align_up((size_t)S * g.k * g.k * cop * cip * 4, 256) + align_up((size_t)S * cop * 4, 256);
}

int launch_repack_oihw_dgrad(const float *w, void *out, int Cout, int Cin, int Npad, int taps, int dtype, hipStream_t s)
{
    const int CoPad = conv_bwd_cpad(Cout);
    return launch_pack(dtype, out, (long long)Npad * taps * CoPad, RepackOihwDgradMap{w, Cout, Cin, taps, CoPad}, s);
}

int launch_slab_reduce(const SlabReduce &r, const float *slab, const float *bslab, float *gw, float *gb, int S, hipStream_t s)
{
    const long long total = (long long)r.taps * r.Cout * r.Cin + (gb ? r.Cout : 0);
    hipLaunchKernelGGL(slab_reduce_kernel, stride_grid(total, 4096), dim3(256), 0, s, slab, bslab, gw, gb, r, S);
    return hip_status(hipGetLastError());
}

int launch_conv_wgrad_slabs(const ConvBwdGeom &g, const void *x_nhwc, const void *go_nhwc, const void *zero_page, void *slab, int dtype,
                            hipStream_t s, int &splits, const float *&bias_slab)
{
    if ((g.k != 1 && g.k != 3 && g.k != 5) || g.stride < 1 || !x_nhwc || !go_nhwc || !zero_page || !slab) return TDRN_E_UNSUPPORTED;
    int S, per_split;
    conv_wgrad_splits(g, S, per_split);
    const int taps = g.k * g.k;
    WgradParams p;
    p.x = (const char *)x_nhwc; p.go = (const char *)go_nhwc; p.zero = (const char *)zero_page;
    p.CiPad = conv_bwd_cpad(g.Cin); p.CoPad = conv_bwd_cpad(g.Cout);
    p.slab = (float *)slab;
    p.bslab = (float *)((char *)slab + align_up((size_t)S * taps * p.CoPad * p.CiPad * 4, 256));
    p.M = g.N * g.Ho * g.Wo; p.H = g.H; p.W = g.W; p.Ho = g.Ho; p.Wo = g.Wo; p.HoWo = g.Ho * g.Wo;
    p.pad = g.pad; p.dil = g.dil; p.per_split = per_split; p.stride = g.stride;
    const dim3 grid((unsigned)S, (unsigned)(p.CiPad / kWgTile), (unsigned)(p.CoPad / kWgTile));
    splits = S;
    bias_slab = p.bslab;
    return dispatch_dtype(dtype, [&](auto tag) { return launch_wgrad_dt<typename decltype(tag)::type>(p, taps, grid, s); });
}

int launch_conv_wgrad(const ConvBwdGeom &g, const void *x_nhwc, const void *go_nhwc, const void *zero_page, void *slab, float *grad_weight,
                      float *grad_bias, float scale, int dtype, hipStream_t s)
{
    if (!grad_weight) return TDRN_E_UNSUPPORTED;
    int S;
    const float *bslab;
    TDRN_TRY(launch_conv_wgrad_slabs(g, x_nhwc, go_nhwc, zero_page, slab, dtype, s, S, bslab));
    const int taps = g.k * g.k, CoPad = conv_bwd_cpad(g.Cout), CiPad = conv_bwd_cpad(g.Cin);
    SlabReduce r;
    r.Cout = g.Cout; r.Cin = g.Cin; r.taps = taps;
    r.d_co = (long long)g.Cin * taps; r.d_ci = taps; r.d_t = 1;                 // OIHW
    r.pitch = CoPad; r.CiPad = CiPad; r.sstride = (size_t)taps * CoPad * CiPad;
    r.bias_rows = 1; r.scale = scale; r.accumulate = true;
    return launch_slab_reduce(r, (const float *)slab, bslab, grad_weight, grad_bias, S, s);
}

}  // namespace tdrn
