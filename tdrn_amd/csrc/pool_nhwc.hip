// pool_nhwc.hip -- trainable MaxPool2d on resident tensors: 16-bit NHWC activations and gradients (tdrn_hip.h section i-k).
//
// The geometries, the selection rule and the codes are those of pool_l2norm.hip: 2x2 / stride 2 / pad 0 (floor or ceil) and 3x3 /
// stride 1 / pad 1; a window's in-bounds elements are scanned row-major and a value replaces the running maximum when it is strictly
// greater or is NaN (compared as fp32, which orders the 16-bit values exactly); the code is the selected slot dy * k + dx of the
// unclipped window, one byte per output element, laid out like the output ([N][Ho][Wo][C]).  A thread handles 8 channels -- one
// 16-byte access per pixel, 8 bytes of codes -- of one OUTPUT pixel in the forward and of one INPUT pixel in the backward, which
// reads grad_output and codes only and writes every element of grad_input exactly once.  The 3x3 backward adds the up-to-nine
// contributions in window row-major order in fp32, starting from +0.0, and rounds once.  No atomics: bitwise reproducible.
#include "kernels.h"

namespace tdrn {

namespace {

constexpr int kT = 256;
constexpr unsigned kGroups = 2048;      // 256 CUs x 8 workgroups: the grid-stride cap

struct PoolNhwcGeom { unsigned N, H, W, Ho, Wo, CG; };          // CG = C / 8 channel groups

// eight codes at once; the code tensor may start on any byte
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_u __attribute__((aligned(1)));
__device__ __forceinline__ void ldc8(const unsigned char *p, unsigned *cd)
{
    const u32x2 m = *(const u32x2_u *)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        cd[i] = (m.x >> (8 * i)) & 0xffu;
        cd[4 + i] = (m.y >> (8 * i)) & 0xffu;
    }
}
__device__ __forceinline__ void stc8(unsigned char *p, const unsigned *cd)
{
    u32x2 m;
    m.x = cd[0] | cd[1] << 8 | cd[2] << 16 | cd[3] << 24;
    m.y = cd[4] | cd[5] << 8 | cd[6] << 16 | cd[7] << 24;
    *(u32x2_u *)p = m;
}

// torch's update rule
__device__ __forceinline__ bool pool_takes(float v, float best) { return v > best || v != v; }

// K = 2: windows (2 ho + dy, 2 wo + dx), clipped at the bottom and right edge (ceil mode); K = 3: (h + dy - 1, w + dx - 1), clipped all round
template <typename DT, int K, bool CODE>
__global__ __launch_bounds__(kT) void pool_nhwc_fwd_kernel(const char *__restrict__ x, char *__restrict__ y, unsigned char *__restrict__ code,
                                                            PoolNhwcGeom g)
{
    const unsigned items = g.N * g.Ho * g.Wo * g.CG;
    for (unsigned it = blockIdx.x * kT + threadIdx.x; it < items; it += gridDim.x * kT) {
        const unsigned cg = it % g.CG, pix = it / g.CG, wo = pix % g.Wo, r = pix / g.Wo, ho = r % g.Ho, n = r / g.Ho;
        float best[8];
        unsigned cd[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { best[c] = -INFINITY; cd[c] = K == 2 ? 0 : 9; }
#pragma unroll
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
            for (int dx = 0; dx < K; ++dx) {
                const unsigned h = K == 2 ? 2 * ho + dy : ho + dy - 1, w = K == 2 ? 2 * wo + dx : wo + dx - 1;    // (wraps when negative)
                if (h < g.H && w < g.W) {
                    float v[8];
                    unpack16<DT>(*(const u32x4 *)(x + ((((size_t)n * g.H + h) * g.W + w) * g.CG + cg) * 16), v);
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        // 3x3: the first in-bounds slot is taken whatever it holds (torch starts its index there); 2x2: slot 0 is always in bounds
                        if ((K == 3 && cd[c] == 9) || pool_takes(v[c], best[c])) { best[c] = v[c]; cd[c] = dy * K + dx; }
                }
            }
        *(u32x4 *)(y + (size_t)it * 16) = pack16<DT>(best);
        if (CODE) stc8(code + (size_t)it * 8, cd);
    }
}

template <typename DT, int K>
__global__ __launch_bounds__(kT) void pool_nhwc_bwd_kernel(const char *__restrict__ go, const unsigned char *__restrict__ code,
                                                            char *__restrict__ gi, PoolNhwcGeom g)
{
    const unsigned items = g.N * g.H * g.W * g.CG;
    for (unsigned it = blockIdx.x * kT + threadIdx.x; it < items; it += gridDim.x * kT) {
        const unsigned cg = it % g.CG, pix = it / g.CG, w = pix % g.W, r = pix / g.W, h = r % g.H, n = r / g.H;
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.f;
        if (K == 2) {
            // the one window that holds this element, in slot (h & 1) * 2 + (w & 1); rows and columns no window covers get +0.0
            const unsigned ho = h >> 1, wo = w >> 1, slot = (h & 1) * 2 + (w & 1);
            if (ho < g.Ho && wo < g.Wo) {
                const size_t o = (((size_t)n * g.Ho + ho) * g.Wo + wo) * g.CG + cg;
                float d[8];
                unsigned cd[8];
                unpack16<DT>(*(const u32x4 *)(go + o * 16), d);
                ldc8(code + o * 8, cd);
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (cd[c] == slot) acc[c] += d[c];
            }
        } else {
            // window (h + r - 1, w + c - 1) holds this element in slot (2 - r) * 3 + (2 - c)
#pragma unroll
            for (int wr = 0; wr < 3; ++wr)
#pragma unroll
                for (int wc = 0; wc < 3; ++wc) {
                    const unsigned ho = h + wr - 1, wo = w + wc - 1;
                    if (ho < g.Ho && wo < g.Wo) {
                        const size_t o = (((size_t)n * g.Ho + ho) * g.Wo + wo) * g.CG + cg;
                        float d[8];
                        unsigned cd[8];
                        unpack16<DT>(*(const u32x4 *)(go + o * 16), d);
                        ldc8(code + o * 8, cd);
#pragma unroll
                        for (int c = 0; c < 8; ++c)
                            if (cd[c] == (unsigned)((2 - wr) * 3 + (2 - wc))) acc[c] += d[c];
                    }
                }
        }
        *(u32x4 *)(gi + (size_t)it * 16) = pack16<DT>(acc);
    }
}

unsigned pool_nhwc_grid(unsigned items)
{
    const unsigned blocks = (items + kT - 1) / kT;
    return blocks > kGroups * 4 ? kGroups * 4 : blocks;
}

}  // namespace

int launch_max_pool_nhwc_forward(const void *input, void *output, unsigned char *code, int N, int C, int H, int W, int Ho, int Wo, int kernel,
                                 int dtype, hipStream_t s)
{
    if (C % 8 || (kernel != 2 && kernel != 3)) return TDRN_E_UNSUPPORTED;
    const PoolNhwcGeom g{(unsigned)N, (unsigned)H, (unsigned)W, (unsigned)Ho, (unsigned)Wo, (unsigned)C / 8};
    const dim3 grid(pool_nhwc_grid(g.N * g.Ho * g.Wo * g.CG)), block(kT);
    return dispatch_dtype16(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        auto k = kernel == 2 ? (code ? pool_nhwc_fwd_kernel<DT, 2, true> : pool_nhwc_fwd_kernel<DT, 2, false>)
                             : (code ? pool_nhwc_fwd_kernel<DT, 3, true> : pool_nhwc_fwd_kernel<DT, 3, false>);
        hipLaunchKernelGGL(k, grid, block, 0, s, (const char *)input, (char *)output, code, g);
        return hip_status(hipGetLastError());
    });
}

int launch_max_pool_nhwc_backward(const void *grad_output, const unsigned char *code, void *grad_input, int N, int C, int H, int W, int Ho,
                                  int Wo, int kernel, int dtype, hipStream_t s)
{
    if (C % 8 || (kernel != 2 && kernel != 3)) return TDRN_E_UNSUPPORTED;
    const PoolNhwcGeom g{(unsigned)N, (unsigned)H, (unsigned)W, (unsigned)Ho, (unsigned)Wo, (unsigned)C / 8};
    const dim3 grid(pool_nhwc_grid(g.N * g.H * g.W * g.CG)), block(kT);
    return dispatch_dtype16(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        hipLaunchKernelGGL((kernel == 2 ? pool_nhwc_bwd_kernel<DT, 2> : pool_nhwc_bwd_kernel<DT, 3>), grid, block, 0, s,
                           (const char *)grad_output, code, (char *)grad_input, g);
        return hip_status(hipGetLastError());
    });
}

}  // namespace tdrn
