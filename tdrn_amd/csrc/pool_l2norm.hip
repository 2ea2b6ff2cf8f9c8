// pool_l2norm.hip -- trainable MaxPool2d and L2Norm, forward and backward, fp32 NCHW (tdrn_hip.h section i-e).
//
// MaxPool2d: 2x2 / stride 2 / pad 0 (floor or ceil) and 3x3 / stride 1 / pad 1.  The forward writes the output and one uint8 code per
// output element, the selected element's slot dy * k + dx in the unclipped window; the backward reads grad_output and the codes, never
// the input, and writes every element of grad_input exactly once (no zero fill, no scatter).  Selection is torch's: a window's
// in-bounds elements are scanned row-major and a value replaces the running maximum when it is strictly greater or is NaN.
//
// L2Norm: y = weight x / (sqrt(sum_c x^2) + eps).  A workgroup owns 64 consecutive pixels (one per lane) and all channels; its four
// waves take the channels c = wave, wave + 4, ...; the per-pixel partial sums merge through LDS in wave order.
//
// Which elements a thread takes is decided by the logical index alone, never by an address (the rule of batch_norm.hip): a caller's
// buffer on any 4-byte boundary gives the bits of an aligned one.  No float atomics: every output is bitwise reproducible.
#include "kernels.h"

namespace tdrn {

namespace {

constexpr int kT = 256;                 // threads per workgroup
constexpr unsigned kGroups = 2048;      // 256 CUs x 8 workgroups: the grid-stride kernels' cap

typedef f32x4 f32x4_u __attribute__((aligned(4)));
__device__ __forceinline__ f32x4 ld4(const float *p) { return *(const f32x4_u *)p; }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *(f32x4_u *)p = v; }
// four codes at once; the code tensor may start on any byte
typedef uint32_t u32_u __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t ldc4(const unsigned char *p) { return *(const u32_u *)p; }
__device__ __forceinline__ void stc4(unsigned char *p, uint32_t v) { *(u32_u *)p = v; }

struct PoolGeom { unsigned H, W, Ho, Wo, planes; };

// torch's update rule
__device__ __forceinline__ bool pool_takes(float v, float best) { return v > best || v != v; }

// ---- 2x2 / 2 -------------------------------------------------------------------------------------------------------------------------
// one window, clipped to the input (ceil mode's last row and column): slot 0 is always in bounds
__device__ __forceinline__ float pool2_one(const float *__restrict__ x, const PoolGeom &g, unsigned base, unsigned ho, unsigned wo, unsigned &code)
{
    float best = -INFINITY;
    code = 0;
#pragma unroll
    for (unsigned dy = 0; dy < 2; ++dy)
#pragma unroll
        for (unsigned dx = 0; dx < 2; ++dx) {
            const unsigned h = 2 * ho + dy, w = 2 * wo + dx;
            if (h < g.H && w < g.W) {
                const float v = x[base + h * g.W + w];
                if (pool_takes(v, best)) { best = v; code = dy * 2 + dx; }
            }
        }
    return best;
}

// item = (plane, output row, quad of four adjacent outputs): two row segments of eight floats in, one 16-byte store and one 4-byte
// code store out
template <bool CODE>
__global__ __launch_bounds__(kT) void pool2_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, unsigned char *__restrict__ code,
                                                        PoolGeom g)
{
    const unsigned qpr = (g.Wo + 3) / 4, items = g.planes * g.Ho * qpr;
    for (unsigned it = blockIdx.x * kT + threadIdx.x; it < items; it += gridDim.x * kT) {
        const unsigned row = it / qpr, q = it - row * qpr, plane = row / g.Ho, ho = row - plane * g.Ho;
        const unsigned wo0 = 4 * q, ibase = plane * g.H * g.W, obase = (plane * g.Ho + ho) * g.Wo + wo0;
        if (wo0 + 4 <= g.Wo && 2 * wo0 + 8 <= g.W && 2 * ho + 2 <= g.H) {
            const float *r0 = x + ibase + 2 * ho * g.W + 2 * wo0, *r1 = r0 + g.W;
            const f32x4 a0 = ld4(r0), a1 = ld4(r0 + 4), b0 = ld4(r1), b1 = ld4(r1 + 4);
            const float top[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            const float bot[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
            f32x4 o;
            uint32_t codes = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float best = -INFINITY;
                unsigned c = 0;
                if (pool_takes(top[2 * j], best)) { best = top[2 * j]; c = 0; }
                if (pool_takes(top[2 * j + 1], best)) { best = top[2 * j + 1]; c = 1; }
                if (pool_takes(bot[2 * j], best)) { best = bot[2 * j]; c = 2; }
                if (pool_takes(bot[2 * j + 1], best)) { best = bot[2 * j + 1]; c = 3; }
                o[j] = best;
                codes |= c << (8 * j);
            }
            st4(y + obase, o);
            if (CODE) stc4(code + obase, codes);
        } else {
            for (unsigned j = 0; j < 4 && wo0 + j < g.Wo; ++j) {
                unsigned c;
                y[obase + j] = pool2_one(x, g, ibase, ho, wo0 + j, c);
                if (CODE) code[obase + j] = (unsigned char)c;
            }
        }
    }
}

// item = (plane, pair of input rows 2 hp and 2 hp + 1, eight adjacent input columns): four grad_output values and four codes in, up
// to four 16-byte stores out.  An element gets +0.0 + grad_output if its window's code names it (torch's accumulation into a zeroed
// tensor), +0.0 otherwise; rows and columns that no window covers get +0.0 as well.
__global__ __launch_bounds__(kT) void pool2_bwd_kernel(const float *__restrict__ go, const unsigned char *__restrict__ code,
                                                        float *__restrict__ gi, PoolGeom g)
{
    const unsigned hp_n = (g.H + 1) / 2, opr = (g.W + 7) / 8, items = g.planes * hp_n * opr;
    for (unsigned it = blockIdx.x * kT + threadIdx.x; it < items; it += gridDim.x * kT) {
        const unsigned row = it / opr, o8 = it - row * opr, plane = row / hp_n, hp = row - plane * hp_n;
        const unsigned w0 = 8 * o8, wo0 = 4 * o8, ibase = plane * g.H * g.W, obase = (plane * g.Ho + hp) * g.Wo;
        if (w0 + 8 <= g.W && 2 * hp + 2 <= g.H && hp < g.Ho && wo0 + 4 <= g.Wo) {
            const f32x4 d = ld4(go + obase + wo0);
            const uint32_t codes = ldc4(code + obase + wo0);
            f32x4 t0, t1, b0, b1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned c = (codes >> (8 * j)) & 0xffu;
                const float v = 0.f + d[j];
                const float e0 = c == 0 ? v : 0.f, e1 = c == 1 ? v : 0.f, e2 = c == 2 ? v : 0.f, e3 = c == 3 ? v : 0.f;
                if (j < 2) { t0[2 * j] = e0; t0[2 * j + 1] = e1; b0[2 * j] = e2; b0[2 * j + 1] = e3; }
                else { t1[2 * j - 4] = e0; t1[2 * j - 3] = e1; b1[2 * j - 4] = e2; b1[2 * j - 3] = e3; }
            }
            float *r0 = gi + ibase + 2 * hp * g.W + w0, *r1 = r0 + g.W;
            st4(r0, t0); st4(r0 + 4, t1); st4(r1, b0); st4(r1 + 4, b1);
        } else {
            for (unsigned dy = 0; dy < 2 && 2 * hp + dy < g.H; ++dy)
                for (unsigned j = 0; j < 8 && w0 + j < g.W; ++j) {
                    const unsigned w = w0 + j, wo = w / 2;
                    float v = 0.f;
                    if (hp < g.Ho && wo < g.Wo && code[obase + wo] == dy * 2 + (w & 1)) v = 0.f + go[obase + wo];
                    gi[ibase + (2 * hp + dy) * g.W + w] = v;
                }
        }
    }
}

// ---- 3x3 / 1 / 1 (output H x W) ------------------------------------------------------------------------------------------------------
// item = (plane, row, quad of four adjacent elements).  Both directions gather the 3 x 6 neighbourhood of the quad and store the quad
// with one 16-byte store where it is whole.
__device__ __forceinline__ void pool3_load4(const float *p, float *out)
{
    const f32x4 m = ld4(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = m[i];
}
__device__ __forceinline__ void pool3_load4(const unsigned char *p, unsigned char *out)
{
    const uint32_t m = ldc4(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = (unsigned char)(m >> (8 * i));
}

// v = the neighbourhood of the quad at (h, w0) of `plane`, ok = which of its positions exist.  Every load is unconditional, on a row
// and a column clamped into the plane, so that all of them are in flight together (what a position outside holds is dropped by the
// caller through ok); the four in the middle are one vector load where the quad is whole.
template <typename T>
__device__ __forceinline__ void pool3_gather(const T *__restrict__ plane, const PoolGeom &g, unsigned h, unsigned w0, T (&v)[3][6], bool (&ok)[3][6])
{
    unsigned col[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const unsigned ww = w0 + c - 1;                 // wraps past 2^31 when negative
        col[c] = ww < g.W ? ww : (c == 0 ? 0 : g.W - 1);
    }
    const T *rp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const unsigned hh = h + r - 1;
        rp[r] = plane + (hh < g.H ? hh : h) * g.W;
#pragma unroll
        for (int c = 0; c < 6; ++c) ok[r][c] = hh < g.H && w0 + c - 1 < g.W;
    }
    if (w0 + 4 <= g.W) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            v[r][0] = rp[r][col[0]];
            pool3_load4(rp[r] + w0, &v[r][1]);
            v[r][5] = rp[r][col[5]];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) v[r][c] = rp[r][col[c]];
    }
}

template <bool CODE>
__global__ __launch_bounds__(kT) void pool3_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, unsigned char *__restrict__ code,
                                                        PoolGeom g)
{
    const unsigned qpr = (g.W + 3) / 4, items = g.planes * g.H * qpr;
    for (unsigned it = blockIdx.x * kT + threadIdx.x; it < items; it += gridDim.x * kT) {
        const unsigned row = it / qpr, q = it - row * qpr, plane = row / g.H, h = row - plane * g.H;
        const unsigned w0 = 4 * q, base = plane * g.H * g.W;
        float v[3][6];
        bool ok[3][6];
        pool3_gather(x + base, g, h, w0, v, ok);
        float o[4];
        unsigned cd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float best = -INFINITY;
            unsigned c = 9;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
                    // the first in-bounds slot is taken whatever it holds (torch starts its index there)
                    if (ok[dy][j + dx] && (c == 9 || pool_takes(v[dy][j + dx], best))) { best = v[dy][j + dx]; c = dy * 3 + dx; }
            o[j] = best;
            cd[j] = c;
        }
        const unsigned off = base + h * g.W + w0;
        if (w0 + 4 <= g.W) {
            st4(y + off, f32x4{o[0], o[1], o[2], o[3]});
            if (CODE) stc4(code + off, cd[0] | cd[1] << 8 | cd[2] << 16 | cd[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (w0 + j < g.W) {
                    y[off + j] = o[j];
                    if (CODE) code[off + j] = (unsigned char)cd[j];
                }
        }
    }
}

// an input element adds the grad_output of the up to nine windows that selected it, in window row-major order, starting from +0.0
__global__ __launch_bounds__(kT) void pool3_bwd_kernel(const float *__restrict__ go, const unsigned char *__restrict__ code,
                                                        float *__restrict__ gi, PoolGeom g)
{
    const unsigned qpr = (g.W + 3) / 4, items = g.planes * g.H * qpr;
    for (unsigned it = blockIdx.x * kT + threadIdx.x; it < items; it += gridDim.x * kT) {
        const unsigned row = it / qpr, q = it - row * qpr, plane = row / g.H, h = row - plane * g.H;
        const unsigned w0 = 4 * q, base = plane * g.H * g.W;
        float d[3][6];
        unsigned char cd[3][6];
        bool ok[3][6];
        pool3_gather(go + base, g, h, w0, d, ok);
        pool3_gather(code + base, g, h, w0, cd, ok);
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int r = 0; r < 3; ++r)          // window (h + r - 1, w0 + j + c - 1) holds this element in slot (2 - r) * 3 + (2 - c)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (ok[r][j + c] && cd[r][j + c] == (2 - r) * 3 + (2 - c)) acc += d[r][j + c];
            o[j] = acc;
        }
        const unsigned off = base + h * g.W + w0;
        if (w0 + 4 <= g.W) {
            st4(gi + off, f32x4{o[0], o[1], o[2], o[3]});
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (w0 + j < g.W) gi[off + j] = o[j];
        }
    }
}

unsigned pool_grid(unsigned long long items)
{
    const unsigned long long b = (items + kT - 1) / kT;
    return (unsigned)(b < kGroups ? (b ? b : 1) : kGroups);
}

// ---- L2Norm --------------------------------------------------------------------------------------------------------------------------
constexpr int kTile = 64;               // pixels per workgroup, one per lane
constexpr int kWaves = kT / 64;

struct L2Geom { unsigned C, HW, NP; };  // NP = N * HW pixels

// A wave walks its channels c = wave, wave + 4, ... in groups of G: f(c0, i0) gets the group's first channel and its first slot.
// NG > 0: exactly NG groups, unrolled, so that i0 is a compile-time constant (register-kept values); NG = 0: as many as C needs.
// Inside a group every load comes first and is unconditional (a channel past C is clamped into the tensor and its value dropped), so
// the G loads are in flight together; a branch around each load leaves one in flight.
template <int G, int NG, typename F> __device__ __forceinline__ void l2_groups(unsigned wave, unsigned C, F f)
{
    if (NG) {
#pragma unroll
        for (int gi = 0; gi < (NG ? NG : 1); ++gi) f(wave + kWaves * G * gi, G * gi);
    } else {
        for (unsigned c0 = wave; c0 < C; c0 += kWaves * G) f(c0, 0);
    }
}
// channel j of the group at c0, clamped; whether it exists
__device__ __forceinline__ unsigned l2_c(unsigned c0, int j, unsigned C) { const unsigned c = c0 + kWaves * j; return c < C ? c : C - 1; }
__device__ __forceinline__ bool l2_ok(unsigned c0, int j, unsigned C) { return c0 + kWaves * j < C; }

constexpr int kG = 8;                   // channels per group where nothing is kept, and of every storing pass
constexpr int kKeep = 128;              // channels a lane keeps in the forward's register-kept instantiation

// the four waves' per-pixel partial sums, added in wave order; every lane of every wave gets the total
__device__ __forceinline__ float l2_merge(float part, float (*sh)[kTile], unsigned wave, unsigned lane)
{
    sh[wave][lane] = part;
    __syncthreads();
    float t = sh[0][lane];
#pragma unroll
    for (int i = 1; i < kWaves; ++i) t += sh[i][lane];
    return t;
}

// KEEP: the channels of its pixel a lane keeps in registers (C <= 4 KEEP), so x is read once, all KEEP loads in flight; 0: nothing is
// kept and x is read twice.  A lane past the last pixel works on pixel 0 and stores nothing.
template <int KEEP>
__global__ __launch_bounds__(kT) void l2norm_fwd_kernel(const float *__restrict__ x, const float *__restrict__ weight, float *__restrict__ y,
                                                         float *__restrict__ norm, L2Geom g, float eps)
{
    __shared__ float sh[kWaves][kTile];
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned P = blockIdx.x * kTile + lane;
    const bool live = P < g.NP;
    const unsigned n = live ? P / g.HW : 0, base = live ? n * g.C * g.HW + (P - n * g.HW) : 0;
    const float *px = x + base;
    float *py = y + base;
    constexpr int G1 = KEEP ? KEEP : kG;
    float v[KEEP ? KEEP : 1];
    float ss[4] = {0.f, 0.f, 0.f, 0.f};
    l2_groups<G1, KEEP ? 1 : 0>(wave, g.C, [&](unsigned c0, int) {
        float t[G1];
#pragma unroll
        for (int j = 0; j < G1; ++j) t[j] = px[l2_c(c0, j, g.C) * g.HW];
#pragma unroll
        for (int j = 0; j < G1; ++j) {
            const float a = l2_ok(c0, j, g.C) ? t[j] : 0.f;
            if (KEEP) v[j] = a;
            ss[j & 3] = __builtin_fmaf(a, a, ss[j & 3]);
        }
    });
    const float total = l2_merge((ss[0] + ss[1]) + (ss[2] + ss[3]), sh, wave, lane);
    const float nrm = sqrtf(total) + eps, inv = 1.f / nrm;
    if (!live) return;
    if (norm && wave == 0) norm[P] = nrm;
    l2_groups<kG, KEEP / kG>(wave, g.C, [&](unsigned c0, int i0) {
        float w[kG], a[kG];
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            w[j] = weight[l2_c(c0, j, g.C)];
            a[j] = KEEP ? v[i0 + j] : px[l2_c(c0, j, g.C) * g.HW];
        }
#pragma unroll
        for (int j = 0; j < kG; ++j)
            if (l2_ok(c0, j, g.C)) py[(c0 + kWaves * j) * g.HW] = w[j] * (a[j] * inv);
    });
}

// grad_input = (weight go - x t) / norm with t = s / (norm r), s = sum_c weight go x, r = norm - eps; t = 0 at an all-zero pixel (r = 0).
// part (or null): [tile][C] sums over the tile's pixels of go x / norm, lanes merged by a fixed shuffle tree.  x and grad_output are
// read twice, the second time from cache: keeping them costs 235 VGPRs and more for a gain of 15 % at 128 channels.
__global__ __launch_bounds__(kT) void l2norm_bwd_kernel(const float *__restrict__ x, const float *__restrict__ go, const float *__restrict__ weight,
                                                         const float *__restrict__ norm, float *__restrict__ gi, float *__restrict__ part,
                                                         L2Geom g, float eps)
{
    __shared__ float sh[kWaves][kTile];
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned P = blockIdx.x * kTile + lane;
    const bool live = P < g.NP;
    const unsigned n = live ? P / g.HW : 0, base = live ? n * g.C * g.HW + (P - n * g.HW) : 0;
    const float *px = x + base, *pg = go + base;
    float *pi = gi + base;
    const float nrm = norm[live ? P : 0], inv = 1.f / nrm, r = nrm - eps;
    float s4[4] = {0.f, 0.f, 0.f, 0.f};
    l2_groups<kG, 0>(wave, g.C, [&](unsigned c0, int) {
        float a[kG], d[kG], w[kG];
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            const unsigned c = l2_c(c0, j, g.C);
            a[j] = px[c * g.HW];
            d[j] = pg[c * g.HW];
            w[j] = weight[c];
        }
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            d[j] = l2_ok(c0, j, g.C) && live ? a[j] * d[j] : 0.f;          // (never 0 times a stray NaN)
            s4[j & 3] = __builtin_fmaf(w[j], d[j], s4[j & 3]);
        }
        if (part) {
#pragma unroll
            for (int j = 0; j < kG; ++j) d[j] *= inv;
            // the kG trees side by side, so that their shuffles overlap
#pragma unroll
            for (int o = 32; o; o >>= 1)
#pragma unroll
                for (int j = 0; j < kG; ++j) d[j] += __shfl_down(d[j], o);
#pragma unroll
            for (int j = 0; j < kG; ++j)
                if (lane == 0 && l2_ok(c0, j, g.C)) part[(size_t)blockIdx.x * g.C + c0 + kWaves * j] = d[j];
        }
    });
    if (!gi) return;                    // the same in every thread of the grid
    const float s = l2_merge((s4[0] + s4[1]) + (s4[2] + s4[3]), sh, wave, lane);
    if (!live) return;
    const float t = r > 0.f ? s * inv / r : 0.f;
    l2_groups<kG, 0>(wave, g.C, [&](unsigned c0, int) {
        float a[kG], d[kG], w[kG];
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            const unsigned c = l2_c(c0, j, g.C);
            a[j] = px[c * g.HW];
            d[j] = pg[c * g.HW];
            w[j] = weight[c];
        }
#pragma unroll
        for (int j = 0; j < kG; ++j)
            if (l2_ok(c0, j, g.C)) pi[(c0 + kWaves * j) * g.HW] = (w[j] * d[j] - a[j] * t) * inv;
    });
}

// grad_weight[c] += scale sum over the tiles, in tile order: lane = channel, the 16 waves of a workgroup take 16 consecutive ranges
// of tiles and merge in wave order
constexpr int kFinT = 1024, kFinSlices = kFinT / 64;

__global__ __launch_bounds__(kFinT) void l2norm_gw_finalize_kernel(const float *__restrict__ part, float *grad_weight, unsigned C, unsigned tiles,
                                                                    float scale)
{
    __shared__ double sh[kFinSlices][64];
    const unsigned lane = threadIdx.x & 63, slice = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    const unsigned per = (tiles + kFinSlices - 1) / kFinSlices, lo = slice * per, hi = lo + per < tiles ? lo + per : tiles;
    double t = 0.0;
    if (c < C) {
        unsigned i = lo;
        for (; i + kG <= hi; i += kG) {         // the loads of a step in flight together, added in tile order
            float v[kG];
#pragma unroll
            for (int j = 0; j < kG; ++j) v[j] = part[(size_t)(i + j) * C + c];
#pragma unroll
            for (int j = 0; j < kG; ++j) t += (double)v[j];
        }
        for (; i < hi; ++i) t += (double)part[(size_t)i * C + c];
    }
    sh[slice][lane] = t;
    __syncthreads();
    if (slice == 0 && c < C) {
        for (int i = 1; i < kFinSlices; ++i) t += sh[i][lane];
        grad_weight[c] += scale * (float)t;
    }
}

unsigned l2_tiles(int N, int HW) { return (unsigned)(((long long)N * HW + kTile - 1) / kTile); }

}  // namespace

int launch_max_pool_forward(const float *input, float *output, unsigned char *code, int planes, int H, int W, int Ho, int Wo, int kernel,
                            hipStream_t s)
{
    const PoolGeom g{(unsigned)H, (unsigned)W, (unsigned)Ho, (unsigned)Wo, (unsigned)planes};
    if (kernel == 2) {
        const unsigned grid = pool_grid((unsigned long long)planes * Ho * ((Wo + 3) / 4));
        if (code) hipLaunchKernelGGL(pool2_fwd_kernel<true>, dim3(grid), dim3(kT), 0, s, input, output, code, g);
        else hipLaunchKernelGGL(pool2_fwd_kernel<false>, dim3(grid), dim3(kT), 0, s, input, output, code, g);
    } else {
        const unsigned grid = pool_grid((unsigned long long)planes * H * ((W + 3) / 4));
        if (code) hipLaunchKernelGGL(pool3_fwd_kernel<true>, dim3(grid), dim3(kT), 0, s, input, output, code, g);
        else hipLaunchKernelGGL(pool3_fwd_kernel<false>, dim3(grid), dim3(kT), 0, s, input, output, code, g);
    }
    return hip_status(hipGetLastError());
}

int launch_max_pool_backward(const float *grad_output, const unsigned char *code, float *grad_input, int planes, int H, int W, int Ho, int Wo,
                             int kernel, hipStream_t s)
{
    const PoolGeom g{(unsigned)H, (unsigned)W, (unsigned)Ho, (unsigned)Wo, (unsigned)planes};
    if (kernel == 2)
        hipLaunchKernelGGL(pool2_bwd_kernel, dim3(pool_grid((unsigned long long)planes * ((H + 1) / 2) * ((W + 7) / 8))), dim3(kT), 0, s,
                           grad_output, code, grad_input, g);
    else
        hipLaunchKernelGGL(pool3_bwd_kernel, dim3(pool_grid((unsigned long long)planes * H * ((W + 3) / 4))), dim3(kT), 0, s, grad_output,
                           code, grad_input, g);
    return hip_status(hipGetLastError());
}

// the [tile][C] partial sums of grad_weight
size_t l2norm_workspace_bytes(int N, int C, int HW) { return (size_t)l2_tiles(N, HW) * (size_t)C * 4; }

// The forward keeps a pixel's channels in registers (x read once) where that was measured faster: 256 < C <= 512 on at most 256 tiles,
// one workgroup per CU.  The kept kernel holds 256 VGPRs, one workgroup per CU at a time: 800 tiles take four rounds and lose to the
// two-read kernel, whose 800 workgroups are all resident.
int launch_l2norm_forward(const float *input, const float *weight, float *output, float *norm, int N, int C, int HW, float eps, hipStream_t s)
{
    const L2Geom g{(unsigned)C, (unsigned)HW, (unsigned)((long long)N * HW)};
    const unsigned tiles = l2_tiles(N, HW);
    if (C > 256 && C <= 4 * kKeep && tiles <= 256)
        hipLaunchKernelGGL(l2norm_fwd_kernel<kKeep>, dim3(tiles), dim3(kT), 0, s, input, weight, output, norm, g, eps);
    else
        hipLaunchKernelGGL(l2norm_fwd_kernel<0>, dim3(tiles), dim3(kT), 0, s, input, weight, output, norm, g, eps);
    return hip_status(hipGetLastError());
}

int launch_l2norm_backward(const float *input, const float *grad_output, const float *weight, const float *norm, float *grad_input,
                           float *grad_weight, int N, int C, int HW, float eps, float scale, void *ws, hipStream_t s)
{
    const L2Geom g{(unsigned)C, (unsigned)HW, (unsigned)((long long)N * HW)};
    const unsigned tiles = l2_tiles(N, HW);
    float *part = grad_weight ? (float *)ws : nullptr;
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(tiles), dim3(kT), 0, s, input, grad_output, weight, norm, grad_input, part, g, eps);
    if (grad_weight)
        hipLaunchKernelGGL(l2norm_gw_finalize_kernel, dim3((C + 63) / 64), dim3(kFinT), 0, s, part, grad_weight, (unsigned)C, tiles, scale);
    return hip_status(hipGetLastError());
}

}  // namespace tdrn
