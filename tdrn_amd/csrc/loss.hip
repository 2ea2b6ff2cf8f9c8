// loss.hip -- the training losses MultiBoxLoss / RefineMultiBoxLoss on the device, fp32, forward and backward.
//
// Replaces layers/box_utils.py:81-172 (match, refine_match, encode), :216-223 (log_sum_exp) and
// layers/modules/{multibox_loss.py:59-110, refine_multibox_loss.py:28-102}: a Python loop over the batch, a second one
// over the ground truths, two full sorts of a B x P tensor for hard-negative mining and boolean-mask gathers.  The
// semantics (the reference's, quirks included) are stated in tdrn_hip.h section (ii-b).
//
// Pipeline, all on one stream, no host synchronisation, no float atomics, every sum in a fixed order:
//   match_iou_kernel     (image, 256-prior chunk): truths staged in LDS; IoU (intersect/jaccard op order, correctly
//                        rounded division); per-prior best truth (ascending j, strict >); per-chunk (IoU, prior) maxima
//                        of every truth as order-preserving 64-bit keys into the workspace
//   match_encode_kernel  (image, chunk): per-truth best prior = max of the chunk keys (lowest prior on ties); forced
//                        matches of this chunk in an LDS map (integer atomicMax: the last truth j wins, as the
//                        reference's ascending loop); labels, threshold, encode -> loc_t, conf_t
//   (encode_kernel       : box_utils.encode alone, for the Python helper of the same name)
//   loss_rows_kernel     (image, chunk): per-row log-sum-exp with the row's own max -> CE of the row; block max
//   loss_score_kernel    (image, chunk): batch max from the block maxima; mining score with it, 0 on positives,
//                        as an order-preserving uint32 key
//   loss_select_kernel   (image): num_pos; radix select of the top num_neg keys, ties by prior index (= a stable
//                        descending sort's first num_neg); sel; per-image smooth-L1 and CE sums
//   loss_finish_kernel   (1 block): sums of the images in order, divided by N
//   loss_backward_kernel (image, chunk): grad_loc and grad_conf written in full; the softmax is recomputed
//
// Rounding: every operation that a test compares bit for bit against the reference (IoU, decode, encode, the
// threshold) must round as torch's separate elementwise ops do.  hipcc contracts a*b+c into an FMA by default, and the
// _rn intrinsics are plain operators here, so the helpers of box_coder.h would fuse (detect.hip's tdrn_decode does, and
// keeps doing: its bits are unchanged).  The Makefile compiles this file alone with -ffp-contract=off.

#include <climits>
#include <cmath>

#include "box_coder.h"
#include "kernels.h"

namespace tdrn {

namespace {

constexpr int kChunk = 256;          // priors (rows) per workgroup of the per-chunk kernels
constexpr int kSelThreads = 1024;    // one workgroup per image in loss_select_kernel

// order-preserving float -> uint32 (larger float -> larger key; -0 < +0; NaN above +inf)
__device__ __forceinline__ unsigned order_key(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct TruthSpan { int t0, n; };
__device__ __forceinline__ TruthSpan truth_span(const int32_t *off, int b, int T_total, int Tmax)
{
    // the caller promises off[b] <= off[b+1] <= T_total and counts <= Tmax; the clamps only keep memory safe
    int t0 = off[b], t1 = off[b + 1];
    t0 = t0 < 0 ? 0 : (t0 > T_total ? T_total : t0);
    t1 = t1 < t0 ? t0 : (t1 > T_total ? T_total : t1);
    const int n = t1 - t0 > Tmax ? Tmax : t1 - t0;
    return {t0, n};
}

// the box a prior is matched with: point_form(prior) (box_utils.py:4-13), or for refine_match the ARM decode of it
template <bool REFINE>
__device__ __forceinline__ void match_box(const float *priors, const float *arm, int b, int P, int p, float v0, float v1,
                                          float *box, float *enc)
{
    const f32x4 pr = *(const f32x4 *)(priors + (size_t)p * 4);
    float pf[4] = {pr[0], pr[1], pr[2], pr[3]};
    if (REFINE) {
        const f32x4 a = *(const f32x4 *)(arm + ((size_t)b * P + p) * 4);
        float af[4] = {a[0], a[1], a[2], a[3]};
        decode_one(af, pf, v0, v1, box);
        center_size_one(box, enc);              // refine_match encodes against center_size(decode_arm) (box_utils.py:148)
    } else {
        const float hw = __fdiv_rn(pf[2], 2.f), hh = __fdiv_rn(pf[3], 2.f);
        box[0] = __fsub_rn(pf[0], hw);
        box[1] = __fsub_rn(pf[1], hh);
        box[2] = __fadd_rn(pf[0], hw);
        box[3] = __fadd_rn(pf[1], hh);
        for (int i = 0; i < 4; ++i) enc[i] = pf[i];
    }
}

template <bool REFINE>
__global__ __launch_bounds__(kChunk) void match_iou_kernel(const float *__restrict__ truths, const int32_t *__restrict__ off,
                                                           int T_total, int Tmax, const float *__restrict__ priors, int P,
                                                           const float *__restrict__ arm, float v0, float v1,
                                                           int32_t *__restrict__ bt_idx, float *__restrict__ bt_ov,
                                                           unsigned long long *__restrict__ partial, int nch)
{
    __shared__ f32x4 tb[kMaxMatchTruths];
    __shared__ float ta[kMaxMatchTruths];
    __shared__ unsigned long long wbest[kChunk / 64][kMaxMatchTruths];
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = ch * kChunk + tid;
    const TruthSpan ts = truth_span(off, b, T_total, Tmax);
    for (int j = tid; j < ts.n; j += kChunk) {
        const float *t = truths + (size_t)(ts.t0 + j) * 5;
        const float x1 = t[0], y1 = t[1], x2 = t[2], y2 = t[3];
        tb[j] = f32x4{x1, y1, x2, y2};
        ta[j] = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));              // area_a (box_utils.py:63)
    }
    __syncthreads();
    const bool valid = p < P;
    float box[4] = {0.f, 0.f, 0.f, 0.f}, enc[4];
    if (valid) match_box<REFINE>(priors, arm, b, P, valid ? p : 0, v0, v1, box, enc);
    const float area_b = __fmul_rn(__fsub_rn(box[2], box[0]), __fsub_rn(box[3], box[1]));
    const unsigned pkey = 0xFFFFFFFFu - (unsigned)p;                           // lower prior index wins a tie
    float best = 0.f;
    int best_j = 0;
    for (int j = 0; j < ts.n; ++j) {
        const f32x4 t = tb[j];
        // intersect (box_utils.py:28-46): clamp(min(max_xy) - max(min_xy), 0), then the product
        const float iw = fmaxf(__fsub_rn(fminf(t[2], box[2]), fmaxf(t[0], box[0])), 0.f);
        const float ih = fmaxf(__fsub_rn(fminf(t[3], box[3]), fmaxf(t[1], box[1])), 0.f);
        const float inter = __fmul_rn(iw, ih);
        const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ta[j], area_b), inter));    // jaccard (:49-67)
        if (j == 0 || iou > best) {
            best = iou;
            best_j = j;
        }
        unsigned long long key = valid ? ((unsigned long long)order_key(iou) << 32) | pkey : 0ull;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long o = __shfl_xor(key, m, 64);
            key = o > key ? o : key;
        }
        if (lane == 0) wbest[wave][j] = key;
    }
    __syncthreads();
    for (int j = tid; j < ts.n; j += kChunk) {
        unsigned long long k = wbest[0][j];
        for (int w = 1; w < kChunk / 64; ++w) k = wbest[w][j] > k ? wbest[w][j] : k;
        partial[((size_t)b * nch + ch) * Tmax + j] = k;
    }
    if (valid) {
        bt_idx[(size_t)b * P + p] = best_j;
        bt_ov[(size_t)b * P + p] = best;
    }
}

template <bool REFINE>
__global__ __launch_bounds__(kChunk) void match_encode_kernel(const float *__restrict__ truths, const int32_t *__restrict__ off,
                                                              int T_total, int Tmax, const float *__restrict__ priors, int P,
                                                              const float *__restrict__ arm, float thr, float v0, float v1,
                                                              const int32_t *__restrict__ bt_idx, const float *__restrict__ bt_ov,
                                                              const unsigned long long *__restrict__ partial, int nch,
                                                              float *__restrict__ loc_t, int32_t *__restrict__ conf_t)
{
    __shared__ int forced[kChunk];
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
    const int p0 = ch * kChunk, p = p0 + tid;
    const TruthSpan ts = truth_span(off, b, T_total, Tmax);
    forced[tid] = -1;
    __syncthreads();
    // best prior of truth j = max over the chunks' keys (overlaps.max(1): lowest prior on a tie).  Forced matches
    // (box_utils.py:112-115): overlap 2 at that prior, and in ascending j best_truth_idx[best_prior_idx[j]] = j, so the
    // largest j of a shared best prior wins -- an integer max, independent of arrival order.
    for (int j = tid; j < ts.n; j += kChunk) {
        const unsigned long long *pj = partial + (size_t)b * nch * Tmax + j;
        unsigned long long k = pj[0];
        for (int c = 1; c < nch; ++c) {
            const unsigned long long o = pj[(size_t)c * Tmax];
            k = o > k ? o : k;
        }
        const int bp = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
        if (bp >= p0 && bp < p0 + kChunk) atomicMax(&forced[bp - p0], j);
    }
    __syncthreads();
    if (p >= P) return;
    const size_t r = (size_t)b * P + p;
    if (ts.n == 0) {                       // no truths: all background, zero targets (the reference fails in max here)
        *(f32x4 *)(loc_t + r * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        conf_t[r] = 0;
        return;
    }
    int j = bt_idx[r];
    float ov = bt_ov[r];
    if (forced[tid] >= 0) {
        j = forced[tid];
        ov = 2.f;
    }
    const float *t = truths + (size_t)(ts.t0 + j) * 5;
    const float m0 = t[0], m1 = t[1], m2 = t[2], m3 = t[3];
    // conf = labels + 1, stored into a LongTensor (truncation); background below the threshold (:117-118)
    const int conf = ov < thr ? 0 : (int)__fadd_rn(t[4], 1.f);
    float box[4], c[4];
    match_box<REFINE>(priors, arm, b, P, p, v0, v1, box, c);
    const float m[4] = {m0, m1, m2, m3};
    float g[4];
    encode_one(m, c, v0, v1, g);
    *(f32x4 *)(loc_t + r * 4) = f32x4{g[0], g[1], g[2], g[3]};
    conf_t[r] = conf;
}

__global__ __launch_bounds__(256) void encode_kernel(const float *__restrict__ matched, const float *__restrict__ priors, int P,
                                                     float v0, float v1, float *__restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const f32x4 a = *(const f32x4 *)(matched + (size_t)p * 4), b = *(const f32x4 *)(priors + (size_t)p * 4);
    const float m[4] = {a[0], a[1], a[2], a[3]}, pr[4] = {b[0], b[1], b[2], b[3]};
    float g[4];
    encode_one(m, pr, v0, v1, g);
    *(f32x4 *)(out + (size_t)p * 4) = f32x4{g[0], g[1], g[2], g[3]};
}

__device__ __forceinline__ int clamp_class(int t, int C) { return t < 0 ? 0 : (t >= C ? C - 1 : t); }

// per-row cross entropy with the row's own max (F.cross_entropy's log_softmax) and the block's max of the logits
__global__ __launch_bounds__(kChunk) void loss_rows_kernel(const float *__restrict__ conf, const int32_t *__restrict__ conf_t,
                                                           int P, int C, float *__restrict__ ce_row, float *__restrict__ gmax_part)
{
    __shared__ float red[kChunk / 64];
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, p = ch * kChunk + tid;
    float m = -INFINITY;
    if (p < P) {
        const size_t r = (size_t)b * P + p;
        const float *x = conf + r * C;
        for (int c = 0; c < C; ++c) m = fmaxf(m, x[c]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = __fadd_rn(s, expf(__fsub_rn(x[c], m)));
        ce_row[r] = __fsub_rn(__fadd_rn(m, logf(s)), x[clamp_class(conf_t[r], C)]);
    }
    for (int k = 32; k >= 1; k >>= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        float g = red[0];
        for (int w = 1; w < kChunk / 64; ++w) g = fmaxf(g, red[w]);
        gmax_part[blockIdx.y * gridDim.x + blockIdx.x] = g;
    }
}

// mining score (refine_multibox_loss.py:80-83): log_sum_exp with the BATCH max (box_utils.py:216-223) minus the target
// logit, 0 on positives; kept as its order-preserving key
__global__ __launch_bounds__(kChunk) void loss_score_kernel(const float *__restrict__ conf, const int32_t *__restrict__ conf_t,
                                                            int P, int C, const float *__restrict__ gmax_part, int nparts,
                                                            unsigned *__restrict__ key)
{
    __shared__ float red[kChunk / 64];
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, p = ch * kChunk + tid;
    float g = -INFINITY;
    for (int i = tid; i < nparts; i += kChunk) g = fmaxf(g, gmax_part[i]);
    for (int k = 32; k >= 1; k >>= 1) g = fmaxf(g, __shfl_xor(g, k, 64));
    if ((tid & 63) == 0) red[tid >> 6] = g;
    __syncthreads();
    g = red[0];
    for (int w = 1; w < kChunk / 64; ++w) g = fmaxf(g, red[w]);
    if (p >= P) return;
    const size_t r = (size_t)b * P + p;
    const int t = conf_t[r];
    float sc = 0.f;
    if (t <= 0) {
        const float *x = conf + r * C;
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = __fadd_rn(s, expf(__fsub_rn(x[c], g)));
        sc = __fsub_rn(__fadd_rn(logf(s), g), x[clamp_class(t, C)]);      // -inf when every exp underflows: ranks last
    }
    key[r] = order_key(sc);
}

// block-wide helpers of loss_select_kernel (kSelThreads threads)
__device__ __forceinline__ int block_sum_int(int v, int *red)
{
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < kSelThreads / 64; ++w) s += red[w];
    return s;
}
// exclusive prefix sum over the workgroup in thread order
__device__ __forceinline__ int block_exclusive_scan(int v, int *red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int k = 1; k < 64; k <<= 1) {
        const int o = __shfl_up(inc, k, 64);
        if (lane >= k) inc += o;
    }
    __syncthreads();
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += red[w];
    return base + inc - v;
}
// fixed-order float sum over the workgroup (a tree in LDS: the same bits on every run)
__device__ __forceinline__ float block_sum_float(float v, float *buf)
{
    __syncthreads();
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int s = kSelThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) buf[threadIdx.x] = __fadd_rn(buf[threadIdx.x], buf[threadIdx.x + s]);
        __syncthreads();
    }
    return buf[0];
}

__device__ __forceinline__ float smooth_l1(float x, float y)
{
    const float z = fabsf(__fsub_rn(x, y));
    return z < 1.f ? __fmul_rn(__fmul_rn(0.5f, z), z) : __fsub_rn(z, 0.5f);     // beta = 1 (F.smooth_l1_loss)
}

// One workgroup per image.  num_neg = min(negpos * num_pos, P - 1); a row is a mined negative when its rank in a stable
// descending sort of the score is below num_neg (refine_multibox_loss.py:85-88).  The rank threshold is found by a radix
// select over the 32-bit keys (4 passes of 8 bits, LDS histogram); keys equal to the threshold are taken in ascending
// prior index (a block scan over contiguous per-thread ranges).  key == NULL: only_loc (no mining, no CE).
__global__ __launch_bounds__(kSelThreads) void loss_select_kernel(const float *__restrict__ loc, const float *__restrict__ loc_t,
                                                                  const int32_t *__restrict__ conf_t,
                                                                  const unsigned *__restrict__ key, const float *__restrict__ ce_row,
                                                                  int P, int negpos, uint8_t *__restrict__ sel,
                                                                  int32_t *__restrict__ num_pos, float *__restrict__ img_part)
{
    __shared__ int hist[256];
    __shared__ int red[kSelThreads / 64];
    __shared__ float fbuf[kSelThreads];
    __shared__ unsigned s_digit;
    __shared__ int s_gt;
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)b * P;
    int cnt = 0;
    for (int i = tid; i < P; i += kSelThreads) cnt += conf_t[base + i] > 0;
    const int npos = block_sum_int(cnt, red);
    const long long want = key ? (long long)negpos * npos : 0;
    const int k = (int)(want < P - 1 ? want : P - 1);
    unsigned T = 0xFFFFFFFFu;
    int need = 0;                             // keys equal to T that are taken, lowest prior index first
    if (k > 0) {
        unsigned prefix = 0, pmask = 0;
        int kk = k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < P; i += kSelThreads) {
                const unsigned u = key[base + i];
                if ((u & pmask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
            }
            __syncthreads();
            // suffix sums: hist[d] <- number of candidates with digit >= d
            for (int s = 1; s < 256; s <<= 1) {
                int v = 0;
                if (tid < 256) v = tid + s < 256 ? hist[tid + s] : 0;
                __syncthreads();
                if (tid < 256) hist[tid] += v;
                __syncthreads();
            }
            if (tid < 256) {
                const int ge = hist[tid], gt = tid < 255 ? hist[tid + 1] : 0;
                if (gt < kk && ge >= kk) {
                    s_digit = (unsigned)tid;
                    s_gt = gt;
                }
            }
            __syncthreads();
            prefix |= s_digit << shift;
            pmask |= 255u << shift;
            kk -= s_gt;
            __syncthreads();
        }
        T = prefix;
        need = kk;
    }
    const int per = (P + kSelThreads - 1) / kSelThreads, i0 = tid * per, i1 = min(P, i0 + per);
    int eq = 0;
    if (k > 0)
        for (int i = i0; i < i1; ++i) eq += key[base + i] == T;
    int rank = block_exclusive_scan(eq, red);
    float sl = 0.f, sc = 0.f;
    for (int i = i0; i < i1; ++i) {
        const size_t r = base + i;
        const bool pos = conf_t[r] > 0;
        bool neg = false;
        if (k > 0) {
            const unsigned u = key[r];
            neg = u > T || (u == T && rank++ < need);
        }
        sel[r] = pos ? 1 : (neg ? 2 : 0);
        if (pos) {
            const f32x4 a = *(const f32x4 *)(loc + r * 4), t = *(const f32x4 *)(loc_t + r * 4);
            sl = __fadd_rn(sl, __fadd_rn(__fadd_rn(smooth_l1(a[0], t[0]), smooth_l1(a[1], t[1])),
                                         __fadd_rn(smooth_l1(a[2], t[2]), smooth_l1(a[3], t[3]))));
        }
        if (ce_row && (pos || neg)) sc = __fadd_rn(sc, ce_row[r]);
    }
    sl = block_sum_float(sl, fbuf);
    sc = block_sum_float(sc, fbuf);
    if (tid == 0) {
        img_part[2 * b] = sl;
        img_part[2 * b + 1] = sc;
        num_pos[b] = npos;
    }
}

__global__ void loss_finish_kernel(const float *__restrict__ img_part, const int32_t *__restrict__ num_pos, int B, int with_conf,
                                   float *__restrict__ loss_out)
{
    if (threadIdx.x != 0) return;
    long long n = 0;
    float sl = 0.f, sc = 0.f;
    for (int b = 0; b < B; ++b) {
        n += num_pos[b];
        sl = __fadd_rn(sl, img_part[2 * b]);
        sc = __fadd_rn(sc, img_part[2 * b + 1]);
    }
    const float N = (float)n;                 // num_pos.sum().float(); N = 0 gives 0/0, as the reference
    loss_out[0] = __fdiv_rn(sl, N);
    if (with_conf) loss_out[1] = __fdiv_rn(sc, N);
}

// d loss_l / d loc = g_l / N * clamp(loc - loc_t, -1, 1) on positives; d loss_c / d conf = g_c / N * (softmax - onehot) on
// pos u neg; 0 elsewhere.  The softmax is recomputed from the logits (one more read of a selected row, no saved B x P x C).
__global__ __launch_bounds__(kChunk) void loss_backward_kernel(const float *__restrict__ loc, const float *__restrict__ conf,
                                                               const float *__restrict__ loc_t, const int32_t *__restrict__ conf_t,
                                                               const uint8_t *__restrict__ sel, const int32_t *__restrict__ num_pos,
                                                               const float *__restrict__ grad_loss, int B, int P, int C,
                                                               float *__restrict__ grad_loc, float *__restrict__ grad_conf)
{
    __shared__ float s_q[2];
    const int b = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * kChunk + tid;
    if (tid == 0) {
        long long n = 0;
        for (int i = 0; i < B; ++i) n += num_pos[i];
        const float N = (float)n;
        s_q[0] = __fdiv_rn(grad_loss[0], N);
        s_q[1] = conf ? __fdiv_rn(grad_loss[1], N) : 0.f;
    }
    __syncthreads();
    if (p >= P) return;
    const size_t r = (size_t)b * P + p;
    const int s = sel[r];
    f32x4 gl = {0.f, 0.f, 0.f, 0.f};
    if (s == 1) {
        const float q = s_q[0];
        const f32x4 a = *(const f32x4 *)(loc + r * 4), t = *(const f32x4 *)(loc_t + r * 4);
        for (int i = 0; i < 4; ++i) gl[i] = __fmul_rn(q, fminf(fmaxf(__fsub_rn(a[i], t[i]), -1.f), 1.f));
    }
    *(f32x4 *)(grad_loc + r * 4) = gl;
    if (!conf) return;
    float *g = grad_conf + r * C;
    if (s == 0) {
        for (int c = 0; c < C; ++c) g[c] = 0.f;
        return;
    }
    const float q = s_q[1];
    const float *x = conf + r * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, x[c]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum = __fadd_rn(sum, expf(__fsub_rn(x[c], m)));
    const int t = clamp_class(conf_t[r], C);
    for (int c = 0; c < C; ++c) {
        const float sm = __fdiv_rn(expf(__fsub_rn(x[c], m)), sum);
        g[c] = __fmul_rn(q, c == t ? __fsub_rn(sm, 1.f) : sm);
    }
}

struct MatchWs { int32_t *bt_idx; float *bt_ov; unsigned long long *partial; size_t bytes; };
MatchWs match_ws(void *ws, int B, int P, int Tmax)
{
    const int nch = cdiv(P, kChunk);
    MatchWs w;
    char *c = (char *)ws;
    size_t o = 0;
    w.bt_idx = (int32_t *)(c + o);
    o += align_up((size_t)B * P * 4, 256);
    w.bt_ov = (float *)(c + o);
    o += align_up((size_t)B * P * 4, 256);
    w.partial = (unsigned long long *)(c + o);
    o += align_up((size_t)B * nch * Tmax * 8, 256);
    w.bytes = o;
    return w;
}

struct LossWs { float *ce_row; unsigned *key; float *gmax_part; float *img_part; size_t bytes; };
LossWs loss_ws(void *ws, int B, int P, int C)
{
    const int nch = cdiv(P, kChunk);
    LossWs w;
    char *c = (char *)ws;
    size_t o = 0;
    w.ce_row = nullptr;
    w.key = nullptr;
    w.gmax_part = nullptr;
    if (C > 0) {
        w.ce_row = (float *)(c + o);
        o += align_up((size_t)B * P * 4, 256);
        w.key = (unsigned *)(c + o);
        o += align_up((size_t)B * P * 4, 256);
        w.gmax_part = (float *)(c + o);
        o += align_up((size_t)B * nch * 4, 256);
    }
    w.img_part = (float *)(c + o);
    o += align_up((size_t)B * 2 * 4, 256);
    w.bytes = o;
    return w;
}

bool misaligned16(const void *p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

int launch_encode(const float *matched, const float *priors, int P, float v0, float v1, float *out, hipStream_t s)
{
    if (!matched || !priors || !out || P < 0) return TDRN_E_ARG;
    if (misaligned16(matched) || misaligned16(priors) || misaligned16(out)) return TDRN_E_ARG;
    if (P == 0) return TDRN_OK;
    hipLaunchKernelGGL(encode_kernel, dim3(cdiv(P, 256)), dim3(256), 0, s, matched, priors, P, v0, v1, out);
    return hip_status(hipGetLastError());
}

size_t match_workspace_bytes(int B, int P, int max_truths)
{
    if (B <= 0 || P <= 0 || max_truths < 0 || max_truths > kMaxMatchTruths || (long long)B * P > INT_MAX) return 0;
    return match_ws(nullptr, B, P, max_truths).bytes;
}

int launch_match(const float *truths, const int32_t *truth_off, int T_total, int max_truths, int B, const float *priors, int P,
                 const float *arm_loc, float threshold, float var0, float var1, float *loc_t, int32_t *conf_t, void *ws,
                 size_t ws_bytes, hipStream_t s)
{
    if (!truth_off || !priors || !loc_t || !conf_t || B <= 0 || P <= 0 || T_total < 0 || max_truths < 0) return TDRN_E_ARG;
    if (T_total > 0 && !truths) return TDRN_E_ARG;
    if (misaligned16(priors) || misaligned16(arm_loc) || misaligned16(loc_t)) return TDRN_E_ARG;   // (.,4) rows as 16-byte vectors
    if (max_truths > kMaxMatchTruths || (long long)B * P > INT_MAX) return TDRN_E_UNSUPPORTED;
    const size_t need = match_workspace_bytes(B, P, max_truths);
    if (ws_bytes < need) return TDRN_E_WORKSPACE;
    if (!ws) return TDRN_E_ARG;
    const MatchWs w = match_ws(ws, B, P, max_truths);
    const int nch = cdiv(P, kChunk);
    const dim3 grid(nch, B);
    if (arm_loc) {
        hipLaunchKernelGGL(match_iou_kernel<true>, grid, dim3(kChunk), 0, s, truths, truth_off, T_total, max_truths, priors, P,
                           arm_loc, var0, var1, w.bt_idx, w.bt_ov, w.partial, nch);
        hipLaunchKernelGGL(match_encode_kernel<true>, grid, dim3(kChunk), 0, s, truths, truth_off, T_total, max_truths, priors, P,
                           arm_loc, threshold, var0, var1, w.bt_idx, w.bt_ov, w.partial, nch, loc_t, conf_t);
    } else {
        hipLaunchKernelGGL(match_iou_kernel<false>, grid, dim3(kChunk), 0, s, truths, truth_off, T_total, max_truths, priors, P,
                           arm_loc, var0, var1, w.bt_idx, w.bt_ov, w.partial, nch);
        hipLaunchKernelGGL(match_encode_kernel<false>, grid, dim3(kChunk), 0, s, truths, truth_off, T_total, max_truths, priors, P,
                           arm_loc, threshold, var0, var1, w.bt_idx, w.bt_ov, w.partial, nch, loc_t, conf_t);
    }
    return hip_status(hipGetLastError());
}

size_t multibox_loss_workspace_bytes(int B, int P, int C)
{
    if (B <= 0 || P <= 0 || C < 0 || C > kMaxLossClasses || (long long)B * P > INT_MAX) return 0;
    return loss_ws(nullptr, B, P, C).bytes;
}

int launch_multibox_loss_forward(const float *loc, const float *conf, const float *loc_t, const int32_t *conf_t, int B, int P,
                                 int C, int negpos_ratio, float *loss_out, uint8_t *sel, int32_t *num_pos, void *ws,
                                 size_t ws_bytes, hipStream_t s)
{
    if (!loc || !loc_t || !conf_t || !loss_out || !sel || !num_pos || B <= 0 || P <= 0 || negpos_ratio < 0) return TDRN_E_ARG;
    if (conf && C <= 0) return TDRN_E_ARG;
    if (misaligned16(loc) || misaligned16(loc_t)) return TDRN_E_ARG;
    if ((conf && C > kMaxLossClasses) || (long long)B * P > INT_MAX) return TDRN_E_UNSUPPORTED;
    const int Cw = conf ? C : 0;
    const size_t need = multibox_loss_workspace_bytes(B, P, Cw);
    if (ws_bytes < need) return TDRN_E_WORKSPACE;
    if (!ws) return TDRN_E_ARG;
    const LossWs w = loss_ws(ws, B, P, Cw);
    const int nch = cdiv(P, kChunk);
    if (conf) {
        hipLaunchKernelGGL(loss_rows_kernel, dim3(nch, B), dim3(kChunk), 0, s, conf, conf_t, P, C, w.ce_row, w.gmax_part);
        hipLaunchKernelGGL(loss_score_kernel, dim3(nch, B), dim3(kChunk), 0, s, conf, conf_t, P, C, w.gmax_part, nch * B, w.key);
    }
    hipLaunchKernelGGL(loss_select_kernel, dim3(B), dim3(kSelThreads), 0, s, loc, loc_t, conf_t, (const unsigned *)w.key,
                       (const float *)w.ce_row, P, negpos_ratio, sel, num_pos, w.img_part);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, s, w.img_part, num_pos, B, conf ? 1 : 0, loss_out);
    return hip_status(hipGetLastError());
}

int launch_multibox_loss_backward(const float *loc, const float *conf, const float *loc_t, const int32_t *conf_t,
                                  const uint8_t *sel, const int32_t *num_pos, const float *grad_loss, int B, int P, int C,
                                  float *grad_loc, float *grad_conf, hipStream_t s)
{
    if (!loc || !loc_t || !conf_t || !sel || !num_pos || !grad_loss || !grad_loc || B <= 0 || P <= 0) return TDRN_E_ARG;
    if (conf && (C <= 0 || !grad_conf)) return TDRN_E_ARG;
    if (misaligned16(loc) || misaligned16(loc_t) || misaligned16(grad_loc)) return TDRN_E_ARG;
    if ((conf && C > kMaxLossClasses) || (long long)B * P > INT_MAX) return TDRN_E_UNSUPPORTED;
    hipLaunchKernelGGL(loss_backward_kernel, dim3(cdiv(P, kChunk), B), dim3(kChunk), 0, s, loc, conf, loc_t, conf_t, sel, num_pos,
                       grad_loss, B, P, C, grad_loc, conf ? grad_conf : nullptr);
    return hip_status(hipGetLastError());
}

}  // namespace tdrn
