// augment_pair.hip -- pairSSDAugmentation (utils/augmentations.py:637-689 of the reference) and the translated second frame
// of VOCDetection.pull_translational_item (data/voc0712.py:400-458) on the device, for a batch of raw uint8 frames.
// Semantics, quirks and deviations: tdrn_hip.h section (ii-d).  The shared device functions are augment_common.h's.
//
//   augment_pair_sample_kernel (1 block, one wave per image in turn): the translation attempts (the boxes on the lanes, a
//                         ballot per attempt), then every decision of the chain with the two-frame centre test inside the
//                         crop trials, the pair record, then -- after a block barrier and a scan of the kept counts -- both
//                         frames' moved boxes as two packed fp32 row sets behind one CSR offset array.
//   augment_pair_apply_kernel (256 output pixels of one pair per block): the geometry of an output pixel once (resize taps,
//                         mirror, crop, canvas); each tap is the mean for both frames or a source pixel of each frame -- the
//                         second frame's is the first's at (x - trans_x, y - trans_y), black outside -- distorted in
//                         registers with the shared values; blend, subtract the mean, store three planes per frame
//                         coalesced along x.  The translated frame, the distorted images, the canvases and the crops never
//                         exist.
//
// Built with -ffp-contract=off like augment.hip: pixels and boxes are compared bit for bit with unfused numpy arithmetic.

#include "augment_common.h"

namespace tdrn {
namespace {

// The two box sets of a pair.  Frame 1's fractions are the caller's rows, or frame 0's moved by (sx, sy) and clipped to
// [0, 1] when a translation attempt was accepted (sx = sy = 0 and no clip: the fallback's copy).
struct PairBoxes {
    ImageBoxes a;
    const double *rows_t;
    double sx, sy;
    bool clip;
    int n;
    __device__ void shift(int x, int y) { a.shift(x, y); }
    __device__ double frac_t(int i, int k) const
    {
        if (rows_t) return rows_t[(size_t)i * 5 + k];
        double v = a.rows[(size_t)i * 5 + k] + ((k & 1) ? sy : sx);
        if (clip) v = fmin(fmax(v, 0.0), 1.0);
        return v;
    }
    __device__ double label_t(int i) const { return (rows_t ? rows_t : a.rows)[(size_t)i * 5 + 4]; }
    __device__ void box_t(int i, double &x1, double &y1, double &x2, double &y2) const
    {
        x1 = frac_t(i, 0) * a.W + (double)a.dx;
        y1 = frac_t(i, 1) * a.H + (double)a.dy;
        x2 = frac_t(i, 2) * a.W + (double)a.dx;
        y2 = frac_t(i, 3) * a.H + (double)a.dy;
    }
    __device__ void centre_t(int i, double &cx, double &cy) const
    {
        double x1, y1, x2, y2;
        box_t(i, x1, y1, x2, y2);
        cx = (x1 + x2) / 2.0;
        cy = (y1 + y2) / 2.0;
    }
    // box i keeps its centre inside the rect in both frames (augmentations.py:374-388)
    __device__ bool centre_in(int i, const int rect[4]) const
    {
        double cx, cy;
        centre_t(i, cx, cy);
        return a.centre_in(i, rect) && inside(rect, cx, cy);
    }
    __device__ bool any_centre_in(const int r4[4]) const
    {
        bool found = false;
        for (int i = 0; i < n && !found; ++i) found = centre_in(i, r4);
        return found;
    }
    __device__ bool lanes_pass(bool cand, const int r4[4]) const
    {
        const int lane = threadIdx.x % kWave;
        bool pass = false;
        for (int c0 = 0; c0 < n; c0 += kWave) {
            double ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0;
            if (c0 + lane < n) {
                a.centre(c0 + lane, ax, ay);
                centre_t(c0 + lane, bx, by);
            }
            const int m = min(kWave, n - c0);
            for (int j = 0; j < m; ++j) {
                const double x0 = __shfl(ax, j, kWave), y0 = __shfl(ay, j, kWave);
                const double x1 = __shfl(bx, j, kWave), y1 = __shfl(by, j, kWave);
                pass = pass || (cand && inside(r4, x0, y0) && inside(r4, x1, y1));
            }
        }
        return pass;
    }
};

struct PairSampleArgs {
    const int32_t *hw;
    const double *truths, *truths_t;
    const int32_t *truth_off;
    int T_total, max_truths, B;
    double r;
    uint2 key;
    const int64_t *sample_ids;
    const double *tape;
    const int32_t *tape_off;
    tdrn_augment_pair_params *params;
    float *out_truths, *out_truths_t;
    int32_t *out_off;
};

__device__ PairBoxes pair_boxes(const PairSampleArgs &A, int b)
{
    int t0, n;
    span(A.truth_off, b, A.T_total, A.max_truths, t0, n);
    PairBoxes pb;
    pb.a.rows = A.truths + (size_t)t0 * 5;
    pb.a.n = n;
    pb.a.W = (double)A.hw[2 * b + 1];
    pb.a.H = (double)A.hw[2 * b];
    pb.a.dx = pb.a.dy = 0;
    pb.rows_t = A.truths_t ? A.truths_t + (size_t)t0 * 5 : nullptr;
    pb.sx = pb.sy = 0.0;
    pb.clip = false;
    pb.n = n;
    return pb;
}

// The translation of voc0712.py:411-434 for one image, every lane alike: up to three attempts, each drawing u_x then u_y; an
// attempt is accepted when every moved box keeps its centre strictly inside (0, 1) on both axes.  true: accepted.
template <class D>
__device__ bool translate(D &d, const ImageBoxes &ib, double r, int W, int H, tdrn_augment_pair_params &q)
{
    const int lane = threadIdx.x % kWave;
    for (int a = 1; a <= 3; ++a) {
        const double ux = d.uniform(0.0, 1.0, kSlotTrans + 2u * (uint32_t)(a - 1));
        const double uy = d.uniform(0.0, 1.0, kSlotTrans + 2u * (uint32_t)(a - 1) + 1u);
        const double xt = (-r / (double)a) + ((ux * 2.0) * r) / (double)a;
        const double yt = (-r / (double)a) + ((uy * 2.0) * r) / (double)a;
        q.attempts = a;
        bool out = false;
        for (int i0 = 0; i0 < ib.n; i0 += kWave) {
            const int i = i0 + lane;
            bool bad = false;
            if (i < ib.n) {
                const double *row = ib.rows + (size_t)i * 5;
                const double cx = ((row[0] + xt) + (row[2] + xt)) / 2.0, cy = ((row[1] + yt) + (row[3] + yt)) / 2.0;
                bad = !(cx > 0.0 && cy > 0.0 && cx < 1.0 && cy < 1.0);
            }
            out = out || __ballot(bad) != 0ull;
        }
        if (!out) {
            q.shift_x = xt;
            q.shift_y = yt;
            q.trans_x = (int)(xt * (double)W);
            q.trans_y = (int)(yt * (double)H);
            return true;
        }
    }
    return false;
}

template <class D>
__device__ tdrn_augment_pair_params decide_pair(D &d, PairBoxes &pb, double r, int W, int H)
{
    tdrn_augment_pair_params q;
    q.shift_x = q.shift_y = 0.0;
    q.trans_x = q.trans_y = q.attempts = q.reserved = 0;
    bool fallback = false;
    if (!pb.rows_t && pb.n > 0) {
        if (translate(d, pb.a, r, W, H, q)) {
            pb.sx = q.shift_x;
            pb.sy = q.shift_y;
            pb.clip = true;
        } else {
            fallback = true;
        }
    }
    q.base = decide(d, pb, W, H);
    if (fallback) q.base.status |= TDRN_AUGMENT_TRANS_FALLBACK;
    return q;
}

__global__ void __launch_bounds__(kSampleWaves * kWave) augment_pair_sample_kernel(PairSampleArgs A)
{
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
    // phase 1: the translation, the decisions and the kept count of every pair
    for (int b = wave; b < A.B; b += nw) {
        PairBoxes pb = pair_boxes(A, b);
        const int W = A.hw[2 * b + 1], H = A.hw[2 * b];
        tdrn_augment_pair_params q;
        if (A.sample_ids) {
            PhiloxDraws d;
            d.key = A.key;
            d.sid = (uint64_t)A.sample_ids[b];
            d.prefetch();
            q = decide_pair(d, pb, A.r, W, H);
        } else {
            TapeDraws d;
            int t0, n;
            span(A.tape_off, b, INT_MAX, INT_MAX, t0, n);
            d.tape = A.tape + t0;
            d.n = n;
            d.pos = 0;
            d.exhausted = false;
            q = decide_pair(d, pb, A.r, W, H);
        }
        int kept = pb.n;
        if (q.base.cropped) {
            pb.shift(q.base.img_x, q.base.img_y);
            const int rect[4] = {q.base.crop_x0, q.base.crop_y0, q.base.crop_x1, q.base.crop_y1};
            kept = 0;
            for (int i0 = 0; i0 < pb.n; i0 += kWave) {
                const bool in = i0 + lane < pb.n && pb.centre_in(i0 + lane, rect);
                kept += __popcll(__ballot(in));
            }
        }
        q.base.kept = kept;
        if (lane == 0) A.params[b] = q;
    }
    __syncthreads();
    // phase 2: CSR offsets of the kept rows, one array for both frames
    if (wave == 0) scan_kept(A.B, A.out_off, [&](int b) { return A.params[b].base.kept; });
    __syncthreads();
    // phase 3: the kept boxes of both frames, moved as the reference moves them (fp64), cast to fp32
    for (int b = wave; b < A.B; b += nw) {
        const tdrn_augment_pair_params q = A.params[b];
        const tdrn_augment_params &p = q.base;
        PairBoxes pb = pair_boxes(A, b);
        pb.shift(p.img_x, p.img_y);
        pb.sx = q.shift_x;
        pb.sy = q.shift_y;
        pb.clip = q.attempts > 0 && !(p.status & TDRN_AUGMENT_TRANS_FALLBACK);
        const int rect[4] = {p.crop_x0, p.crop_y0, p.crop_x1, p.crop_y1};
        const int wc = min(p.crop_x1, p.canvas_w) - p.crop_x0, hc = min(p.crop_y1, p.canvas_h) - p.crop_y0;
        int o = A.out_off[b];
        for (int i0 = 0; i0 < pb.n; i0 += kWave) {
            const int i = i0 + lane;
            const bool in = i < pb.n && (!p.cropped || pb.centre_in(i, rect));
            const unsigned long long ball = __ballot(in);
            const int j = o + __popcll(ball & ((1ull << lane) - 1ull));
            if (in && j < A.T_total) {          // j < T_total unless the offsets broke their promise (overlapping images)
                double x1, y1, x2, y2;
                pb.a.box(i, x1, y1, x2, y2);
                store_moved_box(p, wc, hc, x1, y1, x2, y2, pb.a.rows[(size_t)i * 5 + 4], A.out_truths + (size_t)j * 5);
                pb.box_t(i, x1, y1, x2, y2);
                store_moved_box(p, wc, hc, x1, y1, x2, y2, pb.label_t(i), A.out_truths_t + (size_t)j * 5);
            }
            o += __popcll(ball);
        }
    }
}

// ------------------------------------------------------------------------------------------------ pixels
struct PairApplyArgs {
    const tdrn_augment_image *images, *images_t;
    const tdrn_augment_pair_params *params;
    float mean[3];
    int S, to_rgb;
    float *out, *out_t;
};

__device__ __forceinline__ uint32_t load_bgr(const tdrn_augment_image &im, int x, int y)
{
    const uint8_t *q = im.data + ((size_t)y * im.w + x) * 3;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
}

__global__ void __launch_bounds__(kApplyBlock) augment_pair_apply_kernel(PairApplyArgs A)
{
    const int b = blockIdx.y;
    const int pix = blockIdx.x * kApplyBlock + threadIdx.x;
    const int S = A.S;
    if (pix >= S * S) return;
    const int oy = pix / S, ox = pix - oy * S;
    const tdrn_augment_params p = A.params[b].base;
    const tdrn_augment_image im = A.images[b];
    tdrn_augment_image it = im;                                           // where frame 1's pixels are read
    int tx = A.params[b].trans_x, ty = A.params[b].trans_y;
    if (A.images_t) {
        it = A.images_t[b];
        tx = ty = 0;
    }
    const int wc = max(min(p.crop_x1, p.canvas_w) - p.crop_x0, 1), hc = max(min(p.crop_y1, p.canvas_h) - p.crop_y0, 1);
    int xs[2], ys[2];
    float aw[2], bw[2];
    lin_coef(ox, S, wc, xs[0], xs[1], aw[0], aw[1]);
    lin_coef(oy, S, hc, ys[0], ys[1], bw[0], bw[1]);
    float hrow[2][2][3];                                                  // [frame][tap row][channel]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int iy = p.crop_y0 + ys[j] - p.img_y;                      // frame row of this tap row
        float t[2][2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int col = p.mirror ? wc - 1 - xs[i] : xs[i];
            const int ix = p.crop_x0 + col - p.img_x;
            if ((unsigned)ix < (unsigned)im.w && (unsigned)iy < (unsigned)im.h) {
                distort_tap(load_bgr(im, ix, iy), p, t[0][i]);
                // frame 1 at this place: its own pixel, or frame 0's at (x - tx, y - ty); black where that is outside
                const int sx = ix - tx, sy = iy - ty;
                const bool in = (unsigned)sx < (unsigned)it.w && (unsigned)sy < (unsigned)it.h;
                distort_tap(in ? load_bgr(it, sx, sy) : 0u, p, t[1][i]);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) t[0][i][c] = t[1][i][c] = A.mean[c];
            }
        }
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int c = 0; c < 3; ++c) hrow[f][j][c] = t[f][0][c] * aw[0] + t[f][1][c] * aw[1];
    }
    const size_t plane = (size_t)S * S;
    float *o0 = A.out + (size_t)b * 3 * plane + pix, *o1 = A.out_t + (size_t)b * 3 * plane + pix;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t at = (size_t)(A.to_rgb ? 2 - c : c) * plane;
        o0[at] = (hrow[0][0][c] * bw[0] + hrow[0][1][c] * bw[1]) - A.mean[c];
        o1[at] = (hrow[1][0][c] * bw[0] + hrow[1][1][c] * bw[1]) - A.mean[c];
    }
}

}  // namespace

int launch_augment_pair_sample(const int32_t *hw, const double *truths, const double *truths_t, const int32_t *truth_off,
                               int T_total, int max_truths, int B, double max_trans_ratio, uint64_t seed,
                               const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                               tdrn_augment_pair_params *params, float *out_truths, float *out_truths_t, int32_t *out_off,
                               hipStream_t s)
{
    if (!hw || !truth_off || !params || !out_off || B <= 0 || T_total < 0 || max_truths < 0) return TDRN_E_ARG;
    if (T_total > 0 && (!truths || !out_truths || !out_truths_t)) return TDRN_E_ARG;
    if ((sample_ids != nullptr) == (tape != nullptr || tape_off != nullptr)) return TDRN_E_ARG;   // exactly one source
    if (!sample_ids && (!tape || !tape_off)) return TDRN_E_ARG;
    if (!(max_trans_ratio >= 0.0 && max_trans_ratio < 1.0)) return TDRN_E_ARG;
    if (max_truths > TDRN_AUGMENT_MAX_TRUTHS) return TDRN_E_UNSUPPORTED;
    PairSampleArgs A;
    A.hw = hw;
    A.truths = truths;
    A.truths_t = truths_t;
    A.truth_off = truth_off;
    A.T_total = T_total;
    A.max_truths = max_truths;
    A.B = B;
    A.r = max_trans_ratio;
    A.key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    A.sample_ids = sample_ids;
    A.tape = tape;
    A.tape_off = tape_off;
    A.params = params;
    A.out_truths = out_truths;
    A.out_truths_t = out_truths_t;
    A.out_off = out_off;
    const int waves = B < kSampleWaves ? B : kSampleWaves;
    hipLaunchKernelGGL(augment_pair_sample_kernel, dim3(1), dim3(waves * kWave), 0, s, A);
    return hip_status(hipGetLastError());
}

int launch_augment_pair_apply(const tdrn_augment_image *images, const tdrn_augment_image *images_t,
                              const tdrn_augment_pair_params *params, int B, const float *mean, int S, int to_rgb, float *out,
                              float *out_t, hipStream_t s)
{
    if (!images || !params || !mean || !out || !out_t || B <= 0 || S <= 0) return TDRN_E_ARG;
    if (S > TDRN_AUGMENT_MAX_SIZE || B > 65535) return TDRN_E_UNSUPPORTED;
    PairApplyArgs A;
    A.images = images;
    A.images_t = images_t;
    A.params = params;
    A.mean[0] = mean[0];
    A.mean[1] = mean[1];
    A.mean[2] = mean[2];
    A.S = S;
    A.to_rgb = to_rgb ? 1 : 0;
    A.out = out;
    A.out_t = out_t;
    hipLaunchKernelGGL(augment_pair_apply_kernel, dim3(cdiv(S * S, kApplyBlock), B), dim3(kApplyBlock), 0, s, A);
    return hip_status(hipGetLastError());
}

}  // namespace tdrn
