// augment.hip -- SSDAugmentation (utils/augmentations.py:618-635 of the reference) on the device, for a batch of raw uint8
// frames.  Semantics, quirks and deviations: tdrn_hip.h section (ii-c).
//
//   augment_sample_kernel (1 block, one wave per image in turn): every decision of one image from its draw source, the
//                         parameter record, then -- after a block barrier and a scan of the kept counts -- the moved boxes as
//                         packed fp32 rows with CSR offsets.  Draw sources: Philox4x32-10 (the crop trials of a mode round on
//                         the lanes, lowest passing lane wins) or a tape of recorded draws (sequential, every lane alike).
//   augment_apply_kernel  (256 output pixels of one image per block): output pixel -> resize taps -> mirror -> crop ->
//                         canvas; a tap is the mean or a source pixel, distorted in registers (brightness, contrast, HSV
//                         round trip, saturation, hue, contrast, channel permutation); blend, subtract the mean, store the
//                         three planes coalesced along x.  The distorted image, the canvas and the crop never exist.
//
// Rounding: the pixels and boxes are compared bit for bit with the reference's unfused numpy / cv2 arithmetic, so the
// Makefile builds this file with -ffp-contract=off (no a*b+c -> FMA); fp32 division and the fp64 box arithmetic are
// correctly rounded.

#include <cmath>

#include "common.h"
#include "kernels.h"

namespace tdrn {
namespace {

constexpr int kWave = 64;
constexpr int kTrials = 50;
constexpr int kSampleWaves = 16;
constexpr int kApplyBlock = 256;

// ------------------------------------------------------------------------------------------------ draw sources
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k)
{
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += W0;
        k.y += W1;
    }
    return c;
}

// Draw slots of the Philox source: a fixed counter per decision, so that lanes can run crop trials side by side.
enum : uint32_t {
    kSlotBrightOn, kSlotBright, kSlotPre, kSlotContrastOn, kSlotContrast, kSlotSatOn, kSlotSat, kSlotHueOn, kSlotHue,
    kSlotPermOn, kSlotPerm, kSlotExpandOn, kSlotRatio, kSlotLeft, kSlotTop, kSlotMirror, kSlotRounds = 32
};
__device__ __forceinline__ uint32_t slot_mode(int r) { return kSlotRounds + (uint32_t)r * 256u; }
__device__ __forceinline__ uint32_t slot_trial(int r, int t, int k) { return slot_mode(r) + 1u + (uint32_t)t * 4u + (uint32_t)k; }

struct PhiloxDraws {
    uint2 key;
    uint64_t sid;
    static constexpr bool kTape = false;
    bool exhausted = false;
    uint32_t pre_x, pre_y;   // lane l < kSlotMirror + 1: words of slot l; lane 16 + r (r < 32): words of slot_mode(r)
    __device__ uint4 raw(uint32_t slot) const
    {
        return philox4x32_10(make_uint4(slot, 0u, (uint32_t)sid, (uint32_t)(sid >> 32)), key);
    }
    // every lane of the wave calls this first (converged): one Philox per lane instead of ~50 in a row per image
    __device__ void prefetch()
    {
        const int lane = threadIdx.x % kWave;
        const uint4 w = raw(lane < 16 ? (uint32_t)lane : slot_mode(lane < 48 ? lane - 16 : 0));
        pre_x = w.x;
        pre_y = w.y;
    }
    // the two words of `slot`; called with the same slot on every active lane
    __device__ void words(uint32_t slot, uint32_t &x, uint32_t &y) const
    {
        const int src = slot < 16 ? (int)slot : ((slot - kSlotRounds) % 256u == 0 && slot < slot_mode(32) ? 16 + (int)((slot - kSlotRounds) / 256u) : -1);
        if (src >= 0) {
            x = (uint32_t)__shfl((int)pre_x, src, kWave);
            y = (uint32_t)__shfl((int)pre_y, src, kWave);
        } else {
            const uint4 w = raw(slot);
            x = w.x;
            y = w.y;
        }
    }
    __device__ int randint(int n, uint32_t slot) const
    {
        uint32_t x, y;
        words(slot, x, y);
        return (int)(((uint64_t)x * (uint32_t)n) >> 32);
    }
    __device__ double uniform(double lo, double hi, uint32_t slot) const
    {
        uint32_t x, y;                   // 53-bit double in [0, 1), as numpy builds one from two words
        words(slot, x, y);
        const double u = ((double)(x >> 5) * 67108864.0 + (double)(y >> 6)) * (1.0 / 9007199254740992.0);
        return lo + (hi - lo) * u;
    }
};

struct TapeDraws {
    const double *tape;
    int n, pos;
    static constexpr bool kTape = true;
    bool exhausted;
    __device__ double next()
    {
        if (pos >= n) { exhausted = true; return 0.0; }
        return tape[pos++];
    }
    __device__ int randint(int, uint32_t) { return (int)next(); }
    __device__ double uniform(double, double, uint32_t) { return next(); }
};

// ------------------------------------------------------------------------------------------------ boxes
struct ImageBoxes {
    const double *rows;   // (n,5) fp64 fractions
    int n;
    double W, H;          // the frame's size
    int dx, dy;           // expand shift
    // absolute box i after ToAbsoluteCoords and Expand, in the reference's op order
    __device__ void box(int i, double &x1, double &y1, double &x2, double &y2) const
    {
        const double *r = rows + (size_t)i * 5;
        x1 = r[0] * W + (double)dx;
        y1 = r[1] * H + (double)dy;
        x2 = r[2] * W + (double)dx;
        y2 = r[3] * H + (double)dy;
    }
    __device__ void centre(int i, double &cx, double &cy) const
    {
        double x1, y1, x2, y2;
        box(i, x1, y1, x2, y2);
        cx = (x1 + x2) / 2.0;
        cy = (y1 + y2) / 2.0;
    }
    __device__ bool centre_in(int i, const int rect[4]) const;
};

__device__ __forceinline__ bool inside(const int rect[4], double cx, double cy);
__device__ bool ImageBoxes::centre_in(int i, const int rect[4]) const
{
    double cx, cy;
    centre(i, cx, cy);
    return inside(rect, cx, cy);
}

// One RandomSampleCrop trial's rect (augmentations.py:266-278).  false: rejected by the aspect test; stop: the tape ran out.
template <class D>
__device__ bool crop_rect(D &d, int r, int t, int cw, int ch, int rect[4], bool &stop)
{
    const double w = d.uniform(0.3 * cw, (double)cw, slot_trial(r, t, 0));
    const double h = d.uniform(0.3 * ch, (double)ch, slot_trial(r, t, 1));
    if (d.exhausted) { stop = true; return false; }
    if (h / w < 0.5 || h / w > 2) return false;
    const double left = d.uniform((double)cw - w, 1.0, slot_trial(r, t, 2));
    const double top = d.uniform((double)ch - h, 1.0, slot_trial(r, t, 3));
    rect[0] = (int)left;
    rect[1] = (int)top;
    rect[2] = (int)(left + w);
    rect[3] = (int)(top + h);
    return true;
}

__device__ __forceinline__ bool inside(const int rect[4], double cx, double cy)
{
    return (double)rect[0] < cx && (double)rect[1] < cy && (double)rect[2] > cx && (double)rect[3] > cy;
}

// Every decision of one image; all lanes of the wave compute the same record (the Philox crop trials meet in a ballot).
template <class D>
__device__ tdrn_augment_params decide(D &d, const ImageBoxes &ib_in, int W, int H)
{
    tdrn_augment_params p;
    p.brightness = 0.f;
    p.contrast_pre = p.contrast_post = p.saturation = 1.f;
    p.hue = 0.f;
    p.perm[0] = 0; p.perm[1] = 1; p.perm[2] = 2;
    p.status = 0;
    if (d.randint(2, kSlotBrightOn)) p.brightness = (float)d.uniform(-32.0, 32.0, kSlotBright);
    const int pre = d.randint(2, kSlotPre);
    if (pre && d.randint(2, kSlotContrastOn)) p.contrast_pre = (float)d.uniform(0.5, 1.5, kSlotContrast);
    if (d.randint(2, kSlotSatOn)) p.saturation = (float)d.uniform(0.5, 1.5, kSlotSat);
    if (d.randint(2, kSlotHueOn)) p.hue = (float)d.uniform(-18.0, 18.0, kSlotHue);
    if (!pre && d.randint(2, kSlotContrastOn)) p.contrast_post = (float)d.uniform(0.5, 1.5, kSlotContrast);
    if (d.randint(2, kSlotPermOn)) {
        const int k = d.randint(6, kSlotPerm);
        const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        const int kk = k < 0 ? 0 : (k > 5 ? 5 : k);
        p.perm[0] = perms[kk][0]; p.perm[1] = perms[kk][1]; p.perm[2] = perms[kk][2];
    }
    int cw = W, ch = H, ix = 0, iy = 0;
    if (!d.randint(2, kSlotExpandOn)) {
        const double ratio = d.uniform(1.0, 4.0, kSlotRatio);
        const double left = d.uniform(0.0, (double)W * ratio - (double)W, kSlotLeft);
        const double top = d.uniform(0.0, (double)H * ratio - (double)H, kSlotTop);
        cw = (int)((double)W * ratio);
        ch = (int)((double)H * ratio);
        ix = (int)left;
        iy = (int)top;
    }
    p.canvas_w = cw; p.canvas_h = ch; p.img_x = ix; p.img_y = iy;
    ImageBoxes ib = ib_in;
    ib.dx = ix;
    ib.dy = iy;
    int rect[4] = {0, 0, cw, ch};
    p.cropped = 0;
    if (ib.n > 0) {
        int round = 0;
        for (;; ++round) {
            if (round == TDRN_AUGMENT_MAX_ROUNDS) { p.status |= TDRN_AUGMENT_CROP_FALLBACK; break; }
            if (d.randint(6, slot_mode(round)) == 0) break;
            bool stop = false, found = false;
            int r4[4];
            if (D::kTape) {
                for (int t = 0; t < kTrials && !found && !stop; ++t) {
                    if (!crop_rect(d, round, t, cw, ch, r4, stop)) continue;
                    for (int i = 0; i < ib.n && !found; ++i) found = ib.centre_in(i, r4);
                }
            } else {
                // the trials on the lanes; the box centres go round the wave by shuffles, 64 at a time (converged code)
                const int lane = threadIdx.x % kWave;
                const bool cand = lane < kTrials && crop_rect(d, round, lane, cw, ch, r4, stop);
                bool pass = false;
                for (int c0 = 0; c0 < ib.n; c0 += kWave) {
                    double cx = 0.0, cy = 0.0;
                    if (c0 + lane < ib.n) ib.centre(c0 + lane, cx, cy);
                    const int m = min(kWave, ib.n - c0);
                    for (int j = 0; j < m; ++j) {
                        const double x = __shfl(cx, j, kWave), y = __shfl(cy, j, kWave);
                        pass = pass || (cand && inside(r4, x, y));
                    }
                }
                const unsigned long long ball = __ballot(pass);
                if (ball) {
                    const int win = __ffsll((long long)ball) - 1;
                    for (int k = 0; k < 4; ++k) r4[k] = __shfl(r4[k], win, kWave);
                    found = true;
                }
            }
            if (found) {
                for (int k = 0; k < 4; ++k) rect[k] = r4[k];
                p.cropped = 1;
                break;
            }
            if (stop || d.exhausted) break;
        }
    }
    p.crop_x0 = rect[0]; p.crop_y0 = rect[1]; p.crop_x1 = rect[2]; p.crop_y1 = rect[3];
    p.mirror = d.randint(2, kSlotMirror) ? 1 : 0;
    if (d.exhausted) p.status |= TDRN_AUGMENT_TAPE_EXHAUSTED;
    return p;
}

struct SampleArgs {
    const int32_t *hw;
    const double *truths;
    const int32_t *truth_off;
    int T_total, max_truths, B;
    uint2 key;
    const int64_t *sample_ids;
    const double *tape;
    const int32_t *tape_off;
    tdrn_augment_params *params;
    float *out_truths;
    int32_t *out_off;
};

__device__ __forceinline__ void span(const int32_t *off, int b, int total, int cap, int &t0, int &n)
{
    // the caller promises off[b] <= off[b+1] <= total and counts <= cap; the clamps only keep memory safe
    int a = off[b], e = off[b + 1];
    a = a < 0 ? 0 : (a > total ? total : a);
    e = e < a ? a : (e > total ? total : e);
    if (e - a > cap) e = a + cap;
    t0 = a;
    n = e - a;
}

__device__ ImageBoxes image_boxes(const SampleArgs &A, int b)
{
    int t0, n;
    span(A.truth_off, b, A.T_total, A.max_truths, t0, n);
    ImageBoxes ib;
    ib.rows = A.truths + (size_t)t0 * 5;
    ib.n = n;
    ib.W = (double)A.hw[2 * b + 1];
    ib.H = (double)A.hw[2 * b];
    ib.dx = ib.dy = 0;
    return ib;
}

__global__ void __launch_bounds__(kSampleWaves * kWave) augment_sample_kernel(SampleArgs A)
{
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
    // phase 1: the decisions and the kept count of every image
    for (int b = wave; b < A.B; b += nw) {
        const ImageBoxes ib = image_boxes(A, b);
        const int W = A.hw[2 * b + 1], H = A.hw[2 * b];
        tdrn_augment_params p;
        if (A.sample_ids) {
            PhiloxDraws d;
            d.key = A.key;
            d.sid = (uint64_t)A.sample_ids[b];
            d.prefetch();
            p = decide(d, ib, W, H);
        } else {
            TapeDraws d;
            int t0, n;
            span(A.tape_off, b, INT_MAX, INT_MAX, t0, n);
            d.tape = A.tape + t0;
            d.n = n;
            d.pos = 0;
            d.exhausted = false;
            p = decide(d, ib, W, H);
        }
        int kept = ib.n;
        if (p.cropped) {
            ImageBoxes sb = ib;
            sb.dx = p.img_x;
            sb.dy = p.img_y;
            const int rect[4] = {p.crop_x0, p.crop_y0, p.crop_x1, p.crop_y1};
            kept = 0;
            for (int i0 = 0; i0 < ib.n; i0 += kWave) {
                const bool in = i0 + lane < ib.n && sb.centre_in(i0 + lane, rect);
                kept += __popcll(__ballot(in));
            }
        }
        p.kept = kept;
        if (lane == 0) A.params[b] = p;
    }
    __syncthreads();
    // phase 2: CSR offsets of the kept rows (wave 0, 64 images per step)
    if (wave == 0) {
        int base = 0;
        for (int b0 = 0; b0 < A.B; b0 += kWave) {
            const int b = b0 + lane;
            const int k = b < A.B ? A.params[b].kept : 0;
            int incl = k;
            for (int o = 1; o < kWave; o <<= 1) {
                const int v = __shfl_up(incl, o, kWave);
                if (lane >= o) incl += v;
            }
            if (b < A.B) A.out_off[b] = base + incl - k;
            base += __shfl(incl, kWave - 1, kWave);
        }
        if (lane == 0) A.out_off[A.B] = base;
    }
    __syncthreads();
    // phase 3: the kept boxes, moved as the reference moves them (fp64), cast to fp32
    for (int b = wave; b < A.B; b += nw) {
        const tdrn_augment_params p = A.params[b];
        ImageBoxes ib = image_boxes(A, b);
        ib.dx = p.img_x;
        ib.dy = p.img_y;
        const int rect[4] = {p.crop_x0, p.crop_y0, p.crop_x1, p.crop_y1};
        const int wc = min(p.crop_x1, p.canvas_w) - p.crop_x0, hc = min(p.crop_y1, p.canvas_h) - p.crop_y0;
        int o = A.out_off[b];
        for (int i0 = 0; i0 < ib.n; i0 += kWave) {
            const int i = i0 + lane;
            const bool in = i < ib.n && (!p.cropped || ib.centre_in(i, rect));
            const unsigned long long ball = __ballot(in);
            const int j = o + __popcll(ball & ((1ull << lane) - 1ull));
            if (in && j < A.T_total) {          // j < T_total unless the offsets broke their promise (overlapping images)
                double x1, y1, x2, y2;
                ib.box(i, x1, y1, x2, y2);
                if (p.cropped) {
                    x1 = fmax(x1, (double)rect[0]) - (double)rect[0];
                    y1 = fmax(y1, (double)rect[1]) - (double)rect[1];
                    x2 = fmin(x2, (double)rect[2]) - (double)rect[0];
                    y2 = fmin(y2, (double)rect[3]) - (double)rect[1];
                }
                if (p.mirror) {
                    const double m1 = (double)wc - x2, m2 = (double)wc - x1;
                    x1 = m1;
                    x2 = m2;
                }
                x1 /= (double)wc;
                x2 /= (double)wc;
                y1 /= (double)hc;
                y2 /= (double)hc;
                float *row = A.out_truths + (size_t)j * 5;
                row[0] = (float)x1;
                row[1] = (float)y1;
                row[2] = (float)x2;
                row[3] = (float)y2;
                row[4] = (float)ib.rows[(size_t)i * 5 + 4];
            }
            o += __popcll(ball);
        }
    }
}

// ------------------------------------------------------------------------------------------------ pixels
// cv2.cvtColor BGR2HSV / HSV2BGR, fp32 (OpenCV's scalar float path, restated from memory; pinned by tests/_augment_ref.py's
// known answers).  diff: (float)(60. / (diff + FLT_EPSILON)) equals the fp32 quotient (double rounding of a quotient of floats
// is innocuous).
__device__ __forceinline__ void distort_tap(uint32_t bgr, const tdrn_augment_params &p, float out[3])
{
    const float eps = 1.1920928955078125e-7f;
    float b = (float)(bgr & 0xff), g = (float)((bgr >> 8) & 0xff), r = (float)((bgr >> 16) & 0xff);
    b = (b + p.brightness) * p.contrast_pre;
    g = (g + p.brightness) * p.contrast_pre;
    r = (r + p.brightness) * p.contrast_pre;
    float v = r, vmin = r;
    if (v < g) v = g;
    if (v < b) v = b;
    if (vmin > g) vmin = g;
    if (vmin > b) vmin = b;
    const float diff = v - vmin;
    float s = diff / (fabsf(v) + eps);
    const float d = 60.f / (diff + eps);
    float h;
    if (v == r) h = (g - b) * d;
    else if (v == g) h = (b - r) * d + 120.f;
    else h = (r - g) * d + 240.f;
    if (h < 0.f) h += 360.f;
    s = s * p.saturation;
    h = h + p.hue;
    if (h > 360.f) h -= 360.f;
    if (h < 0.f) h += 360.f;
    float c[3];
    if (s == 0.f) {
        c[0] = c[1] = c[2] = v;
    } else {
        h = h * (6.f / 360.f);
        while (h < 0.f) h += 6.f;
        while (h >= 6.f) h -= 6.f;
        int sector = (int)floorf(h);
        h = h - (float)sector;
        if ((unsigned)sector >= 6u) { sector = 0; h = 0.f; }
        const float tab[4] = {v, v * (1.f - s), v * (1.f - s * h), v * (1.f - s * (1.f - h))};
        const int sd[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};
        c[0] = tab[sd[sector][0]];
        c[1] = tab[sd[sector][1]];
        c[2] = tab[sd[sector][2]];
    }
    c[0] *= p.contrast_post;
    c[1] *= p.contrast_post;
    c[2] *= p.contrast_post;
    out[0] = c[p.perm[0]];
    out[1] = c[p.perm[1]];
    out[2] = c[p.perm[2]];
}

// cv2.resize INTER_LINEAR index and weight of destination d over n_src (oracle.base_transform_u8's rule, float weights)
__device__ __forceinline__ void lin_coef(int d, int n_dst, int n_src, int &s0, int &s1, float &w0, float &w1)
{
    float f = (float)(((double)d + 0.5) * ((double)n_src / (double)n_dst) - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
    s0 = s;
    s1 = min(s + 1, n_src - 1);
    w0 = 1.f - f;
    w1 = f;
}

struct ApplyArgs {
    const tdrn_augment_image *images;
    const tdrn_augment_params *params;
    float mean[3];
    int S, to_rgb;
    float *out;
};

__global__ void __launch_bounds__(kApplyBlock) augment_apply_kernel(ApplyArgs A)
{
    const int b = blockIdx.y;
    const int pix = blockIdx.x * kApplyBlock + threadIdx.x;
    const int S = A.S;
    if (pix >= S * S) return;
    const int oy = pix / S, ox = pix - oy * S;
    const tdrn_augment_params p = A.params[b];
    const tdrn_augment_image im = A.images[b];
    const int wc = max(min(p.crop_x1, p.canvas_w) - p.crop_x0, 1), hc = max(min(p.crop_y1, p.canvas_h) - p.crop_y0, 1);
    int xs[2], ys[2];
    float aw[2], bw[2];
    lin_coef(ox, S, wc, xs[0], xs[1], aw[0], aw[1]);
    lin_coef(oy, S, hc, ys[0], ys[1], bw[0], bw[1]);
    float hrow[2][3];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int iy = p.crop_y0 + ys[j] - p.img_y;                      // frame row of this tap row
        float t[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int col = p.mirror ? wc - 1 - xs[i] : xs[i];
            const int ix = p.crop_x0 + col - p.img_x;
            if ((unsigned)ix < (unsigned)im.w && (unsigned)iy < (unsigned)im.h) {
                const uint8_t *q = im.data + ((size_t)iy * im.w + ix) * 3;
                distort_tap((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16), p, t[i]);
            } else {
                t[i][0] = A.mean[0]; t[i][1] = A.mean[1]; t[i][2] = A.mean[2];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) hrow[j][c] = t[0][c] * aw[0] + t[1][c] * aw[1];
    }
    const size_t plane = (size_t)S * S;
    float *o = A.out + (size_t)b * 3 * plane + pix;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = (hrow[0][c] * bw[0] + hrow[1][c] * bw[1]) - A.mean[c];
        o[(A.to_rgb ? 2 - c : c) * plane] = v;
    }
}

}  // namespace

int launch_augment_sample(const int32_t *hw, const double *truths, const int32_t *truth_off, int T_total, int max_truths, int B,
                          uint64_t seed, const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                          tdrn_augment_params *params, float *out_truths, int32_t *out_off, hipStream_t s)
{
    if (!hw || !truth_off || !params || !out_off || B <= 0 || T_total < 0 || max_truths < 0) return TDRN_E_ARG;
    if (T_total > 0 && (!truths || !out_truths)) return TDRN_E_ARG;
    if ((sample_ids != nullptr) == (tape != nullptr || tape_off != nullptr)) return TDRN_E_ARG;   // exactly one source
    if (!sample_ids && (!tape || !tape_off)) return TDRN_E_ARG;
    if (max_truths > TDRN_AUGMENT_MAX_TRUTHS) return TDRN_E_UNSUPPORTED;
    SampleArgs A;
    A.hw = hw;
    A.truths = truths;
    A.truth_off = truth_off;
    A.T_total = T_total;
    A.max_truths = max_truths;
    A.B = B;
    A.key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    A.sample_ids = sample_ids;
    A.tape = tape;
    A.tape_off = tape_off;
    A.params = params;
    A.out_truths = out_truths;
    A.out_off = out_off;
    const int waves = B < kSampleWaves ? B : kSampleWaves;
    hipLaunchKernelGGL(augment_sample_kernel, dim3(1), dim3(waves * kWave), 0, s, A);
    return hip_status(hipGetLastError());
}

int launch_augment_apply(const tdrn_augment_image *images, const tdrn_augment_params *params, int B, const float *mean, int S,
                         int to_rgb, float *out, hipStream_t s)
{
    if (!images || !params || !mean || !out || B <= 0 || S <= 0) return TDRN_E_ARG;
    if (S > TDRN_AUGMENT_MAX_SIZE || B > 65535) return TDRN_E_UNSUPPORTED;
    ApplyArgs A;
    A.images = images;
    A.params = params;
    A.mean[0] = mean[0];
    A.mean[1] = mean[1];
    A.mean[2] = mean[2];
    A.S = S;
    A.to_rgb = to_rgb ? 1 : 0;
    A.out = out;
    hipLaunchKernelGGL(augment_apply_kernel, dim3(cdiv(S * S, kApplyBlock), B), dim3(kApplyBlock), 0, s, A);
    return hip_status(hipGetLastError());
}

}  // namespace tdrn
