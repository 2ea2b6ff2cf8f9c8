// augment_common.h -- device functions shared by augment.hip (SSDAugmentation) and augment_pair.hip (pairSSDAugmentation):
// the draw sources, the box helpers, one crop trial, every decision of one image, the photometric distortion of one tap and
// the resize coefficients.  Semantics: tdrn_hip.h sections (ii-c) and (ii-d).  Both files are built with -ffp-contract=off.
#pragma once

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
// kSlotTrans + 2 * a and + 2 * a + 1 are the pair sampler's translation draws of attempt a (section ii-d).
enum : uint32_t {
    kSlotBrightOn, kSlotBright, kSlotPre, kSlotContrastOn, kSlotContrast, kSlotSatOn, kSlotSat, kSlotHueOn, kSlotHue,
    kSlotPermOn, kSlotPerm, kSlotExpandOn, kSlotRatio, kSlotLeft, kSlotTop, kSlotMirror, kSlotTrans = 16, kSlotRounds = 32
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
__device__ __forceinline__ bool inside(const int rect[4], double cx, double cy)
{
    return (double)rect[0] < cx && (double)rect[1] < cy && (double)rect[2] > cx && (double)rect[3] > cy;
}

struct ImageBoxes {
    const double *rows;   // (n,5) fp64 fractions
    int n;
    double W, H;          // the frame's size
    int dx, dy;           // expand shift
    __device__ void shift(int x, int y) { dx = x; dy = y; }
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
    __device__ bool centre_in(int i, const int rect[4]) const
    {
        double cx, cy;
        centre(i, cx, cy);
        return inside(rect, cx, cy);
    }
    // a crop trial's test, one trial after the other (tape): does some box keep its centre inside r4
    __device__ bool any_centre_in(const int r4[4]) const
    {
        bool found = false;
        for (int i = 0; i < n && !found; ++i) found = centre_in(i, r4);
        return found;
    }
    // the same with a trial per lane: the box centres go round the wave by shuffles, 64 at a time (converged code)
    __device__ bool lanes_pass(bool cand, const int r4[4]) const
    {
        const int lane = threadIdx.x % kWave;
        bool pass = false;
        for (int c0 = 0; c0 < n; c0 += kWave) {
            double cx = 0.0, cy = 0.0;
            if (c0 + lane < n) centre(c0 + lane, cx, cy);
            const int m = min(kWave, n - c0);
            for (int j = 0; j < m; ++j) {
                const double x = __shfl(cx, j, kWave), y = __shfl(cy, j, kWave);
                pass = pass || (cand && inside(r4, x, y));
            }
        }
        return pass;
    }
};

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

// Every decision of one image; all lanes of the wave compute the same record (the Philox crop trials meet in a ballot).
// BX holds the image's boxes (ImageBoxes, or the two box sets of a pair): n, shift(), any_centre_in(), lanes_pass().
template <class D, class BX>
__device__ tdrn_augment_params decide(D &d, const BX &bx_in, int W, int H)
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
    BX bx = bx_in;
    bx.shift(ix, iy);
    int rect[4] = {0, 0, cw, ch};
    p.cropped = 0;
    if (bx.n > 0) {
        int round = 0;
        for (;; ++round) {
            if (round == TDRN_AUGMENT_MAX_ROUNDS) { p.status |= TDRN_AUGMENT_CROP_FALLBACK; break; }
            if (d.randint(6, slot_mode(round)) == 0) break;
            bool stop = false, found = false;
            int r4[4];
            if (D::kTape) {
                for (int t = 0; t < kTrials && !found && !stop; ++t) {
                    if (!crop_rect(d, round, t, cw, ch, r4, stop)) continue;
                    found = bx.any_centre_in(r4);
                }
            } else {
                const int lane = threadIdx.x % kWave;
                const bool cand = lane < kTrials && crop_rect(d, round, lane, cw, ch, r4, stop);
                const bool pass = bx.lanes_pass(cand, r4);
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

// A kept box from the canvas to fractions of the output, as the reference moves it (fp64): clamp to the crop and shift,
// mirror, divide by the crop's own (clipped) size; one fp32 row [x1, y1, x2, y2, label].
__device__ __forceinline__ void store_moved_box(const tdrn_augment_params &p, int wc, int hc, double x1, double y1, double x2,
                                                double y2, double label, float *row)
{
    if (p.cropped) {
        x1 = fmax(x1, (double)p.crop_x0) - (double)p.crop_x0;
        y1 = fmax(y1, (double)p.crop_y0) - (double)p.crop_y0;
        x2 = fmin(x2, (double)p.crop_x1) - (double)p.crop_x0;
        y2 = fmin(y2, (double)p.crop_y1) - (double)p.crop_y0;
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
    row[0] = (float)x1;
    row[1] = (float)y1;
    row[2] = (float)x2;
    row[3] = (float)y2;
    row[4] = (float)label;
}

// CSR offsets of the kept rows from per-image counts (one wave, 64 images per step); kept(b) reads image b's count
template <class F>
__device__ __forceinline__ void scan_kept(int B, int32_t *out_off, F kept)
{
    const int lane = threadIdx.x % kWave;
    int base = 0;
    for (int b0 = 0; b0 < B; b0 += kWave) {
        const int b = b0 + lane;
        const int k = b < B ? kept(b) : 0;
        int incl = k;
        for (int o = 1; o < kWave; o <<= 1) {
            const int v = __shfl_up(incl, o, kWave);
            if (lane >= o) incl += v;
        }
        if (b < B) out_off[b] = base + incl - k;
        base += __shfl(incl, kWave - 1, kWave);
    }
    if (lane == 0) out_off[B] = base;
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

}  // namespace
}  // namespace tdrn
