// augment.hip -- SSDAugmentation (utils/augmentations.py:618-635 of the reference) and pairSSDAugmentation (:637-689, with the
// translated second frame of VOCDetection.pull_translational_item, data/voc0712.py:400-458) on the device, for a batch of raw
// uint8 frames.  Semantics, quirks and deviations: tdrn_hip.h sections (ii-c) and (ii-d).
//
// One chain over F frames under shared decisions: the single chain is F = 1, a TRN training pair is F = 2.  A box set
// (BoxSet<OneFrame>, BoxSet<TwoFrames>) holds an image's truths in every frame and where its kept rows go; a crop trial passes
// when some box keeps its centre inside the rect in every frame.  What only a pair has -- the translation attempts before the
// chain's draws (translate) and the 32 bytes behind the embedded record -- sits in TwoFrames and its decide_record.
//
//   augment_sample_kernel<FR> (1 block, one wave per image in turn): every decision of one image from its draw source, the
//                         record, then -- after a block barrier and a scan of the kept counts -- the moved boxes of every
//                         frame as packed fp32 rows behind one CSR offset array.  Draw sources: Philox4x32-10 (the crop
//                         trials of a mode round on the lanes, lowest passing lane wins) or a tape of recorded draws
//                         (sequential, every lane alike).
//   augment_apply_kernel<F> (256 output pixels of one image per block): the geometry of an output pixel once (resize taps,
//                         mirror, crop, canvas); a tap is the mean in every frame or a source pixel of each -- frame 0's own,
//                         a later frame's own or frame 0's at (x - trans_x, y - trans_y), black outside -- distorted in
//                         registers with the shared values (brightness, contrast, HSV round trip, saturation, hue, contrast,
//                         channel permutation); blend, subtract the mean, store three planes per frame coalesced along x.
//                         The translated frame, the distorted images, the canvases and the crops never exist.
//
// Rounding: the pixels and boxes are compared bit for bit with the reference's unfused numpy / cv2 arithmetic, so the
// Makefile builds this file with -ffp-contract=off (no a*b+c -> FMA); fp32 division and the fp64 box arithmetic are
// correctly rounded.

#include <climits>
#include <cmath>
#include <type_traits>

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

// ------------------------------------------------------------------------------------------------ kept rows
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

// ------------------------------------------------------------------------------------------------ boxes
__device__ __forceinline__ bool inside(const int rect[4], double cx, double cy)
{
    return (double)rect[0] < cx && (double)rect[1] < cy && (double)rect[2] > cx && (double)rect[3] > cy;
}

// The frames of an image's truths: frac(f, i, k) is column k of box i in frame f as a fraction, label(f, i) its label,
// out[f] the frame's packed fp32 rows; Record is what the sampler writes per image, Args the frames' kernel arguments.
struct OneFrame {
    static constexpr int kFrames = 1;
    using Record = tdrn_augment_params;
    struct Args {
        const double *truths[1];
        float *out[1];
        __host__ bool valid() const { return true; }
    };
    const double *rows;   // (n,5) fp64 fractions
    __device__ OneFrame(const Args &a, size_t t0) : rows(a.truths[0] + t0 * 5) {}
    __device__ double frac(int, int i, int k) const { return rows[(size_t)i * 5 + k]; }
    __device__ double label(int, int i) const { return rows[(size_t)i * 5 + 4]; }
    __device__ void restore(const Record &) {}
};

// Frame 1's fractions are the caller's rows, or frame 0's moved by (sx, sy) and clipped to [0, 1] when a translation attempt
// was accepted (sx = sy = 0 and no clip: the fallback's copy).
struct TwoFrames {
    static constexpr int kFrames = 2;
    using Record = tdrn_augment_pair_params;
    struct Args {
        const double *truths[2];   // [1] NULL: translate frame 0's
        float *out[2];
        double r;                  // max_trans_ratio
        __host__ bool valid() const { return r >= 0.0 && r < 1.0; }
    };
    const double *rows, *rows_t;
    double sx, sy;
    bool clip;
    __device__ TwoFrames(const Args &a, size_t t0)
        : rows(a.truths[0] + t0 * 5), rows_t(a.truths[1] ? a.truths[1] + t0 * 5 : nullptr), sx(0.0), sy(0.0), clip(false) {}
    __device__ double frac(int f, int i, int k) const
    {
        if (f == 0) return rows[(size_t)i * 5 + k];
        if (rows_t) return rows_t[(size_t)i * 5 + k];
        double v = rows[(size_t)i * 5 + k] + ((k & 1) ? sy : sx);
        if (clip) v = fmin(fmax(v, 0.0), 1.0);
        return v;
    }
    __device__ double label(int f, int i) const { return (f && rows_t ? rows_t : rows)[(size_t)i * 5 + 4]; }
    // the translation a record holds, for phase 3 (phase 1 has it from decide_record)
    __device__ void restore(const Record &q)
    {
        sx = q.shift_x;
        sy = q.shift_y;
        clip = q.attempts > 0 && !(q.base.status & TDRN_AUGMENT_TRANS_FALLBACK);
    }
};

__device__ __forceinline__ tdrn_augment_params &base(tdrn_augment_params &p) { return p; }
__device__ __forceinline__ tdrn_augment_params &base(tdrn_augment_pair_params &q) { return q.base; }
__device__ __forceinline__ void translation(const tdrn_augment_params &, int &tx, int &ty) { tx = ty = 0; }
__device__ __forceinline__ void translation(const tdrn_augment_pair_params &q, int &tx, int &ty)
{
    tx = q.trans_x;
    ty = q.trans_y;
}

// The boxes of one image in the frames FR, on the expand canvas.
template <class FR>
struct BoxSet {
    static constexpr int F = FR::kFrames;
    FR fr;
    float *out[F];
    int n;
    double W, H;          // the frames' size
    int dx, dy;           // expand shift
    __device__ BoxSet(const typename FR::Args &a, size_t t0, int n_, int W_, int H_)
        : fr(a, t0), n(n_), W((double)W_), H((double)H_), dx(0), dy(0)
    {
        for (int f = 0; f < F; ++f) out[f] = a.out[f];
    }
    __device__ void shift(int x, int y) { dx = x; dy = y; }
    // absolute box i of frame f after ToAbsoluteCoords and Expand, in the reference's op order
    __device__ void box(int f, int i, double &x1, double &y1, double &x2, double &y2) const
    {
        x1 = fr.frac(f, i, 0) * W + (double)dx;
        y1 = fr.frac(f, i, 1) * H + (double)dy;
        x2 = fr.frac(f, i, 2) * W + (double)dx;
        y2 = fr.frac(f, i, 3) * H + (double)dy;
    }
    __device__ void centre(int f, int i, double &cx, double &cy) const
    {
        double x1, y1, x2, y2;
        box(f, i, x1, y1, x2, y2);
        cx = (x1 + x2) / 2.0;
        cy = (y1 + y2) / 2.0;
    }
    // box i keeps its centre inside the rect in every frame (augmentations.py:374-388 for a pair)
    __device__ bool centre_in(int i, const int rect[4]) const
    {
        bool in = true;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            double cx, cy;
            centre(f, i, cx, cy);
            in = in && inside(rect, cx, cy);
        }
        return in;
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
            double cx[F], cy[F];
#pragma unroll
            for (int f = 0; f < F; ++f) {
                cx[f] = cy[f] = 0.0;
                if (c0 + lane < n) centre(f, c0 + lane, cx[f], cy[f]);
            }
            const int m = min(kWave, n - c0);
            for (int j = 0; j < m; ++j) {
                bool in = cand;
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const double x = __shfl(cx[f], j, kWave), y = __shfl(cy[f], j, kWave);   // every lane, whatever cand says
                    in = in && inside(r4, x, y);
                }
                pass = pass || in;
            }
        }
        return pass;
    }
    // kept box i of every frame to packed row j, moved as the reference moves it
    __device__ void store_kept(const tdrn_augment_params &p, int wc, int hc, int i, int j) const
    {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            double x1, y1, x2, y2;
            box(f, i, x1, y1, x2, y2);
            store_moved_box(p, wc, hc, x1, y1, x2, y2, fr.label(f, i), out[f] + (size_t)j * 5);
        }
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
// BX holds the image's boxes in every frame (a BoxSet<FR>): n, shift(), any_centre_in(), lanes_pass().
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

// The translation of voc0712.py:411-434 for one image, every lane alike: up to three attempts, each drawing u_x then u_y; an
// attempt is accepted when every moved box keeps its centre strictly inside (0, 1) on both axes.  true: accepted.
template <class D>
__device__ bool translate(D &d, const BoxSet<TwoFrames> &bx, double r, int W, int H, tdrn_augment_pair_params &q)
{
    const int lane = threadIdx.x % kWave;
    for (int a = 1; a <= 3; ++a) {
        const double ux = d.uniform(0.0, 1.0, kSlotTrans + 2u * (uint32_t)(a - 1));
        const double uy = d.uniform(0.0, 1.0, kSlotTrans + 2u * (uint32_t)(a - 1) + 1u);
        const double xt = (-r / (double)a) + ((ux * 2.0) * r) / (double)a;
        const double yt = (-r / (double)a) + ((uy * 2.0) * r) / (double)a;
        q.attempts = a;
        bool out = false;
        for (int i0 = 0; i0 < bx.n; i0 += kWave) {
            const int i = i0 + lane;
            bool bad = false;
            if (i < bx.n) {
                const double *row = bx.fr.rows + (size_t)i * 5;
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

// An image's record: the chain's decisions, for a pair behind the translation that makes frame 1's boxes.
template <class D>
__device__ tdrn_augment_params decide_record(D &d, BoxSet<OneFrame> &bx, const OneFrame::Args &, int W, int H)
{
    return decide(d, bx, W, H);
}

template <class D>
__device__ tdrn_augment_pair_params decide_record(D &d, BoxSet<TwoFrames> &bx, const TwoFrames::Args &a, int W, int H)
{
    tdrn_augment_pair_params q;
    q.shift_x = q.shift_y = 0.0;
    q.trans_x = q.trans_y = q.attempts = q.reserved = 0;
    bool fallback = false;
    if (!bx.fr.rows_t && bx.n > 0) {
        if (translate(d, bx, a.r, W, H, q)) {
            bx.fr.sx = q.shift_x;
            bx.fr.sy = q.shift_y;
            bx.fr.clip = true;
        } else {
            fallback = true;
        }
    }
    q.base = decide(d, bx, W, H);
    if (fallback) q.base.status |= TDRN_AUGMENT_TRANS_FALLBACK;
    return q;
}

template <class FR>
struct SampleArgs {
    const int32_t *hw;
    typename FR::Args frames;
    const int32_t *truth_off;
    int T_total, max_truths, B;
    uint2 key;
    const int64_t *sample_ids;
    const double *tape;
    const int32_t *tape_off;
    typename FR::Record *params;
    int32_t *out_off;
};

template <class FR>
__device__ BoxSet<FR> box_set(const SampleArgs<FR> &A, int b)
{
    int t0, n;
    span(A.truth_off, b, A.T_total, A.max_truths, t0, n);
    return BoxSet<FR>(A.frames, (size_t)t0, n, A.hw[2 * b + 1], A.hw[2 * b]);
}

template <class FR>
__global__ void __launch_bounds__(kSampleWaves * kWave) augment_sample_kernel(SampleArgs<FR> A)
{
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
    // phase 1: the decisions and the kept count of every image
    for (int b = wave; b < A.B; b += nw) {
        BoxSet<FR> bx = box_set(A, b);
        const int W = A.hw[2 * b + 1], H = A.hw[2 * b];
        typename FR::Record rec;
        if (A.sample_ids) {
            PhiloxDraws d;
            d.key = A.key;
            d.sid = (uint64_t)A.sample_ids[b];
            d.prefetch();
            rec = decide_record(d, bx, A.frames, W, H);
        } else {
            TapeDraws d;
            int t0, n;
            span(A.tape_off, b, INT_MAX, INT_MAX, t0, n);
            d.tape = A.tape + t0;
            d.n = n;
            d.pos = 0;
            d.exhausted = false;
            rec = decide_record(d, bx, A.frames, W, H);
        }
        tdrn_augment_params &p = base(rec);
        int kept = bx.n;
        if (p.cropped) {
            bx.shift(p.img_x, p.img_y);
            const int rect[4] = {p.crop_x0, p.crop_y0, p.crop_x1, p.crop_y1};
            kept = 0;
            for (int i0 = 0; i0 < bx.n; i0 += kWave) {
                const bool in = i0 + lane < bx.n && bx.centre_in(i0 + lane, rect);
                kept += __popcll(__ballot(in));
            }
        }
        p.kept = kept;
        if (lane == 0) A.params[b] = rec;
    }
    __syncthreads();
    // phase 2: CSR offsets of the kept rows (wave 0, 64 images per step), one array for every frame
    if (wave == 0) scan_kept(A.B, A.out_off, [&](int b) { return base(A.params[b]).kept; });
    __syncthreads();
    // phase 3: the kept boxes of every frame, moved as the reference moves them (fp64), cast to fp32
    for (int b = wave; b < A.B; b += nw) {
        typename FR::Record rec = A.params[b];
        const tdrn_augment_params &p = base(rec);
        BoxSet<FR> bx = box_set(A, b);
        bx.shift(p.img_x, p.img_y);
        bx.fr.restore(rec);
        const int rect[4] = {p.crop_x0, p.crop_y0, p.crop_x1, p.crop_y1};
        const int wc = min(p.crop_x1, p.canvas_w) - p.crop_x0, hc = min(p.crop_y1, p.canvas_h) - p.crop_y0;
        int o = A.out_off[b];
        for (int i0 = 0; i0 < bx.n; i0 += kWave) {
            const int i = i0 + lane;
            const bool in = i < bx.n && (!p.cropped || bx.centre_in(i, rect));
            const unsigned long long ball = __ballot(in);
            const int j = o + __popcll(ball & ((1ull << lane) - 1ull));
            if (in && j < A.T_total) bx.store_kept(p, wc, hc, i, j);   // j < T_total unless the offsets broke their promise
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

template <int F>
struct ApplyArgs {
    using Record = std::conditional_t<F == 1, tdrn_augment_params, tdrn_augment_pair_params>;
    const tdrn_augment_image *images[F];   // [f > 0] NULL: frame f is frame 0, translated
    const Record *params;
    float mean[3];
    int S, to_rgb;
    float *out[F];
};

// (a frame's fields by value: through a reference to the struct the compiler no longer sees that frame 0's data is a global
// pointer, and reads it with flat loads)
__device__ __forceinline__ uint32_t load_bgr(const uint8_t *data, int w, int x, int y)
{
    const uint8_t *q = data + ((size_t)y * w + x) * 3;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
}

template <int F>
__global__ void __launch_bounds__(kApplyBlock) augment_apply_kernel(ApplyArgs<F> A)
{
    const int b = blockIdx.y;
    const int pix = blockIdx.x * kApplyBlock + threadIdx.x;
    const int S = A.S;
    if (pix >= S * S) return;
    const int oy = pix / S, ox = pix - oy * S;
    typename ApplyArgs<F>::Record rec = A.params[b];
    const tdrn_augment_params p = base(rec);
    const tdrn_augment_image im = A.images[0][b];
    tdrn_augment_image it[F];                                             // where a later frame's pixels are read, and how far
    int tx[F], ty[F];                                                     // from frame 0's place
#pragma unroll
    for (int f = 1; f < F; ++f) {
        it[f] = im;
        translation(rec, tx[f], ty[f]);
        if (A.images[f]) {
            it[f] = A.images[f][b];
            tx[f] = ty[f] = 0;
        }
    }
    const float mean[3] = {A.mean[0], A.mean[1], A.mean[2]};
    const int wc = max(min(p.crop_x1, p.canvas_w) - p.crop_x0, 1), hc = max(min(p.crop_y1, p.canvas_h) - p.crop_y0, 1);
    int xs[2], ys[2];
    float aw[2], bw[2];
    lin_coef(ox, S, wc, xs[0], xs[1], aw[0], aw[1]);
    lin_coef(oy, S, hc, ys[0], ys[1], bw[0], bw[1]);
    float hrow[F][2][3];                                                  // [frame][tap row][channel]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int iy = p.crop_y0 + ys[j] - p.img_y;                      // frame row of this tap row
        float t[F][2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int col = p.mirror ? wc - 1 - xs[i] : xs[i];
            const int ix = p.crop_x0 + col - p.img_x;
            if ((unsigned)ix < (unsigned)im.w && (unsigned)iy < (unsigned)im.h) {
                distort_tap(load_bgr(im.data, im.w, ix, iy), p, t[0][i]);
                // a later frame at this place: its own pixel, or frame 0's at (x - tx, y - ty); black where that is outside
#pragma unroll
                for (int f = 1; f < F; ++f) {
                    const int sx = ix - tx[f], sy = iy - ty[f];
                    const bool in = (unsigned)sx < (unsigned)it[f].w && (unsigned)sy < (unsigned)it[f].h;
                    distort_tap(in ? load_bgr(it[f].data, it[f].w, sx, sy) : 0u, p, t[f][i]);
                }
            } else {
#pragma unroll
                for (int f = 0; f < F; ++f)
#pragma unroll
                    for (int c = 0; c < 3; ++c) t[f][i][c] = mean[c];
            }
        }
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
            for (int c = 0; c < 3; ++c) hrow[f][j][c] = t[f][0][c] * aw[0] + t[f][1][c] * aw[1];
    }
    const size_t plane = (size_t)S * S;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t at = (size_t)b * 3 * plane + pix + (size_t)(A.to_rgb ? 2 - c : c) * plane;
#pragma unroll
        for (int f = 0; f < F; ++f) A.out[f][at] = (hrow[f][0][c] * bw[0] + hrow[f][1][c] * bw[1]) - mean[c];
    }
}

// ------------------------------------------------------------------------------------------------ launchers
template <class FR>
int launch_sample(const int32_t *hw, const typename FR::Args &frames, const int32_t *truth_off, int T_total, int max_truths,
                  int B, uint64_t seed, const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                  typename FR::Record *params, int32_t *out_off, hipStream_t s)
{
    if (!hw || !truth_off || !params || !out_off || B <= 0 || T_total < 0 || max_truths < 0) return TDRN_E_ARG;
    if (T_total > 0 && !frames.truths[0]) return TDRN_E_ARG;
    for (float *rows : frames.out)
        if (T_total > 0 && !rows) return TDRN_E_ARG;
    if ((sample_ids != nullptr) == (tape != nullptr || tape_off != nullptr)) return TDRN_E_ARG;   // exactly one source
    if (!sample_ids && (!tape || !tape_off)) return TDRN_E_ARG;
    if (!frames.valid()) return TDRN_E_ARG;
    if (max_truths > TDRN_AUGMENT_MAX_TRUTHS) return TDRN_E_UNSUPPORTED;
    SampleArgs<FR> A;
    A.hw = hw;
    A.frames = frames;
    A.truth_off = truth_off;
    A.T_total = T_total;
    A.max_truths = max_truths;
    A.B = B;
    A.key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    A.sample_ids = sample_ids;
    A.tape = tape;
    A.tape_off = tape_off;
    A.params = params;
    A.out_off = out_off;
    const int waves = B < kSampleWaves ? B : kSampleWaves;
    hipLaunchKernelGGL(augment_sample_kernel<FR>, dim3(1), dim3(waves * kWave), 0, s, A);
    return hip_status(hipGetLastError());
}

template <int F>
int launch_apply(const tdrn_augment_image *const (&images)[F], const typename ApplyArgs<F>::Record *params, int B,
                 const float *mean, int S, int to_rgb, float *const (&out)[F], hipStream_t s)
{
    if (!images[0] || !params || !mean || B <= 0 || S <= 0) return TDRN_E_ARG;
    for (float *o : out)
        if (!o) return TDRN_E_ARG;
    if (S > TDRN_AUGMENT_MAX_SIZE || B > 65535) return TDRN_E_UNSUPPORTED;
    ApplyArgs<F> A;
    for (int f = 0; f < F; ++f) {
        A.images[f] = images[f];
        A.out[f] = out[f];
    }
    A.params = params;
    A.mean[0] = mean[0];
    A.mean[1] = mean[1];
    A.mean[2] = mean[2];
    A.S = S;
    A.to_rgb = to_rgb ? 1 : 0;
    hipLaunchKernelGGL(augment_apply_kernel<F>, dim3(cdiv(S * S, kApplyBlock), B), dim3(kApplyBlock), 0, s, A);
    return hip_status(hipGetLastError());
}

}  // namespace

int launch_augment_sample(const int32_t *hw, const double *truths, const int32_t *truth_off, int T_total, int max_truths, int B,
                          uint64_t seed, const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                          tdrn_augment_params *params, float *out_truths, int32_t *out_off, hipStream_t s)
{
    return launch_sample<OneFrame>(hw, {{truths}, {out_truths}}, truth_off, T_total, max_truths, B, seed, sample_ids, tape,
                                   tape_off, params, out_off, s);
}

int launch_augment_apply(const tdrn_augment_image *images, const tdrn_augment_params *params, int B, const float *mean, int S,
                         int to_rgb, float *out, hipStream_t s)
{
    return launch_apply<1>({images}, params, B, mean, S, to_rgb, {out}, s);
}

int launch_augment_pair_sample(const int32_t *hw, const double *truths, const double *truths_t, const int32_t *truth_off,
                               int T_total, int max_truths, int B, double max_trans_ratio, uint64_t seed,
                               const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                               tdrn_augment_pair_params *params, float *out_truths, float *out_truths_t, int32_t *out_off,
                               hipStream_t s)
{
    return launch_sample<TwoFrames>(hw, {{truths, truths_t}, {out_truths, out_truths_t}, max_trans_ratio}, truth_off, T_total,
                                    max_truths, B, seed, sample_ids, tape, tape_off, params, out_off, s);
}

int launch_augment_pair_apply(const tdrn_augment_image *images, const tdrn_augment_image *images_t,
                              const tdrn_augment_pair_params *params, int B, const float *mean, int S, int to_rgb, float *out,
                              float *out_t, hipStream_t s)
{
    return launch_apply<2>({images, images_t}, params, B, mean, S, to_rgb, {out, out_t}, s);
}

}  // namespace tdrn
