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
// The device functions both kernels are made of (draw sources, decide, crop_rect, distort_tap, lin_coef, the box move) live
// in augment_common.h, shared with augment_pair.hip.
//
// Rounding: the pixels and boxes are compared bit for bit with the reference's unfused numpy / cv2 arithmetic, so the
// Makefile builds this file with -ffp-contract=off (no a*b+c -> FMA); fp32 division and the fp64 box arithmetic are
// correctly rounded.

#include "augment_common.h"

namespace tdrn {
namespace {

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
    if (wave == 0) scan_kept(A.B, A.out_off, [&](int b) { return A.params[b].kept; });
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
                store_moved_box(p, wc, hc, x1, y1, x2, y2, ib.rows[(size_t)i * 5 + 4], A.out_truths + (size_t)j * 5);
            }
            o += __popcll(ball);
        }
    }
}

// ------------------------------------------------------------------------------------------------ pixels
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
