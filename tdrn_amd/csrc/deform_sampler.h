// deform_sampler.h -- the bilinear sampling rule of deformable conv v1, shared by the forward kernels (deform.hip
// deform_gemm_kernel and deform_sample_kernel), the backward kernels (deform_bwd.hip) and the transform-domain op (deform_ts.hip).
//
// utils/deformconv/deform_conv_cuda_kernel.cu:15-51 and :189-203, including the asymmetric border rule: a sample
// coordinate < 0 or >= H (W) is rejected (returns false); a coordinate in [H-1, H) clamps to row H-1 with fraction 0.
// The coordinates are formed in fp32 exactly as the reference forms them (h_im for the rejection test, map_h relative to
// h_in for the floor), so every floor / border decision is the forward's.
#pragma once
#include <hip/hip_runtime.h>

namespace tdrn {

// h_in / w_in: top-left input coordinate of the output pixel (ho * stride - pad); ti_dil / tj_dil: the tap's dilated
// position.  On success: absolute corner rows r0 <= r1 and columns q0 <= q1 (clamped into the map only for memory
// safety -- a no-op whenever the reference itself stays in bounds) and the fractions lh, lw (0 inside the clamp band).
// Bilinear weights: (1-lh)(1-lw), (1-lh)lw, lh(1-lw), lh lw for corners (r0,q0), (r0,q1), (r1,q0), (r1,q1).
__device__ __forceinline__ bool deform_sample(int H, int W, int h_in, int w_in, int ti_dil, int tj_dil, float offset_h,
                                              float offset_w, int &r0, int &r1, int &q0, int &q1, float &lh, float &lw)
{
    const float h_im = (float)(h_in + ti_dil) + offset_h;
    const float w_im = (float)(w_in + tj_dil) + offset_w;
    if (!(h_im >= 0.f && w_im >= 0.f && h_im < (float)H && w_im < (float)W)) return false;
    float h = (float)ti_dil + offset_h;     // map_h, relative to h_in
    float w = (float)tj_dil + offset_w;
    const int height = H - h_in, width = W - w_in;
    int h_low = (int)floorf(h), w_low = (int)floorf(w), h_high, w_high;
    if (h_low >= height - 1) { h_high = h_low = height - 1; h = (float)h_low; } else { h_high = h_low + 1; }
    if (w_low >= width - 1) { w_high = w_low = width - 1; w = (float)w_low; } else { w_high = w_low + 1; }
    lh = h - (float)h_low;
    lw = w - (float)w_low;
    r0 = min(max(h_in + h_low, 0), H - 1);
    r1 = min(max(h_in + h_high, 0), H - 1);
    q0 = min(max(w_in + w_low, 0), W - 1);
    q1 = min(max(w_in + w_high, 0), W - 1);
    return true;
}

}  // namespace tdrn
