// box_coder.h -- the box arithmetic of layers/box_utils.py shared by Detect (detect.hip) and the training losses
// (loss.hip): decode (:176-195), center_size (:16-25) and encode (:151-172).  Every fp32 operation is issued un-fused and in the
// reference's order (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn), so both users apply one rule.
#pragma once
#include <hip/hip_runtime.h>

namespace tdrn {

// loc (4) against a center-size prior pr (4): point-form box b (4) = [x1, y1, x2, y2]
__device__ __forceinline__ void decode_one(const float *l, const float *pr, float v0, float v1, float *b)
{
    const float cx = __fadd_rn(pr[0], __fmul_rn(__fmul_rn(l[0], v0), pr[2]));
    const float cy = __fadd_rn(pr[1], __fmul_rn(__fmul_rn(l[1], v0), pr[3]));
    const float w = __fmul_rn(pr[2], expf(__fmul_rn(l[2], v1)));
    const float h = __fmul_rn(pr[3], expf(__fmul_rn(l[3], v1)));
    const float x1 = __fsub_rn(cx, __fdiv_rn(w, 2.f));
    const float y1 = __fsub_rn(cy, __fdiv_rn(h, 2.f));
    b[0] = x1;
    b[1] = y1;
    b[2] = __fadd_rn(w, x1);
    b[3] = __fadd_rn(h, y1);
}
// point-form b (4) -> center-size o (4)
__device__ __forceinline__ void center_size_one(const float *b, float *o)
{
    o[0] = __fdiv_rn(__fadd_rn(b[2], b[0]), 2.f);
    o[1] = __fdiv_rn(__fadd_rn(b[3], b[1]), 2.f);
    o[2] = __fsub_rn(b[2], b[0]);
    o[3] = __fsub_rn(b[3], b[1]);
}

// encode (box_utils.py:151-172) of a point-form box m (4) against a center-size prior pr (4), op for op:
// ((m_lo + m_hi) / 2 - c) / (v0 * wh), log((m_hi - m_lo) / wh) / v1
__device__ __forceinline__ void encode_one(const float *m, const float *pr, float v0, float v1, float *g)
{
    g[0] = __fdiv_rn(__fsub_rn(__fdiv_rn(__fadd_rn(m[0], m[2]), 2.f), pr[0]), __fmul_rn(v0, pr[2]));
    g[1] = __fdiv_rn(__fsub_rn(__fdiv_rn(__fadd_rn(m[1], m[3]), 2.f), pr[1]), __fmul_rn(v0, pr[3]));
    g[2] = __fdiv_rn(logf(__fdiv_rn(__fsub_rn(m[2], m[0]), pr[2])), v1);
    g[3] = __fdiv_rn(logf(__fdiv_rn(__fsub_rn(m[3], m[1]), pr[3])), v1);
}

}  // namespace tdrn
