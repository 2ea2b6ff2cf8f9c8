// conv_route.hip -- which kernel runs a dense conv layer.  Host code only; the one file that names more than one conv kernel: it puts
// the kernel files' X_takes predicates (kernels.h) in order, and launch_conv switches on the answer.
#include "kernels.h"

namespace tdrn {

// (by layer geometry only, never by batch size: the 10x10 / 5x5 pyramid levels stay on the implicit GEMM with its split-K)
constexpr int kPatchMinPixels = 400;

ConvKernel conv_route(const ConvArgs &a, bool pooled)
{
    const bool split = a.splitk > 1 && a.partial;           // (only conv_igemm.hip reduces K slices)
    if (!split && pooled) {
        // NO kPatchMinPixels threshold on this path, and there never was: a pool is fused only where the planner found 2-D tiles
        // (Plan::can_fuse_pool), which start at 16 x 16 -- kept exactly so.
        if (ws_takes(a, true)) return CONV_WS;
        if (patch_takes(a, true)) return CONV_PATCH;
    } else if (!split && a.H * a.W >= kPatchMinPixels) {
        if (pp_takes(a, false)) return CONV_PP;
        if (patch_takes(a, false)) return CONV_PATCH;
    }
    if (a.fuse_x || a.fuse_x8) return CONV_NONE;            // only the patch family computes the first conv itself
    if (split || pooled) return CONV_IGEMM;                 // (pooled: and a separate MaxPool2d launch)
    if (head3x3_takes(a, false)) return CONV_HEAD3X3;
    return pw1x1_takes(a, false) ? CONV_PW1X1 : CONV_IGEMM;
}

const char *conv_kernel_name(ConvKernel k)
{
    static const char *const names[] = {"igemm", "patch", "pp", "ws", "head3x3", "pw1x1", "none"};
    return names[k];
}

int launch_conv(const ConvArgs &a, hipStream_t s, void *out_pool)
{
    ConvArgs f = a;
    if (out_pool) f.out = nullptr;       // a kernel that pools in its epilogue: only the pooled map leaves the chip
    switch (conv_route(a, out_pool != nullptr)) {
        case CONV_WS: return launch_conv3x3_ws(f, out_pool, s);
        case CONV_PATCH: return launch_conv3x3_patch(f, out_pool, s);
        case CONV_PP: return launch_conv3x3_pp(a, s);
        case CONV_HEAD3X3: return launch_head3x3(a, s);
        case CONV_PW1X1: return launch_pw1x1(a, s);
        case CONV_IGEMM:
            TDRN_TRY(launch_conv_igemm(a, s));
            return out_pool ? launch_maxpool2(a.out, out_pool, a.B, a.Ho, a.Wo, (int)a.o_cs, 0, a.dtype, s) : TDRN_OK;
        default: return TDRN_E_UNSUPPORTED;
    }
}

// only layers that stay on conv_igemm.hip are split (head3x3.hip takes its launches whole; a split wide 1x1 layer stays there too)
int conv_splitk_choice(const ConvArgs &a)
{
    const ConvKernel k = conv_route(a, false);
    return k == CONV_PATCH || k == CONV_PP || k == CONV_HEAD3X3 ? 1 : igemm_splitk_choice(a);
}

}  // namespace tdrn
