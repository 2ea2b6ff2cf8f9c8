// api.hip -- C ABI entry points of tdrn_hip.h sections (i), (i-b), (i-c), (i-d), (i-e), (i-f), (i-g), (i-h), (i-i), (i-j), (i-k) and (ii) (section (iii) is in net.hip).
// Sections (i-c), (i-f), (i-g) and (i-i), the trainable dense conv families, share one plan, one workspace layout and one runner
// (ConvTrainPlan); the depthwise conv (i-h) works on NCHW planes and has its own small plan (DwConvPlan).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"

using namespace tdrn;

namespace {

struct DeformPlan {
    int Ho, Wo, taps, ck, cpg_pad, Cin_pad, Npad_total, chunks;
    size_t o_zero, o_in, o_w, o_off, o_out, total;
};

int deform_plan(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilH,
                int dilW, int G, int dtype, DeformPlan &p)
{
    // shape_check, utils/deformconv/deform_conv_cuda.c:7-96
    if (kW <= 0 || kH <= 0) return TDRN_E_SHAPE;
    if (dW <= 0 || dH <= 0) return TDRN_E_SHAPE;
    if (dilW <= 0 || dilH <= 0) return TDRN_E_SHAPE;
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return TDRN_E_SHAPE;
    if (G <= 0 || Cin % G != 0) return TDRN_E_SHAPE;
    if (dtype < 0 || dtype > 2) return TDRN_E_ARG;
    p.Ho = (H + 2 * padH - (dilH * (kH - 1) + 1)) / dH + 1;
    p.Wo = (W + 2 * padW - (dilW * (kW - 1) + 1)) / dW + 1;
    if (p.Ho < 1 || p.Wo < 1) return TDRN_E_SHAPE;
    if (H < kH || W < kW) return TDRN_E_SHAPE;
    if (padH < 0 || padW < 0) return TDRN_E_SHAPE;
    const int es = dtype_bytes(dtype);
    p.taps = kH * kW;
    p.ck = 128 / es;
    p.cpg_pad = (int)align_up((size_t)(Cin / G), p.ck);
    p.Cin_pad = p.cpg_pad * G;
    p.chunks = cdiv(Cout, 128);
    p.Npad_total = (p.chunks - 1) * 128 + deform_n_pad(Cout - (p.chunks - 1) * 128);
    size_t o = 0;
    p.o_zero = o; o += kZeroPageBytes;
    p.o_in = o;   o += align_up((size_t)N * H * W * p.Cin_pad * es, 256);
    p.o_w = o;    o += align_up((size_t)p.Npad_total * p.taps * p.Cin_pad * es, 256);
    p.o_off = o;  o += align_up((size_t)N * p.Ho * p.Wo * G * 2 * p.taps * 4, 256);
    p.o_out = o;  o += align_up((size_t)N * p.Ho * p.Wo * Cout * 4, 256);
    p.total = o;
    return TDRN_OK;
}

// backward workspace: the input as group-padded NHWC fp32 (both entries); backward_input: the NHWC grad_input accumulator and the
// repacked weight; backward_parameters: the split-K slabs.  One size serves both entries.
struct DeformBwdPlan {
    DeformBwdGeom g;
    size_t o_in, o_gin, o_w, o_slab, total;
};

int deform_bwd_plan(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilH, int dilW,
                    int G, DeformBwdPlan &b)
{
    DeformPlan p;
    TDRN_TRY(deform_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilH, dilW, G, TDRN_F32, p));
    b.g = DeformBwdGeom{N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilH, dilW, G, p.Ho, p.Wo};
    const size_t cpad = (size_t)deform_bwd_cpg64(b.g) * G;
    int splits, per_split;
    deform_bwd_weight_splits(b.g, splits, per_split);
    const size_t nhwc = align_up((size_t)N * H * W * cpad * 4, 256);
    size_t o = 0;
    b.o_in = o;   o += nhwc;
    const size_t rest = o;
    b.o_gin = o;  o += nhwc;
    b.o_w = o;    o += align_up((size_t)Cout * p.taps * cpad * 4, 256);
    b.o_slab = rest;
    const size_t slab_end = rest + align_up((size_t)splits * p.taps * Cout * cpad * 4, 256);
    b.total = o > slab_end ? o : slab_end;
    return TDRN_OK;
}

// The four trainable conv families: dense conv2d at stride 1 (section i-c), ConvTranspose2d(k = 2, s = 2) (section i-f), the 3x3
// conv at stride 2 (section i-g) and the 5x5 conv (section i-i).  In each the forward and the input gradient are one launch_conv with
// an fp32 NHWC result, and the weight gradient is one conv_bwd.hip GEMM.  The three dense families are one plan (conv_dense_plan) and
// one set of run bodies (conv_dense_*): a family is the predicate that says which geometries it covers.  ConvTranspose2d has its own
// description (convt2d_plan) and bodies; layout, bias staging and the run are shared by all four.
// Workspace: zero page | x NHWC | the grad_output image NHWC (what the input gradient convolves) | the rest, which is either {packed
// weight, padded bias, NHWC fp32 result, split-K partials of launch_conv} (forward, backward_input; each the larger of the two) or the
// split-K slabs of the weight gradient (backward_parameters).
struct ConvTrainPlan {
    ConvArgs fwd, dgrad;    // launch_conv's arguments without their pointers; fwd.Cin = CiPad, dgrad.Cin = the image's padded channels
    ConvBwdGeom wg;         // the weight gradient's geometry
    size_t o_zero, o_x, o_go, o_w, o_bias, o_out, o_partial, o_slab, total;
};

// an fp32 NHWC result without gaps: [B][Ho][Wo][Cout]
void conv_train_dense_out(ConvArgs &a)
{
    a.o_cs = a.Cout; a.o_rs = (long long)a.Wo * a.Cout; a.o_bs = (long long)a.Ho * a.Wo * a.Cout;
}

// what the families' launches share, set once their geometry and output strides are: fp32 result, no ReLU
void conv_train_args(ConvArgs &a, int dtype)
{
    a.relu = 0; a.out_f32 = 1;
    a.dtype = dtype;
    // every shape on conv_igemm.hip: head3x3.hip would take the narrow 16-bit layers with another fp32 K order, and a layer's
    // gradient should not change its rounding with its channel count; and every tap formed (tdrn_hip.h i-c: the padding's zeros meet
    // a non-finite weight wherever the tiles fall)
    a.kdisable = KOFF_HEAD3X3 | KOFF_TAP_SKIP;
    // the small-M layers (the 10 x 10 and 5 x 5 maps, the extras layer between them) fill the chip by K slices, as in the engine
    a.splitk = conv_splitk_choice(a);
}

// offsets and total from the two launches (each one's input image, packed weight [phases][Npad][taps][Cin] and result) and the slabs
void conv_train_layout(ConvTrainPlan &p, int dtype)
{
    conv_train_args(p.fwd, dtype);
    conv_train_args(p.dgrad, dtype);
    const ConvArgs &f = p.fwd, &d = p.dgrad;
    const size_t es = dtype_bytes(dtype);
    const size_t wf = (size_t)f.phases * f.Npad * f.kh * f.kw * f.Cin * es, wd = (size_t)d.phases * d.Npad * d.kh * d.kw * d.Cin * es;
    const size_t of = (size_t)f.B * f.o_bs * 4, od = (size_t)d.B * d.o_bs * 4;
    const size_t pf = conv_splitk_bytes(f, f.splitk), pd = conv_splitk_bytes(d, d.splitk);
    size_t o = 0;
    p.o_zero = o; o += kZeroPageBytes;
    p.o_x = o;    o += align_up((size_t)f.B * f.H * f.W * f.Cin * es, 256);
    p.o_go = o;   o += align_up((size_t)d.B * d.H * d.W * d.Cin * es, 256);
    p.o_slab = o;
    const size_t slab_end = o + conv_wgrad_slab_bytes(p.wg);
    p.o_w = o;    o += align_up(wf > wd ? wf : wd, 256);
    p.o_bias = o; o += align_up((size_t)(f.Npad > d.Npad ? f.Npad : d.Npad) * 4, 256);
    p.o_out = o;  o += align_up(of > od ? of : od, 256);
    p.o_partial = o; o += align_up(pf > pd ? pf : pd, 256);
    p.total = o > slab_end ? o : slab_end;
}

// what every entry does after its pointer check: the plan's verdict, the workspace, the zero page
int conv_train_begin(int plan_rc, const ConvTrainPlan &p, void *workspace, size_t workspace_bytes, hipStream_t s)
{
    TDRN_TRY(plan_rc);
    if (!workspace || workspace_bytes < p.total) return TDRN_E_WORKSPACE;
    return launch_fill_zero((char *)workspace + p.o_zero, kZeroPageBytes, s);
}

// launch_conv's bias: Npad zeros, under the caller's Cout values when there are any
int conv_train_bias(const ConvArgs &a, char *ws_bias, const float *bias, hipStream_t s)
{
    TDRN_TRY(launch_fill_zero(ws_bias, (size_t)a.Npad * 4, s));
    if (bias) TDRN_HIP_TRY(hipMemcpyAsync(ws_bias, bias, (size_t)a.Cout * 4, hipMemcpyDeviceToDevice, s));
    return TDRN_OK;
}

// launch_conv with its fp32 NHWC result in the workspace ([pixels][Cout], pixels = Ho Wo or, through four phases, 4 H W), then NCHW
// into `out`
int conv_train_run(const ConvTrainPlan &p, char *ws, bool dgrad, float *out, hipStream_t s)
{
    ConvArgs a = dgrad ? p.dgrad : p.fwd;
    a.in = ws + (dgrad ? p.o_go : p.o_x); a.w = ws + p.o_w; a.zero_page = ws + p.o_zero; a.bias = (const float *)(ws + p.o_bias);
    a.out = ws + p.o_out;
    if (a.splitk > 1) a.partial = ws + p.o_partial;
    TDRN_TRY(launch_conv(a, s));
    return launch_nhwc_to_nchw_f32((const float *)(ws + p.o_out), a.o_bs, a.Cout, out, a.B, a.Cout, a.phases * a.Ho * a.Wo, s);
}

// what every conv plan checks first, each in its own order: positive sizes and no negative padding ...
bool conv_sizes_ok(int N, int Cin, int Cout, int H, int W, int kH, int kW, int dH, int dW, int padH, int padW, int dilH, int dilW)
{
    if (kW <= 0 || kH <= 0 || dW <= 0 || dH <= 0 || dilW <= 0 || dilH <= 0) return false;
    return N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && padH >= 0 && padW >= 0;
}

// ... a tdrn_dtype ...
bool dtype_ok(int dtype) { return dtype >= 0 && dtype <= 2; }

// ... and a dilated window that fits into the padded image
bool conv_window_fits(int H, int W, int kH, int kW, int padH, int padW, int dilH, int dilW)
{
    return (long long)H + 2ll * padH >= (long long)dilH * (kH - 1) + 1 && (long long)W + 2ll * padW >= (long long)dilW * (kW - 1) + 1;
}

// The dense families (sections i-c, i-g, i-i): which of the public entry families is asking.  It decides what is covered, nothing else:
// the three are disjoint, and a geometry outside the asking family is unsupported even where another family covers it.
enum DenseFamily { DENSE_STRIDE1, DENSE_STRIDE2, DENSE_5X5 };

// One plan for the dense families.  The input gradient is a stride-1 conv with pad' = dil (k - 1) - pad and the same dilation, kernel
// rotated and transposed (launch_repack_oihw_dgrad), over D: grad_output itself at stride 1, its zero-inserted image at stride 2,
// (N, CoPad, Hd, Wd) -> (Cin, H, W).  Hd = H + 2 pad - dil (k - 1) is the stride-1 output size, so Hd = Ho at stride 1; at stride 2
// backward_parameters keeps the plain grad_output image in D's place (Hd >= Ho, Wd >= Wo: it fits).
int conv_dense_plan(DenseFamily family, int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilH,
                    int dilW, int dtype, ConvTrainPlan &p)
{
    if (!conv_sizes_ok(N, Cin, Cout, H, W, kH, kW, dH, dW, padH, padW, dilH, dilW)) return TDRN_E_SHAPE;
    if (!dtype_ok(dtype)) return TDRN_E_ARG;
    if (!conv_window_fits(H, W, kH, kW, padH, padW, dilH, dilW)) return TDRN_E_SHAPE;
    switch (family) {       // what the kernels cover
        case DENSE_STRIDE1:  // square k = 1 | 3, stride 1, one pad / dilation for both axes, pad <= dil (k - 1) (pad' >= 0)
            if (kH != kW || (kH != 1 && kH != 3) || dH != 1 || dW != 1 || padH != padW || dilH != dilW) return TDRN_E_UNSUPPORTED;
            if ((long long)padH > (long long)dilH * (kH - 1)) return TDRN_E_UNSUPPORTED;
            break;
        case DENSE_STRIDE2:  // k = 3 at stride 2, dilation 1, one pad <= 2 for both axes (pad' >= 0).  Stride 1 is DENSE_STRIDE1's
            if (kH != 3 || kW != 3 || dH != 2 || dW != 2 || dilH != 1 || dilW != 1 || padH != padW || padH > 2) return TDRN_E_UNSUPPORTED;
            break;
        case DENSE_5X5:      // kH = kW = 5, stride 1, dilation 1, pad 2, so Ho x Wo = H x W; 25 taps, as the engine runs this layer
            if (kH != 5 || kW != 5 || dH != 1 || dW != 1 || padH != 2 || padW != 2 || dilH != 1 || dilW != 1) return TDRN_E_UNSUPPORTED;
            break;
    }
    // so from here on one k, stride, pad and dilation serve both axes
    const int k = kH, stride = dH, pad = padH, dil = dilH;
    const long long reach = (long long)dil * (k - 1);
    const long long Hd = (long long)H + 2ll * pad - reach, Wd = (long long)W + 2ll * pad - reach;
    const long long Ho = (Hd - 1) / stride + 1, Wo = (Wd - 1) / stride + 1;
    const int CiPad = conv_bwd_cpad(Cin), CoPad = conv_bwd_cpad(Cout);
    // 32-bit offsets of the kernels (conv_igemm.hip: elements of its input; conv_bwd.hip: pixels): every padded tensor below 2^31
    if ((long long)N * H * W * CiPad >= (1ll << 31) || (long long)N * Ho * Wo * CoPad >= (1ll << 31) ||
        (long long)N * Hd * Wd * CoPad >= (1ll << 31))
        return TDRN_E_UNSUPPORTED;
    if (reach >= (1 << 20)) return TDRN_E_UNSUPPORTED;      // only stride 1 has a dilation to choose
    p.wg = ConvBwdGeom{N, Cin, H, W, Cout, k, pad, dil, (int)Ho, (int)Wo, stride};
    ConvArgs &f = p.fwd, &d = p.dgrad;
    f.B = d.B = N;
    f.H = d.Ho = H; f.W = d.Wo = W; f.Ho = (int)Ho; f.Wo = (int)Wo; d.H = (int)Hd; d.W = (int)Wd;
    f.Cin = CiPad; f.Cout = Cout; f.Npad = conv_n_pad(Cout); f.pad = pad; f.stride = stride;
    d.Cin = CoPad; d.Cout = Cin; d.Npad = conv_n_pad(Cin); d.pad = (int)reach - pad;
    f.kh = f.kw = d.kh = d.kw = k; f.dil = d.dil = dil;
    conv_train_dense_out(f);
    conv_train_dense_out(d);
    conv_train_layout(p, dtype);
    return TDRN_OK;
}

// Resident tensors (section i-k): what the entries check of an activation pointer and of the type
bool off_16(const void *p) { return ((uintptr_t)p & 15) != 0; }
bool dtype16_ok(int dtype) { return dtype == TDRN_BF16 || dtype == TDRN_F16; }

// The resident conv (section i-k): conv_dense_plan's geometry for DENSE_STRIDE1 with whole 64-channel blocks on both sides, so that the
// caller's tensors ARE launch_conv's input and output and conv_wgrad's two operands.  The result is 16-bit (out_f32 = 0), which opens
// conv3x3_patch / conv3x3_pp / pw1x1 to conv_route; conv3x3_pp gets no chained-split scratch (sk_ws stays null: whole items only), so
// no launch polls another workgroup's flag.  Workspace: zero page | packed weight | padded bias | the split-K partials of launch_conv
// or the weight gradient's slabs (they share their place).
int conv_nhwc_plan(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilH, int dilW, int dtype,
                   int flags, ConvTrainPlan &p)
{
    if (!dtype16_ok(dtype) || (flags & ~TDRN_CONV_NHWC_IGEMM_ONLY)) return TDRN_E_ARG;
    TDRN_TRY(conv_dense_plan(DENSE_STRIDE1, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilH, dilW, dtype, p));
    if (Cin % kChanPad || Cout % kChanPad) return TDRN_E_UNSUPPORTED;
    const size_t es = dtype_bytes(dtype);
    size_t w_bytes = 0, partial = 0;
    int npad = 0;
    for (ConvArgs *a : {&p.fwd, &p.dgrad}) {
        a->out_f32 = 0;
        a->sk_ws = nullptr;
        // the K slices are those of the default route (a direct-conv layer has none), whatever the flag says: a split would add one
        // more difference in fp32 order to those the two routes already have (tdrn_hip.h section i-k: bit-equal only for one
        // 64-channel chunk and no bias), and the workspace size stays the same
        a->kdisable = KOFF_HEAD3X3 | KOFF_TAP_SKIP;
        a->splitk = 1;
        a->splitk = conv_splitk_choice(*a);
        if (flags & TDRN_CONV_NHWC_IGEMM_ONLY) a->kdisable |= KOFF_CONV_PATCH | KOFF_CONV_PP | KOFF_PW1X1;
        w_bytes = std::max(w_bytes, (size_t)a->Npad * a->kh * a->kw * a->Cin * es);
        partial = std::max(partial, conv_splitk_bytes(*a, a->splitk));
        npad = std::max(npad, a->Npad);
    }
    size_t o = 0;
    p.o_zero = o; o += kZeroPageBytes;
    p.o_w = o;    o += align_up(w_bytes, 256);
    p.o_bias = o; o += align_up((size_t)npad * 4, 256);
    p.o_partial = p.o_slab = o;
    p.o_x = p.o_go = p.o_out = 0;       // (the caller's tensors)
    p.total = o + std::max(align_up(partial, 256), conv_wgrad_slab_bytes(p.wg));
    return TDRN_OK;
}

// launch_conv from the caller's tensor into the caller's tensor
int conv_nhwc_run(const ConvTrainPlan &p, char *ws, bool dgrad, const void *in, void *out, hipStream_t s)
{
    ConvArgs a = dgrad ? p.dgrad : p.fwd;
    a.in = in; a.w = ws + p.o_w; a.zero_page = ws + p.o_zero; a.bias = (const float *)(ws + p.o_bias);
    a.out = out;
    if (a.splitk > 1) a.partial = ws + p.o_partial;
    return launch_conv(a, s);
}

// ConvTranspose2d(k = 2, s = 2) (section i-f).  The forward is four phase GEMMs, each a 1x1 conv that writes every second pixel of
// every second row; the input gradient is one 1x1 conv over the space-to-depth image of grad_output, whose C4 = 4 CoPad channels are
// the (tap, cout) pairs of the sum; the weight gradient is the one-tap GEMM over that image with C4 "output channels".
int convt2d_plan(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int opadH, int opadW, int dilH,
                 int dilW, int dtype, ConvTrainPlan &p)
{
    if (!conv_sizes_ok(N, Cin, Cout, H, W, kH, kW, dH, dW, padH, padW, dilH, dilW) || opadH < 0 || opadW < 0) return TDRN_E_SHAPE;
    if (!dtype_ok(dtype)) return TDRN_E_ARG;
    // what the kernels cover: the four taps of a 2x2 kernel at stride 2 write four disjoint phases of the output
    if (kH != 2 || kW != 2 || dH != 2 || dW != 2 || padH || padW || opadH || opadW || dilH != 1 || dilW != 1) return TDRN_E_UNSUPPORTED;
    const long long CiPad = ((long long)Cin + kChanPad - 1) / kChanPad * kChanPad, CoPad = ((long long)Cout + kChanPad - 1) / kChanPad * kChanPad;
    // 32-bit offsets of the kernels (conv_igemm.hip: elements of its input; conv_bwd.hip: pixels; the NCHW <-> NHWC conversions)
    if ((long long)H * W >= (1ll << 31)) return TDRN_E_UNSUPPORTED;
    const long long px = (long long)N * ((long long)H * W);
    if (px >= (1ll << 31) || px * CiPad >= (1ll << 31) || px * 4 * CoPad >= (1ll << 31) || px * 4 * Cout >= (1ll << 31)) return TDRN_E_UNSUPPORTED;
    const int C4 = 4 * (int)CoPad;
    p.wg = ConvBwdGeom{N, Cin, H, W, C4, 1, 0, 1, H, W};
    ConvArgs &f = p.fwd, &d = p.dgrad;      // both 1x1 at stride 1 over H x W pixels: ConvArgs' defaults
    f.B = d.B = N;
    f.H = f.Ho = d.H = d.Ho = H; f.W = f.Wo = d.W = d.Wo = W;
    f.Cin = (int)CiPad; f.Cout = Cout; f.Npad = conv_n_pad(Cout); f.phases = 4;
    f.o_cs = 2ll * Cout; f.o_rs = 4ll * W * Cout; f.o_bs = 4ll * H * W * Cout;
    f.o_pr = 2ll * W * Cout; f.o_pc = Cout;
    d.Cin = C4; d.Cout = Cin; d.Npad = conv_n_pad(Cin);
    conv_train_dense_out(d);
    conv_train_layout(p, dtype);
    return TDRN_OK;
}

// depthwise 3x3 conv (section i-h): fp32 NCHW planes straight through dwconv_train.hip, no ConvTrainPlan.  The workspace holds the
// weight gradient's partials and nothing else; one size serves the three entries.
struct DwConvPlan {
    int stride, Ho, Wo;
    size_t total;
};

int dwconv2d_plan(int N, int C, int H, int W, int kH, int kW, int dH, int dW, int padH, int padW, int dilH, int dilW, int dtype, DwConvPlan &p)
{
    if (!conv_sizes_ok(N, C, C, H, W, kH, kW, dH, dW, padH, padW, dilH, dilW)) return TDRN_E_SHAPE;
    if (!conv_window_fits(H, W, kH, kW, padH, padW, dilH, dilW)) return TDRN_E_SHAPE;
    if (!dtype_ok(dtype)) return TDRN_E_ARG;
    // what the kernels cover: k = 3, one stride of 1 or 2 for both axes, pad 1, dilation 1, fp32 (the op is bandwidth-bound, and the
    // inference engine keeps depthwise weights in fp32 in its 16-bit plans too)
    if (kH != 3 || kW != 3 || dH != dW || dH > 2 || padH != 1 || padW != 1 || dilH != 1 || dilW != 1) return TDRN_E_UNSUPPORTED;
    if (dtype != TDRN_F32) return TDRN_E_UNSUPPORTED;
    // N C H W below 2^31 (every factor is >= 1, so a partial product at the limit settles it before anything can overflow)
    long long elems = 1;
    for (int f : {N, C, H, W}) {
        elems *= f;
        if (elems >= (1ll << 31)) return TDRN_E_UNSUPPORTED;
    }
    p.stride = dH;
    p.Ho = (H - 1) / dH + 1;
    p.Wo = (W - 1) / dW + 1;
    p.total = dwconv_workspace_bytes(N, C, p.Ho, p.Wo);
    return TDRN_OK;
}

// BatchNorm2d (section i-d) and L2Norm (section i-e): the geometry checks of their queries and entries
int nchw_plan(int N, int C, int H, int W)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return TDRN_E_SHAPE;
    // 32-bit element offsets of the kernels
    const long long HW = (long long)H * W, NC = (long long)N * C;
    if (HW >= (1ll << 31) || NC >= (1ll << 31) || NC * HW >= (1ll << 31)) return TDRN_E_UNSUPPORTED;
    return TDRN_OK;
}

// the checks the resident BatchNorm and MaxPool entries share, after their pointers and type: nchw_plan's, and whole channel blocks
int nhwc_plan(int N, int C, int H, int W)
{
    const int rc = nchw_plan(N, C, H, W);
    if (rc != TDRN_OK) return rc;
    return C % kChanPad ? TDRN_E_UNSUPPORTED : TDRN_OK;
}

bool off_dword(const void *p) { return ((uintptr_t)p & 3) != 0; }

// MaxPool2d (section i-e).  The output size of any well-formed window (torch's rule: in ceil mode the last window starts inside the
// input or its left padding); 0 when nothing fits
int pool_out(int in, int k, int s, int p, int ceil_mode)
{
    if (in <= 0 || k <= 0 || s <= 0 || p < 0) return 0;
    const long long num = (long long)in + 2ll * p - k;
    if (num < 0) return ceil_mode && num + s - 1 >= 0 && in + p > 0 ? 1 : 0;
    long long o = (ceil_mode ? (num + s - 1) / s : num / s) + 1;
    if (ceil_mode && (o - 1) * s >= (long long)in + p) --o;
    return (int)o;
}

bool pool_geometry_supported(int k, int s, int p) { return (k == 2 && s == 2 && p == 0) || (k == 3 && s == 1 && p == 1); }

// the checks both pool entries share, after their pointers
int max_pool_plan(int N, int C, int H, int W, int k, int s, int p, int ceil_mode, int &Ho, int &Wo)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return TDRN_E_SHAPE;
    const bool formed = k > 0 && s > 0 && p >= 0;
    Ho = pool_out(H, k, s, p, ceil_mode);
    Wo = pool_out(W, k, s, p, ceil_mode);
    if (formed && (Ho == 0 || Wo == 0)) return TDRN_E_SHAPE;
    if (!pool_geometry_supported(k, s, p)) return TDRN_E_UNSUPPORTED;
    if ((long long)N * C * H * W >= (1ll << 31) || (long long)N * C >= (1ll << 31) || (long long)H * W >= (1ll << 31))
        return TDRN_E_UNSUPPORTED;
    return TDRN_OK;
}

// The transform-domain deformable conv (section i-l): one plan and one workspace size for the forward and the backward.
// Workspace: zero page | X 16-bit NHWC | Y (when the caller holds none) | the packed weight of the GEMM that runs (Y's or grad_input's)
// | a zero bias | launch_conv's split-K partials | grad_output / the sampled result as fp32 [pixel][Cout] | Z fp32 | Z 16-bit | the
// NHWC fp32 grad_input or, after it, the weight gradient's slabs.
struct DeformTsPlan {
    DeformBwdGeom g;
    ConvArgs ygemm, dgrad;      // launch_conv's arguments without their pointers: X -> Y (16-bit result), Z -> grad_input (fp32 NHWC)
    ConvBwdGeom wg;             // the weight gradient: a one-tap GEMM with Z as its "grad_output"
    int YC;
    size_t y_bytes, z_elems;
    size_t o_zero, o_x, o_y, o_w, o_bias, o_partial, o_go, o_z32, o_z16, o_gin, o_slab, total;
};

// the product of positive factors stays below 2^31 (a partial product at the limit settles it before anything can overflow)
bool below_2_31(std::initializer_list<long long> factors)
{
    long long e = 1;
    for (long long f : factors) {
        if (f >= (1ll << 31)) return false;
        e *= f;
        if (e >= (1ll << 31)) return false;
    }
    return true;
}

int deform_ts_plan(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilH, int dilW, int G,
                   int dtype, DeformTsPlan &t)
{
    // shape_check as in deform_plan, without its "input image is smaller than kernel" rule: Y lives on input pixels and a padded
    // window that fits is all the sampling needs (a 1 x 1 map under a 3 x 3 kernel with pad 1 is covered)
    if (!conv_sizes_ok(N, Cin, Cout, H, W, kH, kW, dH, dW, padH, padW, dilH, dilW) || G <= 0 || Cin % G != 0) return TDRN_E_SHAPE;
    if (!dtype_ok(dtype)) return TDRN_E_ARG;
    if (!conv_window_fits(H, W, kH, kW, padH, padW, dilH, dilW)) return TDRN_E_SHAPE;
    // what the kernels cover
    if (G != 1 || !dtype16_ok(dtype) || Cin % kChanPad != 0 || Cout > 256) return TDRN_E_UNSUPPORTED;
    if (!below_2_31({kH, kW}) || !below_2_31({dilH, kH}) || !below_2_31({dilW, kW})) return TDRN_E_UNSUPPORTED;
    const long long Ho = ((long long)H + 2ll * padH - ((long long)dilH * (kH - 1) + 1)) / dH + 1;
    const long long Wo = ((long long)W + 2ll * padW - ((long long)dilW * (kW - 1) + 1)) / dW + 1;
    const long long taps = (long long)kH * kW, cols = (taps * deform_ts_cp(Cout) + kChanPad - 1) / kChanPad * kChanPad;
    // every buffer below 2^31 elements: the tensors, Y and Z, the packed weights; and the coordinates of deform_sample stay ints
    if (!below_2_31({N, H, W, Cin}) || !below_2_31({N, H, W, cols}) || !below_2_31({N, Ho, Wo, Cout}) || !below_2_31({N, Ho, Wo, 2 * taps}) ||
        !below_2_31({Cout, Cin, taps}) || !below_2_31({conv_n_pad(Cin), cols}) || !below_2_31({cols + 128, Cin}) ||
        !below_2_31({Ho, dH}) || !below_2_31({Wo, dW}))
        return TDRN_E_UNSUPPORTED;
    t.g = DeformBwdGeom{N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilH, dilW, G, (int)Ho, (int)Wo};
    t.YC = deform_ts_cols(t.g);
    const size_t es = dtype_bytes(dtype), Mx = (size_t)N * H * W, M = (size_t)N * Ho * Wo;
    t.z_elems = Mx * t.YC;
    t.y_bytes = t.z_elems * es;
    t.wg = ConvBwdGeom{N, Cin, H, W, t.YC, 1, 0, 1, H, W};
    ConvArgs &y = t.ygemm, &d = t.dgrad;        // both 1x1 at stride 1 over H x W pixels: ConvArgs' defaults
    y.B = d.B = N;
    y.H = y.Ho = d.H = d.Ho = H; y.W = y.Wo = d.W = d.Wo = W;
    y.Cin = Cin; y.Cout = t.YC; y.Npad = conv_n_pad(t.YC);
    d.Cin = t.YC; d.Cout = Cin; d.Npad = conv_n_pad(Cin);
    conv_train_dense_out(y);
    conv_train_dense_out(d);
    conv_train_args(y, dtype);
    y.out_f32 = 0;                              // Y is rounded once, in the GEMM's epilogue
    y.splitk = 1;
    y.splitk = conv_splitk_choice(y);
    conv_train_args(d, dtype);
    const size_t wy = (size_t)y.Npad * y.Cin * es, wd = (size_t)d.Npad * d.Cin * es;
    const size_t py = conv_splitk_bytes(y, y.splitk), pd = conv_splitk_bytes(d, d.splitk);
    size_t o = 0;
    t.o_zero = o;    o += kZeroPageBytes;
    t.o_x = o;       o += align_up(Mx * Cin * es, 256);
    t.o_y = o;       o += align_up(t.y_bytes, 256);
    t.o_w = o;       o += align_up(std::max(wy, wd), 256);
    t.o_bias = o;    o += align_up((size_t)std::max(y.Npad, d.Npad) * 4, 256);
    t.o_partial = o; o += align_up(std::max(py, pd), 256);
    t.o_go = o;      o += align_up(M * Cout * 4, 256);
    t.o_z32 = o;     o += align_up(t.z_elems * 4, 256);
    t.o_z16 = o;     o += align_up(t.z_elems * es, 256);
    t.o_gin = t.o_slab = o;
    t.total = o + std::max(align_up(Mx * Cin * 4, 256), conv_wgrad_slab_bytes(t.wg));
    return TDRN_OK;
}

// Y = X W^T into `y` (the caller's buffer or the workspace's): X is in the workspace already
int deform_ts_ygemm(const DeformTsPlan &t, char *ws, const float *weight, void *y, int dtype, hipStream_t s)
{
    ConvArgs a = t.ygemm;
    TDRN_TRY(launch_deform_ts_repack(t.g, weight, ws + t.o_w, a.Npad, 0, dtype, s));
    TDRN_TRY(conv_train_bias(a, ws + t.o_bias, nullptr, s));
    a.in = ws + t.o_x; a.w = ws + t.o_w; a.zero_page = ws + t.o_zero; a.bias = (const float *)(ws + t.o_bias); a.out = y;
    if (a.splitk > 1) a.partial = ws + t.o_partial;
    return launch_conv(a, s);
}

}  // namespace

extern "C" {

const char *tdrn_version(void) { return "tdrn_hip 0.6 (gfx950)"; }

const char *tdrn_error_string(int code)
{
    switch (code) {
        case TDRN_OK: return "ok";
        case TDRN_E_ARG: return "invalid argument";
        case TDRN_E_SHAPE: return "shape check failed";
        case TDRN_E_WORKSPACE: return "workspace too small";
        case TDRN_E_UNSUPPORTED: return "unsupported configuration";
        case TDRN_E_PARAM: return "unknown, missing or mis-shaped parameter";
        case TDRN_E_STATE: return "invalid call order";
        case TDRN_E_VALUE: return "nms_threshold must be non negative.";
        case TDRN_E_DEVICE: return "a device-side hand-off of an earlier forward timed out (its outputs are invalid)";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

size_t tdrn_deform_conv_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH,
                                        int padW, int dilationH, int dilationW, int deformable_group, tdrn_dtype compute)
{
    DeformPlan p;
    if (deform_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, deformable_group, compute, p) != TDRN_OK)
        return 0;
    return p.total;
}

int tdrn_deform_conv_forward(const float *input, const float *weight, const float *offset, float *output, int N, int Cin,
                             int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH, int dilationH,
                             int dilationW, int deformable_group, tdrn_dtype compute, void *workspace,
                             size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !offset || !output) return TDRN_E_ARG;
    DeformPlan p;
    TDRN_TRY(deform_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, deformable_group, compute, p));
    if (!workspace || workspace_bytes < p.total) return TDRN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int G = deformable_group, es = dtype_bytes(compute);
    TDRN_TRY(launch_fill_zero(ws + p.o_zero, kZeroPageBytes, s));
    TDRN_TRY(launch_nchw_to_nhwc_grouped(input, ws + p.o_in, N, Cin, H * W, G, p.cpg_pad, compute, s));
    TDRN_TRY(launch_repack_oihw(weight, ws + p.o_w, Cout, p.Npad_total, Cin, p.taps, G, p.cpg_pad, compute, s));
    const int offC = G * 2 * p.taps;
    TDRN_TRY(launch_nchw_to_nhwc(offset, ws + p.o_off, N, offC, p.Ho * p.Wo, offC, TDRN_F32, s));
    float *out_nhwc = (float *)(ws + p.o_out);
    for (int c = 0; c < p.chunks; ++c) {
        const int c0 = c * 128, cn = (Cout - c0) < 128 ? (Cout - c0) : 128;
        DeformArgs a;
        a.in = ws + p.o_in; a.zero_page = ws + p.o_zero; a.n_branches = 1;
        a.br[0] = DeformBranch{(const float *)(ws + p.o_off), offC, ws + p.o_w + (size_t)c0 * p.taps * p.Cin_pad * es,
                               kH, kW, padH, dH, dilationH, G, padW, dW, dilationW};
        a.B = N; a.H = H; a.W = W; a.Cin = p.Cin_pad; a.Ho = p.Ho; a.Wo = p.Wo; a.Cout = cn; a.Npad = deform_n_pad(cn);
        a.out0 = out_nhwc + c0; a.o0_bs = (long long)p.Ho * p.Wo * Cout; a.o0_ps = Cout; a.split = cn;
        a.dtype = compute;
        TDRN_TRY(launch_deform(a, s));
    }
    return launch_nhwc_to_nchw_f32(out_nhwc, (long long)p.Ho * p.Wo * Cout, Cout, output, N, Cout, p.Ho * p.Wo, s);
}

size_t tdrn_deform_conv_backward_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH,
                                                 int padW, int dilationH, int dilationW, int deformable_group)
{
    DeformBwdPlan b;
    if (deform_bwd_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, deformable_group, b) != TDRN_OK) return 0;
    return b.total;
}

int tdrn_deform_conv_backward_input(const float *input, const float *offset, const float *grad_output, float *grad_input,
                                    float *grad_offset, const float *weight, int N, int Cin, int H, int W, int Cout, int kW, int kH,
                                    int dW, int dH, int padW, int padH, int dilationH, int dilationW, int deformable_group,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !offset || !grad_output || !grad_input || !grad_offset || !weight) return TDRN_E_ARG;
    DeformBwdPlan b;
    TDRN_TRY(deform_bwd_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, deformable_group, b));
    if (!workspace || workspace_bytes < b.total) return TDRN_E_WORKSPACE;
    if (deform_bwd_data_px(b.g) == 0) return TDRN_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int G = deformable_group, cpg64 = deform_bwd_cpg64(b.g), taps = kH * kW;
    float *in_nhwc = (float *)(ws + b.o_in), *gin = (float *)(ws + b.o_gin), *wr = (float *)(ws + b.o_w);
    TDRN_TRY(launch_nchw_to_nhwc_grouped(input, in_nhwc, N, Cin, H * W, G, cpg64, TDRN_F32, s));
    TDRN_TRY(launch_repack_oihw(weight, wr, Cout, Cout, Cin, taps, G, cpg64, TDRN_F32, s));
    TDRN_TRY(launch_fill_zero(gin, (size_t)N * H * W * cpg64 * G * 4, s));
    TDRN_TRY(launch_deform_bwd_data(b.g, in_nhwc, offset, grad_output, wr, gin, grad_offset, s));
    return launch_deform_bwd_input_add(b.g, gin, grad_input, s);
}

int tdrn_deform_conv_backward_parameters(const float *input, const float *offset, const float *grad_output, float *grad_weight, int N,
                                         int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH,
                                         int dilationH, int dilationW, int deformable_group, float scale, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    if (!input || !offset || !grad_output || !grad_weight) return TDRN_E_ARG;
    DeformBwdPlan b;
    TDRN_TRY(deform_bwd_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, deformable_group, b));
    if (!workspace || workspace_bytes < b.total) return TDRN_E_WORKSPACE;
    // the same limits as backward_input (32-bit element offsets, its LDS budget): a layer is served by both entries or by neither
    if (deform_bwd_data_px(b.g) == 0) return TDRN_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *in_nhwc = (float *)(ws + b.o_in);
    TDRN_TRY(launch_nchw_to_nhwc_grouped(input, in_nhwc, N, Cin, H * W, deformable_group, deform_bwd_cpg64(b.g), TDRN_F32, s));
    return launch_deform_bwd_weight(b.g, in_nhwc, offset, grad_output, (float *)(ws + b.o_slab), grad_weight, scale, s);
}

// ---- section (i-l): the transform-domain deformable conv ---------------------------------------------------------------------------------
size_t tdrn_deform_conv_ts_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH,
                                           int dilationH, int dilationW, int deformable_group, tdrn_dtype dtype)
{
    DeformTsPlan t;
    return deform_ts_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, deformable_group, dtype, t) == TDRN_OK ? t.total : 0;
}

size_t tdrn_deform_conv_ts_y_bytes(int N, int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH, int dilationH,
                                   int dilationW, int deformable_group, tdrn_dtype dtype)
{
    DeformTsPlan t;
    return deform_ts_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, deformable_group, dtype, t) == TDRN_OK ? t.y_bytes : 0;
}

int tdrn_deform_conv_ts_forward(const float *input, const float *weight, const float *offset, float *output, void *y_save, int N, int Cin,
                                int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH, int dilationH, int dilationW,
                                int deformable_group, tdrn_dtype dtype, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !offset || !output) return TDRN_E_ARG;
    if (off_dword(input) || off_dword(weight) || off_dword(offset) || off_dword(output) || off_16(y_save)) return TDRN_E_ARG;
    DeformTsPlan t;
    TDRN_TRY(deform_ts_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, deformable_group, dtype, t));
    if (!workspace || workspace_bytes < t.total) return TDRN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    void *y = y_save ? y_save : (void *)(ws + t.o_y);
    const int HoWo = t.g.Ho * t.g.Wo;
    TDRN_TRY(launch_fill_zero(ws + t.o_zero, kZeroPageBytes, s));
    TDRN_TRY(launch_nchw_to_nhwc(input, ws + t.o_x, N, Cin, H * W, Cin, dtype, s));
    TDRN_TRY(deform_ts_ygemm(t, ws, weight, y, dtype, s));
    TDRN_TRY(launch_deform_ts_sample(t.g, y, offset, (float *)(ws + t.o_go), dtype, s));
    return launch_nhwc_to_nchw_f32((const float *)(ws + t.o_go), (long long)HoWo * Cout, Cout, output, N, Cout, HoWo, s);
}

int tdrn_deform_conv_ts_backward(const float *input, const float *weight, const float *offset, const float *grad_output, const void *y_saved,
                                 float *grad_input, float *grad_offset, float *grad_weight, int N, int Cin, int H, int W, int Cout, int kW,
                                 int kH, int dW, int dH, int padW, int padH, int dilationH, int dilationW, int deformable_group,
                                 tdrn_dtype dtype, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !offset || !grad_output || (!grad_input && !grad_offset && !grad_weight)) return TDRN_E_ARG;
    if (off_dword(input) || off_dword(weight) || off_dword(offset) || off_dword(grad_output) || off_16(y_saved) || off_dword(grad_input) ||
        off_dword(grad_offset) || off_dword(grad_weight))
        return TDRN_E_ARG;
    DeformTsPlan t;
    TDRN_TRY(deform_ts_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, deformable_group, dtype, t));
    if (!workspace || workspace_bytes < t.total) return TDRN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const bool need_z = grad_input || grad_weight, need_y = grad_offset != nullptr;
    const int HW = H * W, HoWo = t.g.Ho * t.g.Wo;
    TDRN_TRY(launch_fill_zero(ws + t.o_zero, kZeroPageBytes, s));
    if (grad_weight || (need_y && !y_saved)) TDRN_TRY(launch_nchw_to_nhwc(input, ws + t.o_x, N, Cin, HW, Cin, dtype, s));
    const void *y = nullptr;
    if (need_y) {
        y = y_saved;
        if (!y) {
            TDRN_TRY(deform_ts_ygemm(t, ws, weight, ws + t.o_y, dtype, s));
            y = ws + t.o_y;
        }
    }
    float *go = (float *)(ws + t.o_go), *z32 = (float *)(ws + t.o_z32);
    TDRN_TRY(launch_nchw_to_nhwc(grad_output, go, N, Cout, HoWo, Cout, TDRN_F32, s));
    if (need_z) TDRN_TRY(launch_fill_zero(z32, t.z_elems * 4, s));
    // one pass over (pixel, tap): grad_offset from Y's corners, Z by atomics
    TDRN_TRY(launch_deform_ts_backward(t.g, y, offset, go, need_z ? z32 : nullptr, grad_offset, dtype, s));
    if (!need_z) return TDRN_OK;
    TDRN_TRY(launch_deform_ts_round(z32, ws + t.o_z16, (long long)t.z_elems, dtype, s));
    if (grad_input) {
        ConvArgs a = t.dgrad;
        TDRN_TRY(launch_deform_ts_repack(t.g, weight, ws + t.o_w, a.Npad, 1, dtype, s));
        TDRN_TRY(conv_train_bias(a, ws + t.o_bias, nullptr, s));
        a.in = ws + t.o_z16; a.w = ws + t.o_w; a.zero_page = ws + t.o_zero; a.bias = (const float *)(ws + t.o_bias); a.out = ws + t.o_gin;
        if (a.splitk > 1) a.partial = ws + t.o_partial;
        TDRN_TRY(launch_conv(a, s));
        TDRN_TRY(launch_nhwc_to_nchw_f32((const float *)(ws + t.o_gin), a.o_bs, a.Cout, grad_input, N, Cin, HW, s));
    }
    if (grad_weight) {
        int splits;
        const float *bslab;
        TDRN_TRY(launch_conv_wgrad_slabs(t.wg, ws + t.o_x, ws + t.o_z16, ws + t.o_zero, ws + t.o_slab, dtype, s, splits, bslab));
        TDRN_TRY(launch_deform_ts_wgrad_reduce(t.g, (const float *)(ws + t.o_slab), grad_weight, splits, s));
    }
    return TDRN_OK;
}

// The entries of the trainable conv families (ConvTrainPlan above): pointer check, plan, then conv_train_begin, layout conversion(s),
// weight packing and tail -- for the dense families in the three bodies below, for ConvTranspose2d in its entries.
namespace {

// what the dense families (i-c, i-g, i-i) do once their plan has spoken: conversions, packing, one launch
int conv_dense_forward(int plan_rc, const ConvTrainPlan &p, const float *input, const float *weight, const float *bias, float *output,
                       int Cin, int dtype, void *workspace, size_t workspace_bytes, hipStream_t s)
{
    char *ws = (char *)workspace;
    TDRN_TRY(conv_train_begin(plan_rc, p, workspace, workspace_bytes, s));
    const ConvArgs &f = p.fwd;
    TDRN_TRY(launch_nchw_to_nhwc(input, ws + p.o_x, f.B, Cin, f.H * f.W, f.Cin, dtype, s));
    TDRN_TRY(launch_repack_oihw(weight, ws + p.o_w, f.Cout, f.Npad, Cin, f.kh * f.kw, 1, f.Cin, dtype, s));
    TDRN_TRY(conv_train_bias(f, ws + p.o_bias, bias, s));
    return conv_train_run(p, ws, false, output, s);
}

int conv_dense_backward_input(int plan_rc, const ConvTrainPlan &p, const float *grad_output, const float *weight, float *grad_input,
                              int dtype, void *workspace, size_t workspace_bytes, hipStream_t s)
{
    char *ws = (char *)workspace;
    TDRN_TRY(conv_train_begin(plan_rc, p, workspace, workspace_bytes, s));
    const ConvArgs &d = p.dgrad;
    if (p.wg.stride == 2)   // the zero-inserted image: the kernel stores every element of it, zeros included
        TDRN_TRY(launch_nchw_to_nhwc_dilate2(grad_output, ws + p.o_go, d.B, p.wg.Cout, p.wg.Ho, p.wg.Wo, d.H, d.W, dtype, s));
    else
        TDRN_TRY(launch_nchw_to_nhwc(grad_output, ws + p.o_go, d.B, p.wg.Cout, p.wg.Ho * p.wg.Wo, d.Cin, dtype, s));
    TDRN_TRY(launch_repack_oihw_dgrad(weight, ws + p.o_w, p.wg.Cout, p.wg.Cin, d.Npad, d.kh * d.kw, dtype, s));
    TDRN_TRY(conv_train_bias(d, ws + p.o_bias, nullptr, s));
    return conv_train_run(p, ws, true, grad_input, s);
}

int conv_dense_backward_parameters(int plan_rc, const ConvTrainPlan &p, const float *input, const float *grad_output, float *grad_weight,
                                   float *grad_bias, float scale, int dtype, void *workspace, size_t workspace_bytes, hipStream_t s)
{
    char *ws = (char *)workspace;
    TDRN_TRY(conv_train_begin(plan_rc, p, workspace, workspace_bytes, s));
    TDRN_TRY(launch_nchw_to_nhwc(input, ws + p.o_x, p.wg.N, p.wg.Cin, p.wg.H * p.wg.W, p.fwd.Cin, dtype, s));
    TDRN_TRY(launch_nchw_to_nhwc(grad_output, ws + p.o_go, p.wg.N, p.wg.Cout, p.wg.Ho * p.wg.Wo, p.dgrad.Cin, dtype, s));
    return launch_conv_wgrad(p.wg, ws + p.o_x, ws + p.o_go, ws + p.o_zero, ws + p.o_slab, grad_weight, grad_bias, scale, dtype, s);
}

}  // namespace

size_t tdrn_conv2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                   int dilationH, int dilationW, tdrn_dtype compute)
{
    ConvTrainPlan p;
    return conv_dense_plan(DENSE_STRIDE1, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p) == TDRN_OK ? p.total : 0;
}

int tdrn_conv2d_forward(const float *input, const float *weight, const float *bias, float *output, int N, int Cin, int H, int W, int Cout,
                        int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW, tdrn_dtype compute,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !output) return TDRN_E_ARG;
    ConvTrainPlan p;
    const int rc = conv_dense_plan(DENSE_STRIDE1, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p);
    return conv_dense_forward(rc, p, input, weight, bias, output, Cin, compute, workspace, workspace_bytes, (hipStream_t)stream);
}

int tdrn_conv2d_backward_input(const float *grad_output, const float *weight, float *grad_input, int N, int Cin, int H, int W, int Cout,
                               int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW, tdrn_dtype compute,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    if (!grad_output || !weight || !grad_input) return TDRN_E_ARG;
    ConvTrainPlan p;
    const int rc = conv_dense_plan(DENSE_STRIDE1, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p);
    return conv_dense_backward_input(rc, p, grad_output, weight, grad_input, compute, workspace, workspace_bytes, (hipStream_t)stream);
}

int tdrn_conv2d_backward_parameters(const float *input, const float *grad_output, float *grad_weight, float *grad_bias, int N, int Cin,
                                    int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH,
                                    int dilationW, float scale, tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !grad_output || !grad_weight) return TDRN_E_ARG;
    ConvTrainPlan p;
    const int rc = conv_dense_plan(DENSE_STRIDE1, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p);
    return conv_dense_backward_parameters(rc, p, input, grad_output, grad_weight, grad_bias, scale, compute, workspace, workspace_bytes,
                                          (hipStream_t)stream);
}

// ---- section (i-k): resident tensors ----------------------------------------------------------------------------------------------------
int tdrn_nhwc16_from_nchw(const float *in, void *out, int N, int C, int H, int W, tdrn_dtype dtype, void *stream)
{
    if (!in || !out || off_dword(in) || off_16(out) || !dtype16_ok(dtype)) return TDRN_E_ARG;
    TDRN_TRY(nhwc_plan(N, C, H, W));
    return launch_nchw_to_nhwc(in, out, N, C, H * W, C, dtype, (hipStream_t)stream);
}

int tdrn_nchw_from_nhwc16(const void *in, float *out, int N, int C, int H, int W, tdrn_dtype dtype, void *stream)
{
    if (!in || !out || off_16(in) || off_dword(out) || !dtype16_ok(dtype)) return TDRN_E_ARG;
    TDRN_TRY(nhwc_plan(N, C, H, W));
    return launch_nhwc_any_to_nchw_f32(in, dtype, C, out, N, C, H * W, (hipStream_t)stream);
}

size_t tdrn_conv2d_nhwc_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                        int dilationH, int dilationW, tdrn_dtype dtype, int flags)
{
    ConvTrainPlan p;
    return conv_nhwc_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, dtype, flags, p) == TDRN_OK ? p.total : 0;
}

const char *tdrn_conv2d_nhwc_route(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH,
                                   int dilationW, tdrn_dtype dtype, int flags, int dgrad)
{
    ConvTrainPlan p;
    if (conv_nhwc_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, dtype, flags, p) != TDRN_OK) return nullptr;
    ConvArgs a = dgrad ? p.dgrad : p.fwd;
    if (a.splitk > 1) a.partial = &p;       // (conv_route tests the pointer for null only)
    return conv_kernel_name(conv_route(a, false));
}

int tdrn_conv2d_nhwc_splits(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH,
                            int dilationW, tdrn_dtype dtype, int flags, int *splitk_forward, int *splitk_dgrad, int *wgrad_splits)
{
    if (!splitk_forward || !splitk_dgrad || !wgrad_splits) return TDRN_E_ARG;
    ConvTrainPlan p;
    TDRN_TRY(conv_nhwc_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, dtype, flags, p));
    int per_split;
    *splitk_forward = p.fwd.splitk;
    *splitk_dgrad = p.dgrad.splitk;
    conv_wgrad_splits(p.wg, *wgrad_splits, per_split);
    return TDRN_OK;
}

int tdrn_conv2d_nhwc_forward(const void *input, const float *weight, const float *bias, void *output, int N, int Cin, int H, int W, int Cout,
                             int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW, tdrn_dtype dtype,
                             void *workspace, size_t workspace_bytes, void *stream, int flags)
{
    if (!input || !weight || !output || off_16(input) || off_16(output) || off_dword(weight) || off_dword(bias)) return TDRN_E_ARG;
    ConvTrainPlan p;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    TDRN_TRY(conv_train_begin(conv_nhwc_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, dtype, flags, p), p,
                              workspace, workspace_bytes, s));
    const ConvArgs &f = p.fwd;
    TDRN_TRY(launch_repack_oihw(weight, ws + p.o_w, f.Cout, f.Npad, Cin, f.kh * f.kw, 1, f.Cin, dtype, s));
    TDRN_TRY(conv_train_bias(f, ws + p.o_bias, bias, s));
    return conv_nhwc_run(p, ws, false, input, output, s);
}

int tdrn_conv2d_nhwc_backward_input(const void *grad_output, const float *weight, void *grad_input, int N, int Cin, int H, int W, int Cout,
                                    int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW, tdrn_dtype dtype,
                                    void *workspace, size_t workspace_bytes, void *stream, int flags)
{
    if (!grad_output || !weight || !grad_input || off_16(grad_output) || off_16(grad_input) || off_dword(weight)) return TDRN_E_ARG;
    ConvTrainPlan p;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    TDRN_TRY(conv_train_begin(conv_nhwc_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, dtype, flags, p), p,
                              workspace, workspace_bytes, s));
    const ConvArgs &d = p.dgrad;
    TDRN_TRY(launch_repack_oihw_dgrad(weight, ws + p.o_w, Cout, Cin, d.Npad, d.kh * d.kw, dtype, s));
    TDRN_TRY(conv_train_bias(d, ws + p.o_bias, nullptr, s));
    return conv_nhwc_run(p, ws, true, grad_output, grad_input, s);
}

int tdrn_conv2d_nhwc_backward_parameters(const void *input, const void *grad_output, float *grad_weight, float *grad_bias, int N, int Cin,
                                         int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH,
                                         int dilationW, float scale, tdrn_dtype dtype, void *workspace, size_t workspace_bytes, void *stream,
                                         int flags)
{
    if (!input || !grad_output || !grad_weight || off_16(input) || off_16(grad_output) || off_dword(grad_weight) || off_dword(grad_bias))
        return TDRN_E_ARG;
    ConvTrainPlan p;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    TDRN_TRY(conv_train_begin(conv_nhwc_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, dtype, flags, p), p,
                              workspace, workspace_bytes, s));
    return launch_conv_wgrad(p.wg, input, grad_output, ws + p.o_zero, ws + p.o_slab, grad_weight, grad_bias, scale, dtype, s);
}

int tdrn_batch_norm_nhwc_splits(int N, int C, int H, int W, int *splits, int *per_split)
{
    if (!splits || !per_split) return TDRN_E_ARG;
    TDRN_TRY(nhwc_plan(N, C, H, W));
    batch_norm_nhwc_splits(N, C, H * W, *splits, *per_split);
    return TDRN_OK;
}

size_t tdrn_batch_norm_nhwc_workspace_bytes(int N, int C, int H, int W)
{
    return nhwc_plan(N, C, H, W) == TDRN_OK ? batch_norm_nhwc_workspace_bytes(N, C, H * W) : 0;
}

int tdrn_batch_norm_nhwc_forward(const void *input, const float *weight, const float *bias, float *running_mean, float *running_var,
                                 void *output, float *save_mean, float *save_invstd, int N, int C, int H, int W, int training,
                                 float momentum, float eps, int relu, tdrn_dtype dtype, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !bias || !output || !save_mean || !save_invstd) return TDRN_E_ARG;
    if (!running_mean != !running_var || (!training && !running_mean)) return TDRN_E_ARG;
    if (off_16(input) || off_16(output) || off_dword(weight) || off_dword(bias) || off_dword(running_mean) || off_dword(running_var) ||
        off_dword(save_mean) || off_dword(save_invstd) || off_dword(workspace) || !dtype16_ok(dtype))
        return TDRN_E_ARG;
    TDRN_TRY(nhwc_plan(N, C, H, W));
    if (training && (long long)N * H * W == 1) return TDRN_E_SHAPE;     // one value per channel has no variance
    if (!(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return TDRN_E_ARG;
    if (!workspace || workspace_bytes < batch_norm_nhwc_workspace_bytes(N, C, H * W)) return TDRN_E_WORKSPACE;
    return launch_batch_norm_nhwc_forward(input, weight, bias, running_mean, running_var, output, save_mean, save_invstd, N, C, H * W,
                                          training != 0, momentum, eps, relu != 0, dtype, workspace, (hipStream_t)stream);
}

int tdrn_batch_norm_nhwc_backward(const void *input, const void *grad_output, const float *weight, const float *bias, const float *save_mean,
                                  const float *save_invstd, void *grad_input, float *grad_weight, float *grad_bias, int N, int C, int H,
                                  int W, int training, int relu, float scale, tdrn_dtype dtype, void *workspace, size_t workspace_bytes,
                                  void *stream)
{
    if (!input || !grad_output || !weight || !bias || !save_mean || !save_invstd) return TDRN_E_ARG;
    if (!grad_weight != !grad_bias || (!grad_input && !grad_weight)) return TDRN_E_ARG;
    if (off_16(input) || off_16(grad_output) || off_16(grad_input) || off_dword(weight) || off_dword(bias) || off_dword(save_mean) ||
        off_dword(save_invstd) || off_dword(grad_weight) || off_dword(grad_bias) || off_dword(workspace) || !dtype16_ok(dtype))
        return TDRN_E_ARG;
    TDRN_TRY(nhwc_plan(N, C, H, W));
    if (training && (long long)N * H * W == 1) return TDRN_E_SHAPE;
    if (!workspace || workspace_bytes < batch_norm_nhwc_workspace_bytes(N, C, H * W)) return TDRN_E_WORKSPACE;
    return launch_batch_norm_nhwc_backward(input, grad_output, weight, bias, save_mean, save_invstd, grad_input, grad_weight, grad_bias, N,
                                           C, H * W, training != 0, relu != 0, scale, dtype, workspace, (hipStream_t)stream);
}

int tdrn_max_pool_nhwc_forward(const void *input, void *output, unsigned char *code, int N, int C, int H, int W, int kernel, int stride,
                               int pad, int ceil_mode, tdrn_dtype dtype, void *stream)
{
    if (!input || !output || off_16(input) || off_16(output) || !dtype16_ok(dtype)) return TDRN_E_ARG;
    int Ho, Wo;
    TDRN_TRY(max_pool_plan(N, C, H, W, kernel, stride, pad, ceil_mode, Ho, Wo));
    if (C % kChanPad) return TDRN_E_UNSUPPORTED;
    return launch_max_pool_nhwc_forward(input, output, code, N, C, H, W, Ho, Wo, kernel, dtype, (hipStream_t)stream);
}

int tdrn_max_pool_nhwc_backward(const void *grad_output, const unsigned char *code, void *grad_input, int N, int C, int H, int W, int kernel,
                                int stride, int pad, int ceil_mode, tdrn_dtype dtype, void *stream)
{
    if (!grad_output || !code || !grad_input || off_16(grad_output) || off_16(grad_input) || !dtype16_ok(dtype)) return TDRN_E_ARG;
    int Ho, Wo;
    TDRN_TRY(max_pool_plan(N, C, H, W, kernel, stride, pad, ceil_mode, Ho, Wo));
    if (C % kChanPad) return TDRN_E_UNSUPPORTED;
    return launch_max_pool_nhwc_backward(grad_output, code, grad_input, N, C, H, W, Ho, Wo, kernel, dtype, (hipStream_t)stream);
}

size_t tdrn_conv5x5_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                    int dilationH, int dilationW, tdrn_dtype compute)
{
    ConvTrainPlan p;
    return conv_dense_plan(DENSE_5X5, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p) == TDRN_OK ? p.total : 0;
}

int tdrn_conv5x5_forward(const float *input, const float *weight, const float *bias, float *output, int N, int Cin, int H, int W, int Cout,
                         int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW, tdrn_dtype compute,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !output) return TDRN_E_ARG;
    ConvTrainPlan p;
    const int rc = conv_dense_plan(DENSE_5X5, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p);
    return conv_dense_forward(rc, p, input, weight, bias, output, Cin, compute, workspace, workspace_bytes, (hipStream_t)stream);
}

int tdrn_conv5x5_backward_input(const float *grad_output, const float *weight, float *grad_input, int N, int Cin, int H, int W, int Cout,
                                int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW, tdrn_dtype compute,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    if (!grad_output || !weight || !grad_input) return TDRN_E_ARG;
    ConvTrainPlan p;
    const int rc = conv_dense_plan(DENSE_5X5, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p);
    return conv_dense_backward_input(rc, p, grad_output, weight, grad_input, compute, workspace, workspace_bytes, (hipStream_t)stream);
}

int tdrn_conv5x5_backward_parameters(const float *input, const float *grad_output, float *grad_weight, float *grad_bias, int N, int Cin,
                                     int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH,
                                     int dilationW, float scale, tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !grad_output || !grad_weight) return TDRN_E_ARG;
    ConvTrainPlan p;
    const int rc = conv_dense_plan(DENSE_5X5, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p);
    return conv_dense_backward_parameters(rc, p, input, grad_output, grad_weight, grad_bias, scale, compute, workspace, workspace_bytes,
                                          (hipStream_t)stream);
}

size_t tdrn_conv_transpose2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                             int output_padH, int output_padW, int dilationH, int dilationW, tdrn_dtype compute)
{
    ConvTrainPlan p;
    return convt2d_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, output_padH, output_padW, dilationH, dilationW, compute, p) == TDRN_OK ? p.total : 0;
}

int tdrn_conv_transpose2d_forward(const float *input, const float *weight, const float *bias, float *output, int N, int Cin, int H, int W,
                                  int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int output_padH, int output_padW,
                                  int dilationH, int dilationW, tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !output) return TDRN_E_ARG;
    ConvTrainPlan p;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    TDRN_TRY(conv_train_begin(convt2d_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, output_padH, output_padW, dilationH, dilationW,
                                           compute, p), p, workspace, workspace_bytes, s));
    TDRN_TRY(launch_nchw_to_nhwc(input, ws + p.o_x, N, Cin, H * W, p.fwd.Cin, compute, s));
    TDRN_TRY(launch_repack_iohw_phases(weight, ws + p.o_w, Cin, Cout, p.fwd.Npad, compute, s));
    TDRN_TRY(conv_train_bias(p.fwd, ws + p.o_bias, bias, s));
    return conv_train_run(p, ws, false, output, s);
}

int tdrn_conv_transpose2d_backward_input(const float *grad_output, const float *weight, float *grad_input, int N, int Cin, int H, int W,
                                         int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int output_padH, int output_padW,
                                         int dilationH, int dilationW, tdrn_dtype compute, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    if (!grad_output || !weight || !grad_input) return TDRN_E_ARG;
    ConvTrainPlan p;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    TDRN_TRY(conv_train_begin(convt2d_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, output_padH, output_padW, dilationH, dilationW,
                                           compute, p), p, workspace, workspace_bytes, s));
    TDRN_TRY(launch_nchw_to_nhwc_s2d(grad_output, ws + p.o_go, N, Cout, H, W, compute, s));
    TDRN_TRY(launch_repack_iohw_dgrad(weight, ws + p.o_w, Cin, Cout, p.dgrad.Npad, compute, s));
    TDRN_TRY(conv_train_bias(p.dgrad, ws + p.o_bias, nullptr, s));
    return conv_train_run(p, ws, true, grad_input, s);
}

int tdrn_conv_transpose2d_backward_parameters(const float *input, const float *grad_output, float *grad_weight, float *grad_bias, int N,
                                              int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                              int output_padH, int output_padW, int dilationH, int dilationW, float scale,
                                              tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !grad_output || !grad_weight) return TDRN_E_ARG;
    ConvTrainPlan p;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    TDRN_TRY(conv_train_begin(convt2d_plan(N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, output_padH, output_padW, dilationH, dilationW,
                                           compute, p), p, workspace, workspace_bytes, s));
    TDRN_TRY(launch_nchw_to_nhwc(input, ws + p.o_x, N, Cin, H * W, p.fwd.Cin, compute, s));
    TDRN_TRY(launch_nchw_to_nhwc_s2d(grad_output, ws + p.o_go, N, Cout, H, W, compute, s));
    // the slabs hold (tap, cout) rows: this family reduces them into (Cin, Cout, 2, 2) itself
    int splits;
    const float *bslab;
    TDRN_TRY(launch_conv_wgrad_slabs(p.wg, ws + p.o_x, ws + p.o_go, ws + p.o_zero, ws + p.o_slab, compute, s, splits, bslab));
    return launch_convt_wgrad_reduce((const float *)(ws + p.o_slab), bslab, grad_weight, grad_bias, Cin, Cout, splits, scale, s);
}

size_t tdrn_conv2d_strided_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                           int dilationH, int dilationW, tdrn_dtype compute)
{
    ConvTrainPlan p;
    return conv_dense_plan(DENSE_STRIDE2, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p) == TDRN_OK ? p.total : 0;
}

int tdrn_conv2d_strided_forward(const float *input, const float *weight, const float *bias, float *output, int N, int Cin, int H, int W,
                                int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW,
                                tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !output) return TDRN_E_ARG;
    ConvTrainPlan p;
    const int rc = conv_dense_plan(DENSE_STRIDE2, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p);
    return conv_dense_forward(rc, p, input, weight, bias, output, Cin, compute, workspace, workspace_bytes, (hipStream_t)stream);
}

int tdrn_conv2d_strided_backward_input(const float *grad_output, const float *weight, float *grad_input, int N, int Cin, int H, int W,
                                       int Cout, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW,
                                       tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!grad_output || !weight || !grad_input) return TDRN_E_ARG;
    ConvTrainPlan p;
    const int rc = conv_dense_plan(DENSE_STRIDE2, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p);
    return conv_dense_backward_input(rc, p, grad_output, weight, grad_input, compute, workspace, workspace_bytes, (hipStream_t)stream);
}

int tdrn_conv2d_strided_backward_parameters(const float *input, const float *grad_output, float *grad_weight, float *grad_bias, int N,
                                            int Cin, int H, int W, int Cout, int kH, int kW, int dH, int dW, int padH, int padW,
                                            int dilationH, int dilationW, float scale, tdrn_dtype compute, void *workspace,
                                            size_t workspace_bytes, void *stream)
{
    if (!input || !grad_output || !grad_weight) return TDRN_E_ARG;
    ConvTrainPlan p;
    const int rc = conv_dense_plan(DENSE_STRIDE2, N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p);
    return conv_dense_backward_parameters(rc, p, input, grad_output, grad_weight, grad_bias, scale, compute, workspace, workspace_bytes,
                                          (hipStream_t)stream);
}

size_t tdrn_dwconv2d_workspace_bytes(int N, int C, int H, int W, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH,
                                     int dilationW, tdrn_dtype compute)
{
    DwConvPlan p;
    return dwconv2d_plan(N, C, H, W, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p) == TDRN_OK ? p.total : 0;
}

int tdrn_dwconv2d_forward(const float *input, const float *weight, const float *bias, float *output, int N, int C, int H, int W, int kH,
                          int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW, tdrn_dtype compute, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !output) return TDRN_E_ARG;
    DwConvPlan p;
    TDRN_TRY(dwconv2d_plan(N, C, H, W, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p));
    if (!workspace || workspace_bytes < p.total) return TDRN_E_WORKSPACE;
    return launch_dwconv_forward(input, weight, bias, output, N, C, H, W, p.stride, p.Ho, p.Wo, (hipStream_t)stream);
}

int tdrn_dwconv2d_backward_input(const float *grad_output, const float *weight, float *grad_input, int N, int C, int H, int W, int kH,
                                 int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW, tdrn_dtype compute,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    if (!grad_output || !weight || !grad_input) return TDRN_E_ARG;
    DwConvPlan p;
    TDRN_TRY(dwconv2d_plan(N, C, H, W, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p));
    if (!workspace || workspace_bytes < p.total) return TDRN_E_WORKSPACE;
    return launch_dwconv_backward_input(grad_output, weight, grad_input, N, C, H, W, p.stride, p.Ho, p.Wo, (hipStream_t)stream);
}

int tdrn_dwconv2d_backward_parameters(const float *input, const float *grad_output, float *grad_weight, float *grad_bias, int N, int C,
                                      int H, int W, int kH, int kW, int dH, int dW, int padH, int padW, int dilationH, int dilationW,
                                      float scale, tdrn_dtype compute, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !grad_output || !grad_weight) return TDRN_E_ARG;
    DwConvPlan p;
    TDRN_TRY(dwconv2d_plan(N, C, H, W, kH, kW, dH, dW, padH, padW, dilationH, dilationW, compute, p));
    if (!workspace || workspace_bytes < p.total) return TDRN_E_WORKSPACE;
    return launch_dwconv_backward_parameters(input, grad_output, grad_weight, grad_bias, N, C, H, W, p.stride, p.Ho, p.Wo, scale, workspace,
                                             (hipStream_t)stream);
}

size_t tdrn_batch_norm_workspace_bytes(int N, int C, int H, int W)
{
    return nchw_plan(N, C, H, W) == TDRN_OK ? batch_norm_workspace_bytes(N, C, H * W) : 0;
}

int tdrn_batch_norm_forward(const float *input, const float *weight, const float *bias, float *running_mean, float *running_var,
                            float *output, float *save_mean, float *save_invstd, int N, int C, int H, int W, int training, float momentum,
                            float eps, int relu, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !weight || !bias || !output || !save_mean || !save_invstd) return TDRN_E_ARG;
    if (!running_mean != !running_var || (!training && !running_mean)) return TDRN_E_ARG;
    if (off_dword(input) || off_dword(weight) || off_dword(bias) || off_dword(running_mean) || off_dword(running_var) || off_dword(output) ||
        off_dword(save_mean) || off_dword(save_invstd) || off_dword(workspace))
        return TDRN_E_ARG;
    TDRN_TRY(nchw_plan(N, C, H, W));
    if (training && (long long)N * H * W == 1) return TDRN_E_SHAPE;     // one value per channel has no variance
    if (!(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return TDRN_E_ARG;
    if (!workspace || workspace_bytes < batch_norm_workspace_bytes(N, C, H * W)) return TDRN_E_WORKSPACE;
    return launch_batch_norm_forward(input, weight, bias, running_mean, running_var, output, save_mean, save_invstd, N, C, H * W,
                                     training != 0, momentum, eps, relu != 0, workspace, (hipStream_t)stream);
}

int tdrn_batch_norm_backward(const float *input, const float *grad_output, const float *weight, const float *bias, const float *save_mean,
                             const float *save_invstd, float *grad_input, float *grad_weight, float *grad_bias, int N, int C, int H, int W,
                             int training, int relu, float scale, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!input || !grad_output || !weight || !bias || !save_mean || !save_invstd) return TDRN_E_ARG;
    if (!grad_weight != !grad_bias || (!grad_input && !grad_weight)) return TDRN_E_ARG;
    if (off_dword(input) || off_dword(grad_output) || off_dword(weight) || off_dword(bias) || off_dword(save_mean) || off_dword(save_invstd) ||
        off_dword(grad_input) || off_dword(grad_weight) || off_dword(grad_bias) || off_dword(workspace))
        return TDRN_E_ARG;
    TDRN_TRY(nchw_plan(N, C, H, W));
    if (training && (long long)N * H * W == 1) return TDRN_E_SHAPE;
    if (!workspace || workspace_bytes < batch_norm_workspace_bytes(N, C, H * W)) return TDRN_E_WORKSPACE;
    return launch_batch_norm_backward(input, grad_output, weight, bias, save_mean, save_invstd, grad_input, grad_weight, grad_bias, N, C,
                                      H * W, training != 0, relu != 0, scale, workspace, (hipStream_t)stream);
}

int tdrn_max_pool_output_size(int in, int kernel, int stride, int pad, int ceil_mode)
{
    return pool_geometry_supported(kernel, stride, pad) ? pool_out(in, kernel, stride, pad, ceil_mode) : 0;
}

int tdrn_max_pool_forward(const float *input, float *output, unsigned char *code, int N, int C, int H, int W, int kernel, int stride, int pad,
                          int ceil_mode, void *stream)
{
    if (!input || !output || off_dword(input) || off_dword(output)) return TDRN_E_ARG;
    int Ho, Wo;
    TDRN_TRY(max_pool_plan(N, C, H, W, kernel, stride, pad, ceil_mode, Ho, Wo));
    return launch_max_pool_forward(input, output, code, N * C, H, W, Ho, Wo, kernel, (hipStream_t)stream);
}

int tdrn_max_pool_backward(const float *grad_output, const unsigned char *code, float *grad_input, int N, int C, int H, int W, int kernel,
                           int stride, int pad, int ceil_mode, void *stream)
{
    if (!grad_output || !code || !grad_input || off_dword(grad_output) || off_dword(grad_input)) return TDRN_E_ARG;
    int Ho, Wo;
    TDRN_TRY(max_pool_plan(N, C, H, W, kernel, stride, pad, ceil_mode, Ho, Wo));
    return launch_max_pool_backward(grad_output, code, grad_input, N * C, H, W, Ho, Wo, kernel, (hipStream_t)stream);
}

size_t tdrn_l2norm_workspace_bytes(int N, int C, int H, int W)
{
    return nchw_plan(N, C, H, W) == TDRN_OK ? l2norm_workspace_bytes(N, C, H * W) : 0;
}

int tdrn_l2norm_forward(const float *input, const float *weight, float *output, float *norm, int N, int C, int H, int W, float eps,
                        void *stream)
{
    if (!input || !weight || !output || !(eps > 0.f)) return TDRN_E_ARG;
    if (off_dword(input) || off_dword(weight) || off_dword(output) || off_dword(norm)) return TDRN_E_ARG;
    TDRN_TRY(nchw_plan(N, C, H, W));
    return launch_l2norm_forward(input, weight, output, norm, N, C, H * W, eps, (hipStream_t)stream);
}

int tdrn_l2norm_backward(const float *input, const float *grad_output, const float *weight, const float *norm, float *grad_input,
                         float *grad_weight, int N, int C, int H, int W, float eps, float scale, void *workspace, size_t workspace_bytes,
                         void *stream)
{
    if (!input || !grad_output || !weight || !norm || (!grad_input && !grad_weight) || !(eps > 0.f)) return TDRN_E_ARG;
    if (off_dword(input) || off_dword(grad_output) || off_dword(weight) || off_dword(norm) || off_dword(grad_input) || off_dword(grad_weight) ||
        off_dword(workspace))
        return TDRN_E_ARG;
    TDRN_TRY(nchw_plan(N, C, H, W));
    // the workspace holds grad_weight's partial sums and nothing else
    if (grad_weight && (!workspace || workspace_bytes < l2norm_workspace_bytes(N, C, H * W))) return TDRN_E_WORKSPACE;
    return launch_l2norm_backward(input, grad_output, weight, norm, grad_input, grad_weight, N, C, H * W, eps, scale, workspace,
                                  (hipStream_t)stream);
}

size_t tdrn_nms_workspace_bytes(int n) { return nms_workspace_bytes(n); }

int tdrn_nms(const float *dets, int n, double thresh, int strict_gt, int32_t *keep_out, int32_t *num_out, void *workspace,
             size_t workspace_bytes, void *stream)
{
    return launch_nms(dets, n, thresh, strict_gt, 0, keep_out, num_out, workspace, workspace_bytes, (hipStream_t)stream);
}

int tdrn_nms_topk(const float *dets, int n, float overlap, float min_score, int top_k, int32_t *keep_out, int32_t *num_out,
                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (top_k < 0) return TDRN_E_ARG;
    return launch_nms(dets, n, (double)overlap, 0, 0, keep_out, num_out, workspace, workspace_bytes, (hipStream_t)stream, 1, min_score,
                      top_k);
}

size_t tdrn_nms_topk_classes_workspace_bytes(int n, int num_classes) { return nms_classes_workspace_bytes(n, num_classes); }

int tdrn_nms_topk_classes(const float *boxes, const float *scores, int n, int num_classes, int first_class, float overlap, float min_score,
                          int top_k, int32_t *keep_out, int32_t *num_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (top_k < 0) return TDRN_E_ARG;
    return launch_nms_classes(boxes, scores, n, num_classes, first_class, overlap, min_score, top_k, keep_out, num_out, workspace,
                              workspace_bytes, (hipStream_t)stream);
}

int tdrn_roi_resample(const float *feature, int C, int H, int W, const int32_t *cells, int n, int S, float *out, void *stream)
{
    return launch_roi_resample(feature, C, H, W, cells, n, S, out, (hipStream_t)stream);
}

int tdrn_ota_similarity(const float *boxes, const float *roi, int n, int F, const float *rows, const int32_t *row_off, int m, float *best,
                        int32_t *arg, void *stream)
{
    return launch_ota_similarity(boxes, roi, n, F, rows, row_off, m, best, arg, (hipStream_t)stream);
}

int tdrn_gpu_nms_host(int *keep_out, int *num_out, const float *boxes_host, int boxes_num, int boxes_dim,
                      float nms_overlap_thresh, int device_id)
{
    if (!keep_out || !num_out || (!boxes_host && boxes_num > 0) || boxes_num < 0) return TDRN_E_ARG;
    if (boxes_dim != 5) return TDRN_E_SHAPE;
    *num_out = 0;
    if (boxes_num == 0) return TDRN_OK;
    // the reference's _nms switches the device and never switches back (nms_kernel.cu:21-32); a frame-sharded rank
    // must keep ITS device current, so the previous one is restored on every exit
    int prev_dev = -1;
    TDRN_HIP_TRY(hipGetDevice(&prev_dev));
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore{device_id >= 0 && device_id != prev_dev ? prev_dev : -1};
    if (device_id >= 0 && device_id != prev_dev) TDRN_HIP_TRY(hipSetDevice(device_id));
    const size_t bytes = (size_t)boxes_num * 5 * sizeof(float), wsb = nms_workspace_bytes(boxes_num);
    char *dev = nullptr;
    TDRN_HIP_TRY(hipMalloc((void **)&dev, align_up(bytes, 256) + wsb + align_up((size_t)boxes_num * 4, 256) + 256));
    float *d_boxes = (float *)dev;
    char *d_ws = dev + align_up(bytes, 256);
    int *d_keep = (int *)(d_ws + wsb);
    int *d_num = (int *)((char *)d_keep + align_up((size_t)boxes_num * 4, 256));
    int rc = hip_status(hipMemcpy(d_boxes, boxes_host, bytes, hipMemcpyHostToDevice));
    // the host twin takes a float threshold (gpu_nms.hpp:1-2); nms_kernel.cu:71 compares fp32 > fp32
    if (rc == TDRN_OK) rc = launch_nms(d_boxes, boxes_num, (double)nms_overlap_thresh, 1, 1, d_keep, d_num, d_ws, wsb, 0);
    if (rc == TDRN_OK) rc = hip_status(hipMemcpy(num_out, d_num, sizeof(int), hipMemcpyDeviceToHost));
    if (rc == TDRN_OK && *num_out > 0) rc = hip_status(hipMemcpy(keep_out, d_keep, (size_t)*num_out * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(dev);
    return rc;
}

int tdrn_decode(const float *loc, const float *priors, int P, float var0, float var1, float *boxes_out, void *stream)
{
    if (!loc || !priors || !boxes_out || P < 0) return TDRN_E_ARG;
    if (((uintptr_t)loc | (uintptr_t)priors | (uintptr_t)boxes_out) & 15) return TDRN_E_ARG;     // (P,4) rows as 16-byte vectors
    return launch_decode(loc, priors, P, var0, var1, boxes_out, (hipStream_t)stream);
}

int tdrn_center_size(const float *boxes, int P, float *out, void *stream)
{
    if (!boxes || !out || P < 0) return TDRN_E_ARG;
    if (((uintptr_t)boxes | (uintptr_t)out) & 15) return TDRN_E_ARG;                               // (P,4) rows as 16-byte vectors
    return launch_center_size(boxes, P, out, (hipStream_t)stream);
}

int tdrn_encode(const float *matched, const float *priors, int P, float var0, float var1, float *out, void *stream)
{
    return launch_encode(matched, priors, P, var0, var1, out, (hipStream_t)stream);
}

size_t tdrn_match_workspace_bytes(int B, int P, int max_truths) { return match_workspace_bytes(B, P, max_truths); }

int tdrn_match(const float *truths, const int32_t *truth_off, int T_total, int max_truths, int B, const float *priors, int P,
               const float *arm_loc, float threshold, float var0, float var1, float *loc_t, int32_t *conf_t, void *workspace,
               size_t workspace_bytes, void *stream)
{
    return launch_match(truths, truth_off, T_total, max_truths, B, priors, P, arm_loc, threshold, var0, var1, loc_t, conf_t,
                        workspace, workspace_bytes, (hipStream_t)stream);
}

size_t tdrn_multibox_loss_workspace_bytes(int B, int P, int C) { return multibox_loss_workspace_bytes(B, P, C); }

int tdrn_multibox_loss_forward(const float *loc, const float *conf, const float *loc_t, const int32_t *conf_t, int B, int P, int C,
                               int negpos_ratio, float *loss_out, uint8_t *sel, int32_t *num_pos, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    return launch_multibox_loss_forward(loc, conf, loc_t, conf_t, B, P, C, negpos_ratio, loss_out, sel, num_pos, workspace,
                                        workspace_bytes, (hipStream_t)stream);
}

int tdrn_multibox_loss_backward(const float *loc, const float *conf, const float *loc_t, const int32_t *conf_t, const uint8_t *sel,
                                const int32_t *num_pos, const float *grad_loss, int B, int P, int C, float *grad_loc,
                                float *grad_conf, void *stream)
{
    return launch_multibox_loss_backward(loc, conf, loc_t, conf_t, sel, num_pos, grad_loss, B, P, C, grad_loc, grad_conf,
                                         (hipStream_t)stream);
}

int tdrn_sgd_step(const tdrn_sgd_tensor *tensors_host, int n_tensors, const float *hyper_dev, int n_groups, int flags, void *stream)
{
    return launch_sgd_step(tensors_host, n_tensors, hyper_dev, n_groups, flags, (hipStream_t)stream);
}

int tdrn_amp_check_finite(const tdrn_sgd_tensor *tensors_host, int n_tensors, float *state_dev, void *stream)
{
    return launch_amp_check_finite(tensors_host, n_tensors, state_dev, (hipStream_t)stream);
}

int tdrn_sgd_step_scaled(const tdrn_sgd_tensor *tensors_host, int n_tensors, const float *hyper_dev, int n_groups,
                         const float *state_dev, int flags, void *stream)
{
    return launch_sgd_step_scaled(tensors_host, n_tensors, hyper_dev, n_groups, state_dev, flags, (hipStream_t)stream);
}

int tdrn_amp_update(float *state_dev, float growth_factor, float backoff_factor, int growth_interval, void *stream)
{
    return launch_amp_update(state_dev, growth_factor, backoff_factor, growth_interval, (hipStream_t)stream);
}

int tdrn_augment_sample(const int32_t *hw, const double *truths, const int32_t *truth_off, int T_total, int max_truths, int B,
                        uint64_t seed, const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                        tdrn_augment_params *params, float *out_truths, int32_t *out_off, void *stream)
{
    return launch_augment_sample(hw, truths, truth_off, T_total, max_truths, B, seed, sample_ids, tape, tape_off, params,
                                 out_truths, out_off, (hipStream_t)stream);
}

int tdrn_augment_apply(const tdrn_augment_image *images, const tdrn_augment_params *params, int B, const float *mean, int S,
                       int to_rgb, float *out, void *stream)
{
    return launch_augment_apply(images, params, B, mean, S, to_rgb, out, (hipStream_t)stream);
}

int tdrn_augment_pair_sample(const int32_t *hw, const double *truths, const double *truths_t, const int32_t *truth_off,
                             int T_total, int max_truths, int B, double max_trans_ratio, uint64_t seed, const int64_t *sample_ids,
                             const double *tape, const int32_t *tape_off, tdrn_augment_pair_params *params, float *out_truths,
                             float *out_truths_t, int32_t *out_off, void *stream)
{
    return launch_augment_pair_sample(hw, truths, truths_t, truth_off, T_total, max_truths, B, max_trans_ratio, seed, sample_ids,
                                      tape, tape_off, params, out_truths, out_truths_t, out_off, (hipStream_t)stream);
}

int tdrn_augment_pair_apply(const tdrn_augment_image *images, const tdrn_augment_image *images_t,
                            const tdrn_augment_pair_params *params, int B, const float *mean, int S, int to_rgb, float *out,
                            float *out_t, void *stream)
{
    return launch_augment_pair_apply(images, images_t, params, B, mean, S, to_rgb, out, out_t, (hipStream_t)stream);
}

int tdrn_prior_box(int n_maps, const int *feature_maps, double image_size, const double *steps, const double *min_sizes,
                   const double *max_sizes, int n_max_sizes, const int *ar_count, const double *ars, int clip, int flip,
                   float *out)
{
    // layers/functions/prior_box.py:33-64 -- python floats are C doubles; torch.Tensor(list) rounds to fp32
    if (n_maps <= 0 || !feature_maps || !steps || !min_sizes || !ar_count || image_size <= 0) return TDRN_E_ARG;
    if (n_max_sizes > 0 && (!max_sizes || n_max_sizes < n_maps)) return TDRN_E_ARG;
    long long n = 0;
    int ar_base = 0;
    for (int k = 0; k < n_maps; ++k) {
        const int f = feature_maps[k];
        const double f_k = image_size / steps[k];
        const double s_k = min_sizes[k] / image_size;
        for (int i = 0; i < f; ++i)
            for (int j = 0; j < f; ++j) {
                const double cx = (j + 0.5) / f_k, cy = (i + 0.5) / f_k;
                auto emit = [&](double a, double b, double c, double d) {
                    if (out) {
                        float *o = out + n * 4;
                        o[0] = (float)a; o[1] = (float)b; o[2] = (float)c; o[3] = (float)d;
                    }
                    ++n;
                };
                emit(cx, cy, s_k, s_k);
                if (n_max_sizes > 0) {
                    const double sp = std::sqrt(s_k * (max_sizes[k] / image_size));
                    emit(cx, cy, sp, sp);
                }
                for (int a = 0; a < ar_count[k]; ++a) {
                    const double ar = ars[ar_base + a];
                    emit(cx, cy, s_k * std::sqrt(ar), s_k / std::sqrt(ar));
                    if (flip) emit(cx, cy, s_k / std::sqrt(ar), s_k * std::sqrt(ar));
                }
            }
        ar_base += ar_count[k];
    }
    if (out && clip)
        for (long long i = 0; i < n * 4; ++i) out[i] = out[i] > 1.f ? 1.f : (out[i] < 0.f ? 0.f : out[i]);
    return (int)n;
}

int tdrn_preprocess(const uint8_t *frames, int B, int H0, int W0, int S, const float mean_bgr[3], int to_rgb, float *out,
                    void *stream)
{
    if (!frames || !out || !mean_bgr || B <= 0 || H0 <= 0 || W0 <= 0 || S <= 0) return TDRN_E_ARG;
    return launch_preprocess(frames, B, H0, W0, S, mean_bgr, to_rgb, out, (hipStream_t)stream);
}

int tdrn_preprocess_u8(const uint8_t *frames, int B, int H0, int W0, int S, int to_rgb, uint8_t *out, void *stream)
{
    if (!frames || !out || B <= 0 || H0 <= 0 || W0 <= 0 || S <= 0) return TDRN_E_ARG;
    return launch_preprocess_u8(frames, B, H0, W0, S, to_rgb, out, (hipStream_t)stream);
}

size_t tdrn_detect_workspace_bytes(int B, int P, int C, int top_k)
{
    if (B <= 0 || P <= 0 || C <= 0 || top_k <= 0) return 0;
    return detect_workspace_bytes(B, P, C, top_k);
}

int tdrn_detect(const float *loc, const float *conf, const float *priors, const float *arm_loc, const float *scale_host,
                int B, int P, int C, int top_k, float conf_thresh, double nms_thresh, float *out, int32_t *counts_out,
                void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_detect(loc, conf, priors, arm_loc, scale_host, 0, B, P, C, top_k, conf_thresh, nms_thresh, out, counts_out,
                         workspace, workspace_bytes, (hipStream_t)stream);
}

int tdrn_detect_dev_scale(const float *loc, const float *conf, const float *priors, const float *arm_loc, const float *scale_dev,
                          int B, int P, int C, int top_k, float conf_thresh, double nms_thresh, float *out, int32_t *counts_out,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_detect(loc, conf, priors, arm_loc, scale_dev, 1, B, P, C, top_k, conf_thresh, nms_thresh, out, counts_out,
                         workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
