// kernels.h -- launch interfaces of the HIP kernels (internal to libtdrn_hip).
#pragma once
#include <algorithm>
#include <cmath>

#include "common.h"

namespace tdrn {

// A device buffer every padding tap / out-of-range row reads instead of branching (16-B aligned,
// >= 256 zero bytes).  It lives at the start of the caller-provided workspace / weight blob.
constexpr size_t kZeroPageBytes = 256;

// Raises a kernel's dynamic-LDS limit to the full 160 KiB.  The attribute is per DEVICE: the call is repeated
// for every device a kernel is used on (a small per-device, per-kernel memo keeps it off the hot path; it is
// idempotent, so a race between threads only repeats the call).  (layers.hip)
int allow_big_lds(const void *kernel);

// Kernel-choice switches of a launch (ConvArgs::kdisable, the kdisable argument of launch_dwconv3 / launch_ygemm_multi): each
// turns one kernel or one of its work-distribution schemes OFF.  Plan::build (net_plan.hip) sets them from
// tdrn_net_config.plan_flags; apart from KOFF_HEAD3X3 (another fp32 K order) the output bits are the same either way.
enum KernelOff {
    KOFF_CONV_PP = 1,          // TDRN_PLAN_NO_CONV_PP: conv3x3_pp.hip's layers stay on conv3x3_patch.hip
    KOFF_PP_SK = 2,            // TDRN_PLAN_NO_PP_SK: conv3x3_pp.hip runs whole items only (no chained split)
    KOFF_CONV_PATCH = 4,       // TDRN_PLAN_NO_CONV_PATCH: neither 3x3 direct-conv kernel (everything on conv_igemm.hip)
    KOFF_PW1X1 = 8,            // TDRN_PLAN_NO_PW1X1: the wide 1x1 convs stay on conv_igemm.hip (not dwpw.hip pw1x1_kernel)
    KOFF_DW_SLIDE = 16,        // TDRN_PLAN_NO_DW_SLIDE: depthwise 3x3 on the one-row strip kernel, not the sliding-window one
    KOFF_DW_STRIP_SMALL = 32,  // TDRN_PLAN_DW_SLIDE_ALL: no strip kernel at small batches either (sliding-window, 8-row segments, always)
    KOFF_CONV_WS = 64,         // TDRN_PLAN_NO_CONV_WS: the pooled Cin = 64 layer stays on conv3x3_patch.hip (not conv3x3_ws.hip)
    KOFF_YGEMM_V2 = 128,       // TDRN_PLAN_NO_YGEMM_V2: the heads' transform GEMM on ygemm_k256_kernel's older schedule
    KOFF_HEAD3X3 = 256,        // TDRN_PLAN_NO_HEAD3X3: the narrow fp32 3x3 heads stay on conv_igemm.hip (not head3x3.hip)
    KOFF_TS_RANGES = 512,      // TDRN_PLAN_TS_ONE_RANGE: transform-then-sample heads take the whole batch as one range
    KOFF_PATCH_TAIL = 1024,    // TDRN_PLAN_NO_PATCH_TAIL: conv3x3_patch.hip and pw1x1_kernel run whole items only (no tail split)
    KOFF_TAP_SKIP = 2048,      // (no plan flag: the training entries of api.hip) conv_igemm.hip forms every tap's products, those of a tap that
                               // lies in the padding for a whole pixel tile included: the same bits for finite weights, and a non-finite weight
                               // meets the padding's zeros (inf * 0 = NaN) at every tap, whatever the tiling
};

// Launch glue of the grid-stride kernels: workgroups of 256 threads for `total` elements, at most `cap` of them
inline dim3 stride_grid(long long total, int cap = 16384) { return dim3((unsigned)std::min<long long>((total + 255) / 256, cap)); }

// The one packing kernel: out[i] = map(i) rounded once to DT, i < total.  A packer is its Map: a struct passed by value whose
// __device__ float operator()(long long i) const holds the index map and the range test (zero outside the source).
template <typename DT, typename Map>
__global__ __launch_bounds__(256) void pack_kernel(char *__restrict__ out, long long total, const Map map)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        *(DT *)(out + (size_t)i * elem_traits<DT>::bytes) = from_f32<DT>(map(i));
}
template <typename Map> int launch_pack(int dtype, void *out, long long total, const Map &map, hipStream_t s)
{
    if (total <= 0) return TDRN_OK;
    return dispatch_dtype(dtype, [&](auto tag) {
        using DT = typename decltype(tag)::type;
        hipLaunchKernelGGL((pack_kernel<DT, Map>), stride_grid(total), dim3(256), 0, s, (char *)out, total, map);
        return hip_status(hipGetLastError());
    });
}

// ---------------------------------------------------------------------------------------------
// Dense convolution as implicit GEMM on MFMA (conv_igemm.hip).
//   in  : NHWC [B][H][W][Cin]      (DT; Cin a multiple of the 128-byte K-step)
//   w   : [phases][Npad][kh*kw][Cin] (DT; BatchNorm folded; rows >= Cout are zero)
//   out : element (b,ho,wo,c) at  o_base + b*o_bs + ho*o_rs + wo*o_cs + c   (DT or fp32)
//   res : optional residual with the SAME view as out (DT), added before the ReLU
//   phases = 4 turns the launch into ConvTranspose2d(k=2,s=2): phase z=(i,j) uses weight slab z
//   and adds i*o_pr + j*o_pc to o_base.
// ---------------------------------------------------------------------------------------------
struct ConvArgs {
    const void *in = nullptr, *w = nullptr, *res = nullptr, *zero_page = nullptr;
    const float *bias = nullptr;   // [phases? no: shared][Npad] fp32
    void *out = nullptr;
    int B = 0, H = 0, W = 0, Cin = 0;
    int Ho = 0, Wo = 0, Cout = 0, Npad = 0;
    int kh = 1, kw = 1, stride = 1, pad = 0, dil = 1;
    int relu = 0, out_f32 = 0, phases = 1;
    int splitk = 1;                 // > 1: K is cut into slices over blockIdx.y (small-M layers); needs `partial`
    void *partial = nullptr;        // fp32 scratch of conv_splitk_bytes()
    long long o_bs = 0, o_rs = 0, o_cs = 0, o_base = 0, o_pr = 0, o_pc = 0;
    int dtype = TDRN_BF16;
    // patch kernel, first conv fused in (conv3x3_patch.hip FUSE): frames NCHW fp32, the first conv's folded weights [c][27] and bias
    const float *fuse_x = nullptr, *fuse_w = nullptr, *fuse_b = nullptr;
    int fuse_cout = 0;
    // ... or the frames as uint8 planes (B, 3, S, S) with the per-plane mean still to be subtracted (conv3x3_ws.hip only: tdrn_net_io.reserved[3])
    const unsigned char *fuse_x8 = nullptr;
    float fuse_mean[3] = {0.f, 0.f, 0.f};
    void *sk_ws = nullptr;          // conv3x3_pp.hip: scratch of conv_pp_sk_bytes() for the chained split (one launch at a time), or null
    bool sk_flags_zero = false;     // the first 1024 bytes of sk_ws are zero on entry (every launch leaves them zero): no memset node
    // kernel-choice switches of this launch: an OR of KOFF_* (above).  Same output bits either way.
    int kdisable = 0;
    // host-visible status words (pinned, device-mapped; tdrn_net_check): [0] <- 1 when a chained-split poll runs out,
    // [1] <- 1 when a poll of the chain launch does.  Null: a timed-out poll is not reported (dev harness only).
    unsigned *status = nullptr;
    int fault_handoff = 0;          // fault injection (tests): producers never raise their flag, the polls are short
};
// Which kernel runs a dense conv layer (conv_route.hip: the whole precedence, once).  Pure: it reads geometry, dtype, batch, kdisable, fuse_* and
// splitk, tests pointers for null only and makes no HIP call, so a plan can be asked without a GPU (TDRN_PLAN_DUMP).  pooled: MaxPool2d(2,2) of
// the output is wanted: CONV_WS / CONV_PATCH pool in their epilogue, CONV_IGEMM leaves it to launch_maxpool2.  CONV_NONE: a fused-first launch
// (fuse_x / fuse_x8) nobody takes: the caller runs the first conv on its own.  All but CONV_HEAD3X3 (another fp32 K order; geometry only)
// give the same output bits, so the choice may depend on the batch.
// (Measured on the resident training entries, DESIGN 22: that holds for a launch with one 64-channel chunk and no bias; with a bias, or
// with several chunks, the direct-conv kernels and conv_igemm.hip sum in different fp32 orders and differ by a rounding of the result in a
// few elements per ten thousand.  Do not rely on bit equality across routes beyond that without measuring it.)
enum ConvKernel { CONV_IGEMM, CONV_PATCH, CONV_PP, CONV_WS, CONV_HEAD3X3, CONV_PW1X1, CONV_NONE };
ConvKernel conv_route(const ConvArgs &a, bool pooled);
const char *conv_kernel_name(ConvKernel k);
// the kernel of conv_route(a, out_pool != null); out_pool: the MaxPool2d(2,2) output (a.out is then written on the CONV_IGEMM route only)
int launch_conv(const ConvArgs &a, hipStream_t s, void *out_pool = nullptr);
int conv_splitk_choice(const ConvArgs &a);          // 1 = no split (only layers that stay on conv_igemm.hip are split)
// One predicate per kernel file: X_takes(a, pooled) is all launch_X needs, item-count thresholds included; launch_X returns
// TDRN_E_UNSUPPORTED exactly where it is false.  Only conv_route.hip combines them.  conv_igemm.hip takes every layer:
int launch_conv_igemm(const ConvArgs &a, hipStream_t s);
int igemm_splitk_choice(const ConvArgs &a);         // K slices that fill the chip for a small-M layer
size_t conv_splitk_bytes(const ConvArgs &a, int splits);
// Several small dependent layers in ONE launch (conv_igemm.hip, conv_chain_kernel): layer i may depend on up to two EARLIER
// layers of the list (dep = index or -1); everything else a layer reads must be complete when the launch starts.  Every layer
// keeps its own splitk / partial slab.  `ctr`: conv_chain_ctr_bytes() of zeroed device words.  Output bits equal launch_conv's.
struct ChainLayer { ConvArgs a; int dep[2] = {-1, -1}; };
int conv_chain_supported(const ConvArgs &a);        // (the planner keeps conv3x3_patch / _pp layers out of a chain)
int conv_chain_max_layers();
size_t conv_chain_ctr_bytes();
int launch_conv_chain(const ChainLayer *layers, int n, unsigned *ctr, hipStream_t s, unsigned *status = nullptr);
// narrow 3x3/s1/p1 heads with fp32 output (<= 16 columns: the ARM loc heads at levels of >= 400 pixels), head3x3.hip
bool head3x3_takes(const ConvArgs &a, bool pooled);
int launch_head3x3(const ConvArgs &a, hipStream_t s);
// The layers of the 3x3/s1/p1 direct-conv kernels (conv3x3_patch / _pp / _ws) and their pixel tiles, from the geometry alone (no batch, no
// kdisable): 0 = not such a layer, 32 / 16 = 2-D tiles, -1 = flat tiles of 256 consecutive pixels (+ halo) in a patch buffer of `slots` 8-row pieces
inline int conv3x3_tile_mode(const ConvArgs &a, int slots)
{
    if (a.kh != 3 || a.kw != 3 || a.stride != 1 || a.pad != 1 || a.dil != 1 || a.phases != 1 || a.out_f32 || a.res) return 0;
    if (a.Ho != a.H || a.Wo != a.W || a.Npad % 64) return 0;
    if (a.o_rs != (long long)a.Wo * a.o_cs || a.o_bs != (long long)a.Ho * a.Wo * a.o_cs || a.o_base) return 0;
    if (a.W % 32 == 0 && a.H % 8 == 0) return 32;
    if (a.W % 16 == 0 && a.H % 16 == 0) return 16;
    return 2 * a.W + 2 + 256 <= slots * 8 ? -1 : 0;
}
// ... and their one limit that grows with the batch: 32-bit byte offsets into the input tensor (the fused-first instantiation never reads it)
inline bool conv3x3_input_fits(const ConvArgs &a) { return a.fuse_x || (long long)a.B * a.H * a.W * a.Cin * dtype_bytes(a.dtype) < (1ll << 32); }
// warp-specialised loader/consumer kernel (conv3x3_patch.hip): any such layer unless KOFF_CONV_PATCH; pooled (out_pool = fused MaxPool2d(2,2)
// output, a.out may then be null) with 2-D tiles only
bool patch_takes(const ConvArgs &a, bool pooled);
int launch_conv3x3_patch(const ConvArgs &a, void *out_pool, hipStream_t s);
// all-waves-compute ("ping-pong") kernel for the unpooled 16-bit Cin >= 256, Cout % 256 == 0 layers (conv3x3_pp.hip), from 192 items up
// (KOFF_CONV_PP: off).  pp_takes_geometry: the part of pp_takes that no batch changes (what a plan may depend on).
bool pp_takes_geometry(const ConvArgs &a);
bool pp_takes(const ConvArgs &a, bool pooled);
int launch_conv3x3_pp(const ConvArgs &a, hipStream_t s);
size_t conv_pp_sk_bytes();
// weight-stationary kernel for the POOLED 16-bit Cin == 64 layers (conv3x3_ws.hip: the whole weight tile resident in LDS, the activations in a
// ring of image rows, the first conv optionally computed by its producer waves from fp32 or uint8 frames), from 192 units up (KOFF_CONV_WS: off)
bool ws_takes(const ConvArgs &a, bool pooled);
int launch_conv3x3_ws(const ConvArgs &a, void *out_pool, hipStream_t s);   // out_pool only (a.out is not written)
// Item geometry of the persistent kernels (conv3x3_patch / _pp / _ws, dwpw_kernel, pw1x1_kernel).
// grid: one workgroup per CU, in a multiple of 8 (the item split is per XCD, mfma_prims.h xcd_items); surplus workgroups find no item and exit
inline int persistent_grid(int items) { return items >= 256 ? 256 : ((items + 7) / 8) * 8; }
// pixel tiles: tw = 32 / 16 (conv3x3_tile_mode): 2-D tiles of (px / tw) x tw pixels of one image; tw = 0: flat
// tiles of 256 consecutive NHW pixels
inline void conv_tiles(int B, int H, int W, int tw, int px, int &tiles_x, int &tiles_per_img, int &m_tiles)
{
    tiles_x = tw ? W / tw : 0;
    tiles_per_img = tw ? tiles_x * (H / (px / tw)) : 0;
    m_tiles = tw ? B * tiles_per_img : cdiv(B * H * W, 256);
}
// rows of the packed weight matrix must be padded to a multiple of this
int conv_n_pad(int cout);
// channels of every NHWC activation tensor are padded to a multiple of this
constexpr int kChanPad = 64;

// ---------------------------------------------------------------------------------------------
// HBM-bound layer kernels (layers.hip)
// ---------------------------------------------------------------------------------------------
// first conv: x NCHW fp32 [B][3][S][S] -> NHWC DT [B][Ho][Wo][Cpad], 3x3, pad 1, stride 1|2,
// folded BN + ReLU.  w: fp32 [Cout][27] (k = c*9 + r*3 + q), bias fp32 [Cout].
int launch_first_conv(const float *x, const float *w, const float *bias, void *out, int B, int S,
                      int stride, int Cout, int Cpad, int relu, int dtype, hipStream_t s);
// 2x2 stride-2 max pool, NHWC DT, optional ceil_mode
int launch_maxpool2(const void *in, void *out, int B, int H, int W, int C, int ceil_mode, int dtype,
                    hipStream_t s);
// L2Norm over channels: y = w[c] * (x / (sqrt(sum x^2) + 1e-10)), NHWC DT
int launch_l2norm(const void *in, const float *w, void *out, long long pixels, int C, int dtype,
                  hipStream_t s);
// depthwise 3x3, pad 1, stride 1|2, folded BN + ReLU, NHWC DT.  w: fp32 [9][Cpad], bias [Cpad]
// (KOFF_DW_SLIDE: the one-row strip kernel instead of the sliding-window one, KOFF_DW_STRIP_SMALL: the sliding-window one always -- same bits)
int launch_dwconv3(const void *in, const float *w, const float *bias, void *out, int B, int H, int W,
                   int C, int stride, int relu, int dtype, hipStream_t s, int kdisable = 0);
// conv_dw block fused (dwpw.hip): depthwise 3x3 (stride 1, pad 1, fp32 weights [9][Cin] + bias [Cin], ReLU) -> pointwise 1x1
// (DT weights [Npad][Cin], fp32 bias [Npad], ReLU) in one launch; the depthwise output stays in LDS.  16-bit types only.
struct DwPwArgs {
    const void *in = nullptr, *w = nullptr;
    const float *wdw = nullptr, *bdw = nullptr, *bias = nullptr;   // (bdw must lie behind wdw in the same allocation: the weight blob)
    void *out = nullptr;
    int B = 0, H = 0, W = 0, Cin = 0, Cout = 0, Npad = 0, Cs = 0;  // Cs: channel stride of the output tensor
    int stride = 1, relu_dw = 1, relu = 1, dtype = TDRN_BF16;
};
int dwpw_supported(const DwPwArgs &a);           // 0 = no, else the tile mode
int launch_dwpw(const DwPwArgs &a, hipStream_t s);
// wide 1x1 convs as a persistent 256 x 256-item GEMM (dwpw.hip pw1x1_kernel), from 192 items up (KOFF_PW1X1: off)
bool pw1x1_takes(const ConvArgs &a, bool pooled);
int launch_pw1x1(const ConvArgs &a, hipStream_t s);
// softmax over rows of (R, C) fp32, in place allowed
int launch_softmax_rows(const float *in, float *out, long long R, int C, hipStream_t s);
// 1x1 "offset" convs on the 12-channel ARM loc map: loc fp32 (pixel stride loc_ps, batch stride
// loc_bs, 12 ch) -> off NHWC fp32 [B*H*W][n_out], w fp32 [n_out][12], bias [n_out] (or null)
int launch_offset_conv(const float *loc, long long loc_bs, long long loc_ps, const float *w,
                       const float *bias, float *off, int B, int HW, int n_in, int n_out,
                       hipStream_t s);
// ... of up to four pyramid levels in one launch (n_in = 12); same arithmetic per output
struct OffsetProblem { const float *loc; long long loc_bs, loc_ps; const float *w, *bias; float *off; int B, HW, n_out, blk0; };
struct OffsetMulti { OffsetProblem pr[4]; int n; };
int launch_offset_conv_multi(const OffsetProblem *pr, int n, hipStream_t s);
// layout conversions for the API surfaces that are NCHW fp32
int launch_nchw_to_nhwc(const float *in, void *out, int B, int C, int HW, int Cpad, int dtype,
                        hipStream_t s);   // fp32 NCHW -> DT NHWC (channel-padded with zeros)
int launch_nchw_to_nhwc_grouped(const float *in, void *out, int B, int C, int HW, int G, int cpg_pad, int dtype,
                                hipStream_t s);
int launch_repack_oihw(const float *w, void *out, int Cout, int Npad, int Cin, int taps, int G, int cpg_pad, int dtype,
                       hipStream_t s);
int launch_nhwc_to_nchw_f32(const float *in, long long in_bs, long long in_ps, float *out, int B,
                            int C, int HW, hipStream_t s);   // fp32 "NHWC view" -> fp32 NCHW
// NHWC (channel stride Cpad, dtype DT or fp32) -> fp32 NCHW
int launch_nhwc_any_to_nchw_f32(const void *in, int dtype, int Cpad, float *out, int B, int C, int HW, hipStream_t s);
int launch_preprocess(const unsigned char *in, int B, int H0, int W0, int S, const float *mean_bgr, int to_rgb, float *out,
                      hipStream_t s);
int launch_preprocess_u8(const unsigned char *in, int B, int H0, int W0, int S, int to_rgb, unsigned char *out, hipStream_t s);   // resized uint8 planes
int launch_u8_planes_to_f32(const unsigned char *in, int B, int S, const float *mean, float *out, hipStream_t s);                // (B,3,S,S) u8 -> fp32 - mean[c]
int launch_fill_zero(void *p, size_t bytes, hipStream_t s);       // a kernel, not a memset node: keeps its place in a replayed hipGraph

// ---------------------------------------------------------------------------------------------
// Deformable-conv GEMM (deform.hip): up to two branches (3x3 + 5x5) sharing the input and summed.
//   in  : NHWC DT [B][H][W][Cin]
//   off : NHWC fp32 [B][Ho][Wo][off_stride], branch offsets at off + off_ch0 (G*2*k*k channels,
//         channel order of the reference: g, then 2*(i*kw+j)+{0:dh,1:dw})
//   w   : DT [Npad][taps][Cin]
//   out : fp32, element (pixel m, channel c) at out + m*o_ps + c (c < Cout)
// ---------------------------------------------------------------------------------------------
struct DeformBranch {
    const float *off = nullptr;
    int off_stride = 0;
    const void *w = nullptr;
    int kh = 3, kw = 3, pad = 1, stride = 1, dil = 1, G = 1;      // pad / stride / dil: the H axis
    int pad_w = -1, stride_w = -1, dil_w = -1;                     // W axis; < 0 (< 1): same as the H axis
    // key-frame broadcast (TRN clips): `off` holds off_rows pixel rows (the key frames' maps) and output pixel m of the launch reads row
    // (off_row0 + m) % off_rows; 0 = one row per output pixel
    int off_rows = 0, off_row0 = 0;
};
struct DeformArgs {
    const void *in = nullptr, *zero_page = nullptr;
    DeformBranch br[2];
    int n_branches = 1;
    int B = 0, H = 0, W = 0, Cin = 0, Ho = 0, Wo = 0, Cout = 0, Npad = 0;
    // two output segments so that loc and conf heads fused into one GEMM land in their own buffers:
    // channels [0,split) -> out0 (+ b*o0_bs + pix*o0_ps), [split,Cout) -> out1
    float *out0 = nullptr, *out1 = nullptr;
    int split = 0;
    long long o0_bs = 0, o0_ps = 0, o1_bs = 0, o1_ps = 0;
    int dtype = TDRN_BF16;
};
int launch_deform(const DeformArgs &a, hipStream_t s);
// up to 4 independent problems (same dtype / Npad) in one launch
// split_branches = 1: two-branch problems run as two work items that atomicAdd into PRE-ZEROED outputs
int launch_deform_multi(const DeformArgs *args, int n, hipStream_t s, int split_branches);
int deform_n_pad(int cout);
// Deformable-conv backward, fp32 (deform_bwd.hip).  The input and the grad_input accumulator are NHWC fp32 with every deformable
// group's channels padded to deform_bwd_cpg64() (a multiple of 64); grad_out and offsets are the caller's NCHW tensors.
struct DeformBwdGeom { int N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, G, Ho, Wo; };
int deform_bwd_cpg64(const DeformBwdGeom &g);
int deform_bwd_data_px(const DeformBwdGeom &g);       // output pixels per workgroup of the data kernel; 0 = unsupported shape
// gin_nhwc (zeroed by the caller) += col2im(W^T grad_out); goff (NCHW) = the offset gradient (stored once).  wr: launch_repack_oihw
// of the weight with Npad = Cout and cpg_pad = deform_bwd_cpg64 ([Cout][tap][Cpad] fp32)
int launch_deform_bwd_data(const DeformBwdGeom &g, const float *in_nhwc, const float *off, const float *gout, const float *wr,
                           float *gin_nhwc, float *goff, hipStream_t s);
int launch_deform_bwd_input_add(const DeformBwdGeom &g, const float *gin_nhwc, float *grad_input, hipStream_t s);   // NCHW +=
// split-K partial slabs of [splits][taps][Cout][Cpad] fp32, then grad_weight (OIHW) += scale * their fixed-order sum
void deform_bwd_weight_splits(const DeformBwdGeom &g, int &splits, int &per_split);
int launch_deform_bwd_weight(const DeformBwdGeom &g, const float *in_nhwc, const float *off, const float *gout, float *slab, float *grad_weight,
                             float scale, hipStream_t s);
// Transform-domain deformable conv with gradients, G = 1, 16-bit types (deform_ts.hip; tdrn_hip.h section i-l).  Y and Z are pixel-major
// over INPUT pixels, [N H W][deform_ts_cols] with column t * deform_ts_cp(Cout) + co and zero padding behind the last tap.
int deform_ts_cp(int Cout);                         // Cout rounded up to 8
int deform_ts_cols(const DeformBwdGeom &g);         // kh kw deform_ts_cp(Cout) rounded up to kChanPad
// OIHW fp32 -> DT: dgrad = 0: [Npad][Cin] with row t Cp + co (launch_conv's weight of Y); dgrad = 1: [Npad][cols] with row c (of grad_input)
int launch_deform_ts_repack(const DeformBwdGeom &g, const float *w, void *out, int Npad, int dgrad, int dtype, hipStream_t s);
// out_nhwc [N Ho Wo][Cout] fp32 = the blend of Y's corner rows; off: the caller's NCHW offsets
int launch_deform_ts_sample(const DeformBwdGeom &g, const void *y, const float *off, float *out_nhwc, int dtype, hipStream_t s);
// go_nhwc [N Ho Wo][Cout] fp32.  y and goff both or neither: goff (NCHW) is stored once.  z (or null; fp32, zeroed by the caller) += b gO
int launch_deform_ts_backward(const DeformBwdGeom &g, const void *y, const float *off, const float *go_nhwc, float *z, float *goff,
                              int dtype, hipStream_t s);
int launch_deform_ts_round(const float *in, void *out, long long elems, int dtype, hipStream_t s);      // fp32 -> DT; elems % 8 == 0
// grad_weight (OIHW, overwritten) = the sum in split order of the slabs [splits][cols][Cin] of launch_conv_wgrad_slabs
int launch_deform_ts_wgrad_reduce(const DeformBwdGeom &g, const float *slab, float *grad_weight, int splits, hipStream_t s);
// Dense stride-1 conv backward (conv_bwd.hip; tdrn_hip.h section i-c).  x_nhwc / go_nhwc: the input and grad_output as NHWC in the compute
// type, channels padded to conv_bwd_cpad (launch_nchw_to_nhwc).  Square kernels k = 1 | 3, one pad / dilation for both axes.
// stride (trailing, default 1: every positional initialiser keeps its meaning) steps the output pixel of the weight gradient: 2 for
// the strided family (conv_strided.hip; tdrn_hip.h section i-g), whose K = N*Ho*Wo is that of the strided output.
struct ConvBwdGeom { int N, Cin, H, W, Cout, k, pad, dil, Ho, Wo; int stride = 1; };
int conv_bwd_cpad(int c);
// K splits of the weight gradient, from the geometry alone (the result does not depend on the device's state)
void conv_wgrad_splits(const ConvBwdGeom &g, int &splits, int &per_split);
size_t conv_wgrad_slab_bytes(const ConvBwdGeom &g);     // the fp32 slabs [splits][taps][CoutPad][CinPad] + [splits][CoutPad]
// grad_weight (OIHW) += scale * sum_p go[p][co] x[p (+) tap][ci], grad_bias (or null) += scale * sum_p go[p][co]; fixed order, no atomics
int launch_conv_wgrad(const ConvBwdGeom &g, const void *x_nhwc, const void *go_nhwc, const void *zero_page, void *slab, float *grad_weight,
                      float *grad_bias, float scale, int dtype, hipStream_t s);
// ... its MFMA pass alone: the per-split sums land in `slab`; `splits` and the bias part of the slab ([splits][CoutPad]) are returned
// for the caller's own reduce (conv_transpose.hip)
int launch_conv_wgrad_slabs(const ConvBwdGeom &g, const void *x_nhwc, const void *go_nhwc, const void *zero_page, void *slab, int dtype,
                            hipStream_t s, int &splits, const float *&bias_slab);
// The reduce behind the three weight gradients (conv_bwd.hip slab_reduce_kernel): the fp32 slabs [split][row t * pitch + co][CiPad],
// `sstride` floats apart, are summed in split order into gw[co * d_co + ci * d_ci + t * d_t], co < Cout, ci < Cin, t < taps.
// accumulate: gw += scale * sum, else gw = sum and gw is never read (scale unused).  gb (or null) += scale * the sum over the splits
// (outer) and the bias_rows rows (inner) of bslab[split][z * pitch + co].
struct SlabReduce {
    int Cout = 0, Cin = 0, taps = 0;
    long long d_co = 0, d_ci = 0, d_t = 0;
    int pitch = 0, CiPad = 0;
    size_t sstride = 0;
    int bias_rows = 0;
    float scale = 1.f;
    bool accumulate = true;
};
int launch_slab_reduce(const SlabReduce &r, const float *slab, const float *bslab, float *gw, float *gb, int S, hipStream_t s);
// OIHW fp32 -> launch_conv's packing of the input-gradient conv: out[ci][taps-1-tap][co] = w[co][ci][tap] ([Npad][taps][conv_bwd_cpad(Cout)])
int launch_repack_oihw_dgrad(const float *w, void *out, int Cout, int Cin, int Npad, int taps, int dtype, hipStream_t s);
// ConvTranspose2d(k = 2, s = 2) with gradients (conv_transpose.hip; tdrn_hip.h section i-f).  z = 2i + j names the kernel tap (i, j) = the
// output phase; CoPad = conv_bwd_cpad(Cout).
// grad_output fp32 NCHW (N, Cout, 2H, 2W) -> its space-to-depth image, DT NHWC [N][H][W][z * CoPad + co], padded channels zero
int launch_nchw_to_nhwc_s2d(const float *in, void *out, int N, int Cout, int H, int W, int dtype, hipStream_t s);
// weight (Cin, Cout, 2, 2) fp32 -> launch_conv's phases = 4 packing out[z][co][ci] ([4][Npad][conv_bwd_cpad(Cin)]) ...
int launch_repack_iohw_phases(const float *w, void *out, int Cin, int Cout, int Npad, int dtype, hipStream_t s);
// ... and the packing of the input gradient, a 1x1 conv over the space-to-depth image: out[ci][z * CoPad + co] ([Npad][4 CoPad])
int launch_repack_iohw_dgrad(const float *w, void *out, int Cin, int Cout, int Npad, int dtype, hipStream_t s);
// grad_weight (Cin, Cout, 2, 2) += scale * sum_split slab[split][z * CoPad + co][ci], grad_bias (or null) += scale * sum_split sum_z
// bias_slab[split][z * CoPad + co]: the slabs of launch_conv_wgrad_slabs on ConvBwdGeom{N, Cin, H, W, 4 CoPad, 1, 0, 1, H, W}
int launch_convt_wgrad_reduce(const float *slab, const float *bias_slab, float *grad_weight, float *grad_bias, int Cin, int Cout, int splits,
                              float scale, hipStream_t s);
// Dense 3x3 stride-2 conv with gradients (conv_strided.hip; tdrn_hip.h section i-g).  The input gradient is a stride-1 conv over the
// zero-inserted image of grad_output: fp32 NCHW (N, Cout, Ho, Wo) -> DT NHWC D[n][r][c][CoPad] with Hd x Wd rows and columns
// (Hd = 2 Ho - 1 or 2 Ho, the caller's H + 2 pad - 2; Wd likewise), D[2 ho][2 wo] = go[ho][wo], every other element zero (odd rows and
// columns, padded channels).  The kernel writes EVERY element of D itself.
int launch_nchw_to_nhwc_dilate2(const float *in, void *out, int N, int Cout, int Ho, int Wo, int Hd, int Wd, int dtype, hipStream_t s);
// Depthwise 3x3 conv with gradients, pad 1, stride 1 | 2, fp32 NCHW throughout (dwconv_train.hip; tdrn_hip.h section i-h).  weight
// (C, 1, 3, 3); Ho x Wo is the caller's (H + 2 - 3) / stride + 1.  The weight gradient cuts K = N Ho Wo into `splits` ranges of per_split
// elements, from (N, C, Ho, Wo) alone; the workspace holds its partials [C][splits][10] (nine taps and the bias), padded to 256 bytes
void dwconv_wgrad_splits(int N, int C, int Ho, int Wo, int &splits, long long &per_split);
size_t dwconv_workspace_bytes(int N, int C, int Ho, int Wo);
// y is overwritten; bias (C) or null
int launch_dwconv_forward(const float *x, const float *w, const float *bias, float *y, int N, int C, int H, int W, int stride, int Ho, int Wo,
                          hipStream_t s);
// gx is overwritten, rows and columns that no output touches with 0
int launch_dwconv_backward_input(const float *go, const float *w, float *gx, int N, int C, int H, int W, int stride, int Ho, int Wo, hipStream_t s);
// gw += scale * its sums, gb (or null) += scale * sum go; merged in split order, no atomics
int launch_dwconv_backward_parameters(const float *x, const float *go, float *gw, float *gb, int N, int C, int H, int W, int stride, int Ho,
                                      int Wo, float scale, void *ws, hipStream_t s);
// BatchNorm2d with an optional fused ReLU, fp32 NCHW (batch_norm.hip; tdrn_hip.h section i-d).  Every pass cuts a channel's N*HW values
// into `splits` pieces of per_split elements, from (N, C, HW) alone; the workspace holds the per-(channel, split) records of the reducing
// passes and the backward's per-channel sums: 12 C splits + 8 C bytes
void batch_norm_splits(int N, int C, int HW, int &splits, int &per_split);
size_t batch_norm_workspace_bytes(int N, int C, int HW);
// training: batch statistics -> save_mean / save_invstd, the running buffers (or null) updated once; else they are read.  output is overwritten
int launch_batch_norm_forward(const float *input, const float *weight, const float *bias, float *running_mean, float *running_var,
                              float *output, float *save_mean, float *save_invstd, int N, int C, int HW, int training, float momentum,
                              float eps, int relu, void *ws, hipStream_t s);
// grad_input (or null) is overwritten; grad_weight / grad_bias (both or neither) += scale * their sums, merged in split order
int launch_batch_norm_backward(const float *input, const float *grad_output, const float *weight, const float *bias, const float *save_mean,
                               const float *save_invstd, float *grad_input, float *grad_weight, float *grad_bias, int N, int C, int HW,
                               int training, int relu, float scale, void *ws, hipStream_t s);
// ... its two per-channel finalize kernels for a caller with its own sweeps: the records [C][S][3] (count, mean, M2) in split order ->
// save_mean / save_invstd and the running buffers (training), or the running buffers read (eval); the records [C][S][2] -> sums[C][2] =
// (sum dy' / M, sum dy' xhat / M), grad_weight / grad_bias (both or neither) += scale * their sums.  Both merge in float64.
int launch_bn_stats_finalize(const float *rec, float *running_mean, float *running_var, float *save_mean, float *save_invstd, int C,
                             long long M, int S, int training, float momentum, float eps, hipStream_t s);
int launch_bn_bwd_finalize(const float *rec, float *sums, float *grad_weight, float *grad_bias, int C, long long M, int S, float scale,
                           hipStream_t s);
// BatchNorm2d with an optional fused ReLU on resident tensors: 16-bit NHWC activations [N HW][C], C % 64 == 0, 16-byte aligned; fp32
// parameters and statistics (batch_norm_nhwc.hip; tdrn_hip.h section i-k).  The semantics are those of the fp32 entries above; a
// workgroup owns 64 channels and one of `splits` ranges of per_split pixel rows, from (N, C, HW) alone; the workspace holds the same
// records: 12 C splits + 8 C bytes
void batch_norm_nhwc_splits(int N, int C, int HW, int &splits, int &per_split);
size_t batch_norm_nhwc_workspace_bytes(int N, int C, int HW);
int launch_batch_norm_nhwc_forward(const void *input, const float *weight, const float *bias, float *running_mean, float *running_var,
                                   void *output, float *save_mean, float *save_invstd, int N, int C, int HW, int training, float momentum,
                                   float eps, int relu, int dtype, void *ws, hipStream_t s);
int launch_batch_norm_nhwc_backward(const void *input, const void *grad_output, const float *weight, const float *bias,
                                    const float *save_mean, const float *save_invstd, void *grad_input, float *grad_weight,
                                    float *grad_bias, int N, int C, int HW, int training, int relu, float scale, int dtype, void *ws,
                                    hipStream_t s);
// Trainable MaxPool2d on resident tensors (pool_nhwc.hip; tdrn_hip.h section i-k): the geometries, selection rule and codes of the fp32
// NCHW kernels below, 16-bit NHWC tensors with C % 8 == 0 on 16-byte boundaries, codes [N][Ho][Wo][C] on any byte
int launch_max_pool_nhwc_forward(const void *input, void *output, unsigned char *code, int N, int C, int H, int W, int Ho, int Wo, int kernel,
                                 int dtype, hipStream_t s);
int launch_max_pool_nhwc_backward(const void *grad_output, const unsigned char *code, void *grad_input, int N, int C, int H, int W, int Ho,
                                  int Wo, int kernel, int dtype, hipStream_t s);
// Trainable MaxPool2d and L2Norm, fp32 NCHW (pool_l2norm.hip; tdrn_hip.h section i-e).  kernel = 2: 2x2 / 2 / 0 with a floor or ceil
// Ho x Wo; kernel = 3: 3x3 / 1 / 1 (Ho x Wo = H x W).  code (or null) gets one byte per output element, the selected slot dy * k + dx
int launch_max_pool_forward(const float *input, float *output, unsigned char *code, int planes, int H, int W, int Ho, int Wo, int kernel,
                            hipStream_t s);
// grad_input is written exactly once per element from grad_output and the codes; the input is not read
int launch_max_pool_backward(const float *grad_output, const unsigned char *code, float *grad_input, int planes, int H, int W, int Ho, int Wo,
                             int kernel, hipStream_t s);
// the [ceil(N HW / 64)][C] fp32 partial sums of grad_weight
size_t l2norm_workspace_bytes(int N, int C, int HW);
// norm (or null) = sqrt(sum_c x^2) + eps per pixel
int launch_l2norm_forward(const float *input, const float *weight, float *output, float *norm, int N, int C, int HW, float eps, hipStream_t s);
// grad_input (or null) is overwritten; grad_weight (or null; needs ws) += scale * its sum, merged in tile order
int launch_l2norm_backward(const float *input, const float *grad_output, const float *weight, const float *norm, float *grad_input,
                           float *grad_weight, int N, int C, int HW, float eps, float scale, void *ws, hipStream_t s);
// transform-then-sample path of the 16-bit one-group heads (deform.hip): the caller computes Y = 1x1 GEMM of the input with the
// per-tap weight slabs ([taps][80 columns] per pixel, deform_sample_cols(taps) channels), this launch blends the corners
int deform_sample_supported(const DeformArgs &a);      // 0 = no, else the number of taps of all branches
int deform_sample_cols(int taps);
// column of tap t's 80 outputs in the transform GEMM's output: three taps per 256-column slice (a slice of ygemm_k256 then holds
// whole taps only; columns 240..255 of every slice are zero padding)
constexpr int deform_y_col(int tap) { return (tap / 3) * 256 + (tap % 3) * 80; }
// the largest batch whose Y ([taps][B*H*W][80] tap-major or [B*H*W][ycs]) stays below the kernels' 32-bit byte offsets
int deform_ts_max_batch(int H, int W, int ycs, int taps);
int launch_deform_sample_multi(const DeformArgs *args, const void *const *y, const int *ycs, int n, hipStream_t s, int tap_major = 0);
// Y = X[M][256] * Wt[N][256]^T in the net dtype, weights held in registers (deform.hip); N % 256 == 0
int ygemm_supported(int Cin, int ycols, int dtype);
int launch_ygemm(const void *x, const void *w, void *y, long long M, int N, int ycs, int dtype, hipStream_t s, int taps = 0);   // taps > 0: Y tap-major [taps][M][80]
struct YGemmProblem { const void *x, *w; void *y; long long M; int N, ycs, taps; };
int launch_ygemm_multi(const YGemmProblem *pr, int n, int dtype, hipStream_t s, int kdisable = 0);      // up to 4 problems (pyramid levels) in one launch

// ---------------------------------------------------------------------------------------------
// Detect (detect.hip)
// ---------------------------------------------------------------------------------------------
int launch_decode(const float *loc, const float *priors, int P, float v0, float v1, float *out,
                  hipStream_t s);
int launch_center_size(const float *boxes, int P, float *out, hipStream_t s);
size_t detect_workspace_bytes(int B, int P, int C, int top_k);
int launch_detect(const float *loc, const float *conf, const float *priors, const float *arm_loc,
                  const float *scale4, int scale_on_device, int B, int P, int C, int top_k, float conf_thresh,
                  double nms_thresh, float *out, int32_t *counts, void *ws, size_t ws_bytes,
                  hipStream_t s);
size_t nms_workspace_bytes(int n);
size_t nms_classes_workspace_bytes(int n, int C);
// DetectOTA's association arithmetic (detect.hip): ROI features of kept boxes, similarity of detections to tubelets
int launch_roi_resample(const float *feat, int C, int H, int W, const int32_t *cells, int n, int S, float *out, hipStream_t s);
int launch_ota_similarity(const float *boxes, const float *roi, int n, int F, const float *rows, const int32_t *row_off, int m, float *best,
                          int32_t *arg, hipStream_t s);
int launch_nms_classes(const float *boxes, const float *scores, int n, int C, int first_class, float overlap, float min_score, int top_k,
                       int32_t *keep_out, int32_t *num_out, void *ws, size_t ws_bytes, hipStream_t s);
int launch_nms(const float *dets, int n, double thresh, int strict_gt, int presorted,
               int32_t *keep_out, int32_t *num_out, void *ws, size_t ws_bytes, hipStream_t s,
               int plain_rule = 0, float min_score = -INFINITY, int pre_top_k = 0);

// ---------------------------------------------------------------------------------------------
// MultiBoxLoss / RefineMultiBoxLoss, fp32 (loss.hip; semantics: tdrn_hip.h section ii-b)
// ---------------------------------------------------------------------------------------------
constexpr int kMaxMatchTruths = 512;     // truths per image staged in LDS by the match kernels
constexpr int kMaxLossClasses = 1024;
// truths [T_total][5] (x1,y1,x2,y2,label) of all images back to back, image b = rows [truth_off[b], truth_off[b+1]) (device);
// arm_loc == NULL: match (against point_form(priors)), else refine_match (against the ARM decode).  loc_t (B,P,4), conf_t (B,P).
size_t match_workspace_bytes(int B, int P, int max_truths);
int launch_match(const float *truths, const int32_t *truth_off, int T_total, int max_truths, int B, const float *priors, int P,
                 const float *arm_loc, float threshold, float var0, float var1, float *loc_t, int32_t *conf_t, void *ws,
                 size_t ws_bytes, hipStream_t s);
int launch_encode(const float *matched, const float *priors, int P, float v0, float v1, float *out, hipStream_t s);
// C = 0 in the query (conf == NULL in the launch): only_loc
size_t multibox_loss_workspace_bytes(int B, int P, int C);
int launch_multibox_loss_forward(const float *loc, const float *conf, const float *loc_t, const int32_t *conf_t, int B, int P,
                                 int C, int negpos_ratio, float *loss_out, uint8_t *sel, int32_t *num_pos, void *ws,
                                 size_t ws_bytes, hipStream_t s);
int launch_multibox_loss_backward(const float *loc, const float *conf, const float *loc_t, const int32_t *conf_t,
                                  const uint8_t *sel, const int32_t *num_pos, const float *grad_loss, int B, int P, int C,
                                  float *grad_loc, float *grad_conf, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// SGD, one fused multi-tensor step (sgd.hip; semantics: tdrn_hip.h section i-j)
// ---------------------------------------------------------------------------------------------
int launch_sgd_step(const tdrn_sgd_tensor *tensors, int n_tensors, const float *hyper_dev, int n_groups, int flags, hipStream_t s);
// dynamic loss scaling on top of it (sgd.hip; semantics: tdrn_hip.h section i-m)
int launch_amp_check_finite(const tdrn_sgd_tensor *tensors, int n_tensors, float *state_dev, hipStream_t s);
int launch_sgd_step_scaled(const tdrn_sgd_tensor *tensors, int n_tensors, const float *hyper_dev, int n_groups, const float *state_dev,
                           int flags, hipStream_t s);
int launch_amp_update(float *state_dev, float growth_factor, float backoff_factor, int growth_interval, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// SSDAugmentation on the device (augment.hip; semantics: tdrn_hip.h section ii-c)
// ---------------------------------------------------------------------------------------------
int launch_augment_sample(const int32_t *hw, const double *truths, const int32_t *truth_off, int T_total, int max_truths, int B,
                          uint64_t seed, const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                          tdrn_augment_params *params, float *out_truths, int32_t *out_off, hipStream_t s);
int launch_augment_apply(const tdrn_augment_image *images, const tdrn_augment_params *params, int B, const float *mean, int S,
                         int to_rgb, float *out, hipStream_t s);

// pairSSDAugmentation on the device: the same chain over two frames (augment.hip; semantics: tdrn_hip.h section ii-d)
int launch_augment_pair_sample(const int32_t *hw, const double *truths, const double *truths_t, const int32_t *truth_off,
                               int T_total, int max_truths, int B, double max_trans_ratio, uint64_t seed,
                               const int64_t *sample_ids, const double *tape, const int32_t *tape_off,
                               tdrn_augment_pair_params *params, float *out_truths, float *out_truths_t, int32_t *out_off,
                               hipStream_t s);
int launch_augment_pair_apply(const tdrn_augment_image *images, const tdrn_augment_image *images_t,
                              const tdrn_augment_pair_params *params, int B, const float *mean, int S, int to_rgb, float *out,
                              float *out_t, hipStream_t s);

}  // namespace tdrn
