// net_plan.hip -- host-side layer plan of the reference's model families: op constructors, the five families, Plan::build().
// No device allocation: the weight blob and the activation workspace are caller-owned (tdrn_hip.h).
//
//   model/dualrefinedet_vggbn.py:10-206      build_drn(false)
//   model/dualrefinedet_mobilenet.py:8-199   build_drn(true)
//   model/ssd4scale_mobile.py:9-140          build_ssd4scale(true)
//   model/refinedet_vgg.py:27-219            build_refinedet_vgg()
//   model/ssd4scale_vgg.py                   build_ssd4scale(false)
#include <algorithm>
#include <cstdlib>

#include "net_plan.h"

namespace tdrn {

// ---- plan building --------------------------------------------------------------------
int Plan::T(int C, int H, int W, bool f32)
{
    Tensor t;
    t.C = C; t.H = H; t.W = W; t.f32 = f32;
    t.Cpad = f32 ? C : (int)align_up((size_t)C, kChanPad);
    t.off = ws_per_sample;
    ws_per_sample += align_up((size_t)t.Cpad * H * W * (f32 ? 4 : es), 256);
    tensors.push_back(t);
    return (int)tensors.size() - 1;
}
void Plan::P_(const std::string &name, std::vector<int64_t> shape)
{
    param_index[name] = params.size();
    params.push_back(ParamSpec{name, std::move(shape)});
}
void Plan::bn_params(const std::string &bn, int C)
{
    P_(bn + ".weight", {C}); P_(bn + ".bias", {C}); P_(bn + ".running_mean", {C}); P_(bn + ".running_var", {C});
}
size_t Plan::blob(size_t bytes)
{
    const size_t o = blob_bytes;
    blob_bytes += align_up(bytes, 256);
    return o;
}

// first conv (Cin = 3), BN folded
int Plan::first_conv(const std::string &w, bool bias, const std::string &bn, int Cout, int stride, int S)
{
    const int So = (S + 2 - 3) / stride + 1;
    Op o; o.kind = OP_FIRST; o.stat = ST_FIRST;
    o.Cin = 3; o.Cout = Cout; o.stride = stride; o.relu = 1; o.hw = S;
    o.w = w; o.bn = bn;
    P_(w + ".weight", {Cout, 3, 3, 3});
    if (bias) { o.b = w; P_(w + ".bias", {Cout}); }
    if (!bn.empty()) bn_params(bn, Cout);
    o.out = T(Cout, So, So);
    o.w_off = blob((size_t)Cout * 27 * 4);
    o.b_off = blob((size_t)tensors[o.out].Cpad * 4);
    o.flops = 2.0 * So * So * Cout * 27;
    o.bytes = 3.0 * S * S * 4 + (double)So * So * tensors[o.out].Cpad * es;
    return push(o, w);
}

// dense conv -> NHWC tensor (out_kind == OUT_TENSOR) or fp32 head output view
int Plan::conv(int in, const std::string &w, bool bias, const std::string &bn, int Cout, int k, int stride, int pad, int dil,
         int relu, int res, int out_kind, int scale, const std::string &w2, int k2)
{
    const Tensor ti = tensors[in];
    Op o; o.kind = OP_CONV; o.stat = ST_CONV;
    o.in = in; o.res = res; o.Cin = ti.Cpad; o.Cout = Cout; o.k = k; o.stride = stride; o.pad = pad; o.dil = dil;
    o.relu = relu; o.out_kind = out_kind; o.scale = scale; o.w = w; o.bn = bn; o.w2 = w2; o.k2 = k2;
    const int Ho = (ti.H + 2 * pad - (dil * (k - 1) + 1)) / stride + 1;
    const int Wo = (ti.W + 2 * pad - (dil * (k - 1) + 1)) / stride + 1;
    P_(w + ".weight", {Cout, ti.C, k, k});
    if (bias) { o.b = w; P_(w + ".bias", {Cout}); }
    if (!bn.empty()) bn_params(bn, Cout);
    if (!w2.empty()) {   // a second, smaller conv merged into the same taps (refinedet multihead)
        P_(w2 + ".weight", {Cout, ti.C, k2, k2});
        if (bias) { o.b2 = w2; P_(w2 + ".bias", {Cout}); }
    }
    if (out_kind == OUT_TENSOR) {
        o.out = T(Cout, Ho, Wo);
        o.Cout = tensors[o.out].Cpad;            // pad channels are written as zeros
    }
    o.Npad = conv_n_pad(o.Cout);
    o.hw = Ho * 65536 + Wo;
    o.w_off = blob((size_t)o.Npad * k * k * o.Cin * es);
    o.b_off = blob((size_t)o.Npad * 4);
    o.flops = 2.0 * Ho * Wo * Cout * (double)k * k * ti.C;
    o.bytes = (double)ti.H * ti.W * ti.Cpad * es + (double)Ho * Wo * o.Cout * (out_kind == OUT_TENSOR ? es : 4) +
              (res >= 0 ? (double)Ho * Wo * o.Cout * es : 0.0);
    return push(o, w);
}

// ConvTranspose2d(k=2, s=2) + residual + ReLU as four phase GEMMs
int Plan::conv_transpose2(int in, const std::string &w, bool bias, int Cout, int res, int relu)
{
    const Tensor ti = tensors[in];
    Op o; o.kind = OP_CONV; o.stat = ST_CONV;
    o.in = in; o.res = res; o.Cin = ti.Cpad; o.k = 1; o.relu = relu; o.phases = 4; o.w = w;
    P_(w + ".weight", {ti.C, Cout, 2, 2});
    if (bias) { o.b = w; P_(w + ".bias", {Cout}); }
    o.out = T(Cout, ti.H * 2, ti.W * 2);
    o.Cout = tensors[o.out].Cpad;
    o.Npad = conv_n_pad(o.Cout);
    o.hw = ti.H * 65536 + ti.W;
    o.w_off = blob((size_t)4 * o.Npad * o.Cin * es);
    o.b_off = blob((size_t)o.Npad * 4);
    o.flops = 2.0 * 4 * ti.H * ti.W * (double)Cout * ti.C;
    o.bytes = (double)ti.H * ti.W * ti.Cpad * es + 2.0 * 4 * ti.H * ti.W * o.Cout * es;
    return push(o, w);
}

// MaxPool2d(2,2) right after a 3x3 conv whose full-resolution output nobody else reads: fused into
// the conv's epilogue when the warp-specialised kernel takes the layer with 2-D tiles.
bool Plan::can_fuse_pool(int in) const
{
    if (ops.empty()) return false;
    const Op &o = ops.back();
    if (o.kind != OP_CONV || o.out != in || o.out_kind != OUT_TENSOR || o.k != 3 || o.stride != 1 || o.pad != 1 ||
        o.dil != 1 || o.phases != 1 || o.res >= 0 || o.pool_t >= 0) return false;
    const Tensor &t = tensors[in];
    if ((t.H & 1) || (t.W & 1)) return false;
    return (t.W % 32 == 0 && t.H % 8 == 0) || (t.W % 16 == 0 && t.H % 16 == 0);
}
int Plan::pool(int in, int ceil_mode, bool in_needed_elsewhere)
{
    if (!in_needed_elsewhere && can_fuse_pool(in)) {
        const Tensor ti = tensors[in];
        const int out = T(ti.C, ti.H / 2, ti.W / 2);
        label(out, "pool:" + ti.label);
        ops.back().pool_t = out;
        tensors[in].label = "";                  // not materialised on the fused path
        ops.back().bytes += (double)(ti.H / 2) * (ti.W / 2) * ti.Cpad * es - (double)ti.H * ti.W * ti.Cpad * es;
        return out;
    }
    const Tensor ti = tensors[in];
    Op o; o.kind = OP_POOL; o.stat = ST_POOL; o.in = in; o.ceil = ceil_mode;
    const int Ho = ceil_mode ? (ti.H + 1) / 2 : ti.H / 2, Wo = ceil_mode ? (ti.W + 1) / 2 : ti.W / 2;
    o.out = T(ti.C, Ho, Wo);
    o.bytes = ((double)ti.H * ti.W + (double)Ho * Wo) * ti.Cpad * es;
    return push(o, "pool:" + ti.label);
}

int Plan::l2norm(int in, const std::string &name)
{
    const Tensor ti = tensors[in];
    Op o; o.kind = OP_L2NORM; o.stat = ST_L2; o.in = in; o.w = name;
    P_(name + ".weight", {ti.C});
    o.out = T(ti.C, ti.H, ti.W);
    o.w_off = blob((size_t)ti.Cpad * 4);
    o.bytes = 2.0 * ti.H * ti.W * ti.Cpad * es;
    return push(o, name);
}

int Plan::dwconv(int in, const std::string &w, const std::string &bn, int stride)
{
    const Tensor ti = tensors[in];
    Op o; o.kind = OP_DW; o.stat = ST_DW; o.in = in; o.stride = stride; o.relu = 1; o.w = w; o.bn = bn;
    P_(w + ".weight", {ti.C, 1, 3, 3});
    bn_params(bn, ti.C);
    const int Ho = (ti.H + 2 - 3) / stride + 1, Wo = (ti.W + 2 - 3) / stride + 1;
    o.out = T(ti.C, Ho, Wo);
    o.w_off = blob((size_t)9 * ti.Cpad * 4);
    o.b_off = blob((size_t)ti.Cpad * 4);
    o.flops = 2.0 * Ho * Wo * ti.C * 9;
    o.bytes = ((double)ti.H * ti.W + (double)Ho * Wo) * ti.Cpad * es;
    return push(o, w);
}
// conv_dw block, model/networks.py:736-745
int Plan::conv_dw(int in, const std::string &name, int Cout, int stride)
{
    const int d = dwconv(in, name + ".0", name + ".1", stride);
    return conv(d, name + ".3", false, name + ".4", Cout, 1, 1, 0, 1, 1);
}

// 1x1 offset convs on the 12-channel loc map of pyramid level `scale`
int Plan::offset_conv(int scale, int H, int W, const std::string &w1, const std::string &w2, bool bias, int n1, int n2,
                int loc_src, int ref_tensor)
{
    Op o; o.kind = OP_OFFSET; o.stat = ST_OFFSET; o.scale = scale; o.hw = H * W; o.w = w1; o.w2 = w2;
    o.loc_src = loc_src; o.in = ref_tensor;
    P_(w1 + ".weight", {n1, 12, 1, 1});
    if (bias) { o.b = w1; P_(w1 + ".bias", {n1}); }
    if (!w2.empty()) {
        P_(w2 + ".weight", {n2, 12, 1, 1});
        if (bias) { o.b2 = w2; P_(w2 + ".bias", {n2}); }
    } else {
        n2 = 0;
    }
    o.off_n = n1 + n2; o.off_c0[0] = 0; o.off_c0[1] = n1;
    o.out = T(o.off_n, H, W, true);
    o.w_off = blob((size_t)o.off_n * 12 * 4);
    o.b_off = blob((size_t)o.off_n * 4);
    o.flops = 2.0 * H * W * o.off_n * 12;
    o.bytes = (double)H * W * (12 + o.off_n) * 4;
    return push(o, w1);
}

// fused deformable heads of one pyramid level: [loc ; conf] rows, 1 or 2 branches
void Plan::deform_heads(int in, int off_t, int scale, int G, const std::string &loc1, const std::string &conf1,
                  const std::string &loc2, const std::string &conf2, int off_c1, int out_loc_kind)
{
    const Tensor ti = tensors[in];
    const int nc3 = 3 * cfg.num_classes;
    // shape_check, deform_conv_cuda.c:75-76 "input image is smaller than kernel": the reference throws when a
    // 5x5 multihead branch meets the 3x3 map of a 192-pixel frame
    const int kmax = loc2.empty() ? 3 : 5;
    if (ti.H < kmax || ti.W < kmax) plan_error = TDRN_E_SHAPE;
    Op o; o.kind = OP_DEFORM; o.stat = ST_DEFORM; o.in = in; o.off_t = off_t; o.scale = scale; o.G = G;
    o.Cin = ti.Cpad; o.Cout = 12 + nc3; o.Npad = deform_n_pad(o.Cout);
    o.k = 3; o.pad = 1; o.w = loc1; o.b = conf1; o.out_kind = out_loc_kind;
    P_(loc1 + ".weight", {12, ti.C, 3, 3});
    P_(conf1 + ".weight", {nc3, ti.C, 3, 3});
    o.w_off = blob((size_t)o.Npad * 9 * o.Cin * es);
    o.off_c0[0] = 0;
    o.taps = 9;
    if (!loc2.empty()) {
        o.n_branches = 2; o.k2 = 5; o.pad2 = 2; o.w2 = loc2; o.b2 = conf2; o.off_c0[1] = off_c1;
        P_(loc2 + ".weight", {12, ti.C, 5, 5});
        P_(conf2 + ".weight", {nc3, ti.C, 5, 5});
        o.w2_off = blob((size_t)o.Npad * 25 * o.Cin * es);
        o.taps += 25;
    }
    o.split = o.n_branches == 2 ? 1 : ((G >= 2 && G % 2 == 0) ? 2 : 0);
    o.hw = ti.H * 65536 + ti.W;
    o.flops = 2.0 * ti.H * ti.W * o.Cout * (double)o.taps * ti.C;
    o.bytes = (double)ti.H * ti.W * (ti.Cpad * es + (o.Cout + 2 * o.taps * G) * 4);
    // 16-bit plans, one deformable group: transform (1x1 GEMM into per-tap partial outputs), then sample (deform.hip);
    // TDRN_PLAN_NO_DEFORM_TS keeps the fused gather kernel
    if (!(cfg.plan_flags & TDRN_PLAN_NO_DEFORM_TS) && cfg.dtype != TDRN_F32 && G == 1 && o.taps <= 34) {
        o.y_groups = (o.Cout + 79) / 80;
        o.y_cols = deform_sample_cols(o.taps);
        o.y_t = T(o.y_cols * o.y_groups, ti.H, ti.W);
        o.wt_off = blob((size_t)o.y_groups * o.y_cols * o.Cin * es);
        o.bt_off = blob((size_t)o.y_groups * o.y_cols * 4);
    }
    push(o);
}

void Plan::softmax_op()
{
    Op o; o.kind = OP_SOFTMAX; o.stat = ST_SOFTMAX;
    o.bytes = 2.0 * P * cfg.num_classes * 4;
    push(o);
}
void Plan::offsets_out(int scale, int off_t, int n) { Op o; o.kind = OP_OFF_OUT; o.stat = ST_LAYOUT; o.scale = scale; o.in = off_t; o.Cout = n; push(o); }
void Plan::loc_maps_out(int scale) { Op o; o.kind = OP_LOC_OUT; o.stat = ST_LAYOUT; o.scale = scale; push(o); }
int Plan::ref_loc_in(int scale, int H, int W)
{
    Op o; o.kind = OP_REFLOC_IN; o.stat = ST_LAYOUT; o.scale = scale; o.hw = H * W;
    o.out = T(12, H, W, true);
    push(o);
    return o.out;
}

void Plan::set_pyramid(int s0)
{
    fm[0] = s0; fm[1] = s0 / 2; fm[2] = s0 / 4; fm[3] = s0 / 8;
    scale_off[0] = 0;
    for (int i = 0; i < 4; ++i) scale_off[i + 1] = scale_off[i] + fm[i] * fm[i] * 3;
    P = scale_off[4];
}

// ---- model families ---------------------------------------------------------------------
// VGG16 trunk (model/networks.py:136-163).  Returns conv4_3, conv5_3, fc7 tensors (post-ReLU).
void Plan::vgg_trunk(int S, bool bn, int c7, int &c43, int &c53, int &fc7)
{
    static const int cfgv[] = {64, 64, -1, 128, 128, -1, 256, 256, 256, -2, 512, 512, 512, -1, 512, 512, 512};
    int idx = 0, x = -1, nconv = 0;
    for (int v : cfgv) {
        if (v < 0) {
            x = pool(x, v == -2, nconv == 10 || nconv == 13);
            idx += 1;
            continue;
        }
        const std::string name = "backbone." + std::to_string(idx);
        const std::string bnn = bn ? "backbone." + std::to_string(idx + 1) : "";
        if (x < 0) x = first_conv(name, true, bnn, v, 1, S);
        else x = conv(x, name, true, bnn, v, 3, 1, 1, 1, 1);
        idx += bn ? 3 : 2;
        ++nconv;
        if (nconv == 10) c43 = x;
        if (nconv == 13) { c53 = x; t_late = x; }
    }
    x = pool(x, 0, true);   // pool5_ds (conv5_3 also feeds L2Norm_5_3)
    idx += 1;
    x = conv(x, "backbone." + std::to_string(idx), true, bn ? "backbone." + std::to_string(idx + 1) : "", 1024, 3, 1, 6, 6, 1);
    idx += bn ? 3 : 2;
    fc7 = conv(x, "backbone." + std::to_string(idx), true, bn ? "backbone." + std::to_string(idx + 1) : "", c7, 1, 1, 0, 1, 1);
}

// TCB / FPN (dualrefinedet_vggbn.py:30-34,97-114,166-178).  Returns the 4 ODM sources.
void Plan::tcb(const int src[4], bool bias, int odm[4])
{
    int x = conv(src[3], "last_layer_trans.0", bias, "", 256, 3, 1, 1, 1, 1);
    ops.back().chain_tag = true;
    x = conv(x, "last_layer_trans.2", bias, "", 256, 3, 1, 1, 1, 0);
    ops.back().chain_tag = true;
    x = conv(x, "last_layer_trans.3", bias, "", 256, 3, 1, 1, 1, 0);
    ops.back().chain_tag = true;
    odm[3] = x;
    int t[3];
    for (int s = 0; s < 3; ++s) {
        cur_lane = s == 0 ? 1 : 2;      // lateral branches are independent of the top-down chain
        const std::string n = "trans_layers." + std::to_string(s);
        const int a = conv(src[s], n + ".0", bias, "", 256, 3, 1, 1, 1, 1);
        ops.back().chain_tag = s == 2;
        t[s] = conv(a, n + ".2", bias, "", 256, 3, 1, 1, 1, 0);
        ops.back().chain_tag = s == 2;
    }
    cur_lane = 0;
    for (int i = 0; i < 3; ++i) {
        const int lvl = 2 - i;
        const int u = conv_transpose2(x, "up_layers." + std::to_string(i), bias, 256, t[lvl], 1);
        ops.back().chain_tag = i == 0;
        x = conv(u, "latent_layers." + std::to_string(i), bias, "", 256, 3, 1, 1, 1, 1);
        ops.back().chain_tag = i == 0;
        odm[lvl] = x;
    }
}

void Plan::drn_heads(const int src[4], const int odm[4], bool bias)
{
    int off_t[4];
    cur_lane = 3;                       // ARM heads + offset convs: off the critical path
    // the four ARM loc heads first, then the four offset convs back to back: consecutive OP_OFFSET ops of a lane run as ONE
    // launch (round 6: each was a 16-25 us launch of its own between two heads; same arithmetic per output)
    for (int s = 0; s < 4; ++s) conv(src[s], "arm_loc." + std::to_string(s), bias, "", 12, 3, 1, 1, 1, 0, -1, OUT_ARM_LOC, s);
    for (int s = 0; s < 4; ++s) {
        const std::string ss = std::to_string(s);
        off_t[s] = offset_conv(s, fm[s], fm[s], "offset." + ss, cfg.multihead ? "offset2." + ss : "", bias,
                               cfg.def_groups * 18, cfg.def_groups * 50, OUT_ARM_LOC);
    }
    for (int s = 0; s < 4; ++s) offsets_out(s, off_t[s], cfg.def_groups * 18);
    cur_lane = 0;
    for (int s = 0; s < 4; ++s) {
        const std::string ss = std::to_string(s);
        deform_heads(odm[s], off_t[s], s, cfg.def_groups, "odm_loc." + ss, "odm_conf." + ss,
                     cfg.multihead ? "odm_loc_2." + ss : "", cfg.multihead ? "odm_conf_2." + ss : "",
                     cfg.def_groups * 18, OUT_ODM_LOC);
    }
    if (cfg.test_phase) softmax_op();
}

// the two DRN families: the VGG one has biases on the TCB and head convs, the MobileNet one has none
int Plan::build_drn(bool mobile)
{
    set_pyramid(cfg.size / 8);
    int src[4], odm[4];
    if (mobile) mobilenet_sources(cfg.size, 1024, true, src);
    else vgg_sources(src);
    tcb(src, !mobile, odm);
    drn_heads(src, odm, !mobile);
    return TDRN_OK;
}

// the four ARM sources of the VGG variants: L2Norm of conv4_3 / conv5_3, fc7 and the extras
// (dualrefinedet_vggbn.py:36-45, refinedet_vgg.py:47-56, ssd4scale_vgg.py:25-34)
void Plan::vgg_sources(int src[4])
{
    int c43, c53, fc7;
    vgg_trunk(cfg.size, cfg.bn != 0, cfg.c7_channel, c43, c53, fc7);
    src[0] = l2norm(c43, "L2Norm_4_3");
    src[1] = l2norm(c53, "L2Norm_5_3");
    src[2] = fc7;
    const int e = cfg.bn ? conv(fc7, "extras.0", true, "extras.1", 256, 1, 1, 0, 1, 1) : conv(fc7, "extras.0", true, "", 256, 1, 1, 0, 1, 1);
    ops.back().chain_tag = true;
    const int x = cfg.bn ? conv(e, "extras.3", true, "extras.4", 512, 3, 2, 1, 1, 1) : conv(e, "extras.2", true, "", 512, 3, 2, 1, 1, 1);
    ops.back().chain_tag = true;
    src[3] = x;
}

// RefineDet-VGG: same trunk / TCB, plain (non-deformable) ODM heads (model/refinedet_vgg.py:27-219).
// multihead sums a 3x3 and a 5x5 conv of the same input (:179-182): packed as ONE 5x5 conv whose
// centre taps carry the 3x3 weights (biases added).
int Plan::build_refinedet_vgg()
{
    set_pyramid(cfg.size / 8);
    int src[4], odm[4];
    vgg_sources(src);
    if (cfg.use_refine) {
        cur_lane = 3;
        for (int s = 0; s < 4; ++s) conv(src[s], "arm_loc." + std::to_string(s), true, "", 12, 3, 1, 1, 1, 0, -1, OUT_ARM_LOC, s);
        cur_lane = 0;
    }
    tcb(src, true, odm);
    const int nc3 = 3 * cfg.num_classes;
    for (int s = 0; s < 4; ++s) {
        const std::string ss = std::to_string(s);
        if (cfg.multihead) {
            conv(odm[s], "odm_loc_2." + ss, true, "", 12, 5, 1, 2, 1, 0, -1, OUT_ODM_LOC, s, "odm_loc." + ss, 3);
            conv(odm[s], "odm_conf_2." + ss, true, "", nc3, 5, 1, 2, 1, 0, -1, OUT_CONF, s, "odm_conf." + ss, 3);
        } else {
            conv(odm[s], "odm_loc." + ss, true, "", 12, 3, 1, 1, 1, 0, -1, OUT_ODM_LOC, s);
            conv(odm[s], "odm_conf." + ss, true, "", nc3, 3, 1, 1, 1, 0, -1, OUT_CONF, s);
        }
    }
    if (cfg.test_phase) softmax_op();
    return TDRN_OK;
}

// MobileNet-v1 trunk shared by dualrefinedet_mobilenet.py:19-48 and ssd4scale_mobile.py:20-50, and its four ARM sources
void Plan::mobilenet_sources(int S, int c7, bool extras_bias, int src[4])
{
    static const int couts[] = {64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 0};
    static const int strides[] = {1, 2, 1, 1, 1, 2, 1, 1, 1, 1, 1, 2, 1};
    int x = first_conv("backbone.0.0", false, "backbone.0.1", 32, 2, S);
    for (int i = 0; i < 13; ++i) {
        x = conv_dw(x, "backbone." + std::to_string(i + 1), i == 12 ? c7 : couts[i], strides[i]);
        if (i + 1 == 11) src[0] = x;
    }
    src[1] = x;
    for (int k = 0; k < 2; ++k) {
        const std::string n = "extras." + std::to_string(k);
        x = conv(x, n + ".0", extras_bias, n + ".1", 256, 1, 1, 0, 1, 1);
        x = conv_dw(x, n + ".3", 512, 2);
        src[2 + k] = x;
    }
    src[0] = l2norm(src[0], "L2Norm_4_3");
    src[1] = l2norm(src[1], "L2Norm_5_3");
}

int Plan::build_ssd4scale(bool mobile)
{
    set_pyramid(cfg.size / 8);
    int src[4];
    if (mobile) mobilenet_sources(cfg.size, cfg.c7_channel, true, src);
    else vgg_sources(src);
    const int nc3 = 3 * cfg.num_classes;
    if (cfg.deform) {
        // all four levels' offsets first, then the four deformable heads back to back: consecutive OP_DEFORM ops run as ONE
        // launch (the gather kernel is latency-bound per workgroup -- 72 dependent K steps with 8 groups -- so four launches
        // cost four times the one: 4 x 230-330 us -> 330 us at config #5's batch, profiles/r04_cfg5)
        int ot[4], rl[4];
        for (int s = 0; s < 4; ++s) rl[s] = ref_loc_in(s, fm[s], fm[s]);
        for (int s = 0; s < 4; ++s) ot[s] = offset_conv(s, fm[s], fm[s], "offset." + std::to_string(s), "", true, 8 * 18, 0, -1, rl[s]);     // (one launch)
        for (int s = 0; s < 4; ++s) offsets_out(s, ot[s], 8 * 18);
        for (int s = 0; s < 4; ++s) {
            const std::string ss = std::to_string(s);
            deform_heads(src[s], ot[s], s, 8, "arm_loc." + ss, "arm_conf." + ss, "", "", 0, OUT_ARM_LOC);
        }
    }
    for (int s = 0; s < 4 && !cfg.deform; ++s) {
        const std::string ss = std::to_string(s);
        conv(src[s], "arm_loc." + ss, true, "", 12, 3, 1, 1, 1, 0, -1, OUT_ARM_LOC, s);
        conv(src[s], "arm_conf." + ss, true, "", nc3, 3, 1, 1, 1, 0, -1, OUT_CONF, s);
        loc_maps_out(s);
    }
    if (cfg.test_phase) softmax_op();
    return TDRN_OK;
}

// ---- build(): helpers and passes ------------------------------------------------------------------
int Plan::producer_of(int t) const
{
    int prod = -1;
    for (size_t j = 0; j < ops.size(); ++j)
        if (ops[j].out == t || ops[j].pool_t == t) prod = (int)j;
    return prod;
}

int Plan::readers_of(int t) const
{
    int readers = 0;
    for (const Op &o : ops) readers += (o.in == t) + (o.res == t);
    return readers;
}

void Plan::conv_geometry(const Op &o, int B, ConvArgs &a) const
{
    const Tensor &ti = tensors[o.in];
    a.B = B; a.H = ti.H; a.W = ti.W; a.Cin = o.Cin; a.Ho = o.hw >> 16; a.Wo = o.hw & 0xffff;
    a.Cout = o.Cout; a.Npad = o.Npad; a.kh = a.kw = o.k; a.stride = o.stride; a.pad = o.pad; a.dil = o.dil;
    a.phases = o.phases; a.dtype = cfg.dtype;
    a.kdisable = kdisable;
}

// ... plus what else conv_route reads, for a question asked while planning (no buffers yet: pointers are null or a non-null mark)
ConvArgs Plan::conv_question(const Op &o, int B) const
{
    static const float mark = 0.f;
    ConvArgs a;
    conv_geometry(o, B, a);
    a.relu = o.relu;
    a.out_f32 = o.out_kind != OUT_TENSOR;
    a.o_cs = o.out_kind == OUT_TENSOR ? tensors[o.out].Cpad : 0;
    a.o_rs = (long long)a.Wo * a.o_cs; a.o_bs = (long long)a.Ho * a.Wo * a.o_cs;
    a.res = o.res >= 0 ? &mark : nullptr;
    a.splitk = o.splitk;
    a.partial = o.splitk > 1 ? (void *)&mark : nullptr;
    if (fuse_first >= 0 && &o == &ops[fuse_first]) { a.fuse_x = &mark; a.fuse_cout = ops[0].Cout; }
    return a;
}

// The fp32 (3, S, S) copy of uint8 frames (plans whose first conv reads fp32: every one but the conv3x3_ws route) costs no
// workspace and no tensor index of a layer: it is appended LAST and ALIASED with the first layer output behind the second op
// that is large enough -- that tensor is dead while ops 0 / 1, the only readers of the copy, run (the engine's forwards are
// stream-ordered, a second step in flight has its own workspace).  Round-5 advisor finding: 1.2-3 MB per frame and engine
// clone were allocated in front of every other tensor for a fallback most callers never take.
void Plan::alias_u8_input()
{
    if (ops.empty() || ops[0].kind != OP_FIRST) return;
    const size_t need = align_up((size_t)3 * cfg.size * cfg.size * 4, 256);
    auto touched_early = [&](int t) {
        for (size_t i = 0; i < 2 && i < ops.size(); ++i)
            if (ops[i].in == t || ops[i].out == t || ops[i].res == t || ops[i].pool_t == t || ops[i].off_t == t) return true;
        return false;
    };
    int victim = -1;
    for (size_t i = 2; i < ops.size() && victim < 0; ++i) {
        // (a main-lane layer of the trunk: it runs behind ops 0 / 1 in stream order; an op that does not depend on the trunk --
        // the TRN nets' ref_loc conversions on a side lane -- could otherwise write its output while the copy is still being read)
        if (ops[i].lane != 0 || !(ops[i].kind == OP_CONV || ops[i].kind == OP_DW || ops[i].kind == OP_POOL) || ops[i].in < 0) continue;
        for (int t : {ops[i].out, ops[i].pool_t}) {
            if (t < 0 || victim >= 0 || touched_early(t)) continue;
            const Tensor &v = tensors[t];
            if (align_up((size_t)v.Cpad * v.H * v.W * (v.f32 ? 4 : es), 256) >= need) victim = t;
        }
    }
    if (victim >= 0) {
        Tensor t;
        t.C = 3; t.H = cfg.size; t.W = cfg.size; t.f32 = true; t.Cpad = 3; t.off = tensors[victim].off;
        tensors.push_back(t);
        x_t = (int)tensors.size() - 1;
    } else {
        x_t = T(3, cfg.size, cfg.size, true);
    }
}

// L2Norm of conv4_3 / conv5_3 right behind its producer and on a side lane: it is HBM-bound and needs no
// LDS, so it runs under the next (LDS-filling) conv of the trunk, and the lateral TCB convs and ARM heads
// that read it can start while conv5 / fc6 / fc7 -- which leave CUs idle -- are still running, instead of
// queueing behind fc7 on the main lane.
void Plan::hoist_l2norm_to_side_lanes()
{
    int side = 1;
    for (size_t i = 0; i < ops.size(); ++i) {
        if (ops[i].kind != OP_L2NORM) continue;
        const int prod = producer_of(ops[i].in);
        if (prod < 0) continue;
        Op o = ops[i];
        o.lane = side;
        side = side == 1 ? 2 : 1;
        ops.erase(ops.begin() + (long)i);
        ops.insert(ops.begin() + prod + 1, o);
    }
}

// first conv fused into the loader of the conv behind it (conv3x3_patch.hip FUSE; conv3x3_ws.hip at the batches it takes): where
// patch_takes says so for the fused launch, and nobody else reads the first conv's output (TDRN_PLAN_NO_FUSE_FIRST keeps the two launches)
void Plan::plan_fuse_first()
{
    fuse_first = -1;
    if ((cfg.plan_flags & TDRN_PLAN_NO_FUSE_FIRST) || ops.size() <= 1 || ops[0].kind != OP_FIRST || ops[1].kind != OP_CONV || ops[0].stride != 1 ||
        tensors[ops[0].out].Cpad != 64) return;
    const Op &c = ops[1];
    const Tensor &ti = tensors[ops[0].out];
    fuse_first = 1;                          // (the fused launch never reads the layer's input tensor: no limit of it grows with the batch)
    if (c.in != ops[0].out || readers_of(ops[0].out) != 1 || c.out_kind != OUT_TENSOR || c.lane != 0 || ti.H != ti.W ||
        !patch_takes(conv_question(c, 0), c.pool_t >= 0)) fuse_first = -1;
    if (fuse_first >= 0) {                   // the fused launch carries both layers' algorithmic work
        ops[1].flops += ops[0].flops;
        ops[1].bytes += 3.0 * ops[0].hw * ops[0].hw * 4 - (double)ti.H * ti.W * ti.Cpad * es;
        ops[0].flops = 0; ops[0].bytes = 0;
    }
}

// split-K per layer from its geometry only (at a fixed reference batch: the benchmark's), so that a frame's arithmetic never
// depends on the batch it travels in; the partial slabs live in a per-lane region of the workspace
void Plan::plan_splitk()
{
    for (Op &o : ops) {
        if (o.kind == OP_CONV && o.pool_t >= 0) o.stat = ST_CONV3;
        if (o.kind != OP_CONV || o.pool_t >= 0) continue;
        ConvArgs a;
        conv_geometry(o, kPlanRefBatch, a);
        a.out_f32 = o.out_kind != OUT_TENSOR;
        o.splitk = conv_splitk_choice(a);    // (asked of the bare geometry, as ever: a residual layer of the patch kernels' shape is not split either)
        a = conv_question(o, kPlanRefBatch);
        const ConvKernel k = conv_route(a, false);
        const bool direct = k == CONV_PATCH || k == CONV_PP;
        if (direct) o.stat = ST_CONV3;
        if (o.chain_tag && !(o.out_kind == OUT_TENSOR && !direct && conv_chain_supported(a))) o.chain_tag = false;
    }
}

// The chain launch: tagged layers whose inputs are chain members or exist before the first member starts (a layer
// the patch kernels take at this frame size, and everything behind it, stays an ordinary launch).  Members move to
// the main lane and get their own split-K slabs (stages overlap inside the launch).
void Plan::plan_chain()
{
    chain_ops.clear();
    const bool chain_on = (cfg.plan_flags & TDRN_PLAN_CHAIN) != 0;   // opt-in: it lost (conv_igemm.hip)
    int first = -1;
    for (size_t i = 0; i < ops.size() && chain_on; ++i) {
        Op &o = ops[i];
        if (o.kind != OP_CONV || !o.chain_tag || (int)chain_ops.size() == conv_chain_max_layers()) continue;
        bool ok = true;
        for (int t : {o.in, o.res}) {
            if (t < 0) continue;
            const int prod = producer_of(t);
            const bool member = prod >= 0 && ops[prod].chain >= 0;
            if (!member && first >= 0 && prod > first) ok = false;
        }
        if (!ok) continue;
        if (first < 0) first = (int)i;
        o.chain = (int)chain_ops.size();
        chain_ops.push_back((int)i);
    }
    if (chain_ops.size() < 3) {              // not worth a queue
        for (int i : chain_ops) ops[i].chain = -1;
        chain_ops.clear();
    }
    // Queue order = dependency level (a stage's tasks wait only for EARLIER stages), ties in plan order: the
    // independent lateral convs of the level below then sit between the stages of the serial chain and fill the
    // workgroups that would otherwise spin on the chain's next dependency.
    std::vector<int> level(ops.size(), 0);   // by op index
    for (size_t k = 0; k < chain_ops.size(); ++k)
        for (int t : {ops[chain_ops[k]].in, ops[chain_ops[k]].res})
            for (size_t j = 0; j < k; ++j)
                if (t >= 0 && ops[chain_ops[j]].out == t && level[chain_ops[j]] + 1 > level[chain_ops[k]]) level[chain_ops[k]] = level[chain_ops[j]] + 1;
    std::stable_sort(chain_ops.begin(), chain_ops.end(), [&](int a, int b) { return level[a] < level[b]; });
    for (size_t k = 0; k < chain_ops.size(); ++k) ops[chain_ops[k]].chain = (int)k;
}

void Plan::place_splitk_slabs()
{
    size_t lane_bytes[kLanes] = {0, 0, 0, 0};
    size_t chain_bytes = 0;
    for (Op &o : ops) {
        if (o.kind != OP_CONV || o.pool_t >= 0 || o.splitk <= 1) continue;
        const size_t per_sample = align_up((size_t)o.splitk * o.phases * (o.hw >> 16) * (o.hw & 0xffff) * o.Npad * sizeof(float), 256);
        if (o.chain >= 0) {
            o.chain_partial = chain_bytes;
            chain_bytes += per_sample;
        } else if (per_sample > lane_bytes[o.lane]) {
            lane_bytes[o.lane] = per_sample;
        }
    }
    for (int i : chain_ops) ops[i].lane = 0;
    chain_partial_off = ws_per_sample;
    ws_per_sample += chain_bytes;
    if (const char *pd = getenv("TDRN_PLAN_DUMP")) {
        if (atoi(pd))
            for (const Op &o : ops)
                if (o.kind == OP_CONV)       // (... %s/%s: the kernel at batch 1 / at the reference batch)
                    fprintf(stderr, "plan: %-28s lane %d  %dx%d k%d s%d d%d  Cin %4d Cout %4d  splitk %d  %s/%s  chain %d\n", o.w.c_str(), o.lane,
                            o.hw >> 16, o.hw & 0xffff, o.k, o.stride, o.dil, o.Cin, o.Cout, o.splitk, conv_kernel_name(conv_route(conv_question(o, 1), o.pool_t >= 0)),
                            conv_kernel_name(conv_route(conv_question(o, kPlanRefBatch), o.pool_t >= 0)), o.chain);
    }
    for (int l = 0; l < kLanes; ++l) {
        splitk_off[l] = ws_per_sample;
        ws_per_sample += lane_bytes[l];
    }
}

// OPT-IN (TDRN_PLAN_DWPW; it measured slower than the two launches, dwpw.hip): conv_dw blocks as ONE launch:
// a depthwise op directly followed by its pointwise conv, which is the only
// reader of the depthwise output; decided from the geometry (the batch-dependent 4-GiB limit is re-checked per forward,
// which then falls back to the two launches: the depthwise tensor keeps its place in the workspace)
void Plan::plan_dwpw()
{
    if (cfg.dtype == TDRN_F32 || !(cfg.plan_flags & TDRN_PLAN_DWPW)) return;
    for (size_t i = 0; i + 1 < ops.size(); ++i) {
        Op &d = ops[i];
        Op &c = ops[i + 1];
        if (d.kind != OP_DW || c.kind != OP_CONV || c.in != d.out || c.k != 1 || c.stride != 1 || c.pad != 0 || c.phases != 1 || c.res >= 0 ||
            c.out_kind != OUT_TENSOR || c.splitk != 1 || c.lane != d.lane || c.pool_t >= 0 || c.chain >= 0) continue;
        if (readers_of(d.out) != 1) continue;
        const Tensor &ti = tensors[d.in];
        DwPwArgs a;
        a.B = 1; a.H = ti.H; a.W = ti.W; a.Cin = c.Cin; a.Cout = c.Cout; a.Npad = c.Npad; a.Cs = tensors[c.out].Cpad;
        a.stride = d.stride; a.dtype = cfg.dtype;
        if (ti.Cpad != c.Cin || !dwpw_supported(a)) continue;
        d.fused_dw = 1; c.fused_dw = 1;
        d.stat = ST_DWPW;
        d.flops += c.flops;
        d.bytes = (double)ti.H * ti.W * ti.Cpad * es + (double)ti.H * ti.W * tensors[c.out].Cpad * es;
        c.flops = 0; c.bytes = 0;
    }
}

// conv3x3_pp.hip's chained split needs a slab per workgroup; only launches on the main lane use it (one at a time)
// Batch-independent tail of the workspace: [256 B: the chain launch's counters][1 KiB: the chained split's flag words]
// [its slabs]; the first 1280 bytes are zeroed once per forward.
void Plan::plan_workspace_tail()
{
    ws_fixed = 0;
    pp_sk_planned = false;
    for (const Op &o : ops) {
        if (o.kind != OP_CONV || o.stat != ST_CONV3 || o.lane != 0) continue;
        ConvArgs a = conv_question(o, 0);
        a.kdisable = 0;                      // (the workspace is sized alike whatever the kernel-choice switches say)
        pp_sk_planned = pp_sk_planned || pp_takes_geometry(a);
    }
    if (pp_sk_planned || !chain_ops.empty()) ws_fixed = kTailCtl + (pp_sk_planned ? align_up(conv_pp_sk_bytes(), 256) : 1024);
}

void Plan::mark_shared_tensors()
{
    tensor_lane.assign(tensors.size(), 0);
    tensor_shared.assign(tensors.size(), 0);
    for (const Op &o : ops) {
        if (o.out >= 0) tensor_lane[o.out] = o.lane;
        if (o.pool_t >= 0) tensor_lane[o.pool_t] = o.lane;
    }
    for (const Op &o : ops)
        for (int t : {o.in, o.res, o.off_t})
            if (t >= 0 && tensor_lane[t] != o.lane) tensor_shared[t] = 1;
}

int Plan::build()
{
    es = dtype_bytes(cfg.dtype);
    static const struct { int plan_flag, koff; } kSwitches[] = {
        {TDRN_PLAN_NO_CONV_PP, KOFF_CONV_PP},       {TDRN_PLAN_NO_PP_SK, KOFF_PP_SK},
        {TDRN_PLAN_NO_CONV_PATCH, KOFF_CONV_PATCH}, {TDRN_PLAN_NO_PW1X1, KOFF_PW1X1},
        {TDRN_PLAN_NO_DW_SLIDE, KOFF_DW_SLIDE},     {TDRN_PLAN_DW_SLIDE_ALL, KOFF_DW_STRIP_SMALL},
        {TDRN_PLAN_NO_CONV_WS, KOFF_CONV_WS},       {TDRN_PLAN_NO_YGEMM_V2, KOFF_YGEMM_V2},
        {TDRN_PLAN_NO_HEAD3X3, KOFF_HEAD3X3},       {TDRN_PLAN_TS_ONE_RANGE, KOFF_TS_RANGES},
        {TDRN_PLAN_NO_PATCH_TAIL, KOFF_PATCH_TAIL},
    };
    kdisable = 0;
    for (const auto &sw : kSwitches)
        if (cfg.plan_flags & sw.plan_flag) kdisable |= sw.koff;
    fault_handoff = (cfg.plan_flags & TDRN_PLAN_FAULT_HANDOFF) ? 1 : 0;
    late_side = !(cfg.plan_flags & TDRN_PLAN_NO_LATE_SIDE);
    use_lanes = !(cfg.plan_flags & TDRN_PLAN_ONE_STREAM);
    // build_net() only constructs 320 / 512 nets, but they are fully convolutional and multi_eval.py runs them at
    // 192 ... 1216 (every tested size is a multiple of 64, so all four pyramid levels are exact)
    if (cfg.size < 128 || cfg.size > 1280 || cfg.size % 64 != 0) return TDRN_E_ARG;
    if (cfg.num_classes < 2 || cfg.num_classes > 21 * 4) return TDRN_E_ARG;
    if (cfg.dtype < 0 || cfg.dtype > 2) return TDRN_E_ARG;
    if (cfg.def_groups < 1) return TDRN_E_ARG;
    int rc;
    switch (cfg.model) {
        case TDRN_DRN_VGGBN: rc = build_drn(false); break;
        case TDRN_DRN_MOBILENET: rc = build_drn(true); break;
        case TDRN_SSD4SCALE_MOBILE: rc = build_ssd4scale(true); break;
        case TDRN_SSD4SCALE_VGG: rc = build_ssd4scale(false); break;
        case TDRN_REFINEDET_VGG: rc = build_refinedet_vgg(); break;
        default: return TDRN_E_UNSUPPORTED;
    }
    if (rc != TDRN_OK) return rc;
    if (plan_error != TDRN_OK) return plan_error;
    alias_u8_input();
    hoist_l2norm_to_side_lanes();
    plan_fuse_first();
    plan_splitk();
    plan_chain();
    place_splitk_slabs();
    plan_dwpw();
    plan_workspace_tail();
    // Y layout of the transform-then-sample heads: tap-major [tap][pixel][80] when every level's transform runs on ygemm_k256
    // (which writes it), else the plain [pixel][columns] matrix of the generic GEMM
    y_tap_major = true;
    for (const Op &d : ops)
        if (d.kind == OP_DEFORM && d.y_t >= 0 && !ygemm_supported(d.Cin, d.y_cols, cfg.dtype)) y_tap_major = false;
    mark_shared_tensors();
    return TDRN_OK;
}

}  // namespace tdrn
