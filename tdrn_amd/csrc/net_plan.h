// net_plan.h -- the layer plan of a net (net_plan.hip builds it, net_pack.hip packs its weights, net_run.hip runs it).
// Internal to libtdrn_hip.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "kernels.h"

namespace tdrn {

enum OpKind { OP_FIRST, OP_CONV, OP_POOL, OP_L2NORM, OP_DW, OP_OFFSET, OP_DEFORM, OP_SOFTMAX, OP_OFF_OUT, OP_LOC_OUT,
              OP_REFLOC_IN };
enum OutKind { OUT_TENSOR = 0, OUT_ARM_LOC = 1, OUT_ODM_LOC = 2, OUT_CONF = 3 };
enum { ST_CONV, ST_FIRST, ST_POOL, ST_L2, ST_DW, ST_OFFSET, ST_DEFORM, ST_SOFTMAX, ST_LAYOUT, ST_CONV3, ST_DWPW, ST_COUNT };

struct Tensor { int C, Cpad, H, W; bool f32; size_t off; /* bytes per sample from workspace start */ std::string label; };
struct ParamSpec { std::string name; std::vector<int64_t> shape; };
using StagedParams = std::map<std::string, std::vector<float>>;   // fp32 host copies handed in through tdrn_net_set_param

struct Op {
    OpKind kind;
    int in = -1, out = -1, res = -1;
    int Cin = 0, Cout = 0, Npad = 0, k = 1, stride = 1, pad = 0, dil = 1, relu = 0, phases = 1, ceil = 0;
    int out_kind = OUT_TENSOR, scale = 0, hw = 0;        // head ops: which pyramid level
    int G = 1, n_branches = 1, k2 = 0, pad2 = 0;          // deform
    int taps = 0;                                         // deform: kh * kw summed over the branches
    int split = 0;                                        // deform, gather kernel: 0 = one work item per problem, else the halves accumulate into ZEROED
                                                          // outputs: 1 = by branch (two-branch heads), 2 = by group halves (an even number of deformable
                                                          // groups: the TRN temporal heads).  The transform-then-sample path stores, no atomics.
    int off_t = -1, off_c0[2] = {0, 0}, off_n = 0;        // offset tensor (fp32 NHWC), channel starts
    int loc_src = OUT_ARM_LOC;                            // OP_OFFSET input: ARM loc view or a ref_loc tensor
    std::string w, b, bn, w2, b2;                          // parameter names (w2/b2: second source)
    size_t w_off = 0, b_off = 0, w2_off = 0;               // blob offsets
    int y_t = -1, y_cols = 0;                              // deform, transform-then-sample plans: the Y tensor (per-tap partial outputs)
    int y_groups = 1;                                      // ... output-column groups of <= 80 (12 + 3 * classes > 80: VID's 31 classes = 2, COCO's 81 = 4): one Y region,
                                                           // one transform and one sampling launch per group (region g of the tensor: y_cols * H * W * B elements each)
    size_t wt_off = 0, bt_off = 0;                         // ... its 1x1 GEMM weights [y_groups][y_cols][Cin] and zero bias
    double flops = 0, bytes = 0;                           // algorithmic, per sample
    int stat = 0;
    int lane = 0;                                          // HIP stream lane (0 = the caller's stream)
    int pool_t = -1;                                       // conv: fused MaxPool2d(2,2) output tensor (patch kernel)
    int splitk = 1;                                        // conv: K slices, fixed per layer at plan time
    bool chain_tag = false;                                // conv: candidate for the one-launch chain of small top-of-pyramid layers
    int chain = -1;                                        // ... its stage index in that launch (conv_igemm.hip conv_chain_kernel), or -1
    int fused_dw = 0;                                      // depthwise op: its launch also computes the next op, the pointwise conv (dwpw.hip); that conv: 1 = computed there
    size_t chain_partial = 0;                              // ... its split-K slab inside the chain's slab region (bytes per sample)
};

// independent branches of the tail (TCB laterals, ARM heads) run on side streams; dependencies
// between lanes are hipEvents on the producing tensor.
constexpr int kLanes = 4;
constexpr int kPlanRefBatch = 32; // the batch (the benchmark's) at which split-K is chosen, per layer, from its geometry
constexpr size_t kTailCtl = 256;  // bytes of chain counters in front of the chained split's scratch (workspace tail)

// Everything build() produces; a forward reads it and changes none of it.
struct Plan {
    tdrn_net_config cfg{};
    int es = 2;
    std::vector<Tensor> tensors;
    std::vector<ParamSpec> params;
    std::map<std::string, size_t> param_index;
    std::vector<Op> ops;
    size_t ws_per_sample = 0, blob_bytes = kZeroPageBytes;
    size_t ws_fixed = 0;                 // batch-independent tail of the workspace: scratch of conv3x3_pp.hip's chained split (main lane)
    int P = 0, fm[4] = {0, 0, 0, 0}, scale_off[5] = {0, 0, 0, 0, 0};
    size_t splitk_off[kLanes] = {0, 0, 0, 0};   // per-lane split-K slab region (bytes per sample from workspace start)
    // Side-lane convs (TCB laterals, ARM heads, offset convs) are held back until conv5_3 has been computed: released on their
    // true inputs (L2Norm of conv4_3) they share the CUs with conv5_1..5_3 and stretch the trunk, the critical path, by
    // 0.24 ms; held back, they run beside conv6/conv7 and the small top-down layers instead (+1.4 % frames/s; held until fc7
    // or capped to 128..224 workgroups: no further gain).  TDRN_PLAN_NO_LATE_SIDE: off.
    int t_late = -1;
    std::vector<int> chain_ops;          // the chain launch's member ops in stage order (empty: no chain)
    size_t chain_partial_off = 0;        // the chain's split-K slab region (bytes per sample from workspace start)
    bool pp_sk_planned = false;          // some main-lane conv may use conv3x3_pp.hip's chained split
    int fuse_first = -1;                 // index of the conv whose patch loader computes the first conv itself (16-bit modes), or -1
    int x_t = -1;                        // fp32 (3, S, S) workspace tensor: the net input when the caller hands uint8 planes to a plan whose first conv reads fp32
    bool late_side = true;
    bool use_lanes = true;
    bool y_tap_major = true;            // Y of the transform-then-sample heads is tap-major (every level's transform runs on ygemm_k256)
    int kdisable = 0, fault_handoff = 0;
    std::vector<int> tensor_lane;
    std::vector<char> tensor_shared;

    int build();                        // from cfg
    int producer_of(int t) const;       // index of the (last) op that writes tensor t, or -1
    int readers_of(int t) const;        // number of op inputs / residuals that read tensor t
    // the fields of a conv op's launch that follow from the plan alone (no pointers, no output view), at batch B
    void conv_geometry(const Op &o, int B, ConvArgs &a) const;
    ConvArgs conv_question(const Op &o, int B) const;   // ... as conv_route is asked while planning (no buffers)
    // ops i and i + 1 share ONE launch: consecutive deformable heads / offset convs are batched (up to four, the pyramid levels)
    bool launch_continues(size_t i) const
    {
        return i + 1 < ops.size() && ops[i + 1].kind == ops[i].kind && (ops[i].kind == OP_DEFORM || ops[i].kind == OP_OFFSET);
    }
    // op i issues a launch of its own (not computed inside an earlier op's: a batch, the chain launch, the fused dw+pw launch)
    bool launch_head(size_t i) const
    {
        const Op &o = ops[i];
        return !(i > 0 && launch_continues(i - 1)) && !(o.kind == OP_CONV && (o.chain > 0 || o.fused_dw));
    }

private:
    int cur_lane = 0, plan_error = TDRN_OK;   // build() only
    int T(int C, int H, int W, bool f32 = false);
    void P_(const std::string &name, std::vector<int64_t> shape);
    void bn_params(const std::string &bn, int C);
    int push(Op &o, const std::string &l = "") { o.lane = cur_lane; if (!l.empty()) label(o.out, l); ops.push_back(o); return o.out; }
    void label(int t, const std::string &l) { if (t >= 0) tensors[t].label = l; }
    size_t blob(size_t bytes);
    // op constructors
    int first_conv(const std::string &w, bool bias, const std::string &bn, int Cout, int stride, int S);
    int conv(int in, const std::string &w, bool bias, const std::string &bn, int Cout, int k, int stride, int pad, int dil,
             int relu, int res = -1, int out_kind = OUT_TENSOR, int scale = 0, const std::string &w2 = "", int k2 = 0);
    int conv_transpose2(int in, const std::string &w, bool bias, int Cout, int res, int relu);
    bool can_fuse_pool(int in) const;
    int pool(int in, int ceil_mode, bool in_needed_elsewhere = false);
    int l2norm(int in, const std::string &name);
    int dwconv(int in, const std::string &w, const std::string &bn, int stride);
    int conv_dw(int in, const std::string &name, int Cout, int stride);
    int offset_conv(int scale, int H, int W, const std::string &w1, const std::string &w2, bool bias, int n1, int n2,
                    int loc_src, int ref_tensor = -1);
    void deform_heads(int in, int off_t, int scale, int G, const std::string &loc1, const std::string &conf1,
                      const std::string &loc2, const std::string &conf2, int off_c1, int out_loc_kind);
    void softmax_op();
    void offsets_out(int scale, int off_t, int n);
    void loc_maps_out(int scale);
    int ref_loc_in(int scale, int H, int W);
    void set_pyramid(int s0);
    // model families
    void vgg_trunk(int S, bool bn, int c7, int &c43, int &c53, int &fc7);
    void vgg_sources(int src[4]);
    void tcb(const int src[4], bool bias, int odm[4]);
    void drn_heads(const int src[4], const int odm[4], bool bias);
    void mobilenet_sources(int S, int c7, bool extras_bias, int src[4]);
    int build_drn(bool mobile);
    int build_refinedet_vgg();
    int build_ssd4scale(bool mobile);
    // build()'s passes, in order
    void alias_u8_input();
    void hoist_l2norm_to_side_lanes();
    void plan_fuse_first();
    void plan_splitk();
    void plan_chain();
    void place_splitk_slabs();
    void plan_dwpw();
    void plan_workspace_tail();
    void mark_shared_tensors();
};

// BatchNorm folding and OIHW -> [Cout][tap][Cin] packing of the staged fp32 parameters into the host image of the weight blob (net_pack.hip)
int pack_weights(const Plan &p, const StagedParams &staged, std::vector<char> &host);

}  // namespace tdrn
