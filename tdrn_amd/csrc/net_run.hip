// net_run.hip -- the forward executor of a plan (net_plan.h): one Run per call, one routine per op kind.  No device
// allocation: the weight blob and the activation workspace are caller-owned (tdrn_hip.h).
#include "net.h"

namespace tdrn {
namespace {

// The state of ONE forward.  Fixed-size, on the caller's stack: a forward allocates nothing outside profile mode.
struct Run {
    tdrn_net &n;
    const Plan &p;
    const void *blob; void *ws; size_t ws_bytes; const tdrn_net_io *io; hipStream_t s0;
    const char *wb = nullptr;
    // the batch: fp32 (B,3,S,S) in io->x, or uint8 planes + per-plane mean (tdrn_net_io.reserved[3]); `xin` = the fp32 tensor the first
    // conv reads, null until the uint8 planes have been converted (which only happens when no kernel reads them directly)
    const tdrn_u8_frames *u8 = nullptr;
    const float *xin = nullptr;
    int B = 0, C = 0;
    int Bk = 0;                          // key-frame broadcast (tdrn_net_io.reserved[1]): ref_loc / the offset tensors hold Bk samples, sample b reads those of b % Bk
    bool lanes = false, join_on = false, reuse_offsets = false;
    bool lane_used[kLanes] = {true, false, false, false};
    bool zeroed_early = false, skz_pending = false, dwpw_done = false;
    char *tail = nullptr;                // [kTailCtl: chain counters][chained split: 1 KiB flags, slabs]
    DeformArgs dargs[4];                 // consecutive deformable heads (the pyramid levels): one launch
    int ts_op[4] = {-1, -1, -1, -1}, n_dargs = 0;
    OffsetProblem oq[4];                 // consecutive offset convs of one lane: one launch (layers.hip)
    int oq_op[4], n_oq = 0;
    size_t evi = 0;
    int offset_ops_enqueued = 0;

    Run(tdrn_net &net, const void *blob_, void *ws_, size_t ws_bytes_, const tdrn_net_io *io_, hipStream_t s)
        : n(net), p(net), blob(blob_), ws(ws_), ws_bytes(ws_bytes_), io(io_), s0(s) {}
    // Whatever way the forward is left -- also on a mid-plan error -- the caller's stream is ordered after
    // everything already queued on the side lanes (they write the workspace and the outputs).
    ~Run() { (void)join(); }
    int join()
    {
        if (!join_on) return TDRN_OK;
        join_on = false;
        int rc = TDRN_OK;
        for (int l = 1; l < kLanes; ++l)
            if (lane_used[l]) {
                hipError_t e = hipEventRecord(n.ev_join[l - 1], n.side[l - 1]);
                if (e == hipSuccess) e = hipStreamWaitEvent(s0, n.ev_join[l - 1], 0);
                if (e != hipSuccess && rc == TDRN_OK) rc = (int)e;
            }
        return rc;
    }

    char *tptr(int id) const { return (char *)ws + p.tensors[id].off * (size_t)B; }
    float *loc_out(const Op &o) const { return o.out_kind == OUT_ARM_LOC ? io->arm_loc : io->odm_loc; }
    // a batched launch that op o belongs to is being collected: in front of o's routine, o joins it (no launch begins here);
    // behind it, the launch has not been issued yet
    bool launch_open(const Op &o) const { return (o.kind == OP_DEFORM && n_dargs > 0) || (o.kind == OP_OFFSET && n_oq > 0); }
    int record(int t, hipStream_t s) const
    {
        if (lanes && t >= 0 && p.tensor_shared[t]) TDRN_HIP_TRY(hipEventRecord(n.tensor_ev[t], s));
        return TDRN_OK;
    }

    // ---- prologue ---------------------------------------------------------------------------------
    int check_args()
    {
        if (!n.weights_ready) return TDRN_E_STATE;
        if (!blob || !ws || !io || io->batch <= 0) return TDRN_E_ARG;
        u8 = (const tdrn_u8_frames *)io->reserved[3];
        if (u8 ? !u8->planes : !io->x) return TDRN_E_ARG;
        xin = u8 ? nullptr : io->x;
        B = io->batch;
        if (ws_bytes < p.ws_per_sample * (size_t)B + p.ws_fixed) return TDRN_E_WORKSPACE;
        if (!io->conf) return TDRN_E_ARG;
        // a net's pooled streams / events belong to ONE device: the one current at its first forward
        const int d = pool::cur_dev();
        if (n.dev < 0) n.dev = d;
        else if (n.dev != d) return TDRN_E_STATE;
        // "never continue after an error": a forward whose device-side hand-off timed out makes the NEXT call fail
        // (no synchronisation here: the word is host memory the kernels store to)
        if (p.ws_fixed) {
            if (!n.status) TDRN_TRY(pool::get_status(&n.status));
            TDRN_TRY(n.check_status(nullptr));
        }
        const bool is_drn = p.cfg.model == TDRN_DRN_VGGBN || p.cfg.model == TDRN_DRN_MOBILENET || p.cfg.model == TDRN_REFINEDET_VGG;
        const bool has_arm = p.cfg.model != TDRN_REFINEDET_VGG || p.cfg.use_refine;
        if (is_drn && !io->odm_loc) return TDRN_E_ARG;
        if (has_arm && !io->arm_loc) return TDRN_E_ARG;
        wb = (const char *)blob;
        C = p.cfg.num_classes;
        n.last_batch = B;
        return TDRN_OK;
    }

    int fork()
    {
        if (n.profile && n.ev.size() < 2 * p.ops.size()) {
            const size_t old = n.ev.size();
            n.ev.resize(2 * p.ops.size());
            for (size_t i = old; i < n.ev.size(); ++i) TDRN_TRY(pool::get_timing_event(n.dev, &n.ev[i]));
        }
        n.ev_stat.clear();
        n.ev_op.clear();
        // profile 1 runs single-stream (per-kernel durations without overlap); profile 2 keeps the production lanes, so a
        // launch's duration includes what the concurrent side-lane kernels take from it
        lanes = p.use_lanes && n.profile != 1;
        if (lanes) {
            TDRN_TRY(n.init_lanes());
            TDRN_HIP_TRY(hipEventRecord(n.ev_fork, s0));
        }
        join_on = lanes;
        return TDRN_OK;
    }

    // a lane's first work of this forward is ordered after everything the caller had queued in front of it
    int open_lane(int lane, hipStream_t s)
    {
        if (!lane_used[lane]) TDRN_HIP_TRY(hipStreamWaitEvent(s, n.ev_fork, 0));
        lane_used[lane] = true;
        return TDRN_OK;
    }

    int zero_split_outputs(const Op &o, hipStream_t s) const
    {
        TDRN_HIP_TRY(hipMemsetAsync(loc_out(o), 0, (size_t)B * p.P * 4 * sizeof(float), s));
        TDRN_HIP_TRY(hipMemsetAsync(io->conf, 0, (size_t)B * p.P * C * sizeof(float), s));
        return TDRN_OK;
    }

    int zero_early()
    {
        // split deformable heads of the gather kernel accumulate into zeroed outputs: zero them on a side stream at the very
        // start (under the first conv) instead of in front of the deform launch on the critical path
        if (lanes) {
            const Op *dsplit = nullptr;
            int n_deform_groups = 0;
            for (size_t k = 0; k < p.ops.size(); ++k)
                if (p.ops[k].kind == OP_DEFORM) {
                    if (p.ops[k].split && p.ops[k].y_t < 0 && !dsplit) dsplit = &p.ops[k];
                    if (k == 0 || p.ops[k - 1].kind != OP_DEFORM) ++n_deform_groups;
                }
            if (dsplit && n_deform_groups == 1) {        // (one merged launch writes these outputs; nothing else does)
                TDRN_TRY(open_lane(1, n.side[0]));
                TDRN_TRY(zero_split_outputs(*dsplit, n.side[0]));
                TDRN_HIP_TRY(hipEventRecord(n.ev_zero, n.side[0]));
                zeroed_early = true;
            }
        }
        // the chained split's flag words (conv3x3_pp.hip) are zeroed ONCE per forward, off the critical path; every launch
        // leaves them zero (the consumer of a flag resets it)
        tail = (char *)ws + p.ws_per_sample * (size_t)B;
        if (!p.ws_fixed) return TDRN_OK;
        if (lanes) {
            TDRN_TRY(open_lane(1, n.side[0]));
            TDRN_HIP_TRY(hipMemsetAsync(tail, 0, kTailCtl + 1024, n.side[0]));
            TDRN_HIP_TRY(hipEventRecord(n.ev_skz, n.side[0]));
            skz_pending = true;
        } else {
            TDRN_HIP_TRY(hipMemsetAsync(tail, 0, kTailCtl + 1024, s0));
        }
        return TDRN_OK;
    }

    int check_reuse()
    {
        reuse_offsets = p.cfg.deform && io->reserved[0] != nullptr;
        if (reuse_offsets && (n.offs_ws != ws || n.offs_batch != B)) return TDRN_E_STATE;
        Bk = B;
        if (io->reserved[1]) {
            const long long kb = (long long)(intptr_t)io->reserved[1];
            if (!p.cfg.deform || kb < 1 || kb > B || B % kb) return TDRN_E_ARG;
            Bk = (int)kb;
        }
        if (reuse_offsets && n.offs_key_batch != Bk) return TDRN_E_STATE;
        // The reuse state is valid only once the offset launches of THIS forward have been enqueued and the forward returned OK
        // (an early error return, or a tdrn_net_forward_from that starts behind the offset ops, leaves it invalid: a later
        // reserved[0] call then gets TDRN_E_STATE instead of sampling stale or uninitialised offsets)
        if (p.cfg.deform && !reuse_offsets) { n.offs_ws = nullptr; n.offs_batch = 0; n.offs_key_batch = 0; }
        return TDRN_OK;
    }

    int prologue()
    {
        TDRN_TRY(check_args());
        TDRN_TRY(fork());
        TDRN_TRY(zero_early());
        return check_reuse();
    }

    int epilogue()
    {
        const int jrc = join();
        int offset_ops_planned = 0;
        for (const Op &d : p.ops) offset_ops_planned += d.kind == OP_OFFSET;
        if (jrc == TDRN_OK && p.cfg.deform && !reuse_offsets && offset_ops_planned > 0 && offset_ops_enqueued == offset_ops_planned) {
            n.offs_ws = ws; n.offs_batch = B; n.offs_key_batch = Bk;
        }
        return jrc;
    }

    // ---- per op -----------------------------------------------------------------------------------
    bool skipped(size_t oi)
    {
        const Op &o = p.ops[oi];
        if (o.kind == OP_CONV && o.fused_dw && dwpw_done) { dwpw_done = false; return true; }   // computed by the depthwise op's launch
        if (o.kind == OP_OFF_OUT && !io->offsets[o.scale]) return true;
        if (o.kind == OP_LOC_OUT && !io->loc_maps[o.scale]) return true;
        if (reuse_offsets && (o.kind == OP_REFLOC_IN || o.kind == OP_OFFSET)) return true;   // (their tensors still hold the key frame's)
        if (o.kind == OP_FIRST && p.fuse_first >= 0) return true;            // computed inside the next conv's patch loader
        if (o.kind == OP_CONV && o.chain > 0) return true;                   // computed by the chain launch at its first member's place
        return (int)oi < n.first_op;
    }

    // lane choice plus the cross-lane waits
    int stream_for(const Op &o, int &lane, hipStream_t &s)
    {
        lane = lanes ? o.lane : 0;
        s = lane == 0 ? s0 : n.side[lane - 1];
        if (!lanes) return TDRN_OK;
        TDRN_TRY(open_lane(lane, s));
        for (int t : {o.in, o.res, o.off_t})
            if (t >= 0 && p.tensor_lane[t] != lane) TDRN_HIP_TRY(hipStreamWaitEvent(s, n.tensor_ev[t], 0));
        if (p.late_side && lane != 0 && (o.kind == OP_CONV || o.kind == OP_OFFSET) && p.t_late >= 0 && p.tensor_shared[p.t_late])
            TDRN_HIP_TRY(hipStreamWaitEvent(s, n.tensor_ev[p.t_late], 0));
        return TDRN_OK;
    }

    // the main lane waits for the zeroed flag words only in front of the first launch that reads them
    int wait_tail_zeroed()
    {
        if (!skz_pending) return TDRN_OK;
        TDRN_HIP_TRY(hipStreamWaitEvent(s0, n.ev_skz, 0));
        skz_pending = false;
        return TDRN_OK;
    }

    // ConvArgs of a conv op whose output is a workspace tensor or a head view
    void conv_args(const Op &o, ConvArgs &a) const
    {
        p.conv_geometry(o, B, a);
        a.in = tptr(o.in); a.w = wb + o.w_off; a.bias = (const float *)(wb + o.b_off); a.zero_page = wb;
        a.relu = o.relu;
        a.status = n.status; a.fault_handoff = p.fault_handoff;
        if (o.out_kind == OUT_TENSOR) {
            const Tensor &to = p.tensors[o.out];
            a.out = tptr(o.out);
            if (o.res >= 0) a.res = tptr(o.res);
            a.o_cs = to.Cpad;
            if (o.phases == 4) {
                a.o_bs = (long long)to.H * to.W * to.Cpad; a.o_rs = 2ll * to.W * to.Cpad; a.o_cs = 2ll * to.Cpad;
                a.o_pr = (long long)to.W * to.Cpad; a.o_pc = to.Cpad;
            } else {
                a.o_bs = (long long)to.H * to.W * to.Cpad; a.o_rs = (long long)to.W * to.Cpad;
            }
        } else {
            const int per = o.out_kind == OUT_CONF ? 3 * C : 12;     // channels per pixel
            const int per_prior = o.out_kind == OUT_CONF ? C : 4;
            a.out = o.out_kind == OUT_CONF ? io->conf : loc_out(o); a.out_f32 = 1;
            a.o_base = (long long)p.scale_off[o.scale] * per_prior;
            a.o_bs = (long long)p.P * per_prior; a.o_rs = (long long)a.Wo * per; a.o_cs = per;
        }
        if (o.splitk > 1) {
            a.splitk = o.splitk;
            a.partial = (char *)ws + (o.chain >= 0 ? p.chain_partial_off + o.chain_partial : p.splitk_off[o.lane]) * (size_t)B;
        }
    }

    int ensure_f32_input(hipStream_t s)
    {
        if (xin) return TDRN_OK;
        TDRN_TRY(launch_u8_planes_to_f32(u8->planes, B, p.cfg.size, u8->mean, (float *)tptr(p.x_t), s));
        xin = (const float *)tptr(p.x_t);
        return TDRN_OK;
    }

    int launch_first(const Op &f, hipStream_t s) const
    {
        return launch_first_conv(xin, (const float *)(wb + f.w_off), (const float *)(wb + f.b_off), tptr(f.out), B, f.hw, f.stride, f.Cout,
                                 p.tensors[f.out].Cpad, f.relu, p.cfg.dtype, s);
    }

    // the whole chain as ONE launch at its first member's place; the other members are skipped
    int run_conv_chain(hipStream_t s)
    {
        ChainLayer cl[16];
        const int nl = (int)p.chain_ops.size();
        for (int k = 0; k < nl; ++k) {
            const Op &m = p.ops[p.chain_ops[k]];
            conv_args(m, cl[k].a);
            int nd = 0;
            for (int t : {m.in, m.res}) {
                if (t < 0) continue;
                int dep = -1;
                for (int j = 0; j < k; ++j)
                    if (p.ops[p.chain_ops[j]].out == t) dep = j;
                if (dep >= 0) cl[k].dep[nd++] = dep;
                else if (lanes && p.tensor_lane[t] != 0) TDRN_HIP_TRY(hipStreamWaitEvent(s, n.tensor_ev[t], 0));
            }
        }
        TDRN_TRY(wait_tail_zeroed());
        TDRN_TRY(launch_conv_chain(cl, nl, (unsigned *)tail, s, n.status));
        for (int k = 1; k < nl; ++k) TDRN_TRY(record(p.ops[p.chain_ops[k]].out, s));
        return TDRN_OK;
    }

    int run_conv(size_t oi, hipStream_t s)
    {
        const Op &o = p.ops[oi];
        const bool pooled = o.pool_t >= 0;
        ConvArgs a;
        conv_args(o, a);
        if (o.lane == 0 && p.pp_sk_planned) {
            a.sk_ws = tail + kTailCtl;
            a.sk_flags_zero = true;
            if (skz_pending && pp_takes_geometry(a)) TDRN_TRY(wait_tail_zeroed());
        }
        if ((int)oi == p.fuse_first) {
            const Op &f = p.ops[0];
            a.fuse_w = (const float *)(wb + f.w_off); a.fuse_b = (const float *)(wb + f.b_off);
            a.fuse_cout = f.Cout;
            if (!xin) {
                // uint8 frames: conv3x3_ws.hip's producers read the planes themselves (the frame never exists in fp32)
                a.fuse_x8 = u8->planes; a.fuse_mean[0] = u8->mean[0]; a.fuse_mean[1] = u8->mean[1]; a.fuse_mean[2] = u8->mean[2];
                if (conv_route(a, pooled) != CONV_WS) {           // (a small batch): the fp32 route from here on
                    a.fuse_x8 = nullptr;
                    TDRN_TRY(ensure_f32_input(s));
                }
            }
            a.fuse_x = xin;
            if (conv_route(a, pooled) == CONV_NONE) {
                // the fusion was planned from the layer geometry; should no kernel take THIS launch (a limit that depends on
                // the batch), run the two layers as two launches: the first conv's tensor keeps its place in the workspace
                TDRN_TRY(launch_first(f, s));
                a.fuse_x = nullptr; a.fuse_w = nullptr; a.fuse_b = nullptr; a.fuse_cout = 0;
            }
        }
        return launch_conv(a, s, pooled ? tptr(o.pool_t) : nullptr);
    }

    int run_dw(size_t oi, hipStream_t s)
    {
        const Op &o = p.ops[oi];
        const Tensor &ti = p.tensors[o.in];
        if (o.fused_dw) {
            const Op &c = p.ops[oi + 1];
            DwPwArgs a;
            a.in = tptr(o.in); a.w = wb + c.w_off; a.wdw = (const float *)(wb + o.w_off); a.bdw = (const float *)(wb + o.b_off);
            a.bias = (const float *)(wb + c.b_off); a.out = tptr(c.out);
            a.B = B; a.H = ti.H; a.W = ti.W; a.Cin = c.Cin; a.Cout = c.Cout; a.Npad = c.Npad; a.Cs = p.tensors[c.out].Cpad;
            a.stride = o.stride; a.relu_dw = o.relu; a.relu = c.relu; a.dtype = p.cfg.dtype;
            if (dwpw_supported(a)) {
                dwpw_done = true;
                TDRN_TRY(launch_dwpw(a, s));
                return record(c.out, s);     // (the pointwise op's output tensor is produced HERE, by the depthwise op's launch)
            }
        }
        return launch_dwconv3(tptr(o.in), (const float *)(wb + o.w_off), (const float *)(wb + o.b_off), tptr(o.out), B, ti.H, ti.W, ti.Cpad,
                              o.stride, o.relu, p.cfg.dtype, s, p.kdisable);
    }

    int run_offset(size_t oi, int lane, hipStream_t s)
    {
        const Op &o = p.ops[oi];
        const float *loc;
        long long bs, ps;
        if (o.in >= 0) { loc = (const float *)tptr(o.in); bs = (long long)o.hw * 12; ps = 12; }
        else { loc = io->arm_loc + (size_t)p.scale_off[o.scale] * 4; bs = (long long)p.P * 4; ps = 12; }
        // (offsets from ref_loc maps exist for the Bk key frames only; from the net's own ARM loc for every sample)
        oq[n_oq] = OffsetProblem{loc, bs, ps, (const float *)(wb + o.w_off), (const float *)(wb + o.b_off),
                                 (float *)tptr(o.out), o.in >= 0 ? Bk : B, o.hw, o.off_n, 0};
        oq_op[n_oq++] = (int)oi;
        if (p.launch_continues(oi) && n_oq < 4 && (lanes ? p.ops[oi + 1].lane : 0) == lane) return TDRN_OK;
        TDRN_TRY(launch_offset_conv_multi(oq, n_oq, s));
        // the outputs of the launch's earlier members become visible HERE, not where their ops stood
        for (int i = 0; i + 1 < n_oq; ++i) TDRN_TRY(record(p.ops[oq_op[i]].out, s));
        n_oq = 0;
        return TDRN_OK;
    }

    int run_deform(size_t oi, hipStream_t s)
    {
        const Op &o = p.ops[oi];
        const Tensor &ti = p.tensors[o.in];
        const Tensor &tf = p.tensors[o.off_t];
        DeformArgs a;
        a.in = tptr(o.in); a.zero_page = wb; a.n_branches = o.n_branches;
        const float *off = (const float *)tptr(o.off_t);
        a.br[0] = DeformBranch{off + o.off_c0[0], tf.C, wb + o.w_off, 3, 3, 1, 1, 1, o.G};
        if (o.n_branches == 2) a.br[1] = DeformBranch{off + o.off_c0[1], tf.C, wb + o.w2_off, 5, 5, 2, 1, 1, o.G};
        if (Bk < B)
            for (int k = 0; k < o.n_branches; ++k) a.br[k].off_rows = Bk * ti.H * ti.W;
        a.B = B; a.H = ti.H; a.W = ti.W; a.Cin = o.Cin; a.Ho = ti.H; a.Wo = ti.W; a.Cout = o.Cout; a.Npad = o.Npad;
        a.out0 = loc_out(o) + (size_t)p.scale_off[o.scale] * 4; a.o0_bs = (long long)p.P * 4; a.o0_ps = 12;
        a.out1 = io->conf + (size_t)p.scale_off[o.scale] * C; a.o1_bs = (long long)p.P * C; a.o1_ps = 3 * C;
        a.split = 12; a.dtype = p.cfg.dtype;
        dargs[n_dargs++] = a;
        if (o.y_t >= 0) ts_op[n_dargs - 1] = (int)oi;
        if (p.launch_continues(oi) && n_dargs < 4) return TDRN_OK;      // all pyramid levels in one launch
        const int rc = o.y_t >= 0 ? run_deform_ts(s) : run_deform_gather(o, s);
        n_dargs = 0;
        return rc;
    }

    // transform: Y = X * W_taps (1x1 GEMM, net dtype out) per level, then sample: all pyramid levels in one
    // launch.  Y is addressed with 32-bit byte offsets (deform.hip), so a batch whose Y would pass 4 GiB at
    // some level runs as several batch RANGES through the same Y buffers, one (transforms, sample) group per
    // range on this stream -- per-frame arithmetic untouched (DRN at 512 px: 171 frames and up; at 320 px: 437).
    int run_deform_ts(hipStream_t s)
    {
        int Bc = B;
        size_t per_frame = 0;
        for (int i = 0; i < n_dargs; ++i) {
            const Op &d = p.ops[ts_op[i]];
            const int fit = deform_ts_max_batch(dargs[i].H, dargs[i].W, d.y_cols, d.taps);
            Bc = fit < Bc ? fit : Bc;
            per_frame += (size_t)dargs[i].H * dargs[i].W * d.y_cols * p.es;       // (one column group's Y: a group's two launches are adjacent)
        }
        if (Bc < 1) return TDRN_E_UNSUPPORTED;
        // ... and (round 5) a range's Y is kept below 192 MiB, so that it is still in the 256-MiB memory-side cache when
        // the sampling launch gathers it: the pair of launches 277-285 -> 254-255 us alone at batch 32 (two ranges of
        // 16 frames; ranges of 8 / 4 frames lose it again to the extra launches), 520 -> 488 us at MobileNet's batch 64.
        // Per-frame arithmetic untouched.  TDRN_PLAN_TS_ONE_RANGE switches it off.
        constexpr size_t kRangeBytes = (size_t)192 << 20;
        if (per_frame > 0 && !(p.kdisable & KOFF_TS_RANGES)) {
            long long fit = (long long)kRangeBytes / (long long)per_frame;
            fit = fit < 1 ? 1 : fit;
            if (fit < Bc) Bc = (int)fit;
        }
        // output columns in groups of 80 (deform.hip: a Y row is 80 columns): group g = columns [80 g, 80 g + 80) of
        // [12 loc ; 3 * classes conf], its own weight rows, Y region, transform and sampling launch
        const int n_groups = p.ops[ts_op[0]].y_groups;
        for (int b0 = 0; b0 < B; b0 += Bc)
            for (int yg = 0; yg < n_groups; ++yg) TDRN_TRY(run_deform_ts_range(b0, B - b0 < Bc ? B - b0 : Bc, yg, n_groups, s));
        return TDRN_OK;
    }

    // frames [b0, b0 + nb), column group yg: the levels' transforms, then ONE sampling launch
    int run_deform_ts_range(int b0, int nb, int yg, int n_groups, hipStream_t s)
    {
        DeformArgs ca[4];
        YGemmProblem yq[4];
        const void *ts_y[4] = {nullptr, nullptr, nullptr, nullptr};
        int ts_cs[4] = {0, 0, 0, 0}, n_yq = 0;
        const int es = p.es, dtype = p.cfg.dtype;
        bool all_ygemm = true;
        for (int i = 0; i < n_dargs; ++i) all_ygemm = all_ygemm && ygemm_supported(p.ops[ts_op[i]].Cin, p.ops[ts_op[i]].y_cols, dtype);
        for (int i = 0; i < n_dargs; ++i) {
            const Op &d = p.ops[ts_op[i]];
            DeformArgs &c = ca[i];
            c = dargs[i];
            const size_t px0 = (size_t)b0 * c.H * c.W;
            c.B = nb;
            c.in = (const char *)c.in + px0 * c.Cin * es;
            for (int k = 0; k < c.n_branches; ++k) {
                if (c.br[k].off_rows) c.br[k].off_row0 = (int)(px0 % (size_t)c.br[k].off_rows);
                else c.br[k].off += px0 * c.br[k].off_stride;
            }
            c.out0 += (size_t)b0 * c.o0_bs;
            c.out1 += (size_t)b0 * c.o1_bs;
            if (d.y_groups != n_groups) return TDRN_E_STATE;
            void *ybuf = tptr(d.y_t) + (size_t)yg * d.y_cols * c.H * c.W * es * B;
            const char *wty = wb + d.wt_off + (size_t)yg * d.y_cols * d.Cin * es;
            const int y_taps = p.y_tap_major ? d.taps : 0;
            c.Cout = d.Cout - 80 * yg < 80 ? d.Cout - 80 * yg : 80;
            if (yg > 0) { c.split = 0; c.out1 += 80 * yg - 12; }     // (columns 12.. are conf columns: group g starts at conf column 80 g - 12)
            if (all_ygemm) {                 // all levels' transforms in ONE launch (below)
                yq[n_yq++] = YGemmProblem{c.in, wty, ybuf, (long long)nb * c.H * c.W, d.y_cols, d.y_cols, y_taps};
            } else if (ygemm_supported(d.Cin, d.y_cols, dtype)) {
                TDRN_TRY(launch_ygemm(c.in, wty, ybuf, (long long)nb * c.H * c.W, d.y_cols, d.y_cols, dtype, s, y_taps));
            } else {                         // the generic GEMM: a 1x1 conv over the head's input with y_cols outputs
                ConvArgs g;
                p.conv_geometry(d, nb, g);
                g.Cout = g.Npad = d.y_cols; g.kh = g.kw = 1; g.pad = 0;
                g.in = c.in; g.w = wty; g.bias = (const float *)(wb + d.bt_off); g.zero_page = wb; g.out = ybuf;
                g.o_cs = d.y_cols; g.o_rs = (long long)c.W * d.y_cols; g.o_bs = (long long)c.H * c.W * d.y_cols;
                TDRN_TRY(launch_conv(g, s));
            }
            ts_y[i] = ybuf; ts_cs[i] = d.y_cols;
        }
        if (n_yq > 0) TDRN_TRY(launch_ygemm_multi(yq, n_yq, dtype, s, p.kdisable));
        return launch_deform_sample_multi(ca, ts_y, ts_cs, n_dargs, s, p.y_tap_major ? 1 : 0);
    }

    // the gather kernel, all pyramid levels in one launch
    int run_deform_gather(const Op &o, hipStream_t s)
    {
        if (o.split) {             // the two branches / the two halves of the groups accumulate into zeroed outputs
            if (zeroed_early) TDRN_HIP_TRY(hipStreamWaitEvent(s, n.ev_zero, 0));
            else TDRN_TRY(zero_split_outputs(o, s));
        }
        if (dargs[0].Npad <= 128) return launch_deform_multi(dargs, n_dargs, s, o.split);
        // the gather kernel holds at most 128 output columns per workgroup (deform.hip): COCO's 12 + 243 columns run as
        // column ranges of 128, each with its own weight rows and output columns (round 5; the C-ABI op does the same)
        for (int c0 = 0; c0 < dargs[0].Cout; c0 += 128) {
            DeformArgs ga[4];
            for (int i = 0; i < n_dargs; ++i) {
                ga[i] = dargs[i];
                const int cols = dargs[i].Cout - c0 < 128 ? dargs[i].Cout - c0 : 128;
                ga[i].Cout = cols; ga[i].Npad = deform_n_pad(cols);
                for (int k = 0; k < ga[i].n_branches; ++k)
                    ga[i].br[k].w = (const char *)dargs[i].br[k].w + (size_t)c0 * dargs[i].br[k].kh * dargs[i].br[k].kw * dargs[i].Cin * p.es;
                if (c0 > 0) { ga[i].out1 += c0 - dargs[i].split; ga[i].split = 0; }
            }
            TDRN_TRY(launch_deform_multi(ga, n_dargs, s, o.split));
        }
        return TDRN_OK;
    }

    int run_op(size_t oi)
    {
        const Op &o = p.ops[oi];
        if (skipped(oi)) return TDRN_OK;
        int lane;
        hipStream_t s;
        TDRN_TRY(stream_for(o, lane, s));
        if (n.profile && !launch_open(o)) TDRN_HIP_TRY(hipEventRecord(n.ev[evi], s));
        const Tensor *ti = o.in >= 0 ? &p.tensors[o.in] : nullptr;
        switch (o.kind) {
            case OP_FIRST:
                TDRN_TRY(ensure_f32_input(s));
                TDRN_TRY(launch_first(o, s));
                break;
            case OP_CONV: TDRN_TRY(o.chain >= 0 ? run_conv_chain(s) : run_conv(oi, s)); break;
            case OP_POOL:
                TDRN_TRY(launch_maxpool2(tptr(o.in), tptr(o.out), B, ti->H, ti->W, ti->Cpad, o.ceil, p.cfg.dtype, s));
                break;
            case OP_L2NORM:
                TDRN_TRY(launch_l2norm(tptr(o.in), (const float *)(wb + o.w_off), tptr(o.out), (long long)B * ti->H * ti->W, ti->Cpad, p.cfg.dtype, s));
                break;
            case OP_DW: TDRN_TRY(run_dw(oi, s)); break;
            case OP_REFLOC_IN:
                if (!io->ref_loc[o.scale]) return TDRN_E_ARG;
                // (tdrn_net_io.reserved[2]: the loc maps are still being produced on another stream -- wait for its event HERE, not
                // at the start of the forward: the trunk above does not depend on them)
                if (io->reserved[2]) TDRN_HIP_TRY(hipStreamWaitEvent(s, (hipEvent_t)io->reserved[2], 0));
                TDRN_TRY(launch_nchw_to_nhwc(io->ref_loc[o.scale], tptr(o.out), Bk, 12, o.hw, 12, TDRN_F32, s));
                break;
            case OP_OFFSET: TDRN_TRY(run_offset(oi, lane, s)); break;
            case OP_DEFORM: TDRN_TRY(run_deform(oi, s)); break;
            case OP_SOFTMAX: TDRN_TRY(launch_softmax_rows(io->conf, io->conf, (long long)B * p.P, C, s)); break;
            case OP_OFF_OUT:
                TDRN_TRY(launch_nhwc_to_nchw_f32((const float *)tptr(o.in), (long long)ti->H * ti->W * ti->C, ti->C, io->offsets[o.scale], Bk, o.Cout,
                                                 ti->H * ti->W, s));
                break;
            case OP_LOC_OUT:
                TDRN_TRY(launch_nhwc_to_nchw_f32(io->arm_loc + (size_t)p.scale_off[o.scale] * 4, (long long)p.P * 4, 12, io->loc_maps[o.scale], B, 12,
                                                 p.fm[o.scale] * p.fm[o.scale], s));
                break;
        }
        offset_ops_enqueued += o.kind == OP_OFFSET;
        if (!launch_open(o)) TDRN_TRY(record(o.out, s));
        TDRN_TRY(record(o.pool_t, s));
        if (n.profile && !launch_open(o)) {
            TDRN_HIP_TRY(hipEventRecord(n.ev[evi + 1], s));
            n.ev_stat.push_back(o.stat);
            n.ev_op.push_back((int)oi);
            evi += 2;
        }
        return TDRN_OK;
    }
};

}  // namespace

int run_forward(tdrn_net &n, const void *blob, void *ws, size_t ws_bytes, const tdrn_net_io *io, hipStream_t s0)
{
    Run r(n, blob, ws, ws_bytes, io, s0);
    TDRN_TRY(r.prologue());
    for (size_t oi = 0; oi < n.ops.size(); ++oi) TDRN_TRY(r.run_op(oi));
    return r.epilogue();
}

}  // namespace tdrn
