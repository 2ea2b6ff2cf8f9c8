// net.h -- struct tdrn_net: a plan (net_plan.h) plus the runtime state of its forwards.  net.hip owns the handle pool and
// the C ABI, net_run.hip the forward.  Internal to libtdrn_hip.
#pragma once
#include "net_plan.h"

struct tdrn_net : tdrn::Plan {
    tdrn::StagedParams staged;
    bool weights_ready = false;
    int profile = 0;                   // 0 off; 1 = events around every launch, single stream; 2 = the same with the side lanes on
    std::vector<hipEvent_t> ev;
    std::vector<int> ev_stat;
    std::vector<int> ev_op;
    tdrn_kernel_stat stats[tdrn::ST_COUNT];
    int last_batch = 0;
    const void *offs_ws = nullptr;      // ssd4scale deform: the workspace / batch whose offset tensors the last forward filled
    int offs_batch = 0, offs_key_batch = 0;
    int dev = -1;                       // the device the pooled handles below belong to (the one current at the first forward)
    unsigned *status = nullptr;         // host-visible status words (pinned; tdrn_net_check): [0] chained split, [1] chain launch
    // side lanes: created lazily at the first forward
    bool lanes_ready = false;
    hipStream_t side[tdrn::kLanes - 1] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_zero = nullptr, ev_skz = nullptr, ev_join[tdrn::kLanes - 1] = {nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> tensor_ev;
    int first_op = 0;                    // tdrn_net_forward_from: ops below this index are assumed done (analysis only)

    int init_lanes();
    int check_status(unsigned *detail);
    int collect_stats(tdrn_kernel_stat *out, int max_entries);
};

namespace tdrn {
namespace pool {
int cur_dev();
int get_timing_event(int dev, hipEvent_t *e);
int get_status(unsigned **w);
}  // namespace pool
int run_forward(tdrn_net &n, const void *blob, void *ws, size_t ws_bytes, const tdrn_net_io *io, hipStream_t s0);   // net_run.hip
}  // namespace tdrn
