// net.hip -- struct tdrn_net (net.h): the pooled streams / events of its forwards, the profiler's bookkeeping and the C ABI
// of tdrn_hip.h section (iii).  The plan is built in net_plan.hip, packed in net_pack.hip and run in net_run.hip.
#include <cstring>
#include <mutex>

#include "net.h"

namespace tdrn {

// Side-lane streams and no-timing events are POOLED per process instead of destroyed with their net: a hipGraph captured for
// a net created after another net's streams / events had been destroyed crashed inside hipGraphLaunch (ROCm 7.2; reproduced
// with bench.py's three engines: a 16-bit engine destroyed, then the fp32 engine's step captured and replayed).  A net takes
// them from the pool and hands them back in tdrn_net_destroy; nothing in the pool is ever in use by two nets at a time.
namespace pool {
// (keyed by device: a net created while device 1 is current must not inherit device 0's handles)
std::mutex mu;
std::map<int, std::vector<hipStream_t>> streams;
std::map<int, std::vector<hipEvent_t>> events;
std::map<int, std::vector<hipEvent_t>> timing_events;
std::vector<unsigned *> status_words;      // pinned, device-mapped host memory (visible to every device): 64 bytes each
int cur_dev()
{
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
}
template <class H, class Create>
int get(std::map<int, std::vector<H>> &m, int dev, H *h, Create create)
{
    {
        std::lock_guard<std::mutex> g(mu);
        auto &v = m[dev];
        if (!v.empty()) { *h = v.back(); v.pop_back(); return TDRN_OK; }
    }
    return hip_status(create(h));
}
template <class H>
void put(std::map<int, std::vector<H>> &m, int dev, H h) { if (h) { std::lock_guard<std::mutex> g(mu); m[dev].push_back(h); } }
int get_stream(int dev, hipStream_t *s) { return get(streams, dev, s, [](hipStream_t *p) { return hipStreamCreateWithFlags(p, hipStreamNonBlocking); }); }
int get_event(int dev, hipEvent_t *e) { return get(events, dev, e, [](hipEvent_t *p) { return hipEventCreateWithFlags(p, hipEventDisableTiming); }); }
int get_timing_event(int dev, hipEvent_t *e) { return get(timing_events, dev, e, [](hipEvent_t *p) { return hipEventCreate(p); }); }
int get_status(unsigned **w)
{
    {
        std::lock_guard<std::mutex> g(mu);
        if (!status_words.empty()) { *w = status_words.back(); status_words.pop_back(); memset(*w, 0, 64); return TDRN_OK; }
    }
    void *p = nullptr;
    TDRN_HIP_TRY(hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocPortable));
    memset(p, 0, 64);
    *w = (unsigned *)p;
    return TDRN_OK;
}
void put_status(unsigned *w) { if (w) { std::lock_guard<std::mutex> g(mu); status_words.push_back(w); } }
}  // namespace pool

namespace {
const char *kStatNames[] = {"conv_igemm_mfma", "first_conv", "maxpool2x2", "l2norm", "dwconv3x3", "offset_conv1x1",
                            "deform_gemm_mfma", "softmax21", "layout", "conv3x3_patch_mfma", "dwpw_mfma"};
}  // namespace
}  // namespace tdrn

using namespace tdrn;

int tdrn_net::init_lanes()
{
    if (lanes_ready) return TDRN_OK;
    for (int i = 0; i < kLanes - 1; ++i) {
        TDRN_TRY(pool::get_stream(dev, &side[i]));
        TDRN_TRY(pool::get_event(dev, &ev_join[i]));
    }
    TDRN_TRY(pool::get_event(dev, &ev_fork));
    TDRN_TRY(pool::get_event(dev, &ev_zero));
    TDRN_TRY(pool::get_event(dev, &ev_skz));
    tensor_ev.assign(tensors.size(), nullptr);
    for (size_t t = 0; t < tensors.size(); ++t)
        if (tensor_shared[t]) TDRN_TRY(pool::get_event(dev, &tensor_ev[t]));
    lanes_ready = true;
    return TDRN_OK;
}

int tdrn_net::check_status(unsigned *detail)
{
    unsigned d = 0;
    if (status) {
        volatile unsigned *w = status;
        d = (w[0] ? 1u : 0u) | (w[1] ? 2u : 0u);
        if (d) { w[0] = 0; w[1] = 0; }
    }
    if (detail) *detail = d;
    return d ? TDRN_E_DEVICE : TDRN_OK;
}

int tdrn_net::collect_stats(tdrn_kernel_stat *out, int max_entries)
{
    for (int i = 0; i < ST_COUNT; ++i) {
        memset(&stats[i], 0, sizeof(stats[i]));
        strncpy(stats[i].name, kStatNames[i], sizeof(stats[i].name) - 1);
    }
    for (size_t i = 0; i < ops.size(); ++i) {
        const Op &o = ops[i];
        if (launch_head(i)) stats[o.stat].launches += 1;
        stats[o.stat].flops += o.flops * last_batch;
        stats[o.stat].bytes += o.bytes * last_batch;
    }
    for (size_t i = 0; i < ev_stat.size(); ++i) {
        float ms = 0.f;
        TDRN_HIP_TRY(hipEventSynchronize(ev[2 * i + 1]));
        TDRN_HIP_TRY(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
        stats[ev_stat[i]].ms += ms;
    }
    int n = 0;
    for (int i = 0; i < ST_COUNT && n < max_entries; ++i)
        if (stats[i].launches) out[n++] = stats[i];
    return n;
}

// ---- C ABI (tdrn_hip.h section iii) ------------------------------------------------------------
extern "C" {

int tdrn_net_create(const tdrn_net_config *cfg, tdrn_net **out)
{
    if (!cfg || !out) return TDRN_E_ARG;
    tdrn_net *n = new tdrn_net();
    n->cfg = *cfg;
    const int rc = n->build();
    if (rc != TDRN_OK) {
        delete n;
        return rc;
    }
    *out = n;
    return TDRN_OK;
}

void tdrn_net_destroy(tdrn_net *net)
{
    if (!net) return;
    const int d = net->dev;
    for (hipEvent_t e : net->ev) pool::put(pool::timing_events, d, e);         // (timing events of the profiling passes: never captured; pooled like the rest)
    for (hipEvent_t e : net->tensor_ev) pool::put(pool::events, d, e);
    for (int i = 0; i < kLanes - 1; ++i) {
        pool::put(pool::events, d, net->ev_join[i]);
        pool::put(pool::streams, d, net->side[i]);
    }
    pool::put(pool::events, d, net->ev_fork);
    pool::put(pool::events, d, net->ev_zero);
    pool::put(pool::events, d, net->ev_skz);
    pool::put_status(net->status);
    delete net;
}

int tdrn_net_param_count(const tdrn_net *net) { return net ? (int)net->params.size() : TDRN_E_ARG; }

int tdrn_net_param_info(const tdrn_net *net, int index, const char **name, int64_t shape[4], int *ndim)
{
    if (!net || index < 0 || index >= (int)net->params.size()) return TDRN_E_ARG;
    const ParamSpec &p = net->params[index];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = (int)p.shape.size();
    if (shape)
        for (size_t i = 0; i < 4; ++i) shape[i] = i < p.shape.size() ? p.shape[i] : 1;
    return TDRN_OK;
}

int tdrn_net_set_param(tdrn_net *net, const char *name, const float *data_host, int64_t numel)
{
    if (!net || !name || !data_host) return TDRN_E_ARG;
    auto it = net->param_index.find(name);
    if (it == net->param_index.end()) return TDRN_E_PARAM;
    int64_t want = 1;
    for (int64_t d : net->params[it->second].shape) want *= d;
    if (want != numel) return TDRN_E_PARAM;
    net->staged[name].assign(data_host, data_host + numel);
    net->weights_ready = false;
    return TDRN_OK;
}

size_t tdrn_net_weight_bytes(const tdrn_net *net) { return net ? net->blob_bytes : 0; }
size_t tdrn_net_workspace_bytes(const tdrn_net *net, int batch) { return net && batch > 0 ? net->ws_per_sample * (size_t)batch + net->ws_fixed : 0; }
int tdrn_net_num_priors(const tdrn_net *net) { return net ? net->P : TDRN_E_ARG; }

int tdrn_net_pack_weights(tdrn_net *net, void *weights_dev, size_t weights_bytes, void *stream)
{
    if (!net || !weights_dev) return TDRN_E_ARG;
    if (weights_bytes < net->blob_bytes) return TDRN_E_WORKSPACE;
    for (const ParamSpec &p : net->params)
        if (!net->staged.count(p.name)) return TDRN_E_PARAM;
    std::vector<char> host;
    TDRN_TRY(pack_weights(*net, net->staged, host));
    hipStream_t s = (hipStream_t)stream;
    TDRN_HIP_TRY(hipMemcpyAsync(weights_dev, host.data(), host.size(), hipMemcpyHostToDevice, s));
    TDRN_HIP_TRY(hipStreamSynchronize(s));
    net->weights_ready = true;
    net->staged.clear();   // the fp32 staging copy is no longer needed
    return TDRN_OK;
}

int tdrn_net_adopt_weights(tdrn_net *net)
{
    if (!net) return TDRN_E_ARG;
    net->weights_ready = true;
    return TDRN_OK;
}

int tdrn_net_forward(tdrn_net *net, const void *weights_dev, void *workspace, size_t workspace_bytes, const tdrn_net_io *io,
                     void *stream)
{
    if (!net) return TDRN_E_ARG;
    return run_forward(*net, weights_dev, workspace, workspace_bytes, io, (hipStream_t)stream);
}

int tdrn_net_check(tdrn_net *net, unsigned *detail)
{
    if (!net) return TDRN_E_ARG;
    return net->check_status(detail);
}

int tdrn_net_op_count(const tdrn_net *net) { return net ? (int)net->ops.size() : TDRN_E_ARG; }

int tdrn_net_op_info(const tdrn_net *net, int index, tdrn_op_info *out)
{
    if (!net || !out || index < 0 || index >= (int)net->ops.size()) return TDRN_E_ARG;
    const Op &o = net->ops[index];
    memset(out, 0, sizeof(*out));
    switch (o.kind) {
        case OP_FIRST: out->kind = 0; break;
        case OP_CONV: out->kind = o.phases == 4 ? 2 : 1; break;
        case OP_DW: out->kind = 3; break;
        case OP_POOL: out->kind = 4; break;
        case OP_L2NORM: out->kind = 5; break;
        case OP_OFFSET: out->kind = 6; break;
        case OP_DEFORM: out->kind = 7; break;
        default: out->kind = 8; break;
    }
    out->in = o.in; out->out = o.out; out->res = o.res; out->pool = o.pool_t; out->off = o.off_t; out->y = o.y_t;
    out->k = o.k; out->stride = o.stride; out->pad = o.pad; out->dil = o.dil; out->relu = o.relu; out->ceil_mode = o.ceil;
    out->splitk = o.splitk; out->groups = o.G; out->out_kind = o.out_kind; out->level = o.scale;
    out->n_branches = o.n_branches; out->k2 = o.k2; out->pad2 = o.pad2; out->off_c0[0] = o.off_c0[0]; out->off_c0[1] = o.off_c0[1];
    if (o.kind == OP_DEFORM && o.y_t >= 0) {
        out->y_tap_major = net->y_tap_major ? 1 : 0;
        out->y_groups = o.y_groups;
    }
    out->fused_first = (index == net->fuse_first) ? 1 : 0;
    out->fused_dw = o.fused_dw;
    auto cp = [](char *d, const std::string &v) { strncpy(d, v.c_str(), 47); };
    cp(out->w, o.w); cp(out->b, o.b); cp(out->bn, o.bn); cp(out->w2, o.w2); cp(out->b2, o.b2);
    return TDRN_OK;
}

int tdrn_net_tensor_count(const tdrn_net *net) { return net ? (int)net->tensors.size() : TDRN_E_ARG; }

int tdrn_net_tensor_info(const tdrn_net *net, int index, const char **label, int *C, int *H, int *W)
{
    if (!net || index < 0 || index >= (int)net->tensors.size()) return TDRN_E_ARG;
    const Tensor &t = net->tensors[index];
    if (label) *label = t.label.c_str();
    if (C) *C = t.C;
    if (H) *H = t.H;
    if (W) *W = t.W;
    return TDRN_OK;
}

int tdrn_net_read_tensor(const tdrn_net *net, const void *workspace, int batch, int index, float *out_dev, void *stream)
{
    if (!net || !workspace || !out_dev || batch <= 0 || index < 0 || index >= (int)net->tensors.size()) return TDRN_E_ARG;
    const Tensor &t = net->tensors[index];
    return launch_nhwc_any_to_nchw_f32((const char *)workspace + t.off * (size_t)batch, t.f32 ? TDRN_F32 : net->cfg.dtype,
                                       t.Cpad, out_dev, batch, t.C, t.H * t.W, (hipStream_t)stream);
}

int tdrn_net_write_tensor(const tdrn_net *net, void *workspace, int batch, int index, const float *in_dev, void *stream)
{
    if (!net || !workspace || !in_dev || batch <= 0 || index < 0 || index >= (int)net->tensors.size()) return TDRN_E_ARG;
    const Tensor &t = net->tensors[index];
    return launch_nchw_to_nhwc(in_dev, (char *)workspace + t.off * (size_t)batch, batch, t.C, t.H * t.W, t.Cpad,
                               t.f32 ? TDRN_F32 : net->cfg.dtype, (hipStream_t)stream);
}

int tdrn_net_forward_from(tdrn_net *net, const void *weights_dev, void *workspace, size_t workspace_bytes, const tdrn_net_io *io,
                          int first_op, void *stream)
{
    if (!net || first_op < 0 || first_op > (int)net->ops.size()) return TDRN_E_ARG;
    if (net->use_lanes) return TDRN_E_STATE;
    net->first_op = first_op;
    const int rc = run_forward(*net, weights_dev, workspace, workspace_bytes, io, (hipStream_t)stream);
    net->first_op = 0;
    return rc;
}

int tdrn_net_profile(tdrn_net *net, int enable)
{
    if (!net) return TDRN_E_ARG;
    net->profile = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return TDRN_OK;
}

int tdrn_net_op_stats(tdrn_net *net, tdrn_kernel_stat *out, int max_entries)
{
    if (!net || !out || max_entries <= 0) return TDRN_E_ARG;
    int n = 0;
    for (size_t i = 0; i < net->ev_op.size() && n < max_entries; ++i) {
        const Op &o = net->ops[net->ev_op[i]];
        float ms = 0.f;
        TDRN_HIP_TRY(hipEventSynchronize(net->ev[2 * i + 1]));
        TDRN_HIP_TRY(hipEventElapsedTime(&ms, net->ev[2 * i], net->ev[2 * i + 1]));
        tdrn_kernel_stat &k = out[n++];
        memset(&k, 0, sizeof(k));
        std::string name = std::string(kStatNames[o.stat]) + ":" + (o.w.empty() ? (o.in >= 0 ? net->tensors[o.in].label : "") : o.w);
        if (o.kind == OP_CONV && o.chain == 0) name = "conv_chain:" + o.w + "+" + std::to_string(net->chain_ops.size() - 1);
        strncpy(k.name, name.c_str(), sizeof(k.name) - 1);
        k.launches = 1;
        k.flops = o.flops * net->last_batch;
        k.bytes = o.bytes * net->last_batch;
        if (o.kind == OP_CONV && o.chain == 0)      // one launch covers all members
            for (size_t j = 1; j < net->chain_ops.size(); ++j) {
                k.flops += net->ops[net->chain_ops[j]].flops * net->last_batch;
                k.bytes += net->ops[net->chain_ops[j]].bytes * net->last_batch;
            }
        if (o.kind == OP_DEFORM)   // one launch covers the preceding deform ops of the other pyramid levels
            for (int j = net->ev_op[i] - 1; j >= 0 && net->ops[j].kind == OP_DEFORM; --j) {
                k.flops += net->ops[j].flops * net->last_batch;
                k.bytes += net->ops[j].bytes * net->last_batch;
            }
        k.ms = ms;
    }
    return n;
}

int tdrn_net_op_timeline(tdrn_net *net, float *start_ms, float *end_ms, int *lane, int max_entries)
{
    if (!net || !start_ms || !end_ms || max_entries <= 0) return TDRN_E_ARG;
    int n = 0;
    for (size_t i = 0; i < net->ev_op.size() && n < max_entries; ++i, ++n) {
        TDRN_HIP_TRY(hipEventSynchronize(net->ev[2 * i + 1]));
        TDRN_HIP_TRY(hipEventElapsedTime(&start_ms[n], net->ev[0], net->ev[2 * i]));
        TDRN_HIP_TRY(hipEventElapsedTime(&end_ms[n], net->ev[0], net->ev[2 * i + 1]));
        if (lane) lane[n] = net->profile == 2 && net->use_lanes ? net->ops[net->ev_op[i]].lane : 0;
    }
    return n;
}

int tdrn_net_kernel_stats(tdrn_net *net, tdrn_kernel_stat *out, int max_entries)
{
    if (!net || !out || max_entries <= 0) return TDRN_E_ARG;
    return net->collect_stats(out, max_entries);
}

}  // extern "C"
