// sgd.hip -- one fused fp32 SGD step over a list of tensors (tdrn_hip.h section i-j): what optimizer.step() gives the
// reference's training loops (train.py:259-270, train_trn.py:218-221); and dynamic loss scaling for fp16 training on top of it
// (section i-m): a check of the gradients for inf / NaN, the same step with the unscale and the skip folded in, and the update of
// the scale, all deciding on the device.  Built with -ffp-contract=off: every operation of the update is rounded to fp32 on its own,
// so the result equals the unfused restatement bit for bit.
//
// Multi-tensor apply with the descriptors in the kernel arguments: a launch carries up to kSgdTensors tensors (pointers, numel,
// group, and a prefix sum of their chunk counts) by value.  A workgroup walks chunks of kSgdChunk elements with a grid stride and
// finds each chunk's tensor by a binary search of the prefix sum; the chunk index comes from blockIdx alone, so the search, the
// descriptor reads and the hyper-parameter reads are wave-uniform (scalar loads).  No atomics, no LDS, no workspace.
#include "common.h"
#include "kernels.h"

namespace tdrn {

namespace {

constexpr int kSgdThreads = 256;
constexpr int kSgdChunk = TDRN_SGD_CHUNK;   // elements per chunk: four 16-byte vectors per thread and array
constexpr int kSgdTensors = TDRN_SGD_TENSORS_PER_LAUNCH;     // 96 * 36 + 4 bytes of descriptors, 3.4 KB of the 4 KB of arguments
constexpr int kSgdMaxGrid = 2048;           // 256 CUs x 8 workgroups; the rest of the chunks are strided over
constexpr int kSgdVecs = kSgdChunk / (4 * kSgdThreads);      // 16-byte vectors per thread and array in a whole chunk

struct SgdBatch {
    float *p[kSgdTensors];
    float *g[kSgdTensors];
    float *b[kSgdTensors];
    int32_t numel[kSgdTensors];
    int32_t group[kSgdTensors];
    int32_t first_chunk[kSgdTensors + 1];   // prefix sum of ceil(numel / kSgdChunk); [n] = the launch's chunk count
};
static_assert(sizeof(SgdBatch) + 32 <= 4096, "the descriptors travel as kernel arguments");
static_assert(kSgdChunk % (4 * kSgdThreads) == 0, "a whole chunk is a whole number of 16-byte vectors per thread");

struct SgdHyper {
    float lr, mom, wd;
    bool nesterov;
};

// What the scaled step (i-m) does to a gradient on its way into the update, and whether the step writes at all.  A template
// parameter of everything below, so that the plain step's code stays what it was.
template <bool kScaled> struct SgdScale;
template <> struct SgdScale<false> {
    __device__ __forceinline__ float grad(float g) const { return g; }
    __device__ __forceinline__ bool writes() const { return true; }
};
template <> struct SgdScale<true> {
    float inv;                              // 1 / scale
    bool skip;                              // found_inf != 0: p and b keep their bits
    __device__ __forceinline__ float grad(float g) const { return g * inv; }
    __device__ __forceinline__ bool writes() const { return !skip; }
};

// the four lines of tdrn_hip.h (i-j); -ffp-contract=off keeps each product and sum a rounding of its own
__device__ __forceinline__ void sgd_update(float &p, float g, float &b, const SgdHyper &h)
{
    float d = h.wd != 0.f ? g + h.wd * p : g;
    float u = d;
    if (h.mom != 0.f) {
        b = h.mom * b + d;
        u = h.nesterov ? d + h.mom * b : b;
    }
    p = p - h.lr * u;
}

template <bool kScaled>
__device__ __forceinline__ void sgd_vec4(float *p, float *g, float *b, const SgdHyper &h, const SgdScale<kScaled> &sc, bool zero_grads)
{
    f32x4 pv = *(const f32x4 *)p, gv = *(const f32x4 *)g, bv = {0.f, 0.f, 0.f, 0.f};
    if (h.mom != 0.f) bv = *(const f32x4 *)b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float pi = pv[i], bi = bv[i];
        sgd_update(pi, sc.grad(gv[i]), bi, h);
        pv[i] = pi;
        bv[i] = bi;
    }
    if (sc.writes()) {
        *(f32x4 *)p = pv;
        if (h.mom != 0.f) *(f32x4 *)b = bv;
    }
    if (zero_grads) *(f32x4 *)g = f32x4{0.f, 0.f, 0.f, 0.f};
}

template <bool kScaled>
__device__ __forceinline__ void sgd_scalar(float *p, float *g, float *b, const SgdHyper &h, const SgdScale<kScaled> &sc, bool zero_grads)
{
    float pi = *p, bi = h.mom != 0.f ? *b : 0.f;
    sgd_update(pi, sc.grad(*g), bi, h);
    if (sc.writes()) {
        *p = pi;
        if (h.mom != 0.f) *b = bi;
    }
    if (zero_grads) *g = 0.f;
}

// The walk every kernel of this file shares: chunk c of the launch, for c = blockIdx.x, + gridDim.x, ..., belongs to the tensor t
// with first_chunk[t] <= c < first_chunk[t + 1]; body(t, base, n) gets the chunk's first element and its length.
template <class Body> __device__ __forceinline__ void sgd_walk_chunks(const SgdBatch &batch, int n_tensors, Body body)
{
    const int total = batch.first_chunk[n_tensors];
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        int lo = 0, hi = n_tensors;
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (batch.first_chunk[mid] <= c) lo = mid; else hi = mid;
        }
        const int t = lo;
        const int64_t base = (int64_t)(c - batch.first_chunk[t]) * kSgdChunk;
        const int64_t left = (int64_t)batch.numel[t] - base;
        body(t, base, left < kSgdChunk ? (int)left : kSgdChunk);
    }
}

template <bool kScaled>
__device__ __forceinline__ void sgd_step_body(const SgdBatch &batch, int n_tensors, const float *__restrict__ hyper,
                                              const SgdScale<kScaled> &sc, int zero_grads)
{
    const int tid = threadIdx.x;
    sgd_walk_chunks(batch, n_tensors, [&](int t, int64_t base, int n) {
        float *p = batch.p[t] + base, *g = batch.g[t] + base, *b = batch.b[t] + base;
        const float *hg = hyper + 4 * batch.group[t];
        const SgdHyper h = {hg[0], hg[1], hg[2], hg[3] != 0.f};
        // a chunk starts kSgdChunk * 4 bytes into its tensor: it is 16-byte aligned when the tensor is
        const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15) == 0;
        if (vec) {
            if (n == kSgdChunk) {
                // a whole chunk: all of a thread's loads are issued before its first store (p, g and b may alias for all the
                // compiler knows, so it would not move a load over a store itself)
                f32x4 pv[kSgdVecs], gv[kSgdVecs], bv[kSgdVecs];
#pragma unroll
                for (int i = 0; i < kSgdVecs; ++i) {
                    const int e = (i * kSgdThreads + tid) * 4;
                    pv[i] = *(const f32x4 *)(p + e);
                    gv[i] = *(const f32x4 *)(g + e);
                    bv[i] = h.mom != 0.f ? *(const f32x4 *)(b + e) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int i = 0; i < kSgdVecs; ++i) {
                    const int e = (i * kSgdThreads + tid) * 4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float pi = pv[i][j], bi = bv[i][j];
                        sgd_update(pi, sc.grad(gv[i][j]), bi, h);
                        pv[i][j] = pi;
                        bv[i][j] = bi;
                    }
                    if (sc.writes()) {
                        *(f32x4 *)(p + e) = pv[i];
                        if (h.mom != 0.f) *(f32x4 *)(b + e) = bv[i];
                    }
                    if (zero_grads) *(f32x4 *)(g + e) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            } else {
                const int nvec = n >> 2;
                for (int v = tid; v < nvec; v += kSgdThreads) sgd_vec4(p + 4 * v, g + 4 * v, b + 4 * v, h, sc, zero_grads != 0);
                const int e = 4 * nvec + tid;             // the tail of numel % 4
                if (e < n) sgd_scalar(p + e, g + e, b + e, h, sc, zero_grads != 0);
            }
        } else {
            for (int e = tid; e < n; e += kSgdThreads) sgd_scalar(p + e, g + e, b + e, h, sc, zero_grads != 0);
        }
    });
}

__global__ __launch_bounds__(kSgdThreads) void sgd_step_kernel(const SgdBatch batch, int n_tensors, const float *__restrict__ hyper,
                                                               int zero_grads)
{
    sgd_step_body(batch, n_tensors, hyper, SgdScale<false>{}, zero_grads);
}

// ---- dynamic loss scaling (tdrn_hip.h section i-m): state = {scale, good_steps, found_inf, skipped} ---------------------------------

__device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }   // +-inf, NaN

__device__ __forceinline__ bool not_finite(const f32x4 &v)
{
    return not_finite(v[0]) || not_finite(v[1]) || not_finite(v[2]) || not_finite(v[3]);
}

// The step with g / scale in g's place, and no write to p or b of any tensor when a check has raised found_inf.  state is read as
// hyper is: the address is the same for every lane, so the loads are scalar; one division per workgroup.
__global__ __launch_bounds__(kSgdThreads) void sgd_step_scaled_kernel(const SgdBatch batch, int n_tensors,
                                                                      const float *__restrict__ hyper,
                                                                      const float *__restrict__ state, int zero_grads)
{
    SgdScale<true> sc;
    sc.inv = 1.0f / state[0];
    sc.skip = state[2] != 0.f;
    sgd_step_body(batch, n_tensors, hyper, sc, zero_grads);
}

// Reads every gradient element once, on the step's paths (whole chunk, vectors + tail, scalars off the 16-byte grid, where only g
// counts here), and raises state[2] when one is inf or NaN.  It never lowers it: the flag stays up until amp_update_kernel, so two
// lists may be checked into one state.  Every writer stores the same word, so the store is an ordinary one.
__global__ __launch_bounds__(kSgdThreads) void grad_check_finite_kernel(const SgdBatch batch, int n_tensors, float *state)
{
    const int tid = threadIdx.x;
    bool bad = false;
    sgd_walk_chunks(batch, n_tensors, [&](int t, int64_t base, int n) {
        const float *g = batch.g[t] + base;
        if (((uintptr_t)g & 15) == 0) {
            if (n == kSgdChunk) {
                f32x4 gv[kSgdVecs];
#pragma unroll
                for (int i = 0; i < kSgdVecs; ++i) gv[i] = *(const f32x4 *)(g + (i * kSgdThreads + tid) * 4);
#pragma unroll
                for (int i = 0; i < kSgdVecs; ++i) bad |= not_finite(gv[i]);
            } else {
                const int nvec = n >> 2;
                for (int v = tid; v < nvec; v += kSgdThreads) bad |= not_finite(*(const f32x4 *)(g + 4 * v));
                const int e = 4 * nvec + tid;             // the tail of numel % 4
                if (e < n) bad |= not_finite(g[e]);
            }
        } else {
            for (int e = tid; e < n; e += kSgdThreads) bad |= not_finite(g[e]);
        }
    });
    const bool wave_bad = __ballot(bad) != 0ull;          // every lane of the wave is here: the walk is uniform per workgroup
    if (wave_bad && (tid & 63) == 0) state[2] = 1.0f;
}

// torch's _amp_update_scale_ on the four words, one lane
__global__ void amp_update_kernel(float *state, float growth, float backoff, float interval)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float scale = state[0], good = state[1], skipped = state[3];
    if (state[2] != 0.f) {
        scale = scale * backoff;
        good = 0.f;
        skipped = skipped + 1.f;
    } else {
        good = good + 1.f;
        if (good == interval) {
            const float s = scale * growth;
            if (!not_finite(s)) scale = s;
            good = 0.f;
        }
    }
    state[0] = scale;
    state[1] = good;
    state[2] = 0.f;
    state[3] = skipped;
}

// ---- host: one check of the records and one packing loop for the three multi-tensor launchers ---------------------------------------

// the record errors of (i-j), in its order.  n_groups < 0: the entry has no hyper-parameter rows, any group >= 0 goes;
// need_param: param and momentum_buf of a record that is not skipped must not be null
int check_records(const tdrn_sgd_tensor *tensors, int n_tensors, int n_groups, bool need_param)
{
    bool too_large = false;
    for (int i = 0; i < n_tensors; ++i) {
        const tdrn_sgd_tensor &t = tensors[i];
        if (t.numel < 0 || t.group < 0 || (n_groups >= 0 && t.group >= n_groups)) return TDRN_E_ARG;
        if (t.numel == 0 || !t.grad) continue;            // skipped: nothing else of it is looked at
        if (need_param && (!t.param || !t.momentum_buf)) return TDRN_E_ARG;
        if (t.numel >= ((int64_t)1 << 31)) too_large = true;
    }
    return too_large ? TDRN_E_UNSUPPORTED : TDRN_OK;
}

bool bad_state(const float *state_dev) { return !state_dev || ((uintptr_t)state_dev & 15) != 0; }

// Packs the records that are not skipped into batches of up to kSgdTensors and calls launch(batch, k, grid) for each.
template <class Launch> int for_each_batch(const tdrn_sgd_tensor *tensors, int n_tensors, Launch launch)
{
    SgdBatch batch;
    int k = 0;
    batch.first_chunk[0] = 0;
    for (int i = 0; i <= n_tensors; ++i) {
        if (i < n_tensors) {
            const tdrn_sgd_tensor &t = tensors[i];
            if (t.numel == 0 || !t.grad) continue;
            batch.p[k] = t.param;
            batch.g[k] = t.grad;
            batch.b[k] = t.momentum_buf;
            batch.numel[k] = (int32_t)t.numel;
            batch.group[k] = t.group;
            batch.first_chunk[k + 1] = batch.first_chunk[k] + (int32_t)((t.numel + kSgdChunk - 1) / kSgdChunk);
            ++k;
        }
        if (k == kSgdTensors || (i == n_tensors && k > 0)) {
            // at most 96 * 2^19 chunks: the prefix sum stays inside int32
            const int total = batch.first_chunk[k];
            for (int j = k; j < kSgdTensors; ++j) {       // unused slots: defined values, never read
                batch.p[j] = batch.g[j] = batch.b[j] = nullptr;
                batch.numel[j] = batch.group[j] = 0;
                batch.first_chunk[j + 1] = total;
            }
            launch(batch, k, dim3(total < kSgdMaxGrid ? total : kSgdMaxGrid));
            TDRN_HIP_TRY(hipGetLastError());
            k = 0;
        }
    }
    return TDRN_OK;
}

}  // namespace

int launch_sgd_step(const tdrn_sgd_tensor *tensors, int n_tensors, const float *hyper_dev, int n_groups, int flags, hipStream_t s)
{
    if (!tensors || !hyper_dev || n_tensors < 0 || n_groups < 1 || (flags & ~TDRN_SGD_ZERO_GRADS)) return TDRN_E_ARG;
    if (int rc = check_records(tensors, n_tensors, n_groups, true)) return rc;
    return for_each_batch(tensors, n_tensors, [&](const SgdBatch &batch, int k, dim3 grid) {
        hipLaunchKernelGGL(sgd_step_kernel, grid, dim3(kSgdThreads), 0, s, batch, k, hyper_dev, flags & TDRN_SGD_ZERO_GRADS);
    });
}

int launch_sgd_step_scaled(const tdrn_sgd_tensor *tensors, int n_tensors, const float *hyper_dev, int n_groups,
                           const float *state_dev, int flags, hipStream_t s)
{
    if (!tensors || !hyper_dev || n_tensors < 0 || n_groups < 1 || bad_state(state_dev) || (flags & ~TDRN_SGD_ZERO_GRADS))
        return TDRN_E_ARG;
    if (int rc = check_records(tensors, n_tensors, n_groups, true)) return rc;
    return for_each_batch(tensors, n_tensors, [&](const SgdBatch &batch, int k, dim3 grid) {
        hipLaunchKernelGGL(sgd_step_scaled_kernel, grid, dim3(kSgdThreads), 0, s, batch, k, hyper_dev, state_dev,
                           flags & TDRN_SGD_ZERO_GRADS);
    });
}

int launch_amp_check_finite(const tdrn_sgd_tensor *tensors, int n_tensors, float *state_dev, hipStream_t s)
{
    if (!tensors || n_tensors < 0 || bad_state(state_dev)) return TDRN_E_ARG;
    if (int rc = check_records(tensors, n_tensors, -1, false)) return rc;
    return for_each_batch(tensors, n_tensors, [&](const SgdBatch &batch, int k, dim3 grid) {
        hipLaunchKernelGGL(grad_check_finite_kernel, grid, dim3(kSgdThreads), 0, s, batch, k, state_dev);
    });
}

int launch_amp_update(float *state_dev, float growth_factor, float backoff_factor, int growth_interval, hipStream_t s)
{
    if (bad_state(state_dev)) return TDRN_E_ARG;
    if (!(growth_factor > 1.f) || !(backoff_factor > 0.f && backoff_factor < 1.f)) return TDRN_E_ARG;      // NaN fails both
    if (growth_interval < 1 || growth_interval >= (1 << 24)) return TDRN_E_ARG;    // the count is an fp32 word: exact below 2^24
    hipLaunchKernelGGL(amp_update_kernel, dim3(1), dim3(1), 0, s, state_dev, growth_factor, backoff_factor, (float)growth_interval);
    TDRN_HIP_TRY(hipGetLastError());
    return TDRN_OK;
}

}  // namespace tdrn
