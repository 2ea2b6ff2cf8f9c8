// sgd.hip -- one fused fp32 SGD step over a list of tensors (tdrn_hip.h section i-j): what optimizer.step() gives the
// reference's training loops (train.py:259-270, train_trn.py:218-221).  Built with -ffp-contract=off: every operation of the
// update is rounded to fp32 on its own, so the result equals the unfused restatement bit for bit.
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

__device__ __forceinline__ void sgd_vec4(float *p, float *g, float *b, const SgdHyper &h, bool zero_grads)
{
    f32x4 pv = *(const f32x4 *)p, gv = *(const f32x4 *)g, bv = {0.f, 0.f, 0.f, 0.f};
    if (h.mom != 0.f) bv = *(const f32x4 *)b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float pi = pv[i], bi = bv[i];
        sgd_update(pi, gv[i], bi, h);
        pv[i] = pi;
        bv[i] = bi;
    }
    *(f32x4 *)p = pv;
    if (h.mom != 0.f) *(f32x4 *)b = bv;
    if (zero_grads) *(f32x4 *)g = f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ void sgd_scalar(float *p, float *g, float *b, const SgdHyper &h, bool zero_grads)
{
    float pi = *p, bi = h.mom != 0.f ? *b : 0.f;
    sgd_update(pi, *g, bi, h);
    *p = pi;
    if (h.mom != 0.f) *b = bi;
    if (zero_grads) *g = 0.f;
}

__global__ __launch_bounds__(kSgdThreads) void sgd_step_kernel(const SgdBatch batch, int n_tensors, const float *__restrict__ hyper,
                                                               int zero_grads)
{
    const int total = batch.first_chunk[n_tensors];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        int lo = 0, hi = n_tensors;                       // the tensor with first_chunk[t] <= c < first_chunk[t + 1]
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (batch.first_chunk[mid] <= c) lo = mid; else hi = mid;
        }
        const int t = lo;
        const int64_t base = (int64_t)(c - batch.first_chunk[t]) * kSgdChunk;
        const int64_t left = (int64_t)batch.numel[t] - base;
        const int n = left < kSgdChunk ? (int)left : kSgdChunk;
        float *p = batch.p[t] + base, *g = batch.g[t] + base, *b = batch.b[t] + base;
        const float *hg = hyper + 4 * batch.group[t];
        const SgdHyper h = {hg[0], hg[1], hg[2], hg[3] != 0.f};
        // a chunk starts kSgdChunk * 4 bytes into its tensor: it is 16-byte aligned when the tensor is
        const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15) == 0;
        if (vec) {
            if (n == kSgdChunk) {
                // a whole chunk: all of a thread's loads are issued before its first store (p, g and b may alias for all the
                // compiler knows, so it would not move a load over a store itself)
                constexpr int kV = kSgdChunk / (4 * kSgdThreads);
                f32x4 pv[kV], gv[kV], bv[kV];
#pragma unroll
                for (int i = 0; i < kV; ++i) {
                    const int e = (i * kSgdThreads + tid) * 4;
                    pv[i] = *(const f32x4 *)(p + e);
                    gv[i] = *(const f32x4 *)(g + e);
                    bv[i] = h.mom != 0.f ? *(const f32x4 *)(b + e) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int i = 0; i < kV; ++i) {
                    const int e = (i * kSgdThreads + tid) * 4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float pi = pv[i][j], bi = bv[i][j];
                        sgd_update(pi, gv[i][j], bi, h);
                        pv[i][j] = pi;
                        bv[i][j] = bi;
                    }
                    *(f32x4 *)(p + e) = pv[i];
                    if (h.mom != 0.f) *(f32x4 *)(b + e) = bv[i];
                    if (zero_grads) *(f32x4 *)(g + e) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            } else {
                const int nvec = n >> 2;
                for (int v = tid; v < nvec; v += kSgdThreads) sgd_vec4(p + 4 * v, g + 4 * v, b + 4 * v, h, zero_grads != 0);
                const int e = 4 * nvec + tid;             // the tail of numel % 4
                if (e < n) sgd_scalar(p + e, g + e, b + e, h, zero_grads != 0);
            }
        } else {
            for (int e = tid; e < n; e += kSgdThreads) sgd_scalar(p + e, g + e, b + e, h, zero_grads != 0);
        }
    }
}

}  // namespace

int launch_sgd_step(const tdrn_sgd_tensor *tensors, int n_tensors, const float *hyper_dev, int n_groups, int flags, hipStream_t s)
{
    if (!tensors || !hyper_dev || n_tensors < 0 || n_groups < 1 || (flags & ~TDRN_SGD_ZERO_GRADS)) return TDRN_E_ARG;
    bool too_large = false;
    for (int i = 0; i < n_tensors; ++i) {
        const tdrn_sgd_tensor &t = tensors[i];
        if (t.numel < 0 || t.group < 0 || t.group >= n_groups) return TDRN_E_ARG;
        if (t.numel == 0 || !t.grad) continue;            // skipped: nothing else of it is looked at
        if (!t.param || !t.momentum_buf) return TDRN_E_ARG;
        if (t.numel >= ((int64_t)1 << 31)) too_large = true;
    }
    if (too_large) return TDRN_E_UNSUPPORTED;
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
            hipLaunchKernelGGL(sgd_step_kernel, dim3(total < kSgdMaxGrid ? total : kSgdMaxGrid), dim3(kSgdThreads), 0, s, batch, k,
                               hyper_dev, flags & TDRN_SGD_ZERO_GRADS);
            TDRN_HIP_TRY(hipGetLastError());
            k = 0;
        }
    }
    return TDRN_OK;
}

}  // namespace tdrn
