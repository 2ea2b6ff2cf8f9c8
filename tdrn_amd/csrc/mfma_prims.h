// mfma_prims.h -- the device-side building blocks the MFMA kernels share (conv_igemm, conv3x3_patch, conv3x3_pp, conv3x3_ws,
// head3x3, dwpw, deform): MFMA wrappers, LDS-DMA issue, barrier / wait idioms, the per-XCD item split.  Every helper is
// __device__ __forceinline__: a kernel that uses one compiles to the instructions it had with a private copy.
#pragma once
#include "common.h"

namespace tdrn {

// ---- MFMA ------------------------------------------------------------------------------------
// c += A(32 x K) * B(K x 32) on 16 bytes of K per lane: 16-bit types one v_mfma_f32_32x32x16, fp32 four v_mfma_f32_32x32x2
// (lane half h holds k = 4*(2kk+h)+j of the 128-byte row; A and B use the same map, so the four x2 MFMAs cover each k exactly
// once: an exact fp32 FMA chain).
template <typename DT> struct Mma32;
template <> struct Mma32<bf16_t> {
    __device__ static __forceinline__ void run(const u32x4 &a, const u32x4 &b, f32x16 &c)
    { c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(i16x8, a), __builtin_bit_cast(i16x8, b), c, 0, 0, 0); }
};
template <> struct Mma32<f16_t> {
    __device__ static __forceinline__ void run(const u32x4 &a, const u32x4 &b, f32x16 &c)
    { c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0); }
};
template <> struct Mma32<float> {
    __device__ static __forceinline__ void run(const u32x4 &a, const u32x4 &b, f32x16 &c)
    {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[j]), __uint_as_float(b[j]), c, 0, 0, 0);
    }
};
// 16 x 16 tiles, 32 of K per instruction (16-bit types only)
template <typename DT> struct Mma16;
template <> struct Mma16<bf16_t> {
    __device__ static __forceinline__ f32x4 run(const u32x4 &a, const u32x4 &b, const f32x4 &c)
    { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(i16x8, a), __builtin_bit_cast(i16x8, b), c, 0, 0, 0); }
};
template <> struct Mma16<f16_t> {
    __device__ static __forceinline__ f32x4 run(const u32x4 &a, const u32x4 &b, const f32x4 &c)
    { return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0); }
};

// ---- LDS-DMA ---------------------------------------------------------------------------------
// One LDS-DMA piece (64 lanes x 16 B -> 1 KiB of LDS at lds_dst + 16*lane; lds_dma4: x 4 B -> 256 B at lds_dst + 4*lane) from
// a wave-uniform base plus a 32-bit per-lane byte offset.  Inline asm on purpose: (1) no 64-bit per-lane address arithmetic
// (the accumulators need the registers), (2) hipcc's waitcnt pass does not see it, so it cannot put an `s_waitcnt vmcnt(0)`
// in front of the LDS accesses that follow (cdna_hip_programming.md 5.7 item 1) -- the completion is counted by hand: the
// kernel's own vmcnt(N).  M0 is written in the statement that uses it and restored.  Lanes switched off by the caller's
// branch write nothing.
__device__ __forceinline__ void lds_dma16(const char *sbase, unsigned voff, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}
__device__ __forceinline__ void lds_dma4(const char *sbase, unsigned voff, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}
// The same 1-KiB piece from a per-lane pointer through the compiler's builtin (its waitcnt pass sees this one): dst is the
// piece's wave-uniform LDS base.  COH = agent-coherent access (the `sc1` cache-policy bit: served by / written through to the
// memory side, past the XCD's own L2).
template <bool COH = false>
__device__ __forceinline__ void lds_dma16_ptr(const char *src, char *dst)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)dst, 16, 0, COH ? 16 : 0);
}
// LDS byte address of a __shared__ object (what lds_dma16 / lds_dma4 take as lds_dst)
__device__ __forceinline__ unsigned lds_addr(const void *p)
{
    return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const char *)p;
}

// ---- barrier and waits -----------------------------------------------------------------------
// raw workgroup barrier (all waves of the workgroup take part; nothing may move across it)
__device__ __forceinline__ void wg_barrier()
{
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
// `s_waitcnt vmcnt(n)` for a wave-uniform run-time n (the instruction takes an immediate); n > 14 waits for 14
__device__ __forceinline__ void wait_vmcnt(int n)
{
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
        case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
    }
}
// A copy of v the compiler knows nothing about.  The register-tight kernels derive the lane constants of their rarely
// executed code paths (staging, epilogue) from opaque(lane) where they are used: hipcc otherwise hoists every loop-invariant
// lane expression out of the main loop and then spills it -- re-loaded behind an `s_waitcnt vmcnt(0)` that would drain the
// LDS-DMA pipeline.
__device__ __forceinline__ int opaque(int v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// ---- per-XCD item split ----------------------------------------------------------------------
// Persistent kernels (grid = persistent_grid(items), kernels.h): each XCD label (blockIdx % 8) owns a contiguous range of
// `per_xcd` items -- `avail` of them exist -- so that neighbouring items share its L2; workgroup `slot` of the XCD's
// `istride` runs items item0(), item0() + istride, ... (n_items() of them).
struct XcdItems {
    int xcd, slot, per_xcd, istride, avail;
    __device__ __forceinline__ int n_items() const { return avail > slot ? (avail - slot + istride - 1) / istride : 0; }
    __device__ __forceinline__ int item0() const { return xcd * per_xcd + slot; }
};
__device__ __forceinline__ XcdItems xcd_items(int items)
{
    XcdItems r;
    r.xcd = blockIdx.x & 7;
    r.slot = blockIdx.x >> 3;
    r.per_xcd = (items + 7) >> 3;
    r.istride = ((int)gridDim.x + 7) >> 3;
    int avail = items - r.xcd * r.per_xcd;
    avail = avail < r.per_xcd ? avail : r.per_xcd;
    r.avail = avail < 0 ? 0 : avail;
    return r;
}

// ---- tile origin -----------------------------------------------------------------------------
// Pixel tile mt of the 256-pixel direct-conv items -> where its patch (the tile + 1-pixel halo) starts, as wave-uniform
// scalars.  2-D tiles of TH x TW pixels (TW != 0): image b and the halo's corner (y0, x0); flat tiles (TW == 0): j0 = the NHW
// pixel of patch row 0.  The other outputs are left as they are.
__device__ __forceinline__ void patch_origin(int mt, int tiles_per_img, int tiles_x, int TH, int TW, int W, int &b, int &y0, int &x0, int &j0)
{
    if (TW) {
        const int bb = mt / tiles_per_img, tt = mt - bb * tiles_per_img;
        const int ty = tt / tiles_x, tx = tt - ty * tiles_x;
        b = __builtin_amdgcn_readfirstlane(bb); y0 = __builtin_amdgcn_readfirstlane(ty * TH - 1); x0 = __builtin_amdgcn_readfirstlane(tx * TW - 1);
    } else {
        j0 = __builtin_amdgcn_readfirstlane(mt * 256 - W - 1);
    }
}

}  // namespace tdrn
