// Shared device/host helpers for libacr_hip.so (gfx950 only: wave64, MFMA, 160 KiB LDS).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/acr_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

#define ACR_LOG2E 1.4426950408889634f

// ---- host side error plumbing (thread-local message, never throws) ---------------------------
void acr_set_error(const char* fmt, ...);
#define ACR_CHECK_ARG(cond, ...)            \
    do {                                    \
        if (!(cond)) {                      \
            acr_set_error(__VA_ARGS__);     \
            return ACR_ERR_INVALID;         \
        }                                   \
    } while (0)
// a workspace the entry point `who` cannot do without: there, aligned to `align` bytes (a power of two), of `need` bytes at least
#define ACR_CHECK_WS(who, ws, align, ws_bytes, need)                                                                              \
    do {                                                                                                                          \
        ACR_CHECK_ARG((ws) && ((uintptr_t)(ws) & ((align)-1)) == 0, "%s: null workspace or not aligned to %d bytes", who, align); \
        const long long acr_ws_need_ = (long long)(need);                                                                         \
        ACR_CHECK_ARG((long long)(ws_bytes) >= acr_ws_need_, "%s: workspace of %lld bytes, %lld needed", who, (long long)(ws_bytes), \
                      acr_ws_need_);                                                                                              \
    } while (0)
int acr_check_launch(const char* what);
int32_t acr_opt(int option);          // explicit option table (acr_set_option), api.hip

// ---- barrier that publishes LDS-DMA data ---------------------------------------------------------
// `global_load_lds` writes LDS asynchronously and is tracked by the issuing wave's vmcnt only.  hipcc does NOT always put
// the s_waitcnt vmcnt(0) in front of a __syncthreads() that follows (seen missing when the barrier sits at a loop head
// reached over `continue` edges: waves passed the barrier with their DMA still in flight and a partner read stale LDS,
// once in ~50 launches).  Every barrier that hands DMA'd tiles to other waves therefore goes through this.
__device__ __forceinline__ void acr_dma_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// ---- XCD-aware block remap --------------------------------------------------------------------
// Workgroup barrier WITHOUT __syncthreads()'s fences, for loops that keep LDS-DMA (`global_load_lds`) in flight across it.
// __syncthreads() = release fence + s_barrier + acquire fence, and hipcc implements the workgroup-scope release of LDS as "every
// outstanding LDS-DMA has landed": it puts `s_waitcnt vmcnt(0)` in front of the barrier whenever a DMA may be pending (found in
// the ISA of every ring kernel, round 4) -- a ring that is N stages ahead degenerates to "wait for the newest stage every step".
// Contract of this one: the caller has waited (counted `s_waitcnt vmcnt(n)`) for the DMA pieces the OTHER waves are about to read,
// and `s_waitcnt lgkmcnt(0)` for its own ds_write / ds_read where another wave overwrites or reads those addresses next.
// The "memory" clobber keeps the compiler from moving memory accesses across it.
__device__ __forceinline__ void acr_barrier_nofence() { asm volatile("s_barrier" ::: "memory"); }

// ---- LDS reads the compiler must not see ------------------------------------------------------------------------------------
// hipcc cannot tell an LDS-DMA's LDS write from an LDS load of another slot: behind a global_load_lds it puts s_waitcnt vmcnt(0)
// in front of the next LDS load builtin.  Reads written as inline asm are invisible to that pass; the caller waits on lgkmcnt (LDS
// operations of a wave return in order: "at most n outstanding" = "all but my n newest have landed"; operations the compiler adds
// only make a wait stricter).  Addresses are LDS byte addresses; outputs are early-clobber and the waits name what must have landed.
#define ACR_LDS_RD128(dst, addr, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "i"(OFF))
#define ACR_LDS_RD32(dst, addr, OFF) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "i"(OFF))
#define ACR_LDS_WAIT4(cnt, a, b, c, d) asm volatile("s_waitcnt lgkmcnt(" #cnt ")" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
#define ACR_LDS_WAIT1(cnt, a) asm volatile("s_waitcnt lgkmcnt(" #cnt ")" : "+v"(a))

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share an L2).  Remap the
// linear block id so that each XCD walks one contiguous chunk of the work list: neighbouring
// tiles (same batch/head -> same K/V panels) then hit the same 4 MiB L2.  Bijective for any n.
__device__ __forceinline__ int acr_xcd_remap(int bid, int n) {
    const int q = n >> 3, r = n & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// C/D fragment row of a 32x32 MFMA accumulator register (dtype independent on gfx950):
// element `reg` of lane l sits at row krow(reg, l>>5), column l&31.
__device__ __forceinline__ int acr_krow(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// ---- dtype-generic 4-element loads / stores (fp32 math everywhere) ---------------------------
template <typename T>
__device__ __forceinline__ f32x4 acr_load4(const T* p);
template <>
__device__ __forceinline__ f32x4 acr_load4<float>(const float* p) {
    return *reinterpret_cast<const f32x4*>(p);
}
template <>
__device__ __forceinline__ f32x4 acr_load4<__bf16>(const __bf16* p) {
    bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    f32x4 r = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    return r;
}
template <typename T>
__device__ __forceinline__ void acr_store1(T* p, float v);
template <>
__device__ __forceinline__ void acr_store1<float>(float* p, float v) { *p = v; }
template <>
__device__ __forceinline__ void acr_store1<__bf16>(__bf16* p, float v) { *p = (__bf16)v; }
template <typename T>
__device__ __forceinline__ void acr_store4(T* p, f32x4 v);
template <>
__device__ __forceinline__ void acr_store4<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <>
__device__ __forceinline__ void acr_store4<__bf16>(__bf16* p, f32x4 v) {
    bf16x4 r = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    *reinterpret_cast<bf16x4*>(p) = r;
}
template <typename T>
__device__ __forceinline__ float acr_load1(const T* p) { return (float)*p; }
// ---- slab sums of a K-split product whose OUTPUT is small (gemm_f32.hip): true when the wide kernel took the sum
bool acr_slab_sum_wide(const float* ws, int nslab, int64_t n4, float* out, hipStream_t st);
