// The fixed-order sums of the kernels, stated once.  None uses an atomic and none depends on the launch geometry, so a kernel that
// sums through them is bit-identical run to run.
#pragma once
#include "acr_common.h"

// the sum over the 64 lanes of a wave by a butterfly; every lane gets it
__device__ __forceinline__ float acr_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the sum over W consecutive lanes of a wave (W a power of two up to 64, the group aligned to W) by the same butterfly; every lane of
// the group gets it
template <int W>
__device__ __forceinline__ float acr_lanes_sum(float v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the sum over a workgroup of NT threads: every wave's sum, then the waves in wave order; sh holds NT / 64 floats
template <int NT>
__device__ __forceinline__ float acr_block_sum(float v, float* sh) {
#pragma unroll                                               // acr_wave_sum, spelled out: nested, it changed the code of gn_bwd_kernel
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                                        // sh may still be read from a previous reduction
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += sh[w];           // same fixed order in every thread
    return t;
}

// The LDS tree of a 256-thread workgroup: thread tid has written element tid of every array to be summed, add(i, j) does
// `r[i] += r[j]` for each of them (so any number of arrays shares the one barrier of a round), and afterwards element 0 holds the
// sum, valid in thread 0.  The adds come as a callable rather than as pointers so that every call site is an instantiation of its
// own: a helper shared by several kernels compiled to slightly different code than the loop spelled in place.
template <typename F>
__device__ __forceinline__ void acr_tree_sum256(int tid, F add) {
    for (int off = 128; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off) add(tid, tid + off);
    }
}
