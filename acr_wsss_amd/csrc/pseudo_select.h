// The exact order statistic both pseudo-label rules need (pseudo.hip: sort(S)[int(n * q)] of myTool.py:717-720; pseudo_sal.hip: the
// same of :239-243), as a radix selection on the fp32 bit pattern: the values are positive, and positive floats order as their
// unsigned bit patterns.  Four passes of eight bits, most significant first: a pass counts, per plane, the values that agree with
// the plane's prefix so far in a 256-bin histogram (32-bit counters in LDS per workgroup, nonzero bins merged with integer adds
// into the caller's workspace); one workgroup per plane then picks the bin that holds the wanted rank and extends the prefix.
// Integer adds only: the selected value is a pure function of the input, whatever the order of the workgroups.
#pragma once
#include "acr_common.h"

#define PSEUDO_MAX_BLOCKS 512
#define PSEUDO_BINS 256
#define PSEUDO_PASSES 4
#define PSEUDO_EMPTY 0xffffffffu         // RANK of a plane that selects nothing
#define PSEUDO_INF_BITS 0x7f800000u      // its v: +inf, above which no value lies

static unsigned pseudo_blocks(int64_t pixels) {
    const int64_t b = (pixels + 255) / 256;
    return (unsigned)(b < PSEUDO_MAX_BLOCKS ? b : PSEUDO_MAX_BLOCKS);
}

// a workgroup's LDS counters into the global ones; call between two barriers
__device__ __forceinline__ void pseudo_hist_merge(const uint32_t* hist, uint32_t* __restrict__ g, int count) {
    for (int i = threadIdx.x; i < count; i += 256) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(&g[i], v);
    }
}

// One workgroup of 256 threads, one thread per bin of `hist` (this pass's 256 counters of one plane): the bin that holds the wanted
// rank.  Pass 0 knows n = the number of values and sets the rank int(n * q), the product in double; a plane with n == 0, or with
// rank 0 where zero_rank_selects_nothing (the reference's `if confidence_pos > 0`), gets v = +inf.  incl: 256 words of LDS.
__device__ __forceinline__ void pseudo_pick_bin(const uint32_t* __restrict__ hist, uint32_t* prefix_w, uint32_t* rank_w, int pass, double q,
                                                bool zero_rank_selects_nothing, uint32_t* incl) {
    const int tid = threadIdx.x;
    const int shift = 24 - 8 * pass;
    const uint32_t c = hist[tid];
    uint32_t k = pass ? *rank_w : 0u;
    const uint32_t prefix = pass ? *prefix_w : 0u;
    incl[tid] = c;
    __syncthreads();
    for (int d = 1; d < PSEUDO_BINS; d <<= 1) {          // inclusive prefix sum over the 256 bins
        const uint32_t add = tid >= d ? incl[tid - d] : 0u;
        __syncthreads();
        incl[tid] += add;
        __syncthreads();
    }
    const uint32_t n = incl[PSEUDO_BINS - 1];
    if (pass == 0) {
        if (n) k = (uint32_t)((double)n * q);            // < n: 0 <= q < 1
        if (n == 0 || (zero_rank_selects_nothing && k == 0)) {
            if (tid == 0) {
                *prefix_w = PSEUDO_INF_BITS;
                *rank_w = PSEUDO_EMPTY;
            }
            return;
        }
    } else if (k == PSEUDO_EMPTY) {
        return;
    }
    const uint32_t hi = incl[tid], lo = hi - c;
    if (lo <= k && k < hi) {                             // exactly one bin: 0 <= k < n
        *prefix_w = prefix | ((uint32_t)tid << shift);
        *rank_w = k - lo;
    }
}
