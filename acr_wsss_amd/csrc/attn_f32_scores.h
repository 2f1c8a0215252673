// What the fp32 attention generations share around the 32 x 32 score block: its layout, the cache policy of its streams, the
// counted waits, a wave's private score / G streams in both orientations, the forward's softmax step and epilogue.  Written once
// for attn_f32_dma.hip (recompute), attn_f32_sres.hip with attn_f32_sres_tails.h (resident scores) and attn_f32_x3.hip (split
// products); only the operand tiles and the waves per workgroup differ between them.  Much of it is macro text: a change here is
// checked by comparing every kernel's machine code with its parent's (scripts/device_code_diff.py), and as functions these pieces
// compile to other schedules.  The address-space typedefs (lds_vp / glb_vp) and lds_addr_of are those of attn_f32_tiles.h, the
// asm LDS reads (ACR_LDS_RD128 ...) those of acr_common.h.
#pragma once
#include "acr_common.h"
#include "attn_f32.h"
#include "attn_f32_tiles.h"

// ---- layout (described at the top of attn_f32_sres.hip) --------------------------------------------------------------------------
#define SB_FLOATS 1024                     // one block: 32 keys x 32 queries
__device__ __forceinline__ int64_t attn_score_block(int H, int NB, int b, int hd, int qb, int kb) {
    return ((((int64_t)b * H + hd) * NB + qb) * NB + kb) * SB_FLOATS;
}
static inline int64_t attn_score_floats(int B, int H, int T) {           // floats of the caller's `scores` taken by the blocks
    const int64_t nb = (T + 31) / 32;
    return (int64_t)B * H * nb * nb * SB_FLOATS;
}
// Split tail: one leftover 32-row block beyond a whole number of workgroups (nw blocks each) and at least one full workgroup for
// the split to pay.  That block of every (b, h) goes to a workgroup of attn_f32_sres_tails.h.
static inline bool attn_split_tail(int NB, int nw) { return (NB % nw) == 1 && NB > nw; }

// Cache policy of the score stream.  Every byte of `scores` is written once and read once per consumer, 983 MB per layer
// against 4 MB of L2 per XCD and 256 MB of Infinity Cache.  Measured per kernel (scripts/lab/attn_gen.py with lab builds):
// nontemporal loads take the head-mean stream from 235 to 183 us and the dQ body's loads the backward from 1549 to 1535 us;
// nontemporal stores the forward from 580 to 567 us; the row-term stream gets 5 % SLOWER with them (its G rows want to stay
// cached beside the scores) and the dK/dV body's LDS-DMA with the nt policy (aux = 2) is within noise: both keep the default.
#define SRES_LOAD_NT(p) __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p))
#define SRES_LOAD(p) (*reinterpret_cast<const f32x4*>(p))
#define SRES_STORE(p, v) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p))
#define SRES_LOAD_DQ(p) SRES_LOAD_NT(p)
#define SRES_DMA_AUX 0

// ---- counted waits -----------------------------------------------------------------------------------------------------------------
// A step's tile DMA must have landed at the step's barrier, but the streams that run further ahead (score blocks two steps ahead,
// G one step, the forward's score stores) are YOUNGER vector-memory operations and may stay in flight: vmcnt retires in issue
// order, so "at most n outstanding" with n = the number of younger operations is exactly "the tile has landed".  n is wave-uniform;
// every stream is LDS-DMA (register prefetch rings turn into loop-carried copies that hipcc waits for right behind the loads).
// attn_wait_vm<TEXT, counts above 0, descending>(n): a count that is not listed waits for the next smaller one, in the end for 0
// (stricter, never wrong).  Every body lists the counts its steps can ask for.  (A fold, not a recursion: that compiles to other
// code in the split-product backward.)
// TEXT: the count is written into the instruction text instead of passed as an immediate operand.  Both assemble to the same
// instruction, but hipcc merges the branches around them differently: each file keeps the spelling it was tuned with.
template <bool TEXT, int N>
__device__ __forceinline__ void attn_vmcnt() {
    if constexpr (!TEXT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else { static_assert(N == 0, "add the count's text"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
}
template <bool TEXT, int... Ns>
__device__ __forceinline__ void attn_wait_vm(int n) {
    if (!((n >= Ns ? (attn_vmcnt<TEXT, Ns>(), true) : false) || ...)) attn_vmcnt<TEXT, 0>();
}
// compiler-only fence: vector-memory operations written after it are issued after the ones before it (the counts above rely on the
// issue order; loads from global memory and LDS-DMA writes do not alias, so nothing else orders them for the compiler)
#define ATTN_FENCE() asm volatile("" ::: "memory")

// ---- rows of a 32 x 32 accumulator tile beyond T (keys in the forward and dQ, queries in dK/dV) ---------------------------------------
// (a macro: as a function taking the tile by reference the forward's schedule changes)
#define ATTN_MASK_ROWS(s, row0, T, h)                                   \
    if ((row0) + 32 > (T)) { /* only the last tile has rows beyond T (uniform branch) */ \
        _Pragma("unroll") for (int reg = 0; reg < 16; ++reg)            \
            if ((row0) + acr_krow(reg, h) >= (T)) s[reg] = -INFINITY;   \
    }

// ---- a wave's private score and G streams ---------------------------------------------------------------------------------------------
// Every wave of a backward sweep streams ITS score blocks by LDS-DMA into a private two-slot ring `ssm[wave]`, two steps ahead, and
// ITS 32 x 32 block of G into a private single-slot tile `gsm[wave]`, one step ahead.  The set-up below is macro text that declares
// locals in the body that uses it: as functions or as a struct the G-row selects and the address arithmetic compile to other code.
//
// Query on the lane (dQ): score blocks (qb = q0 / 32, kb = step) copied as stored (lane l of piece gq owns floats gq * 256 + 4 l ..);
// G rows = the wave's queries, 16-byte chunk c of row q in slot c ^ ((q >> 1) & 7) (the lane's row reads are then bank-conflict
// free), columns clamped into the row.
//   ATTN_QLANE_STREAMS  declares srow, sw, dma_scores(kblk, slot), gb0 (G of the sample or nullptr, uniform), gw, grow, gchunk, dma_g(k0)
//   ATTN_QLANE_ADDRS    declares saddr (+ slot * 4096 + gq * 1024) and gaddr[gq] (quad gq = keys 8 gq + 4 h .. + 3 of row r)
//   ATTN_QLANE_READ     s4 / g4 = the step's score block (ring slot SLOT) and G block, landed; G columns of keys >= T hold whatever
//                       the row pitch holds and are zeroed
#define ATTN_QLANE_STREAMS(sres, H, NB, T, b, hd, q0, wave, lane, ssm, gsm, gm, gm_sb, gm_st)                                       \
    const float* srow = sres + attn_score_block(H, NB, b, hd, min(q0 >> 5, NB - 1), 0) + lane * 4;                                  \
    float* sw = ssm + wave * 2 * SB_FLOATS;                                                                                         \
    auto dma_scores = [&](int kblk, int slot) {                                                                                     \
        const float* src = srow + (int64_t)kblk * SB_FLOATS;                                                                        \
        _Pragma("unroll") for (int gq = 0; gq < 4; ++gq)                                                                            \
            __builtin_amdgcn_global_load_lds((glb_vp)(src + gq * 256), (lds_vp)(sw + slot * SB_FLOATS + gq * 256), 16, 0, SRES_DMA_AUX); \
    };                                                                                                                              \
    const float* gb0 = gm ? gm + (int64_t)b * gm_sb : nullptr;                                                                      \
    float* gw = gsm + wave * SB_FLOATS;                                                                                             \
    const float* grow[4];                                                                                                           \
    int gchunk[4];                                                                                                                  \
    _Pragma("unroll") for (int p = 0; p < 4; ++p) {                                                                                 \
        const int row = 8 * p + (lane >> 3);                                                                                        \
        grow[p] = gb0 ? gb0 + (int64_t)min(q0 + row, T - 1) * gm_st : nullptr;                                                      \
        gchunk[p] = 4 * ((lane & 7) ^ ((row >> 1) & 7));                                                                            \
    }                                                                                                                               \
    auto dma_g = [&](int k0) {                                                                                                      \
        if (gb0 == nullptr) return;                                                                                                 \
        _Pragma("unroll") for (int p = 0; p < 4; ++p)                                                                               \
            __builtin_amdgcn_global_load_lds((glb_vp)(grow[p] + min(k0 + gchunk[p], (int)gm_st - 4)), (lds_vp)(gw + p * 256), 16, 0, 0); \
    }
#define ATTN_QLANE_ADDRS(lane, r, h)                                                                                                \
    const uint32_t saddr = lds_addr_of(sw) + lane * 16;                                                                             \
    uint32_t gaddr[4];                                                                                                              \
    _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) gaddr[gq] = lds_addr_of(gw) + r * 128 + (((2 * gq + h) ^ ((r >> 1) & 7)) << 4)
#define ATTN_QLANE_READ(SLOT, s4, g4, k0, T, h)                                                                                     \
    ACR_LDS_RD128(s4[0], saddr, SLOT * 4096); ACR_LDS_RD128(s4[1], saddr, SLOT * 4096 + 1024);                                      \
    ACR_LDS_RD128(s4[2], saddr, SLOT * 4096 + 2048); ACR_LDS_RD128(s4[3], saddr, SLOT * 4096 + 3072);                               \
    if (gb0 != nullptr) {                                                                                                           \
        ACR_LDS_RD128(g4[0], gaddr[0], 0); ACR_LDS_RD128(g4[1], gaddr[1], 0);                                                       \
        ACR_LDS_RD128(g4[2], gaddr[2], 0); ACR_LDS_RD128(g4[3], gaddr[3], 0);                                                       \
        ACR_LDS_WAIT4(0, g4[0], g4[1], g4[2], g4[3]);                                                                               \
        if (k0 + 32 > T) {                                                                                                          \
            _Pragma("unroll") for (int gq = 0; gq < 4; ++gq)                                                                        \
                _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                                       \
                    if (k0 + 8 * gq + 4 * h + e >= T) g4[gq][e] = 0.f;                                                              \
        }                                                                                                                           \
    } else {                                                                                                                        \
        _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) g4[gq] = f32x4{0.f, 0.f, 0.f, 0.f};                                        \
    }                                                                                                                               \
    ACR_LDS_WAIT4(0, s4[0], s4[1], s4[2], s4[3])
// dS^T = exp2(S - lse2) (dP^T + G/H - delta), query on the lane
__device__ __forceinline__ void attn_ds_qlane(f32x16& ds, const f32x4 (&s4)[4], const f32x4 (&g4)[4], const f32x16& dp, float l2q, float dl,
                                              float invH) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
        ds[reg] = __builtin_amdgcn_exp2f(s4[reg >> 2][reg & 3] - l2q) * (dp[reg] + g4[reg >> 2][reg & 3] * invH - dl);
}

// Key on the lane (dK/dV): score blocks (qb = step, kb = key0 / 32) with a chunk permutation on the SOURCE address -- lane c of DMA
// piece gq fetches global chunk c ^ (2 gq + (c >> 5)) -- that makes the transposed ds_read_b32 walk bank-conflict free; the G block as
// natural [query][key] rows (the lane's reads are 32 consecutive floats), columns clamped into the row (the last key block reaches
// beyond T: those lanes' P is exactly 0 and whatever they compute never leaves their own accumulator row).
//   ATTN_KLANE_STREAMS  declares scol, sstep, soff, sw, dma_scores(qblk, slot), gb0, gw, gcol, dma_g(q0)
//   ATTN_KLANE_ADDRS    declares stb[4] and gaddr: lane (kappa = r, h) reads register reg of the score block at
//                       stb[reg & 3] + slot * 4096 + 128 (reg >> 2) and of the G block at gaddr + 128 c_reg
//   ATTN_16(ATTN_RDS, s, SLOT) / ATTN_READ_G(gv)  the sixteen transposed reads of each; every body puts its other reads between them
#define ATTN_KLANE_STREAMS(sres, H, NB, T, b, hd, key0, wave, lane, ssm, gsm, gm, gm_sb, gm_st)                                     \
    const float* scol = sres + attn_score_block(H, NB, b, hd, 0, min(key0 >> 5, NB - 1));                                           \
    const int64_t sstep = (int64_t)NB * SB_FLOATS;                                                                                  \
    int soff[4];                                                                                                                    \
    _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) soff[gq] = gq * 256 + 4 * (lane ^ (2 * gq + (lane >> 5)));                     \
    float* sw = ssm + wave * 2 * SB_FLOATS;                                                                                         \
    auto dma_scores = [&](int qblk, int slot) {                                                                                     \
        const float* src = scol + (int64_t)qblk * sstep;                                                                            \
        _Pragma("unroll") for (int gq = 0; gq < 4; ++gq)                                                                            \
            __builtin_amdgcn_global_load_lds((glb_vp)(src + soff[gq]), (lds_vp)(sw + slot * SB_FLOATS + gq * 256), 16, 0, SRES_DMA_AUX); \
    };                                                                                                                              \
    const float* gb0 = gm ? gm + (int64_t)b * gm_sb : nullptr;                                                                      \
    float* gw = gsm + wave * SB_FLOATS;                                                                                             \
    const int gcol = min(key0 + 4 * (lane & 7), (int)gm_st - 4);                                                                    \
    auto dma_g = [&](int qrow0) {                                                                                                   \
        if (gb0 == nullptr) return;                                                                                                 \
        _Pragma("unroll") for (int p = 0; p < 4; ++p) {                                                                             \
            const float* src = gb0 + (int64_t)min(qrow0 + 8 * p + (lane >> 3), T - 1) * gm_st + gcol;                               \
            __builtin_amdgcn_global_load_lds((glb_vp)src, (lds_vp)(gw + p * 256), 16, 0, 0);                                        \
        }                                                                                                                           \
    }
#define ATTN_KLANE_ADDRS(ssm, gsm, wave, r, h)                                                                                      \
    uint32_t stb[4];                                                                                                                \
    {                                                                                                                               \
        const int gk = r >> 3, hk = (r >> 2) & 1, ek = r & 3, mm = 2 * gk + hk;                                                     \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                               \
            stb[j] = lds_addr_of(ssm) + ((wave * 2 * SB_FLOATS) + gk * 256 + 128 * hk + ek + 4 * ((j + 4 * h) ^ mm)) * 4;           \
    }                                                                                                                               \
    const uint32_t gaddr = lds_addr_of(gsm) + (wave * SB_FLOATS + 4 * h * 32 + r) * 4
#define ATTN_16(M, ...) \
    M(0, __VA_ARGS__); M(1, __VA_ARGS__); M(2, __VA_ARGS__); M(3, __VA_ARGS__); M(4, __VA_ARGS__); M(5, __VA_ARGS__); M(6, __VA_ARGS__); M(7, __VA_ARGS__); \
    M(8, __VA_ARGS__); M(9, __VA_ARGS__); M(10, __VA_ARGS__); M(11, __VA_ARGS__); M(12, __VA_ARGS__); M(13, __VA_ARGS__); M(14, __VA_ARGS__); M(15, __VA_ARGS__)
#define ATTN_RDS(REG, s, SLOT) ACR_LDS_RD32(s[REG], stb[(REG) & 3], SLOT * SB_FLOATS * 4 + 128 * ((REG) >> 2))
#define ATTN_RDG(REG, gv) ACR_LDS_RD32(gv[REG], gaddr, 128 * (((REG) & 3) + 8 * ((REG) >> 2)))
#define ATTN_V16(x) \
    "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), "+v"(x[8]), "+v"(x[9]), "+v"(x[10]), \
        "+v"(x[11]), "+v"(x[12]), "+v"(x[13]), "+v"(x[14]), "+v"(x[15])
#define ATTN_READ_G(gv)                                                     \
    if (gb0 != nullptr) {                                                   \
        ATTN_16(ATTN_RDG, gv);                                              \
        asm volatile("s_waitcnt lgkmcnt(0)" : ATTN_V16(gv));                \
    } else {                                                                \
        _Pragma("unroll") for (int reg = 0; reg < 16; ++reg) gv[reg] = 0.f; \
    }

// ---- the forward's tile step ---------------------------------------------------------------------------------------------------------
// the 32 x 32 logit tile as the block's four 1 KB register quads (keys >= T already -inf: ATTN_MASK_ROWS)
__device__ __forceinline__ void attn_store_scores(float* sp, const f32x16& s) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const f32x4 t = {s[4 * gq], s[4 * gq + 1], s[4 * gq + 2], s[4 * gq + 3]};
        SRES_STORE(sp + gq * 256, t);
    }
}
// Online softmax: p = exp2(s - m), l += rowsum(p).  Deferred rescale: the running reference m moves only when some row's maximum
// has grown by more than 2^8 since it was set (p then stays below 2^8: no overflow, full fp32 precision); most steps skip the 32
// multiplies of O and the exp2 of alpha.  exp2 = one v_exp_f32.
// (Macro text: as a function it changes the register allocation of the split-tail forward.)
#define ATTN_SOFTMAX_STEP(s, m, l, o0, o1, p)                                                             \
    {                                                                                                     \
        float mx_ = s[0];                                                                                 \
        _Pragma("unroll") for (int reg = 1; reg < 16; ++reg) mx_ = fmaxf(mx_, s[reg]);                    \
        mx_ = fmaxf(mx_, __shfl_xor(mx_, 32));                                                            \
        if (__any(mx_ > m + 8.f)) {                                                                       \
            const float mn_ = fmaxf(m, mx_);                                                              \
            const float alpha_ = __builtin_amdgcn_exp2f(m - mn_);                                         \
            l *= alpha_;                                                                                  \
            o0 *= alpha_; o1 *= alpha_;                                                                   \
            m = mn_;                                                                                      \
        }                                                                                                 \
        float rs_ = 0.f;                                                                                  \
        _Pragma("unroll") for (int reg = 0; reg < 16; ++reg) { p[reg] = __builtin_amdgcn_exp2f(s[reg] - m); rs_ += p[reg]; } \
        rs_ += __shfl_xor(rs_, 32);                                                                       \
        l += rs_;                                                                                         \
    }
// ---- the forward's epilogue: row q0 + r of o = O^T / l (lane (r, h): features 8 grp + 4 h .. + 3 of both halves) and
// lse2 = m + log2(l); inv = 1 / l.  g: AttnGeom or X3Geom.  Macro text: as a function it compiles to other code in every forward
// kernel (and so does the lse2 index written as ... + (q0 + r)).
#define ATTN_FWD_FINISH(g, o, lse2, b, hd, q0, r, h, o0, o1, m, l, inv)                                                   \
    {                                                                                                                     \
        float* ob_ = o + (int64_t)b * g.osb + (int64_t)(q0 + r) * g.ost + (int64_t)hd * g.osh;                            \
        _Pragma("unroll") for (int grp = 0; grp < 4; ++grp) {                                                             \
            f32x4 a_ = {o0[4 * grp] * inv, o0[4 * grp + 1] * inv, o0[4 * grp + 2] * inv, o0[4 * grp + 3] * inv};          \
            f32x4 c_ = {o1[4 * grp] * inv, o1[4 * grp + 1] * inv, o1[4 * grp + 2] * inv, o1[4 * grp + 3] * inv};          \
            *reinterpret_cast<f32x4*>(ob_ + 8 * grp + 4 * h) = a_;                                                        \
            *reinterpret_cast<f32x4*>(ob_ + 32 + 8 * grp + 4 * h) = c_;                                                   \
        }                                                                                                                 \
        if (h == 0) lse2[((int64_t)b * g.H + hd) * g.T + q0 + r] = m + log2f(l);                                          \
    }
