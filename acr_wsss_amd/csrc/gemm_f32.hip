// fp32 GEMMs of the transformer blocks at the REFERENCE precision (train_acr.py:137 runs fp32 end to end):
//   NT  y  = x W^T + b (+ resid)      models/vision_transformer.py:158-164 (fc1, fc2), :200 (qkv), :212 (proj)
//   NN  dx = dy W                      their input gradients
//   TN  dW = dy^T x, db = colsum(dy)   their weight / bias gradients (contraction over all tokens, split over workgroups)
// on v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate (a k-ordered fmaf chain, MI355X_MICROARCH.md "Matrix
// cores"), 64 FLOP/clk/SIMD = 157 TFLOP/s.
//
// Design for gfx950.  The fp32 MFMA needs ONE operand register per 4096 FLOP, i.e. 1/8 of the operand bytes per cycle of
// the bf16 32x32x16 form, so neither LDS bandwidth nor the L2 -> LDS path limits it (128x128 tiles: 1 ds_read_b128 per 4
// MFMAs = 256 cycles; 32 KiB of operands per 4096 MFMA cycles per workgroup).  What matters instead is (a) never leaving
// the matrix pipe idle and (b) tile quantisation: a 25 120-token activation against N = 768 is 591 tiles of 128x256 but
// only 297 of 256x256 for 256 CUs.  Hence: 128x128x32 tiles, 256 threads = 4 waves of 64x64 (4 accumulators of 16
// registers), TWO workgroups per CU so that each SIMD holds two waves from different workgroups: while one sits in its
// barrier / LDS refill the other issues MFMAs.  Operands are staged global -> registers -> LDS one K-chunk ahead (the global
// loads of chunk c+1 are in flight during the 64 MFMAs of chunk c) with two LDS buffers and one barrier per chunk.
//
// Operand layouts.  "KC" = contraction index contiguous in memory (x, W in NT): LDS image [i][k] with a 36-float pitch --
// ds_read_b128 fragment reads are bank-conflict free for every 16-lane group of the instruction (36*r mod 64 is a
// permutation of the 16 four-bank slots over any 16 consecutive r).  "KS" = contraction index strided (W in NN, dy and x
// in TN): LDS image [k][i], fragment = 4 ds_read_b32 of 32 consecutive floats.  No transposed copies of any weight.
// The 32x32x2 MFMA sums over k in any order as long as A and B agree: lane half h takes k = 8q + 4h + s of a chunk in
// step (q, s), which is what makes one 16-byte read feed four MFMAs.
#include <math.h>

#include <type_traits>

#include "gemm_f32.h"

// one K-chunk of one operand, global -> registers (4 float4 per thread), addresses clamped into the matrix so that every
// load is unconditional and nothing touches the loaded registers before store_chunk (the loads stay in flight across the
// chunk's MFMAs).  KC: rows = the operand's non-contraction index, k contiguous; KS: rows = k, 128 contiguous elements.
template <bool KC>
__device__ __forceinline__ void load_chunk(f32x4 (&r)[4], const float* __restrict__ p, int64_t ld, int i0, int dim, int k0,
                                           int kend, int tid) {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        const int f = tid + 256 * ps;
        if (KC) {
            const int i = min(i0 + (f >> 3), dim - 1), k = min(k0 + 4 * (f & 7), kend - 4);
            r[ps] = *reinterpret_cast<const f32x4*>(p + (int64_t)i * ld + k);
        } else {
            const int k = min(k0 + (f >> 5), kend - 1), i = min(i0 + 4 * (f & 31), dim - 4);
            r[ps] = *reinterpret_cast<const f32x4*>(p + (int64_t)k * ld + i);
        }
    }
}

// registers -> LDS; contraction indices at or beyond kend are stored as zeros (only the last chunk of a split has any)
template <bool KC>
__device__ __forceinline__ void store_chunk(float* __restrict__ s, f32x4 (&r)[4], int k0, int kend, int tid) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        const int f = tid + 256 * ps;
        if (KC) {
            if (k0 + 4 * (f & 7) >= kend) r[ps] = z;
            *reinterpret_cast<f32x4*>(s + (f >> 3) * F_PKC + 4 * (f & 7)) = r[ps];
        } else {
            if (k0 + (f >> 5) >= kend) r[ps] = z;
            *reinterpret_cast<f32x4*>(s + (f >> 5) * F_PKS + 4 * (f & 31)) = r[ps];
        }
    }
}

// fragment of 32 rows starting at `base` for k-group q of the chunk: v[s] = T[base + r][8q + 4h + s]
template <bool KC>
__device__ __forceinline__ f32x4 read_frag(const float* __restrict__ s, int base, int q, int r, int h) {
    if (KC) return *reinterpret_cast<const f32x4*>(s + (base + r) * F_PKC + 8 * q + 4 * h);
    const float* p = s + (8 * q + 4 * h) * F_PKS + base + r;
    f32x4 v = {p[0], p[F_PKS], p[2 * F_PKS], p[3 * F_PKS]};
    return v;
}

// ACT: 0 = (+bias)(+resid), 1 = c = GELU'(h), c2 = GELU(h) with h = acc + bias, 2 = c = acc * aux, 3 = split slab (no epilogue)
template <bool A_KC, bool B_KC, int ACT>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(const GemmF32Args g) {
    __shared__ __attribute__((aligned(16))) float smem[4 * F_STAGE];      // [buf][A|B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int ntile = g.tiles_launch;
    const int t = acr_xcd_remap(blockIdx.x, ntile * g.nsplit);
    const int split = t / ntile, tt = g.tile0 + (t - split * ntile);
    int tm, tn;
    if (ACT == 3) { tm = tt / g.tiles_n; tn = tt - tm * g.tiles_n; }
    else tile_coords(tt, g.tiles_m, g.tiles_n, tm, tn);
    const int m0 = tm * F_BM, n0 = tn * F_BN;
    const int zs = split / g.ksplit;
    const int kbeg = (split - zs * g.ksplit) * g.k_zs, kend = min(g.K, kbeg + g.kps);
    const float* __restrict__ pa = g.a + (int64_t)zs * g.a_zs;
    const float* __restrict__ pb = g.b + (int64_t)zs * g.b_zs;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // Register sets 0 / 1 hold the chunks in flight from global memory.  Chunk c is computed from LDS buffer c & 1 while
    // chunk c + 1 (loaded during chunk c - 1) waits in set (c + 1) & 1 and the loads of chunk c + 2 are issued into set
    // c & 1: every load has TWO chunks of MFMAs (>= 8192 matrix-pipe cycles) to land before its LDS store.
    f32x4 ra0[4], rb0[4], ra1[4], rb1[4];
    float csum[4] = {0.f, 0.f, 0.f, 0.f};          // TN bias gradient: this thread's column sums of its A chunks (KS layout)
    const bool want_cs = ACT == 3 && !A_KC && g.cs && tn == 0;
    auto add_cs = [&](f32x4 (&x)[4]) {             // after store_chunk: the K tail is already zeroed in x
#pragma unroll
        for (int ps = 0; ps < 4; ++ps)
#pragma unroll
            for (int e = 0; e < 4; ++e) csum[e] += x[ps][e];
    };
    auto compute = [&](int buf) {
        const float* sa = smem + buf * 2 * F_STAGE;
        const float* sb = sa + F_STAGE;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = read_frag<A_KC>(sa, wm * 64 + i * 32, q, r, h);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = read_frag<B_KC>(sb, wn * 64 + j * 32, q, r, h);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][s], bv[j][s], acc[i][j], 0, 0, 0);
        }
    };
    // one chunk: issue the loads of chunk k0 + 2 BK into (la, lb), compute chunk k0 from LDS[buf], then move chunk
    // k0 + BK from (sa_, sb_) to LDS[buf ^ 1]
    auto step = [&](f32x4 (&la)[4], f32x4 (&lb)[4], f32x4 (&sa_)[4], f32x4 (&sb_)[4], int k0, int buf) {
        if (k0 + 2 * F_BK < kend) {
            load_chunk<A_KC>(la, pa, g.lda, m0, g.M, k0 + 2 * F_BK, kend, tid);
            load_chunk<B_KC>(lb, pb, g.ldb, n0, g.N, k0 + 2 * F_BK, kend, tid);
        }
        compute(buf);
        if (k0 + F_BK < kend) {
            float* d = smem + (buf ^ 1) * 2 * F_STAGE;
            store_chunk<A_KC>(d, sa_, k0 + F_BK, kend, tid);
            store_chunk<B_KC>(d + F_STAGE, sb_, k0 + F_BK, kend, tid);
            if (want_cs) add_cs(sa_);
        }
        __syncthreads();
    };
    load_chunk<A_KC>(ra0, pa, g.lda, m0, g.M, kbeg, kend, tid);
    load_chunk<B_KC>(rb0, pb, g.ldb, n0, g.N, kbeg, kend, tid);
    if (kbeg + F_BK < kend) {
        load_chunk<A_KC>(ra1, pa, g.lda, m0, g.M, kbeg + F_BK, kend, tid);
        load_chunk<B_KC>(rb1, pb, g.ldb, n0, g.N, kbeg + F_BK, kend, tid);
    }
    store_chunk<A_KC>(smem, ra0, kbeg, kend, tid);
    store_chunk<B_KC>(smem + F_STAGE, rb0, kbeg, kend, tid);
    if (want_cs) add_cs(ra0);
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += 2 * F_BK) {
        step(ra0, rb0, ra1, rb1, k0, 0);
        if (k0 + F_BK < kend) step(ra1, rb1, ra0, rb0, k0 + F_BK, 1);
    }

    // ---- epilogue: lane (r, h), register e of a 32x32 accumulator = row krow(e, h), column r
    if (ACT == 3) {
        float* slab = g.c + (int64_t)split * g.M * g.ldc;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = n0 + wn * 64 + j * 32 + r;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = m0 + wm * 64 + i * 32 + acr_krow(e, h);
                    if (row < g.M && col < g.N) slab[(int64_t)row * g.ldc + col] = acc[i][j][e];
                }
            }
        if (!A_KC && g.cs && tn == 0) {
            // column sums of this split's A rows: thread (kr = tid/32, i4 = tid%32) holds 4 columns; sum the 8 kr rows via LDS
            float* red = smem;                                   // all fragment reads are behind the loop's last barrier
            *reinterpret_cast<f32x4*>(red + (tid >> 5) * 128 + 4 * (tid & 31)) = *reinterpret_cast<f32x4*>(csum);
            __syncthreads();
            if (tid < 128) {
                float s = 0.f;
#pragma unroll
                for (int kr = 0; kr < 8; ++kr) s += red[kr * 128 + tid];
                if (m0 + tid < g.M) g.cs[(int64_t)split * g.M + m0 + tid] = s;
            }
        }
        return;
    }
    GemmF32Args gz = g;                                     // this slice's output / addend
    gz.c += (int64_t)zs * g.c_zs;
    if (gz.aux) gz.aux += (int64_t)zs * g.aux_zs;
    if (m0 + F_BM <= g.M && n0 + F_BN <= g.N)
        epilogue_f32<ACT, false>(gz, acc, m0 + wm * 64, n0 + wn * 64, r, h);
    else
        epilogue_f32<ACT, true>(gz, acc, m0 + wm * 64, n0 + wn * 64, r, h);
}

// ---------------------------------------------------------------------------------------------------------------
// LDS-DMA variant (contraction length a multiple of 32): chunks go global -> LDS directly (global_load_lds_dwordx4),
// no staging registers and no ds_write path.  Measured on the register-staged kernel above (scripts/lab): its 8 loads +
// 8 ds_write_b128 per 64 MFMAs cost 18 % of the matrix pipe (4096^3: 150 TF with neither, 128 / 134 TF with one of them,
// 120 TF with both) although clocks, prefetch depth and wave priorities are not the cause -- VGPR traffic of loads and
// LDS stores competes with the MFMA operand reads.  A DMA wave-instruction writes 64 lanes x 16 B = 1 KiB linearly:
//   KC operand: 8 unpadded 128-byte rows; ds_read_b128 bank conflicts are removed by an XOR swizzle applied on the
//               SOURCE address (lane fetches 16-byte chunk p ^ ((row >> 1) & 7) into slot p) and mirrored on the read;
//   KS operand: 2 k-rows of 128 floats; fragment reads are 32 consecutive floats, no swizzle needed.
// ---------------------------------------------------------------------------------------------------------------
#define F_DTILE (F_BM * F_BK)        // floats per operand per stage, unpadded (16 KiB)

// Per-lane element offsets of this wave's 4 DMA pieces inside one operand, relative to (row 0 of the tile, contraction index
// 0 of the chunk): computed ONCE per workgroup.  Per chunk the source is then  uniform base (+ k advance, scalar) + this
// offset -- no vector arithmetic inside the loop (VALU instructions run on the lanes the fp32 MFMA uses; the per-chunk
// address math was ~40 of the loop's 58 VALU instructions).  Offsets are 32-bit: the host checks dim * ld < 2^31.
template <bool KC>
__device__ __forceinline__ void dma_offsets(int (&off)[4], int64_t ld, int i0, int dim, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = wave * 4 + i;
        if (KC) {
            const int row = piece * 8 + (lane >> 3);
            const int lc = (lane & 7) ^ ((row >> 1) & 7);
            off[i] = min(i0 + row, dim - 1) * (int)ld + lc * 4;
        } else {
            const int kr = piece * 2 + (lane >> 5);
            off[i] = kr * (int)ld + min(i0 + 4 * (lane & 31), dim - 4);
        }
    }
}
// ub: uniform pointer to (row 0, contraction index k0) of the operand: p + k0 (KC) or p + k0 * ld (KS)
__device__ __forceinline__ void dma_chunk(float* s, const float* __restrict__ ub, const int (&off)[4], int wave) {
    typedef __attribute__((address_space(3))) void* lds_vp;
    typedef const __attribute__((address_space(1))) void* glb_vp;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds((glb_vp)(ub + off[i]), (lds_vp)(s + (wave * 4 + i) * 256), 16, 0, 0);
}

template <bool KC>
__device__ __forceinline__ f32x4 dma_frag(const float* __restrict__ s, int base, int q, int r, int h) {
    if (KC) {
        const int row = base + r;
        return *reinterpret_cast<const f32x4*>(s + row * F_BK + (((2 * q + h) ^ ((row >> 1) & 7)) << 2));
    }
    const float* p = s + (8 * q + 4 * h) * F_BM + base + r;
    f32x4 v = {p[0], p[F_BM], p[2 * F_BM], p[3 * F_BM]};
    return v;
}

template <bool A_KC, bool B_KC, int ACT>
__global__ __launch_bounds__(256, 2) void gemm_f32_dma_kernel(const GemmF32Args g) {
    __shared__ __attribute__((aligned(1024))) float smem[4 * F_DTILE];      // [A0 | B0 | A1 | B1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int ntile = g.tiles_launch;
    const int t = acr_xcd_remap(blockIdx.x, ntile * g.nsplit);
    const int split = t / ntile, tt = g.tile0 + (t - split * ntile);
    int tm, tn;
    if (ACT == 3) { tm = tt / g.tiles_n; tn = tt - tm * g.tiles_n; }
    else tile_coords(tt, g.tiles_m, g.tiles_n, tm, tn);
    const int m0 = tm * F_BM, n0 = tn * F_BN;
    const int zs = split / g.ksplit;
    const int kbeg = (split - zs * g.ksplit) * g.k_zs, kend = min(g.K, kbeg + g.kps);      // host: (kend - kbeg) % F_BK == 0
    const float* __restrict__ pa = g.a + (int64_t)zs * g.a_zs;
    const float* __restrict__ pb = g.b + (int64_t)zs * g.b_zs;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    float csum = 0.f;          // TN bias gradient: column tid & 127 of the A chunks, k rows of parity tid >> 7
    const bool want_cs = ACT == 3 && !A_KC && g.cs && tn == 0;

    int offa[4], offb[4];
    dma_offsets<A_KC>(offa, g.lda, m0, g.M, wave, lane);
    dma_offsets<B_KC>(offb, g.ldb, n0, g.N, wave, lane);
    const int64_t ka = A_KC ? 1 : g.lda, kb = B_KC ? 1 : g.ldb;      // operand advance per contraction index
    dma_chunk(smem, pa + kbeg * ka, offa, wave);
    dma_chunk(smem + F_DTILE, pb + kbeg * kb, offb, wave);
    acr_dma_barrier();
    int cur = 0;
    for (int k0 = kbeg; k0 < kend; k0 += F_BK, cur ^= 1) {
        if (k0 + F_BK < kend) {
            float* d = smem + (cur ^ 1) * 2 * F_DTILE;
            dma_chunk(d, pa + (k0 + F_BK) * ka, offa, wave);
            dma_chunk(d + F_DTILE, pb + (k0 + F_BK) * kb, offb, wave);
        }
        const float* sa = smem + cur * 2 * F_DTILE;
        const float* sb = sa + F_DTILE;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = dma_frag<A_KC>(sa, wm * 64 + i * 32, q, r, h);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = dma_frag<B_KC>(sb, wn * 64 + j * 32, q, r, h);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][s], bv[j][s], acc[i][j], 0, 0, 0);
        }
        if (want_cs) {                                      // [k][i] image: 16 of the chunk's 32 k rows per thread
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) csum += sa[(2 * kk + (tid >> 7)) * F_BM + (tid & 127)];
        }
        acr_dma_barrier();                                  // the chunk in flight has landed; buffer `cur` is free
    }
    gemm_f32_finish<A_KC, ACT>(g, acc, smem, split, tt, tn, m0, n0, zs, wm, wn, r, h, tid, csum, want_cs);
}

// ---------------------------------------------------------------------------------------------------------------
// fp32 products on the bf16 MFMA (math = ACR_MATH_BF16X3, a per-call argument): the same tiles, operands, epilogues and tail plan as the kernels
// above, but every fp32 product is evaluated on v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA's rate) as SIX exact terms of a
// three-way operand split,
//     a = a0 + a1 + a2,  b = b0 + b1 + b2   (a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1): 3 x 8 = 24 mantissa bits)
//     a b ~ a0 b0 + a0 b1 + a1 b0 + a1 b1 + a0 b2 + a2 b0        (the dropped terms are <= 2^-24 |a b|)
// every bf16 x bf16 product is exact in fp32 and the sums accumulate in fp32: against float64 the result is as accurate as the
// exact-fp32 MFMA chain (scripts/lab/gemm_split.py: rms error 8.6e-7 vs 9.9e-7 of rms y at K = 3072).  Operands stay fp32 in
// HBM and in LDS; fragments are split in registers right after their ds_read.
// Structure: a 32-deep chunk is now ~1.5 us of matrix work for two co-resident workgroups, less than the 3 us a first-touch
// DMA takes to land -- with the two-slot ring above the loop is latency-bound (3.2 us per chunk measured, x1.3 only).  So:
// 16-deep stages (one MFMA k-step), a FOUR-slot ring filled three stages ahead with counted vmcnt, and the split of stage t
// interleaved (sched_group_barrier) with the 24 MFMAs of stage t - 1, whose pieces wait in a second register set.
// ---------------------------------------------------------------------------------------------------------------
#define S_SLOTS 4

// per-lane element offsets of this wave's 2 DMA pieces of one 16-deep stage of one operand (computed once per workgroup).
// KC: piece = 16 rows x 64 bytes, lane -> (row = l >> 2, 16-byte chunk l & 3), chunk XOR-swizzled by (row >> 2) & 3 on the
// SOURCE address (mirrored by the fragment reads: every 16-lane group of a ds_read_b128 then hits 16 different bank quads);
// KS: piece = 2 k rows of 128 floats.
template <bool KC>
__device__ __forceinline__ void split_dma_offsets(int (&off)[2], int64_t ld, int i0, int dim, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int piece = wave * 2 + i;
        if (KC) {
            const int row = piece * 16 + (lane >> 2);
            const int lc = (lane & 3) ^ ((row >> 2) & 3);
            off[i] = min(i0 + row, dim - 1) * (int)ld + lc * 4;
        } else {
            const int kr = piece * 2 + (lane >> 5);
            off[i] = kr * (int)ld + min(i0 + 4 * (lane & 31), dim - 4);
        }
    }
}
__device__ __forceinline__ void split_dma_stage(float* s, const float* __restrict__ ub, const int (&off)[2], int wave) {
    typedef __attribute__((address_space(3))) void* lds_vp;
    typedef const __attribute__((address_space(1))) void* glb_vp;
#pragma unroll
    for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds((glb_vp)(ub + off[i]), (lds_vp)(s + (wave * 2 + i) * 256), 16, 0, 0);
}
// the 8 consecutive contraction indices 8 h + (0..7) of lane (r, h) for 32 rows starting at `base`
template <bool KC>
__device__ __forceinline__ void split_frag8(const float* __restrict__ s, int base, int r, int h, f32x4& lo4, f32x4& hi4) {
    if (KC) {
        const int row = base + r, sw = (row >> 2) & 3;
        lo4 = *reinterpret_cast<const f32x4*>(s + row * S_BK + (((2 * h) ^ sw) << 2));
        hi4 = *reinterpret_cast<const f32x4*>(s + row * S_BK + (((2 * h + 1) ^ sw) << 2));
    } else {
        const float* p = s + (8 * h) * F_BM + base + r;
        lo4 = f32x4{p[0], p[F_BM], p[2 * F_BM], p[3 * F_BM]};
        hi4 = f32x4{p[4 * F_BM], p[5 * F_BM], p[6 * F_BM], p[7 * F_BM]};
    }
}

// The same fragment through inline-asm LDS reads.  hipcc cannot tell an LDS-DMA's LDS write from a read of another ring slot:
// in front of the first compiler-visible LDS load behind a DMA it waits for ALL outstanding vector-memory operations
// (`s_waitcnt vmcnt(0)`, found in the ISA right before the stage barrier) -- which turned the three-stages-ahead ring into a
// one-stage-ahead one: every stage waited for the DMAs issued one stage earlier.  asm reads are invisible to that analysis; the
// counted vmcnt wait + barrier in front of them and the lgkmcnt wait behind them (SPLIT_LDS_WAIT8) are the synchronisation.
// Lane bases (LDS byte addresses inside slot 0's A resp. B tile): KC two per fragment (the two swizzled 16-byte chunks), KS one.
template <bool KC>
__device__ __forceinline__ void split_frag_bases(uint32_t (&b)[2], const float* tile0, int base, int r, int h) {
    typedef const __attribute__((address_space(3))) char* lds_cp;
    const uint32_t t = (uint32_t)(uintptr_t)(lds_cp)tile0;
    if (KC) {
        const int row = base + r, sw = (row >> 2) & 3;
        b[0] = t + row * (S_BK * 4) + (((2 * h) ^ sw) << 4);
        b[1] = t + row * (S_BK * 4) + (((2 * h + 1) ^ sw) << 4);
    } else {
        b[0] = b[1] = t + ((8 * h) * F_BM + base + r) * 4;
    }
}
#define SPLIT_RD128(dst, addr) asm volatile("ds_read_b128 %0, %1" : "=&v"(dst) : "v"(addr))
#define SPLIT_RD32(dst, addr, OFF) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "i"(OFF))
template <bool KC>
__device__ __forceinline__ void split_frag8_x(const uint32_t (&b)[2], uint32_t slot_off, f32x4& lo4, f32x4& hi4) {
    if (KC) {
        SPLIT_RD128(lo4, b[0] + slot_off);
        SPLIT_RD128(hi4, b[1] + slot_off);
    } else {
        const uint32_t a = b[0] + slot_off;
        SPLIT_RD32(lo4[0], a, 0); SPLIT_RD32(lo4[1], a, F_BM * 4); SPLIT_RD32(lo4[2], a, 2 * F_BM * 4); SPLIT_RD32(lo4[3], a, 3 * F_BM * 4);
        SPLIT_RD32(hi4[0], a, 4 * F_BM * 4); SPLIT_RD32(hi4[1], a, 5 * F_BM * 4); SPLIT_RD32(hi4[2], a, 6 * F_BM * 4); SPLIT_RD32(hi4[3], a, 7 * F_BM * 4);
    }
}
#define SPLIT_LDS_WAIT8(a0, a1, a2, a3, a4, a5, a6, a7) \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7))

template <bool A_KC, bool B_KC, int ACT>
__global__ __launch_bounds__(256, 2) void gemm_f32_split_kernel(const GemmF32Args g) {
    __shared__ __attribute__((aligned(1024))) float smem[S_SLOTS * 2 * S_TILE];      // [slot][A | B], 64 KiB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int ntile = g.tiles_launch;
    const int t0 = acr_xcd_remap(blockIdx.x, ntile * g.nsplit);
    const int split = t0 / ntile, tt = g.tile0 + (t0 - split * ntile);
    int tm, tn;
    if (ACT == 3) { tm = tt / g.tiles_n; tn = tt - tm * g.tiles_n; }
    else tile_coords(tt, g.tiles_m, g.tiles_n, tm, tn);
    const int m0 = tm * F_BM, n0 = tn * F_BN;
    const int zs = split / g.ksplit;
    const int kbeg = (split - zs * g.ksplit) * g.k_zs, kend = min(g.K, kbeg + g.kps);      // host: (kend - kbeg) % 16 == 0
    const float* __restrict__ pa = g.a + (int64_t)zs * g.a_zs;
    const float* __restrict__ pb = g.b + (int64_t)zs * g.b_zs;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    float csum = 0.f;          // TN bias gradient: column tid & 127 of the A stages, k rows of parity tid >> 7
    const bool want_cs = ACT == 3 && !A_KC && g.cs && tn == 0;
    int offa[2], offb[2];
    split_dma_offsets<A_KC>(offa, g.lda, m0, g.M, wave, lane);
    split_dma_offsets<B_KC>(offb, g.ldb, n0, g.N, wave, lane);
    const int64_t ka = A_KC ? 1 : g.lda, kb = B_KC ? 1 : g.ldb;      // operand advance per contraction index
    const int nst = (kend - kbeg) / S_BK;
    uint32_t fa[2][2], fb[2][2];                             // fragment lane bases in slot 0
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        split_frag_bases<A_KC>(fa[i], smem, wm * 64 + i * 32, r, h);
        split_frag_bases<B_KC>(fb[i], smem + S_TILE, wn * 64 + i * 32, r, h);
    }
    const uint32_t cs_base = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)smem + ((tid >> 7) * F_BM + (tid & 127)) * 4;
    auto issue = [&](int st) {
        float* d = smem + (st & (S_SLOTS - 1)) * 2 * S_TILE;
        split_dma_stage(d, pa + (int64_t)(kbeg + st * S_BK) * ka, offa, wave);
        split_dma_stage(d + S_TILE, pb + (int64_t)(kbeg + st * S_BK) * kb, offb, wave);
    };
#pragma unroll
    for (int st = 0; st < S_SLOTS - 1; ++st)
        if (st < nst) issue(st);
    bf16x8 ap[2][2][3], bp[2][2][3];                        // [register set][block][piece]
    f32x4 ra[2][2], rb[2][2];
    // stage st: wait until it has landed (stages st+1, st+2 may stay in flight: 4 DMA instructions each), publish it, refill the
    // slot stage st-1 was read from, read + split stage st into register set SET while the MFMAs of stage st-1 (set SET^1) run
    auto step = [&](int st, auto set_tag, auto first_tag) {
        constexpr int SET = decltype(set_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value;
        if (st + 2 < nst) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (st + 1 < nst) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        acr_barrier_nofence();                              // stage st landed for every wave; all reads of stage st - 1 were waited for (SPLIT_LDS_WAIT8)
        if (st + S_SLOTS - 1 < nst) issue(st + S_SLOTS - 1);
        const uint32_t so = (uint32_t)(st & (S_SLOTS - 1)) * (2 * S_TILE * 4);
#pragma unroll
        for (int i = 0; i < 2; ++i) split_frag8_x<A_KC>(fa[i], so, ra[i][0], ra[i][1]);
#pragma unroll
        for (int j = 0; j < 2; ++j) split_frag8_x<B_KC>(fb[j], so, rb[j][0], rb[j][1]);
        if (want_cs) {                                      // [k][i] image: 8 of the stage's 16 k rows per thread
            float c8[8];
            const uint32_t ca = cs_base + so;
            SPLIT_RD32(c8[0], ca, 0); SPLIT_RD32(c8[1], ca, 2 * F_BM * 4); SPLIT_RD32(c8[2], ca, 4 * F_BM * 4); SPLIT_RD32(c8[3], ca, 6 * F_BM * 4);
            SPLIT_RD32(c8[4], ca, 8 * F_BM * 4); SPLIT_RD32(c8[5], ca, 10 * F_BM * 4); SPLIT_RD32(c8[6], ca, 12 * F_BM * 4); SPLIT_RD32(c8[7], ca, 14 * F_BM * 4);
            SPLIT_LDS_WAIT8(c8[0], c8[1], c8[2], c8[3], c8[4], c8[5], c8[6], c8[7]);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) csum += c8[kk];
        }
        SPLIT_LDS_WAIT8(ra[0][0], ra[0][1], ra[1][0], ra[1][1], rb[0][0], rb[0][1], rb[1][0], rb[1][1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i) split3_bf16(ra[i][0], ra[i][1], ap[SET][i][0], ap[SET][i][1], ap[SET][i][2]);
#pragma unroll
        for (int j = 0; j < 2; ++j) split3_bf16(rb[j][0], rb[j][1], bp[SET][j][0], bp[SET][j][1], bp[SET][j][2]);
        if (!FIRST) {
            ACR_MFMA6(acc[0][0], ap[SET ^ 1][0], bp[SET ^ 1][0]) ACR_MFMA6(acc[0][1], ap[SET ^ 1][0], bp[SET ^ 1][1]) ACR_MFMA6(acc[1][0], ap[SET ^ 1][1], bp[SET ^ 1][0]) ACR_MFMA6(acc[1][1], ap[SET ^ 1][1], bp[SET ^ 1][1])
#pragma unroll
            for (int it = 0; it < 24; ++it) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA of stage st - 1
                __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);      // eight VALU instructions of stage st's split
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    step(0, std::integral_constant<int, 0>{}, std::true_type{});
    for (int st = 1; st < nst; st += 2) {
        step(st, std::integral_constant<int, 1>{}, std::false_type{});
        if (st + 1 < nst) step(st + 1, std::integral_constant<int, 0>{}, std::false_type{});
    }
    if (nst & 1) { ACR_MFMA6(acc[0][0], ap[0][0], bp[0][0]) ACR_MFMA6(acc[0][1], ap[0][0], bp[0][1]) ACR_MFMA6(acc[1][0], ap[0][1], bp[0][0]) ACR_MFMA6(acc[1][1], ap[0][1], bp[0][1]) }
    else { ACR_MFMA6(acc[0][0], ap[1][0], bp[1][0]) ACR_MFMA6(acc[0][1], ap[1][0], bp[1][1]) ACR_MFMA6(acc[1][0], ap[1][1], bp[1][0]) ACR_MFMA6(acc[1][1], ap[1][1], bp[1][1]) }
    __syncthreads();                                        // every wave is done with the ring: the finish may reuse it
    gemm_f32_finish<A_KC, ACT>(g, acc, smem, split, tt, tn, m0, n0, zs, wm, wn, r, h, tid, csum, want_cs);
}

// out[i] = sum_s slab[s][i] in split order (deterministic), float4 per thread; n4 = elements / 4
__global__ __launch_bounds__(256) void gemm_f32_reduce_kernel(const float* __restrict__ ws, int nsplit, int64_t n4,
                                                              float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 s = reinterpret_cast<const f32x4*>(ws)[i];
    for (int k = 1; k < nsplit; ++k) {
        const f32x4 v = reinterpret_cast<const f32x4*>(ws)[(int64_t)k * n4 + i];
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    reinterpret_cast<f32x4*>(out)[i] = s;
}

__global__ __launch_bounds__(256) void gemm_f32_reduce1_kernel(const float* __restrict__ ws, int nsplit, int n,
                                                               float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = ws[i];
    for (int k = 1; k < nsplit; ++k) s += ws[(int64_t)k * n + i];
    out[i] = s;
}
void gemm_f32_reduce(const float* ws, int nsplit, int64_t n4, float* out, hipStream_t st) {
    hipLaunchKernelGGL(gemm_f32_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, ws, nsplit, n4, out);
}
// ---- slab sums of a K-split product whose OUTPUT is small --------------------------------------------------------------------------
// out[i] = sum_k slab[k][i] (float4 per column index i < n4).  One thread per output float4 walking all slabs (the products' own
// reduce kernels) leaves a 64 x 64 weight gradient with 4 workgroups reading 256 slabs one after the other: 123 us for 4 MB
// (scripts/lab/conv_wgrad_trace.py; the stem's 1x1 / 3x3 weight gradients spent 1.4 ms per step there).  Here a workgroup is
// 32 columns x G slab groups: thread (tx, ty) sums slabs ty, ty + G, ... in ascending order with four loads in flight, and the G
// partial sums meet in LDS, where they are added in group order.  Deterministic: the grouping depends on (n4, nslab) only.
template <int G>
__global__ __launch_bounds__(32 * G) void acr_slab_sum_wide_kernel(const float* __restrict__ ws, int nslab, int64_t n4, float* __restrict__ out) {
    __shared__ f32x4 part[G][32];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t i = (int64_t)blockIdx.x * 32 + tx;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (i < n4) {
        const f32x4* p = reinterpret_cast<const f32x4*>(ws) + i;
        int k = ty;
        for (; k + 3 * G < nslab; k += 4 * G) {
            const f32x4 v0 = p[(int64_t)k * n4], v1 = p[(int64_t)(k + G) * n4], v2 = p[(int64_t)(k + 2 * G) * n4], v3 = p[(int64_t)(k + 3 * G) * n4];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; k < nslab; k += G) s += p[(int64_t)k * n4];
    }
    part[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && i < n4) {
        f32x4 t = part[0][tx];
#pragma unroll
        for (int g = 1; g < G; ++g) t += part[g][tx];
        reinterpret_cast<f32x4*>(out)[i] = t;
    }
}
// slab groups for an output of n4 float4: enough threads to keep ~128k loads in flight, 0 = the one-thread-per-output kernel is fine
static int acr_slab_sum_groups(int nslab, int64_t n4) {
    if (n4 >= 65536 || nslab < 8) return 0;
    int g = 32;
    while (g > 4 && n4 * (g / 2) >= 131072) g >>= 1;
    while (g > 4 && g > nslab) g >>= 1;
    return g;
}
// true when the wide kernel took the sum
bool acr_slab_sum_wide(const float* ws, int nslab, int64_t n4, float* out, hipStream_t st) {
    const int g = acr_slab_sum_groups(nslab, n4);
    if (g == 0) return false;
    const dim3 grid((unsigned)((n4 + 31) / 32));
    if (g == 32) hipLaunchKernelGGL((acr_slab_sum_wide_kernel<32>), grid, dim3(1024), 0, st, ws, nslab, n4, out);
    else if (g == 16) hipLaunchKernelGGL((acr_slab_sum_wide_kernel<16>), grid, dim3(512), 0, st, ws, nslab, n4, out);
    else if (g == 8) hipLaunchKernelGGL((acr_slab_sum_wide_kernel<8>), grid, dim3(256), 0, st, ws, nslab, n4, out);
    else hipLaunchKernelGGL((acr_slab_sum_wide_kernel<4>), grid, dim3(128), 0, st, ws, nslab, n4, out);
    return true;
}

// Tail tiles of an NT / NN product (see gemm_tail_plan): sum the `nsplit` K-parts of every tail tile in part order
// (deterministic) and apply the epilogue of epilogue_f32<ACT> -- the same expressions, so a split tile differs from an
// unsplit one only by the grouping of its fp32 sum.  One thread = 4 consecutive columns of one row.
template <int ACT>
__global__ __launch_bounds__(256) void gemm_f32_tail_epilogue_kernel(const GemmF32Args g, const float* __restrict__ ws, int ntail,
                                                                     int nsplit) {
    const int tix = blockIdx.x >> 4;                        // 16 blocks of 256 threads per 128 x 128 tile
    const int e4 = ((blockIdx.x & 15) << 8) + threadIdx.x;  // float4 index inside the tile
    const int row_t = e4 >> 5, col_t = (e4 & 31) << 2;
    const int tt = g.tile0 + tix;
    int tm, tn;
    tile_coords(tt, g.tiles_m, g.tiles_n, tm, tn);
    const int row = tm * F_BM + row_t, col = tn * F_BN + col_t;
    if (row >= g.M || col >= g.N) return;                   // host: N % 4 == 0
    const float* p = ws + (int64_t)tix * (F_BM * F_BN) + row_t * F_BN + col_t;
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    for (int k = 1; k < nsplit; ++k) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(p + (int64_t)k * ntail * (F_BM * F_BN));
        v[0] += u[0]; v[1] += u[1]; v[2] += u[2]; v[3] += u[3];
    }
    if (ACT != 2 && g.bias) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(g.bias + col);
        v[0] += b4[0]; v[1] += b4[1]; v[2] += b4[2]; v[3] += b4[3];
    }
    float* cp = g.c + (int64_t)row * g.ldc + col;
    if (ACT == 0) {
        if (g.aux) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(g.aux + (int64_t)row * g.ldaux + col);
            v[0] += x[0]; v[1] += x[1]; v[2] += x[2]; v[3] += x[3];
        }
        *reinterpret_cast<f32x4*>(cp) = v;
    } else if (ACT == 1) {
        f32x4 d, a;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float er = erff(v[e] * 0.70710678118654752440f);
            a[e] = v[e] * 0.5f * (1.0f + er);
            d[e] = 0.5f * (1.0f + er) + v[e] * (expf(-0.5f * v[e] * v[e]) * 0.39894228040143267794f);
        }
        *reinterpret_cast<f32x4*>(g.c2 + (int64_t)row * g.ldc + col) = a;
        *reinterpret_cast<f32x4*>(cp) = d;
    } else {
        const f32x4 x = *reinterpret_cast<const f32x4*>(g.aux + (int64_t)row * g.ldaux + col);
        v[0] *= x[0]; v[1] *= x[1]; v[2] *= x[2]; v[3] *= x[3];
        *reinterpret_cast<f32x4*>(cp) = v;
    }
}
void gemm_f32_tail_epilogue(int act, const GemmF32Args& ge, const float* ws, int ntail, int nsplit, hipStream_t st) {
    const dim3 egrid((unsigned)(ntail * 16));
    if (act == 0) hipLaunchKernelGGL((gemm_f32_tail_epilogue_kernel<0>), egrid, dim3(256), 0, st, ge, ws, ntail, nsplit);
    else if (act == 1) hipLaunchKernelGGL((gemm_f32_tail_epilogue_kernel<1>), egrid, dim3(256), 0, st, ge, ws, ntail, nsplit);
    else hipLaunchKernelGGL((gemm_f32_tail_epilogue_kernel<2>), egrid, dim3(256), 0, st, ge, ws, ntail, nsplit);
}

// Tile quantisation of the NT / NN products (measured, scripts/lab/gemm_tail.py): the chip holds 512 workgroups (two per CU)
// and a launch's time is a step function of its tile count in units of 256 -- 1182 tiles (every 25 120 x 768 output of the
// step) cost 2.5 rounds for 2.31 rounds of work.  Plan: the leading multiple of 256 tiles runs as usual; the R remaining tiles
// are split s ways along K (R * s <= 512, all resident at once) into fp32 slabs, and one small kernel sums the parts in order
// and applies the epilogue.  Only worth it from s = 3 on (two halves at two per CU take what R tiles at one per CU take).
// x3 (products on images, gemm_f32_planes_kernel): a workgroup alone on its CU leaves every SIMD with ONE wave of six-term
// MFMA chains and nothing to cover its LDS reads, so launches of up to 256 tiles are split two ways as well.
TailPlan gemm_tail_plan(int M, int N, int K, bool x3) {
    TailPlan p = {0, 1, 0};
    if ((K % F_BK) != 0 || (N % 4) != 0) return p;
    const int tiles = ((M + F_BM - 1) / F_BM) * ((N + F_BN - 1) / F_BN);
    // A product of at most a third of the chip's 512 workgroup slots (CAM generation at batch 2: 18-170 tiles) is all tail:
    // every tile is K-split, up to 16 ways, so that the launch fills the CUs instead of running 24-96 chunks on a few of them.
    const bool small = x3 ? tiles <= 256 : tiles * 3 <= 512;
    const int R = small ? tiles : tiles % 256;
    if ((!small && tiles < 512) || R == 0) return p;
    const int smin = x3 && small ? 2 : 3;
    int s = 512 / R;
    if (s > (small ? 16 : 8)) s = small ? 16 : 8;
    const int maxs = K / (2 * F_BK);                         // at least two chunks per part
    if (s > maxs) s = maxs;
    if (s < smin) return p;
    const int kps = ((K + s - 1) / s + F_BK - 1) / F_BK * F_BK;
    s = (K + kps - 1) / kps;                                // every part non-empty
    if (s < smin) return p;
    p.ntail = R; p.nsplit = s; p.kps = kps;
    return p;
}

// the LDS-DMA kernels address operands with 32-bit element offsets inside one operand
static bool off32_ok(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int mode) {
    const int64_t lim = (1ll << 31) - (1 << 20);
    const int64_t ea = (mode == ACR_GEMM_TN ? K : M) * lda, eb = (mode == ACR_GEMM_NT ? N : K) * ldb;
    return ea < lim && eb < lim;
}
// Weight gradient: the token contraction is split over workgroups.  The chip holds 512 workgroups at a time (two per CU),
// so tiles x splits should fill whole rounds of 512: 576 workgroups take as long as 1024 (measured: fc1's dW with 4
// splits = 576 workgroups ran at 87 TF, the loop itself at the same 8.4k cycles per chunk as NT).  Pick the split count
// that minimises  rounds x chunks-per-split x t_chunk  +  slab traffic  (t_chunk = 3.5 us per 32-token chunk with two
// workgroups sharing a CU; slabs are written and read once at ~4 TB/s), at least 256 tokens per split.
TnPlan tn_plan(int M, int N, int K) {
    const int tiles = ((M + F_BM - 1) / F_BM) * ((N + F_BN - 1) / F_BN);
    const int maxs = (K + 255) / 256;
    double best = 1e30;
    int bns = 1;
    for (int ns = 1; ns <= maxs && ns <= 64; ++ns) {
        const int kps = ((K + ns - 1) / ns + F_BK - 1) / F_BK * F_BK;
        const int rounds = (tiles * ns + 511) / 512;
        const double t = rounds * (kps / (double)F_BK) * 3.5e-6 + (ns > 1 ? ns * (double)M * N * 8.0 / 4e12 : 0.0);
        if (t < best * 0.999) { best = t; bns = ns; }
    }
    int kps = ((K + bns - 1) / bns + F_BK - 1) / F_BK * F_BK;
    const int ns = (K + kps - 1) / kps;
    return {ns, kps};
}

size_t gemm_ws_base_floats(int mode, int M, int N, int K, bool x3) {
    if (mode != ACR_GEMM_TN) {
        const TailPlan tp = gemm_tail_plan(M, N, K, x3);
        return (size_t)tp.ntail * tp.nsplit * (F_BM * F_BN);
    }
    const TnPlan p = tn_plan(M, N, K);
    return (size_t)p.nsplit * ((size_t)M * N + (size_t)M);
}
extern "C" size_t acr_gemm_f32_ws_floats(int32_t mode, int32_t math, int32_t M, int32_t N, int32_t K) {
    const PlanesPlan pl = planes_plan(mode, math, M, N, K);
    return (gemm_ws_base_floats(mode, M, N, K, pl.on) + 3) / 4 * 4 + pl.a_fl + pl.b_fl + pl.cs_fl;
}

extern "C" int acr_gemm_f32(int32_t mode, int32_t math, int32_t act, const float* a, int64_t lda, const float* b, int64_t ldb, const float* bias,
                            const float* aux, int64_t ldaux, float* c, int64_t ldc, float* c2, float* colsum, int32_t M, int32_t N,
                            int32_t K, float* ws, void* stream) {
    ACR_CHECK_ARG(a && b && c, "acr_gemm_f32: null pointer");
    ACR_CHECK_ARG(M > 0 && N > 0 && K > 0, "acr_gemm_f32: empty problem (M=%d N=%d K=%d)", M, N, K);
    ACR_CHECK_ARG(mode >= ACR_GEMM_NT && mode <= ACR_GEMM_TN && act >= 0 && act <= 2, "acr_gemm_f32: bad mode %d / act %d", mode, act);
    ACR_CHECK_ARG(math == ACR_MATH_F32 || math == ACR_MATH_BF16X3 || math == ACR_MATH_FP16X2, "acr_gemm_f32: bad math %d", math);
    ACR_CHECK_ARG(al16(a) && al16(b) && (lda % 4) == 0 && (ldb % 4) == 0, "acr_gemm_f32: operands must be 16-byte aligned with pitches %% 4 == 0");
    hipStream_t st = (hipStream_t)stream;
    GemmF32Args g;
    g.a = a; g.lda = lda; g.b = b; g.ldb = ldb; g.bias = bias; g.aux = aux; g.ldaux = ldaux; g.c = c; g.ldc = ldc; g.c2 = c2;
    g.cs = nullptr; g.M = M; g.N = N; g.K = K;
    g.tiles_m = (M + F_BM - 1) / F_BM; g.tiles_n = (N + F_BN - 1) / F_BN; g.nsplit = 1; g.kps = (K + F_BK - 1) / F_BK * F_BK;
    g.a_zs = g.b_zs = g.c_zs = g.aux_zs = 0; g.k_zs = g.kps; g.ksplit = 1 << 30;
    g.tile0 = 0; g.tiles_launch = g.tiles_m * g.tiles_n;
    dim3 grid((unsigned)(g.tiles_m * g.tiles_n));
    if (mode == ACR_GEMM_TN) {
        // c[M,N] = a[K,M]^T b[K,N]: both operands contraction-strided; M, N are the weight's dims, K the token count
        ACR_CHECK_ARG(act == 0 && !bias && !aux, "acr_gemm_f32: TN takes no epilogue");
        ACR_CHECK_ARG(ws, "acr_gemm_f32: TN needs the acr_gemm_f32_ws_floats workspace");
        ACR_CHECK_ARG((M % 4) == 0 && (N % 4) == 0 && M >= 4 && N >= 4 && ldc == N && al16(c), "acr_gemm_f32: TN needs M, N %% 4 == 0 and a dense output (ldc == N)");
        const TnPlan p = tn_plan(M, N, K);
        g.nsplit = p.nsplit; g.kps = p.kps; g.k_zs = p.kps;
        g.c = ws; g.ldc = N;
        g.cs = colsum ? ws + (size_t)p.nsplit * M * N : nullptr;
        const PlanesPlan pl = planes_plan(mode, math, M, N, K);
        if (pl.on && math == ACR_MATH_FP16X2) {             // column-scaled images of both operands (+ a's column sums), then the product
            ACR_CHECK_ARG(al16(ws), "acr_gemm_f32: ws must be 16-byte aligned");
            float* pa = ws + (gemm_ws_base_floats(mode, M, N, K, true) + 3) / 4 * 4;
            float* pb = pa + pl.a_fl;
            float* cw = pb + pl.b_fl;
            h2_image_cols(a, lda, K, M, pa, colsum, cw, st);
            h2_image_cols(b, ldb, K, N, pb, nullptr, cw, st);
            return gemm_planes<1>(ACR_GEMM_TN, 0, pa, pb, nullptr, nullptr, 0, c, ldc, nullptr, nullptr, M, N, K, ws, h2_exps(pa, K, M), h2_exps(pb, K, N), st);
        }
        if (pl.on) {                                        // both operands split once into images, then the product on the images
            float* wp = ws + (gemm_ws_base_floats(mode, M, N, K, true) + 3) / 4 * 4;
            float* pa = wp;
            float* pb = wp + pl.a_fl;
            int rc = acr_x3_image(a, lda, K, M, pa, colsum, colsum ? wp + pl.a_fl + pl.b_fl : nullptr, stream);
            if (rc == ACR_OK) rc = acr_x3_image(b, ldb, K, N, pb, nullptr, nullptr, stream);
            if (rc == ACR_OK) rc = acr_gemm_x3(ACR_GEMM_TN, 0, pa, pb, nullptr, nullptr, 0, c, ldc, nullptr, nullptr, M, N, K, ws, stream);
            return rc;
        }
        if ((K % F_BK) == 0 && off32_ok(M, N, K, lda, ldb, mode) && math == ACR_MATH_BF16X3)
            hipLaunchKernelGGL((gemm_f32_split_kernel<false, false, 3>), dim3((unsigned)(g.tiles_m * g.tiles_n * p.nsplit)), dim3(256), 0, st, g);
        else if ((K % F_BK) == 0 && off32_ok(M, N, K, lda, ldb, mode))
            hipLaunchKernelGGL((gemm_f32_dma_kernel<false, false, 3>), dim3((unsigned)(g.tiles_m * g.tiles_n * p.nsplit)), dim3(256), 0, st, g);
        else
            hipLaunchKernelGGL((gemm_f32_kernel<false, false, 3>), dim3((unsigned)(g.tiles_m * g.tiles_n * p.nsplit)), dim3(256), 0, st, g);
        gemm_f32_reduce(ws, p.nsplit, (int64_t)M * N / 4, c, st);
        if (colsum)
            hipLaunchKernelGGL(gemm_f32_reduce1_kernel, dim3((M + 255) / 256), dim3(256), 0, st, (const float*)g.cs, p.nsplit, M, colsum);
        return acr_check_launch("acr_gemm_f32(TN)");
    }
    ACR_CHECK_ARG((K % 4) == 0 && K >= 4, "acr_gemm_f32: NT / NN need K %% 4 == 0 (K=%d)", K);
    if (mode == ACR_GEMM_NN) ACR_CHECK_ARG((N % 4) == 0 && N >= 4, "acr_gemm_f32: NN needs N %% 4 == 0 (N=%d)", N);
    ACR_CHECK_ARG(act != 1 || c2, "acr_gemm_f32: act 1 (GELU) needs c2");
    ACR_CHECK_ARG(act != 2 || aux, "acr_gemm_f32: act 2 (GELU') needs the saved pre-activation in aux");
#define ACR_F32_LAUNCH(AK, BK_, ACTV)                                                                              \
    do {                                                                                                            \
        if (dma && split) hipLaunchKernelGGL((gemm_f32_split_kernel<AK, BK_, ACTV>), grid, dim3(256), 0, st, g);   \
        else if (dma) hipLaunchKernelGGL((gemm_f32_dma_kernel<AK, BK_, ACTV>), grid, dim3(256), 0, st, g);          \
        else hipLaunchKernelGGL((gemm_f32_kernel<AK, BK_, ACTV>), grid, dim3(256), 0, st, g);                      \
    } while (0)
    const bool split = math == ACR_MATH_BF16X3;                   // products as six bf16 MFMA terms of a three-way split
    const bool dma = (K % F_BK) == 0 && off32_ok(M, N, K, lda, ldb, mode);
    TailPlan tp = gemm_tail_plan(M, N, K);
    const bool vec_ok = al16(c) && (ldc % 4) == 0 && (!bias || al16(bias)) && (!aux || (al16(aux) && (ldaux % 4) == 0)) &&
                        (!c2 || al16(c2));
    if (!dma || !ws || !al16(ws) || !vec_ok) tp.ntail = 0;
    if (tp.ntail) {                                         // leading whole half-rounds as usual ...
        g.tiles_launch -= tp.ntail;
        grid = dim3((unsigned)g.tiles_launch);
    }
    const PlanesPlan pl = planes_plan(mode, math, M, N, K);
    if (math == ACR_MATH_FP16X2) {                          // row-scaled images of a and b (NN: of b^T), then the product; no other way
        ACR_CHECK_ARG(ws && al16(ws) && vec_ok, "acr_gemm_f32: fp16x2 needs the acr_gemm_f32_ws_floats workspace (16-byte aligned) and 16-byte aligned c / bias / aux / c2");
        float* pa = ws + (gemm_ws_base_floats(mode, M, N, K, true) + 3) / 4 * 4;
        float* pb = pa + pl.a_fl;
        h2_image_rows(a, lda, M, K, pa, nullptr, nullptr, st);
        if (mode == ACR_GEMM_NT) h2_image_rows(b, ldb, N, K, pb, nullptr, nullptr, st);
        else h2_image_t(b, ldb, K, N, pb, pb + pl.b_fl, st);
        return gemm_planes<1>(ACR_GEMM_NT, act, pa, pb, bias, aux, ldaux, c, ldc, c2, nullptr, M, N, K, ws, h2_exps(pa, M, K), h2_exps(pb, N, K), st);
    }
    if (pl.on && ws && al16(ws) && vec_ok) {                // both operands split once into images, then the product on the images
        float* wp = ws + (gemm_ws_base_floats(mode, M, N, K, true) + 3) / 4 * 4;
        float* pa = wp;
        float* pb = wp + pl.a_fl;
        int rc = acr_x3_image(a, lda, M, K, pa, nullptr, nullptr, stream);
        if (rc == ACR_OK) rc = mode == ACR_GEMM_NT ? acr_x3_image(b, ldb, N, K, pb, nullptr, nullptr, stream) : acr_x3_image_t(b, ldb, K, N, pb, stream);
        if (rc == ACR_OK) rc = acr_gemm_x3(ACR_GEMM_NT, act, pa, pb, bias, aux, ldaux, c, ldc, c2, nullptr, M, N, K, ws, stream);
        return rc;
    }
    if (g.tiles_launch == 0) {                              // a small product: every tile goes the K-split way
    } else if (mode == ACR_GEMM_NT) {
        if (act == 0) ACR_F32_LAUNCH(true, true, 0);
        else if (act == 1) ACR_F32_LAUNCH(true, true, 1);
        else ACR_F32_LAUNCH(true, true, 2);
    } else {
        if (act == 0) ACR_F32_LAUNCH(true, false, 0);
        else if (act == 1) ACR_F32_LAUNCH(true, false, 1);
        else ACR_F32_LAUNCH(true, false, 2);
    }
#undef ACR_F32_LAUNCH
    if (tp.ntail) {                                         // ... then the tail tiles, K-split into slabs, and their epilogue
        GemmF32Args gt = g;
        gt.tile0 = g.tiles_launch; gt.tiles_launch = tp.ntail; gt.nsplit = tp.nsplit; gt.kps = tp.kps; gt.k_zs = tp.kps;
        gt.c = ws;
        const dim3 tgrid((unsigned)(tp.ntail * tp.nsplit));
        if (mode == ACR_GEMM_NT && split) hipLaunchKernelGGL((gemm_f32_split_kernel<true, true, 4>), tgrid, dim3(256), 0, st, gt);
        else if (mode == ACR_GEMM_NT) hipLaunchKernelGGL((gemm_f32_dma_kernel<true, true, 4>), tgrid, dim3(256), 0, st, gt);
        else if (split) hipLaunchKernelGGL((gemm_f32_split_kernel<true, false, 4>), tgrid, dim3(256), 0, st, gt);
        else hipLaunchKernelGGL((gemm_f32_dma_kernel<true, false, 4>), tgrid, dim3(256), 0, st, gt);
        GemmF32Args ge = g;
        ge.tile0 = gt.tile0;
        gemm_f32_tail_epilogue(act, ge, ws, tp.ntail, tp.nsplit, st);
    }
    return acr_check_launch("acr_gemm_f32");
}

// The 1x1 convolutions of the stem run on the loops of this file, one z-slice per sample (conv1x1.hip); these are their instances.
void gemm_f32_conv_launch(int loop, bool a_kc, bool b_kc, int act, dim3 grid, const GemmF32Args& g, hipStream_t st) {
#define CONV_LOOPS(AK, BK_, ACTV)                                                                                             \
    do {                                                                                                                      \
        if (loop == GEMM_LOOP_SPLIT) hipLaunchKernelGGL((gemm_f32_split_kernel<AK, BK_, ACTV>), grid, dim3(256), 0, st, g); \
        else if (loop == GEMM_LOOP_DMA) hipLaunchKernelGGL((gemm_f32_dma_kernel<AK, BK_, ACTV>), grid, dim3(256), 0, st, g); \
        else hipLaunchKernelGGL((gemm_f32_kernel<AK, BK_, ACTV>), grid, dim3(256), 0, st, g);                           \
    } while (0)
    if (act == 3 && a_kc && !b_kc) hipLaunchKernelGGL((gemm_f32_split_kernel<true, false, 3>), grid, dim3(256), 0, st, g);   // K-split forward: split products only
    else if (act == 3 && a_kc) CONV_LOOPS(true, true, 3);
    else if (act == 3) CONV_LOOPS(false, false, 3);
    else if (a_kc) CONV_LOOPS(true, false, 0);
    else CONV_LOOPS(false, false, 0);
#undef CONV_LOOPS
}
