// Products on pre-split, pre-tiled operand images (include/acr_hip.h "split-product images"): the image passes, the image
// epilogues, the plane GEMMs and the acr_x3_* / acr_h2_* / acr_gemm_x3 / acr_gemm_h2 entries.
#include <math.h>

#include <mutex>
#include <type_traits>
#include <unordered_map>

#include "gemm_f32.h"

// ---------------------------------------------------------------------------------------------------------------------------------
// Split products on PRE-SPLIT, PRE-TILED operands (round 4).  gemm_f32_split_kernel splits its operand tiles in registers:
// ~200 VALU instructions per 24 MFMAs per wave, and every operand element is split again by every workgroup that reads it
// (N / 128 resp. M / 128 times); its counters (profiles/r04_pmc_split_gemm.txt) show the VALU port -- which also issues the
// MFMAs -- busy 66 % of the time and the matrix pipe 57 %.  Here every operand is split ONCE per product by a streaming pass
// (planes_tile_kernel / planes_tile_t_kernel: HBM-bound, 10 bytes per element) into three bf16 planes in the workspace,
// transposed on the way where the product needs it, so that ONE kernel flavour (both operands [row][k]) serves NT, NN and TN
// and its loop is DMA + ds_read_b128 + MFMA only.
// The planes are stored TILED, in exactly the image the kernel wants in LDS: for row block rb (128 rows) and stage kb (16
// contraction elements) the three 4 KiB planes [128 rows][32 bytes] follow each other,
//     byte offset = IMG_STAGE_OFF(rb, nkb, kb, 3) + p * IMG_PLANE_B + planes_chunk_off(row, khalf) + 2 * (k & 7)      (acr_split.h),
// so a stage of an operand is 12 KiB of CONTIGUOUS memory and every LDS-DMA instruction copies one contiguous KiB.  The first
// version kept dense row-major planes: 32 bytes per row and stage made every DMA instruction touch 32 cache lines, the
// texture-address units were busy 95 % of the kernel and the matrix pipe 37 % (profiles/r04_pmc_planes_gemm_first_version.txt).
// The half swap (bit 3 of the row) makes the 16 lanes a ds_read_b128 serves per cycle hit 16 different 16-byte bank groups.
// Rows past the operand's end and contraction indices past K are zero in the image (no clamps, no K % 16 condition).
// Ring of 3 slots x [A p0 p1 p2 | B p0 p1 p2], DMA two stages ahead (6 pieces per wave and stage; waves 0-1 fetch A, 2-3 B).
// The reads of stage st and the refill of the ring are interleaved with the 24 MFMAs of stage st - 1 in program order
// (sched_barrier between the groups: inline-asm reads are invisible to sched_group_barrier).
// ---------------------------------------------------------------------------------------------------------------------------------

// Image formats of the planes kernels (template parameter FMT):
//   0  bf16x3: three bf16 planes, six MFMA terms per tile and stage (v_mfma_f32_32x32x16_bf16);
//   1  fp16x2: two fp16 planes of x * 2^e, e an exact power-of-two scale per NON-contracted index (row of an NT operand, column of
//      a TN operand, acr_h2_image*), three terms (v_mfma_f32_32x32x16_f16, same lane maps and rate), ldexp(acc, -(e_a + e_b))
//      before the epilogue.  A stage carries 2 planes instead of 3: 16 KiB instead of 24, 4 DMA pieces per wave instead of 6.
// Terms are issued smallest first: (0,2) (2,0) (1,1) (0,1) (1,0) (0,0) resp. (0,1) (1,0) (0,0).
template <int FMT>
__device__ __forceinline__ f32x16 pl_mfma(bf16x8 a, bf16x8 b, f32x16 c) {
    if constexpr (FMT == 0) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// MFMAs M0 .. M1 - 1 of a stage (m = tile * NT + term, tile = 2 I + J) on register sets a[block][plane], b[block][plane]
template <int FMT, int M0, int M1>
__device__ __forceinline__ void pl_mfmas(f32x16 (&acc)[2][2], const bf16x8 (&a)[2][PlanesFmt<FMT>::NP], const bf16x8 (&b)[2][PlanesFmt<FMT>::NP]) {
    if constexpr (M0 < M1) {
        constexpr int NT = PlanesFmt<FMT>::NT, t = M0 / NT, k = M0 % NT;
        acc[t >> 1][t & 1] = pl_mfma<FMT>(a[t >> 1][pl_ta(FMT, k)], b[t & 1][pl_tb(FMT, k)], acc[t >> 1][t & 1]);
        pl_mfmas<FMT, M0 + 1, M1>(acc, a, b);
    }
}
// the same on the transposed reads of gemm_f32_planes_tn_kernel (fragment = lo tokens | hi tokens)
template <int FMT, int M0, int M1>
__device__ __forceinline__ void pt_mfmas(f32x16 (&acc)[2][2], const bf16x4 (&al)[2][PlanesFmt<FMT>::NP], const bf16x4 (&ah)[2][PlanesFmt<FMT>::NP],
                                         const bf16x4 (&bl)[2][PlanesFmt<FMT>::NP], const bf16x4 (&bh)[2][PlanesFmt<FMT>::NP]) {
    if constexpr (M0 < M1) {
        constexpr int NT = PlanesFmt<FMT>::NT, t = M0 / NT, k = M0 % NT;
        constexpr int I = t >> 1, J = t & 1, PA = pl_ta(FMT, k), PB = pl_tb(FMT, k);
        acc[I][J] = pl_mfma<FMT>(__builtin_shufflevector(al[I][PA], ah[I][PA], 0, 1, 2, 3, 4, 5, 6, 7),
                                 __builtin_shufflevector(bl[J][PB], bh[J][PB], 0, 1, 2, 3, 4, 5, 6, 7), acc[I][J]);
        pt_mfmas<FMT, M0 + 1, M1>(acc, al, ah, bl, bh);
    }
}
// fp16x2: acc *= 2^-(e_a[row] + e_b[col]) for one wave's 64 x 64 block (rows mb.., columns nb..); exact unless the result is subnormal
__device__ __forceinline__ void h2_unscale(const GemmF32Args& g, f32x16 (&acc)[2][2], int mb, int nb, int r, int h) {
    const int eb0 = g.eb[min(nb + r, g.N - 1)], eb1 = g.eb[min(nb + 32 + r, g.N - 1)];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ea = g.ea[min(mb + i * 32 + acr_krow(e, h), g.M - 1)];
            acc[i][0][e] = ldexpf(acc[i][0][e], -(ea + eb0));
            acc[i][1][e] = ldexpf(acc[i][1][e], -(ea + eb1));
        }
}

// ---- the split passes (HBM-bound: 4 bytes read, 6 written per element) ----------------------------------------------------------
// the planes of one 16-byte chunk in image format FMT (planes IMG_PLANE_B apart): bf16x3, or fp16x2 with exponents e
template <int FMT>
__device__ __forceinline__ void planes_write8(char* dst, const float (&v)[8], const int (&e)[8]) {
    if constexpr (FMT == 0) {
        bf16x8 p0, p1, p2;
        split3_bf16(v, p0, p1, p2);
        *reinterpret_cast<bf16x8*>(dst) = p0;
        *reinterpret_cast<bf16x8*>(dst + IMG_PLANE_B) = p1;
        *reinterpret_cast<bf16x8*>(dst + 2 * IMG_PLANE_B) = p2;
    } else {
        bf16x8 p0, p1;
        h2_split8(v, e, p0, p1);
        *reinterpret_cast<bf16x8*>(dst) = p0;
        *reinterpret_cast<bf16x8*>(dst + IMG_PLANE_B) = p1;
    }
}

// tiled image of x[row][k] (pitch ld floats; the operand's rows are x's rows).  Workgroup = row block rb x 4 stages (64 k);
// thread -> 4 chunks of 8 k: a row's 256 bytes are read by 8 neighbouring threads, a stage's 8 rows x 32 bytes written by 16.
// FMT 0: bf16x3 image.  FMT 1: fp16x2, exponent ex[row] (row-scaled).  FMT 2: fp16x2, exponent ex[k] (column-scaled).
template <int FMT>
__global__ __launch_bounds__(256) void planes_tile_kernel(const float* __restrict__ x, int64_t ld, int rows, int K, int nkb, char* __restrict__ img,
                                                          float* __restrict__ colpart, const int* __restrict__ ex) {
    constexpr int NP = PlanesFmt<FMT == 0 ? 0 : 1>::NP;
    __shared__ float red[32 * 64];
    const int kq = (nkb + 3) >> 2;
    const int rb = blockIdx.x / kq, k0 = (blockIdx.x - rb * kq) << 6;
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = j * 256 + threadIdx.x, rr = c >> 3, k8 = c & 7;
        const int row = rb * 128 + rr, k = k0 + k8 * 8;
        if (k >= nkb * P_BK) continue;
        float v[8];
        if (row < rows && k + 8 <= K) {
            const float* src = x + (int64_t)row * ld + k;
            const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src));
            const f32x4 b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + 4));
            v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (row < rows && k + e < K) ? x[(int64_t)row * ld + k + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) cs[e] += v[e];
        int ev[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) ev[e] = FMT == 1 ? ex[row] : FMT == 2 ? ex[k + e] : 0;
        planes_write8<FMT == 0 ? 0 : 1>(img + IMG_STAGE_OFF(rb, nkb, k >> 4, NP) + planes_chunk_off(rr, k8 & 1), v, ev);
    }
    if (colpart) {                                          // column sums of this row block (bias gradient part): thread = rows
        const int tid = threadIdx.x;                        // (tid >> 3) + 32 j of the 8 columns 8 (tid & 7) ..; fixed summation order
#pragma unroll
        for (int e = 0; e < 8; ++e) red[(tid >> 3) * 64 + (tid & 7) * 8 + e] = cs[e];
        __syncthreads();
        if (tid < 64 && k0 + tid < K) {
            float t = red[tid];
            for (int q = 1; q < 32; ++q) t += red[q * 64 + tid];
            colpart[(int64_t)rb * K + k0 + tid] = t;
        }
    }
}
// tiled image of the TRANSPOSE of x[rw][c] (pitch ld): operand rows = x's columns, contraction = x's rows (R of them).  64 x 64
// blocks through an fp32 LDS tile (pitch 65: the column reads are conflict-free); thread (c = tid & 63, q = tid >> 6) then
// holds the 16 contraction elements 16 q .. 16 q + 15 of operand row c0 + c = one whole stage row (32 bytes per plane).
// colpart (or null): per 64-row block of x the column sums of the block (bias gradient parts, summed in block order by
// gemm_f32_reduce1_kernel: deterministic).  FMT 0: bf16x3.  FMT 1: fp16x2 with exponent ex[operand row] (row-scaled).
template <int FMT>
__global__ __launch_bounds__(256) void planes_tile_t_kernel(const float* __restrict__ x, int64_t ld, int R, int C, int nkb, char* __restrict__ img,
                                                            float* __restrict__ colpart, const int* __restrict__ ex) {
    constexpr int NP = PlanesFmt<FMT>::NP;
    __shared__ float tile[64 * 65];
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const int cblocks = ((C + 127) >> 7) << 1;             // whole 128-row blocks of the operand (zeros past C)
    const int rb = blockIdx.x / cblocks, cb = blockIdx.x - rb * cblocks;
    const int r0 = rb << 6, c0 = cb << 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {                            // 64 rows x 16 float4
        const int e = i * 256 + tid, rr = e >> 4, c4 = (e & 15) << 2;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + rr < R) {
            const float* src = x + (int64_t)(r0 + rr) * ld + c0 + c4;
            if (c0 + c4 + 4 <= C) v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src));
            else
#pragma unroll
                for (int q = 0; q < 4; ++q) if (c0 + c4 + q < C) v[q] = src[q];
        }
        float* d = tile + rr * 65 + c4;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    __syncthreads();
    const int c = tid & 63, gq = tid >> 6;
    float v0[8], v1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { v0[e] = tile[(gq * 16 + e) * 65 + c]; v1[e] = tile[(gq * 16 + 8 + e) * 65 + c]; }
    if (colpart) {
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += v0[e];
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += v1[e];
        red[tid] = sum;
        __syncthreads();
        if (tid < 64 && c0 + tid < C) colpart[(int64_t)rb * C + c0 + tid] = (red[tid] + red[tid + 64]) + (red[tid + 128] + red[tid + 192]);
    }
    const int kb = (r0 >> 4) + gq;                          // stage of these 16 contraction elements
    if (kb >= nkb) return;
    const int orow = c0 + c;                                // operand row (rows past C inside the last 128-row block: zeros from the loads above)
    char* dst = img + IMG_STAGE_OFF(orow >> 7, nkb, kb, NP);
    const int rr = orow & 127;
    int ev[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) ev[e] = FMT == 1 ? ex[orow] : 0;
    planes_write8<FMT>(dst + planes_chunk_off(rr, 0), v0, ev);
    planes_write8<FMT>(dst + planes_chunk_off(rr, 1), v1, ev);
}

// ---- fp16x2 scale exponents (include/acr_hip.h "fp16x2 images") ------------------------------------------------------------------
// row-scaled: one wave per row of x (rows x K, pitch ld); ex[row] for row < nexp (0 past rows); writes the direction flag
__global__ __launch_bounds__(256) void h2_rowexp_kernel(const float* __restrict__ x, int64_t ld, int rows, int K, int nexp, int* __restrict__ ex,
                                                        int* __restrict__ flag, int dir) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x < 4) flag[threadIdx.x] = threadIdx.x == 0 ? dir : 0;
    if (row >= nexp) return;
    float m = 0.f;
    if (row < rows) {
        const float* p = x + (int64_t)row * ld;
        const int k4 = K >> 2;
#pragma unroll 4
        for (int i = lane; i < k4; i += 64) {
            const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i);
            m = h2_absmax(h2_absmax(m, v[0]), v[1]); m = h2_absmax(h2_absmax(m, v[2]), v[3]);
        }
        for (int k = 4 * k4 + lane; k < K; k += 64) m = h2_absmax(m, p[k]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) ex[row] = h2_exp(m);
}
// column-scaled, pass 1: per 128-row block rb of x (R x C, pitch ld % 4 == 0, 16-byte aligned) the column maxima part[rb][c].
// Workgroup = (rb, 256 columns); thread = 4 columns (4 (tid & 63)) x every 4th row from (tid >> 6), float4 loads; the four row
// quarters are combined through LDS (a maximum: the result does not depend on the order)
__global__ __launch_bounds__(256) void h2_colmax_kernel(const float* __restrict__ x, int64_t ld, int R, int C, float* __restrict__ part) {
    __shared__ f32x4 red[256];
    const int tid = threadIdx.x, rb = blockIdx.x, q = tid >> 6;
    const int c0 = blockIdx.y * 256 + (tid & 63) * 4, r1 = min(R, rb * 128 + 128);
    f32x4 m = {0.f, 0.f, 0.f, 0.f};
    if (c0 + 4 <= C) {
#pragma unroll 8
        for (int r = rb * 128 + q; r < r1; r += 4) {
            const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x + (int64_t)r * ld + c0));
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = h2_absmax(m[e], v[e]);
        }
    } else if (c0 < C) {
        for (int r = rb * 128 + q; r < r1; r += 4)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c0 + e < C) m[e] = h2_absmax(m[e], x[(int64_t)r * ld + c0 + e]);
    }
    red[tid] = m;
    __syncthreads();
    if (tid < 64) {
        const f32x4 u = red[tid], v = red[tid + 64], w = red[tid + 128], z = red[tid + 192];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c0 + e < C) part[(int64_t)rb * C + c0 + e] = fmaxf(fmaxf(u[e], v[e]), fmaxf(w[e], z[e]));
    }
}
// pass 2: ex[c] from the nparts row-block maxima (0 for c in [C, nexp)); workgroup = 64 columns, thread (c, q = tid >> 6) takes
// every 4th part from q, quarters combined through LDS; writes the direction flag
__global__ __launch_bounds__(256) void h2_colexp_kernel(const float* __restrict__ part, int nparts, int C, int nexp, int* __restrict__ ex,
                                                        int* __restrict__ flag, int dir) {
    __shared__ float red[256];
    const int tid = threadIdx.x, c = blockIdx.x * 64 + (tid & 63), q = tid >> 6;
    if (blockIdx.x == 0 && tid < 4) flag[tid] = tid == 0 ? dir : 0;
    float m = 0.f;
    if (c < C) {
#pragma unroll 4
        for (int k = q; k < nparts; k += 4) m = fmaxf(m, part[(int64_t)k * C + c]);
    }
    red[tid] = m;
    __syncthreads();
    if (tid < 64 && c < nexp) ex[c] = h2_exp(fmaxf(fmaxf(red[tid], red[tid + 64]), fmaxf(red[tid + 128], red[tid + 192])));
}

// MANY small images in one launch (round 5): the stem's 52 standardised convolution weights need up to two images each per step
// (W for the forward, W^T resp. the flipped / role-swapped pack for the input gradient) -- as ~130 launches of a few microseconds
// (planes_tile / planes_tile_t plus the permute copies that packed the 3x3 weights) they cost more than the passes move.  Every
// image is described by a strided view of its source: element (r, k) of the rows x K operand is
//     src[r * sr + (k / kin) * sko + (k % kin) * ski]            (kin % 8 == 0: a chunk of 8 k never straddles an outer index)
// which covers W (co x ci: sr = ci, kin = K, ski = 1), W^T (sr = 1, ski = ci), the packed 3x3 weight w[co][t * ci + c] of
// w (co, ci, 3, 3) (sr = 9 ci, kin = ci, sko = 1, ski = 9) and its input-gradient pack w[o][c][8 - t'] as (ci x 9 co)
// (src + 8, sr = 9, kin = co, sko = -1, ski = 9 ci).  Workgroup = (image, row block, 64 k) as in planes_tile_kernel; `blk` maps a
// workgroup to its image.  Reads are strided (the weights are a few MB: L2-resident), writes are the image's contiguous chunks.
struct X3ManyDesc : acr_x3_many_desc {};   // the header's record under the name the kernel's symbol carries
__global__ __launch_bounds__(256) void planes_tile_many_kernel(const X3ManyDesc* __restrict__ descs, const int32_t* __restrict__ blk) {
    const X3ManyDesc d = descs[blk[blockIdx.x]];
    const int local = (int)blockIdx.x - d.wg0;
    const int kq = (d.nkb + 3) >> 2;
    const int rb = local / kq, k0 = (local - rb * kq) << 6;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = j * 256 + threadIdx.x, rr = c >> 3, k8 = c & 7;
        const int row = rb * 128 + rr, k = k0 + k8 * 8;
        if (k >= d.nkb * P_BK) continue;
        float v[8];
        if (row < d.rows && k < d.K) {                      // K % 8 == 0 (host): the chunk is whole
            const int outer = k / d.kin, inner = k - outer * d.kin;
            const float* sp = d.src + (int64_t)row * d.sr + (int64_t)outer * d.sko + (int64_t)inner * d.ski;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = sp[(int64_t)e * d.ski];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
        }
        bf16x8 p0, p1, p2;
        split3_bf16(v, p0, p1, p2);
        char* dst = (char*)d.dst + IMG_STAGE_OFF(rb, d.nkb, k >> 4, 3) + planes_chunk_off(rr, k8 & 1);
        *reinterpret_cast<bf16x8*>(dst) = p0;
        *reinterpret_cast<bf16x8*>(dst + IMG_PLANE_B) = p1;
        *reinterpret_cast<bf16x8*>(dst + 2 * IMG_PLANE_B) = p2;
    }
}
extern "C" int acr_x3_image_many(const void* descs, const int32_t* blk, int32_t nwg, void* stream) {
    ACR_CHECK_ARG(descs && blk && nwg > 0, "acr_x3_image_many: null table or empty launch");
    ACR_CHECK_ARG(((uintptr_t)descs & 7) == 0 && ((uintptr_t)blk & 3) == 0, "acr_x3_image_many: table alignment");
    hipLaunchKernelGGL(planes_tile_many_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const X3ManyDesc*)descs, blk);
    return acr_check_launch("acr_x3_image_many");
}

// ---- image epilogues: the product's output leaves the kernel AS the image the next product reads -----------------------------
// ACT 5 (fc1 forward): h = acc + bias; c = GELU'(h) in fp32 (all the backward needs of h), c2 = IMAGE of GELU(h) -- fc2's operand
//        in the forward and in its weight gradient; the fp32 activation is never written.
// ACT 6 (fc2's input gradient): c2 = IMAGE of acc * aux (aux = the saved GELU'(h)) -- fc1's dy for its input and weight gradient;
//        cs = per-tile-row parts of its column sums (fc1's bias gradient, summed in tile-row order by planes_colsum_kernel);
//        no fp32 output at all.
// Saves the 25 120 x 3072 image passes of both tensors (0.135 ms each, 24 per step) and their fp32 writes.  Rows past M and
// columns past N are written as zeros (the image contract).
#define X3E_PITCH 132                 // floats: 528 bytes, 16-byte aligned rows
// one 16-byte chunk (row row_t of row block tm, columns 8 c8 .. + 7 of output tile column tn) of all three planes
__device__ __forceinline__ void x3_image_chunk_store(char* img, int tm, int tn, int nkb, int row_t, int c8, const float (&v)[8]) {
    const int kb = tn * 8 + (c8 >> 1);
    if (kb >= nkb) return;
    bf16x8 p0, p1, p2;
    split3_bf16(v, p0, p1, p2);
    char* dst = img + IMG_STAGE_OFF(tm, nkb, kb, 3) + planes_chunk_off(row_t, c8 & 1);
    *reinterpret_cast<bf16x8*>(dst) = p0;
    *reinterpret_cast<bf16x8*>(dst + IMG_PLANE_B) = p1;
    *reinterpret_cast<bf16x8*>(dst + 2 * IMG_PLANE_B) = p2;
}
// Thread -> chunks of an output tile: pass (half, j) handles row 32 j + (tid >> 3), columns 64 half + 8 (tid & 7) .. + 7 -- the
// mapping of planes_tile_kernel, so that the column sums below add the same numbers in the same order as the image pass would
// (a bias gradient does not depend on which of the two produced the image, bit for bit).
// column sums of a tile from the per-thread sums csum[half][e], through `red` (>= 4096 floats of LDS nobody else is using)
__device__ __forceinline__ void x3_tile_colsum(const float (&csum)[2][8], float* red, int tid, float* parts_row, int n0, int N) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[(tid >> 3) * 128 + hf * 64 + (tid & 7) * 8 + e] = csum[hf][e];
    __syncthreads();
    if (tid < 128 && n0 + tid < N) {
        float t = red[tid];
        for (int q = 1; q < 32; ++q) t += red[q * 128 + tid];
        parts_row[n0 + tid] = t;
    }
}
template <int ACT>
__device__ __forceinline__ void x3_finish_image(const GemmF32Args& g, f32x16 (&acc)[2][2], float* tl, int tm, int tn, int m0, int n0, int wm,
                                                int wn, int r, int h, int tid) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col_t = wn * 64 + j * 32 + r, col = n0 + col_t;
        const bool cok = col < g.N;
        const float bj = (ACT == 5 && g.bias && cok) ? g.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float x[16];
            if (ACT == 6) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = m0 + wm * 64 + i * 32 + acr_krow(e, h);
                    x[e] = (row < g.M && cok) ? g.aux[(int64_t)row * g.ldaux + col] : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row_t = wm * 64 + i * 32 + acr_krow(e, h), row = m0 + row_t;
                const bool ok = row < g.M && cok;
                float val;
                if (ACT == 5) {
                    const float v = acc[i][j][e] + bj;
                    const float er = erff(v * 0.70710678118654752440f);
                    val = v * 0.5f * (1.0f + er);
                    if (ok) g.c[(int64_t)row * g.ldc + col] = 0.5f * (1.0f + er) + v * (expf(-0.5f * v * v) * 0.39894228040143267794f);
                } else {
                    val = acc[i][j][e] * x[e];
                }
                tl[row_t * X3E_PITCH + col_t] = ok ? val : 0.f;
            }
        }
    }
    __syncthreads();
    char* img = reinterpret_cast<char*>(g.c2);
    float csum[2][8];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int e = 0; e < 8; ++e) csum[hf][e] = 0.f;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row_t = j * 32 + (tid >> 3), c8 = hf * 8 + (tid & 7);
            const f32x4 a = *reinterpret_cast<const f32x4*>(tl + row_t * X3E_PITCH + c8 * 8);
            const f32x4 b = *reinterpret_cast<const f32x4*>(tl + row_t * X3E_PITCH + c8 * 8 + 4);
            const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
            if (ACT == 6) {
#pragma unroll
                for (int e = 0; e < 8; ++e) csum[hf][e] += v[e];
            }
            x3_image_chunk_store(img, tm, tn, g.img_nkb, row_t, c8, v);
        }
    if (ACT == 6 && g.cs) {
        __syncthreads();                                    // every thread is done reading the tile: reuse it for the reduction
        x3_tile_colsum(csum, tl, tid, g.cs + (int64_t)tm * g.N, n0, g.N);
    }
}
// The same for K-split tail tiles (gemm_tail_plan): one workgroup per tail tile sums its `nsplit` slabs in part order -- a slab is
// row-major, so a thread's 8 consecutive columns are two float4 per part -- applies the epilogue and writes the image chunks.
template <int ACT>
__global__ __launch_bounds__(256) void gemm_x3_tail_image_kernel(const GemmF32Args g, const float* __restrict__ ws, int ntail, int nsplit) {
    __shared__ float red[4096];
    const int tid = threadIdx.x, tix = blockIdx.x;
    const int tt = g.tile0 + tix;
    int tm, tn;
    tile_coords(tt, g.tiles_m, g.tiles_n, tm, tn);
    const int m0 = tm * F_BM, n0 = tn * F_BN;
    char* img = reinterpret_cast<char*>(g.c2);
    float csum[2][8];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int e = 0; e < 8; ++e) csum[hf][e] = 0.f;
#pragma unroll
    for (int hj = 0; hj < 8; ++hj) {
        const int hf = hj >> 2, j = hj & 3;
        const int row_t = j * 32 + (tid >> 3), c8 = hf * 8 + (tid & 7);
        const int row = m0 + row_t, col = n0 + c8 * 8;
        const float* p = ws + (int64_t)tix * (F_BM * F_BN) + row_t * F_BN + c8 * 8;
        f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
        for (int k = 1; k < nsplit; ++k) {
            const float* q = p + (int64_t)k * ntail * (F_BM * F_BN);
            const f32x4 u = *reinterpret_cast<const f32x4*>(q), w = *reinterpret_cast<const f32x4*>(q + 4);
            a[0] += u[0]; a[1] += u[1]; a[2] += u[2]; a[3] += u[3]; b[0] += w[0]; b[1] += w[1]; b[2] += w[2]; b[3] += w[3];
        }
        float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        const bool rok = row < g.M;
        if (rok && col < g.N) {                             // host: N % 8 == 0 for the image epilogues
            if (ACT == 5) {
                f32x4 d0, d1;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float hv = v[e] + (g.bias ? g.bias[col + e] : 0.f);
                    const float er = erff(hv * 0.70710678118654752440f);
                    v[e] = hv * 0.5f * (1.0f + er);
                    const float d = 0.5f * (1.0f + er) + hv * (expf(-0.5f * hv * hv) * 0.39894228040143267794f);
                    if (e < 4) d0[e] = d; else d1[e - 4] = d;
                }
                float* cp = g.c + (int64_t)row * g.ldc + col;
                *reinterpret_cast<f32x4*>(cp) = d0; *reinterpret_cast<f32x4*>(cp + 4) = d1;
            } else {
                const float* xp = g.aux + (int64_t)row * g.ldaux + col;
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(xp), x1 = *reinterpret_cast<const f32x4*>(xp + 4);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= e < 4 ? x0[e] : x1[e - 4];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
        }
        if (ACT == 6) {
#pragma unroll
            for (int e = 0; e < 8; ++e) csum[hf][e] += v[e];
        }
        x3_image_chunk_store(img, tm, tn, g.img_nkb, row_t, c8, v);
    }
    if (ACT == 6 && g.cs) x3_tile_colsum(csum, red, tid, g.cs + (int64_t)tm * g.N, n0, g.N);
}

template <int ACT, int FMT = 0>
__global__ __launch_bounds__(256, 2) void gemm_f32_planes_kernel(const GemmF32Args g) {
    constexpr int NP = PlanesFmt<FMT>::NP, NG = 4 * NP, NM = 4 * PlanesFmt<FMT>::NT;     // reads (= groups) and MFMAs per stage
    constexpr int STAGE_B = 2 * NP * IMG_PLANE_B;
    __shared__ __attribute__((aligned(1024))) float smem[P_SLOTS * STAGE_B / 4];          // 72 KiB (bf16x3), 48 KiB (fp16x2)
    typedef __attribute__((address_space(3))) void* lds_vp;
    typedef const __attribute__((address_space(1))) void* glb_vp;
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
    const int kbeg = (split - zs * g.ksplit) * g.k_zs, kend = min(g.K, kbeg + g.kps);      // host: K, kps multiples of 16
    const int nkb = g.K / P_BK;                             // stages per row block in the tiled image
    // this wave's 2 NP KiB of every stage: waves 0, 1 the two halves of A's NP * 4 KiB, waves 2, 3 of B's
    const char* __restrict__ pw = (wave < 2 ? reinterpret_cast<const char*>(g.a) + IMG_STAGE_OFF(tm, nkb, kbeg / P_BK, NP)
                                            : reinterpret_cast<const char*>(g.b) + IMG_STAGE_OFF(tn, nkb, kbeg / P_BK, NP)) +
                                  (wave & 1) * (2 * NP * 1024) + lane * 16;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int nst = (kend - kbeg) / P_BK;
    char* sm = reinterpret_cast<char*>(smem);
    auto dma1 = [&](int st, int slot, int i) {
        __builtin_amdgcn_global_load_lds((glb_vp)(pw + (int64_t)st * (NP * IMG_PLANE_B) + i * 1024), (lds_vp)(sm + slot * STAGE_B + (wave * 2 * NP + i) * 1024), 16, 0, 0);
    };
    const uint32_t lbase = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)sm;
    const uint32_t hx = IMG_FRAG_SWZ(r, h);
    const uint32_t fa = lbase + (wm * 64 + r) * IMG_ROW_B + hx, fb = lbase + NP * IMG_PLANE_B + (wn * 64 + r) * IMG_ROW_B + hx;
#pragma unroll
    for (int i = 0; i < 2 * NP; ++i) dma1(0, 0, i);
#pragma unroll
    for (int i = 0; i < 2 * NP; ++i) dma1(min(1, nst - 1), 1, i);
    bf16x8 ap[2][2][NP], bp[2][2][NP];                      // [register set][block][plane]
    // step st (slot = st % 3): stage st has landed for everyone -> refill the slot stage st - 1 was read from with stage st + 2
    // (past the end: the last stage again, into a slot nobody reads -- keeps the DMA count per step, hence the vmcnt, constant),
    // read stage st into register set SET while the MFMAs of stage st - 1 (set SET ^ 1) run
    auto step = [&](int st, int slot, auto set_tag, auto first_tag) {
        constexpr int SET = decltype(set_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value;
        if constexpr (NP == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");    // younger: the 2 NP pieces of stage st + 1
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        acr_barrier_nofence();
        const int rslot = slot == 0 ? 2 : slot - 1;         // (st + 2) % 3
        const int rst = min(st + 2, nst - 1);
        const uint32_t fas = fa + slot * STAGE_B, fbs = fb + slot * STAGE_B;
#define PL_GROUP(K12)                                                                                                   \
        if constexpr ((K12) < NG) {                                                                                     \
            if constexpr (!FIRST) pl_mfmas<FMT, (K12) * NM / NG, ((K12) + 1) * NM / NG>(acc, ap[SET ^ 1], bp[SET ^ 1]);  \
            if constexpr ((K12) < 2 * NP) ACR_LDS_RD128(ap[SET][(K12) / NP][(K12) % NP], fas, ((K12) % NP) * IMG_PLANE_B + ((K12) / NP) * 1024); \
            else ACR_LDS_RD128(bp[SET][((K12) - 2 * NP) / NP][(K12) % NP], fbs, ((K12) % NP) * IMG_PLANE_B + (((K12) - 2 * NP) / NP) * 1024); \
            if ((K12) & 1) dma1(rst, rslot, (K12) >> 1);                                                                \
            __builtin_amdgcn_sched_barrier(0);                                                                          \
        }
        PL_GROUP(0) PL_GROUP(1) PL_GROUP(2) PL_GROUP(3) PL_GROUP(4) PL_GROUP(5)
        PL_GROUP(6) PL_GROUP(7) PL_GROUP(8) PL_GROUP(9) PL_GROUP(10) PL_GROUP(11)
#undef PL_GROUP
        if constexpr (NP == 3)
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(ap[SET][0][0]), "+v"(ap[SET][0][1]), "+v"(ap[SET][0][2]), "+v"(ap[SET][1][0]), "+v"(ap[SET][1][1]), "+v"(ap[SET][1][2]),
                           "+v"(bp[SET][0][0]), "+v"(bp[SET][0][1]), "+v"(bp[SET][0][2]), "+v"(bp[SET][1][0]), "+v"(bp[SET][1][1]), "+v"(bp[SET][1][2]));
        else
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(ap[SET][0][0]), "+v"(ap[SET][0][1]), "+v"(ap[SET][1][0]), "+v"(ap[SET][1][1]),
                           "+v"(bp[SET][0][0]), "+v"(bp[SET][0][1]), "+v"(bp[SET][1][0]), "+v"(bp[SET][1][1]));
    };
    step(0, 0, std::integral_constant<int, 0>{}, std::true_type{});
    int slot = 1;
    for (int st = 1; st < nst; st += 2) {
        step(st, slot, std::integral_constant<int, 1>{}, std::false_type{});
        slot = slot == 2 ? 0 : slot + 1;
        if (st + 1 < nst) {
            step(st + 1, slot, std::integral_constant<int, 0>{}, std::false_type{});
            slot = slot == 2 ? 0 : slot + 1;
        }
    }
    if (nst & 1) pl_mfmas<FMT, 0, NM>(acc, ap[0], bp[0]);
    else pl_mfmas<FMT, 0, NM>(acc, ap[1], bp[1]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the refills past the end
    __syncthreads();                                        // every wave is done with the ring: the finish may reuse it
    if constexpr (FMT == 1) h2_unscale(g, acc, m0 + wm * 64, n0 + wn * 64, r, h);
    if constexpr (ACT == 5 || ACT == 6) x3_finish_image<ACT>(g, acc, smem, tm, tn, m0, n0, wm, wn, r, h, tid);
    else gemm_f32_finish<true, ACT>(g, acc, smem, split, tt, tn, m0, n0, zs, wm, wn, r, h, tid, 0.f, false);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Weight gradient on the SAME images the forward / input-gradient products read (no transposed copies of dy or x):
//   c[m][n] = sum_t a[t][m] b[t][n],   a = dy image, b = x image, both tiled [token block of 128][stage of 16 features].
// The contraction index is now the image's ROW: a 16-token stage of a 128-feature operand tile is, for each of its 8 feature
// stages and 3 planes, 16 consecutive 32-byte rows = 512 contiguous bytes (one LDS-DMA instruction copies two of them), and a
// fragment -- 8 tokens of one feature per lane -- is read TRANSPOSED from those [16 tokens][16 features] chunks by
// ds_read_b64_tr_b16 (a 16-lane group takes 4 token rows x 16 features = 128 contiguous bytes, conflict-free; lane (r, h)
// receives tokens 4 h + (0..3) and 8 + 4 h + (0..3) of feature r: the same permutation of the contraction index for both
// operands).  Slot = [a: plane][feature stage][512 B] | [b: ...]; ring, waits, interleaving as gemm_f32_planes_kernel.
// ---------------------------------------------------------------------------------------------------------------------------------
#define PL_RDTR(lo, hi, alo, ahi, OFF)                                                                  \
    asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%4\n\tds_read_b64_tr_b16 %1, %3 offset:%4"          \
                 : "=&v"(lo), "=&v"(hi) : "v"(alo), "v"(ahi), "i"(OFF))
template <int FMT = 0>
__global__ __launch_bounds__(256, 2) void gemm_f32_planes_tn_kernel(const GemmF32Args g) {
    constexpr int NP = PlanesFmt<FMT>::NP, NG = 4 * NP, NM = 4 * PlanesFmt<FMT>::NT;
    constexpr int STAGE_B = 2 * NP * IMG_PLANE_B;
    __shared__ __attribute__((aligned(1024))) float smem[P_SLOTS * STAGE_B / 4];          // 72 KiB (bf16x3), 48 KiB (fp16x2)
    typedef __attribute__((address_space(3))) void* lds_vp;
    typedef const __attribute__((address_space(1))) void* glb_vp;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int ntile = g.tiles_launch;
    const int t0 = acr_xcd_remap(blockIdx.x, ntile * g.nsplit);
    const int split = t0 / ntile, tt = g.tile0 + (t0 - split * ntile);
    const int tm = tt / g.tiles_n, tn = tt - tm * g.tiles_n;
    const int m0 = tm * F_BM, n0 = tn * F_BN;
    const int kbeg = split * g.k_zs, kend = min(g.K, kbeg + g.kps);      // tokens; host: K, kps multiples of 16
    const int nkb = wave < 2 ? g.nkb_a : g.nkb_b;          // feature stages per token block of this wave's operand
    const int f0 = (wave < 2 ? tm : tn) * 8;               // first feature stage of the tile
    const char* __restrict__ pw = reinterpret_cast<const char*>(wave < 2 ? g.a : g.b);
    // piece q = 2 NP (wave & 1) + i of the operand's 4 NP: plane q >> 2, chunk pair q & 3 (feature stages f0 + 2 (q & 3) + (lane >> 5));
    // feature stages past the operand's end (M or N not a multiple of 128) alias the last one: rows the finish never stores
    int offd[2 * NP];
#pragma unroll
    for (int i = 0; i < 2 * NP; ++i) {
        const int q = (wave & 1) * 2 * NP + i, pl = q >> 2, fs = min(f0 + 2 * (q & 3) + (lane >> 5), nkb - 1);
        offd[i] = (fs * NP + pl) * IMG_PLANE_B + (lane & 31) * 16;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int nst = (kend - kbeg) / P_BK;
    char* sm = reinterpret_cast<char*>(smem);
    auto dma1 = [&](int st, int slot, int i) {
        const int tk = kbeg + st * P_BK;                    // uniform
        const char* src = pw + ((int64_t)(tk >> 7) * nkb) * (NP * IMG_PLANE_B) + (tk & 127) * 32;
        const int q = (wave & 1) * 2 * NP + i;
        __builtin_amdgcn_global_load_lds((glb_vp)(src + offd[i]), (lds_vp)(sm + slot * STAGE_B + (wave >> 1) * (NP * IMG_PLANE_B) + (q >> 2) * IMG_PLANE_B + (q & 3) * 1024),
                                         16, 0, 0);
    };
    const uint32_t lbase = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)sm;
    const int i16 = lane & 15, g1 = (lane >> 4) & 1, qq = i16 >> 2, pp = i16 & 3;
    // lo: token row 4 h + qq (< 8: halves as stored), hi: row 8 + 4 h + qq (halves swapped)
    const uint32_t tlo = (4 * h + qq) * 32 + ((pp >> 1) << 4) + 8 * (pp & 1), thi = (8 + 4 * h + qq) * 32 + (((pp >> 1) ^ 1) << 4) + 8 * (pp & 1);
    const uint32_t fa_lo = lbase + (wm * 4 + g1) * 512 + tlo, fa_hi = lbase + (wm * 4 + g1) * 512 + thi;
    const uint32_t fb_lo = lbase + NP * IMG_PLANE_B + (wn * 4 + g1) * 512 + tlo, fb_hi = lbase + NP * IMG_PLANE_B + (wn * 4 + g1) * 512 + thi;
#pragma unroll
    for (int i = 0; i < 2 * NP; ++i) dma1(0, 0, i);
#pragma unroll
    for (int i = 0; i < 2 * NP; ++i) dma1(min(1, nst - 1), 1, i);
    bf16x4 al[2][2][NP], ah[2][2][NP], bl[2][2][NP], bh[2][2][NP];      // [register set][block][plane], tokens lo / hi
    auto step = [&](int st, int slot, auto set_tag, auto first_tag) {
        constexpr int SET = decltype(set_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value;
        if constexpr (NP == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");    // younger: the 2 NP pieces of stage st + 1
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        acr_barrier_nofence();
        const int rslot = slot == 0 ? 2 : slot - 1;         // (st + 2) % 3
        const int rst = min(st + 2, nst - 1);
        const uint32_t so = slot * STAGE_B;
        const uint32_t a_lo = fa_lo + so, a_hi = fa_hi + so, b_lo = fb_lo + so, b_hi = fb_hi + so;
#define PT_GROUP(K12)                                                                                                                   \
        if constexpr ((K12) < NG) {                                                                                                     \
            if constexpr (!FIRST) pt_mfmas<FMT, (K12) * NM / NG, ((K12) + 1) * NM / NG>(acc, al[SET ^ 1], ah[SET ^ 1], bl[SET ^ 1], bh[SET ^ 1]); \
            if constexpr ((K12) < 2 * NP) PL_RDTR(al[SET][(K12) / NP][(K12) % NP], ah[SET][(K12) / NP][(K12) % NP], a_lo, a_hi, ((K12) % NP) * IMG_PLANE_B + ((K12) / NP) * 1024); \
            else PL_RDTR(bl[SET][((K12) - 2 * NP) / NP][(K12) % NP], bh[SET][((K12) - 2 * NP) / NP][(K12) % NP], b_lo, b_hi, ((K12) % NP) * IMG_PLANE_B + (((K12) - 2 * NP) / NP) * 1024); \
            if ((K12) & 1) dma1(rst, rslot, (K12) >> 1);                                                                                \
            __builtin_amdgcn_sched_barrier(0);                                                                                          \
        }
        PT_GROUP(0) PT_GROUP(1) PT_GROUP(2) PT_GROUP(3) PT_GROUP(4) PT_GROUP(5)
        PT_GROUP(6) PT_GROUP(7) PT_GROUP(8) PT_GROUP(9) PT_GROUP(10) PT_GROUP(11)
#undef PT_GROUP
        if constexpr (NP == 3)
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(al[SET][0][0]), "+v"(al[SET][0][1]), "+v"(al[SET][0][2]), "+v"(al[SET][1][0]), "+v"(al[SET][1][1]), "+v"(al[SET][1][2]),
                           "+v"(ah[SET][0][0]), "+v"(ah[SET][0][1]), "+v"(ah[SET][0][2]), "+v"(ah[SET][1][0]), "+v"(ah[SET][1][1]), "+v"(ah[SET][1][2]),
                           "+v"(bl[SET][0][0]), "+v"(bl[SET][0][1]), "+v"(bl[SET][0][2]), "+v"(bl[SET][1][0]), "+v"(bl[SET][1][1]), "+v"(bl[SET][1][2]),
                           "+v"(bh[SET][0][0]), "+v"(bh[SET][0][1]), "+v"(bh[SET][0][2]), "+v"(bh[SET][1][0]), "+v"(bh[SET][1][1]), "+v"(bh[SET][1][2]));
        else
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(al[SET][0][0]), "+v"(al[SET][0][1]), "+v"(al[SET][1][0]), "+v"(al[SET][1][1]),
                           "+v"(ah[SET][0][0]), "+v"(ah[SET][0][1]), "+v"(ah[SET][1][0]), "+v"(ah[SET][1][1]),
                           "+v"(bl[SET][0][0]), "+v"(bl[SET][0][1]), "+v"(bl[SET][1][0]), "+v"(bl[SET][1][1]),
                           "+v"(bh[SET][0][0]), "+v"(bh[SET][0][1]), "+v"(bh[SET][1][0]), "+v"(bh[SET][1][1]));
    };
    step(0, 0, std::integral_constant<int, 0>{}, std::true_type{});
    int slot = 1;
    for (int st = 1; st < nst; st += 2) {
        step(st, slot, std::integral_constant<int, 1>{}, std::false_type{});
        slot = slot == 2 ? 0 : slot + 1;
        if (st + 1 < nst) {
            step(st + 1, slot, std::integral_constant<int, 0>{}, std::false_type{});
            slot = slot == 2 ? 0 : slot + 1;
        }
    }
    if (nst & 1) pt_mfmas<FMT, 0, NM>(acc, al[0], ah[0], bl[0], bh[0]);
    else pt_mfmas<FMT, 0, NM>(acc, al[1], ah[1], bl[1], bh[1]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (FMT == 1) h2_unscale(g, acc, m0 + wm * 64, n0 + wn * 64, r, h);
    gemm_f32_finish<true, 3>(g, acc, smem, split, tt, tn, m0, n0, 0, wm, wn, r, h, tid, 0.f, false);
}

// fp16x2 images (include/acr_hip.h "fp16x2 images"): [2 tiled fp16 planes][int32 exponents, nexp][int32 flag, 4]
static int h2_nexp(int rows, int cols) { return max((rows + F_BM - 1) / F_BM, (cols + F_BM - 1) / F_BM) * F_BM; }
static size_t h2_plane_floats(int rows, int cols) { return img_floats(rows, cols, 2); }
static size_t h2_floats(int rows, int cols) { return h2_plane_floats(rows, cols) + h2_nexp(rows, cols) + 4; }
int* h2_exps(const float* img, int rows, int cols) { return (int*)(img + h2_plane_floats(rows, cols)); }
// Workspace of the pre-split operands (gemm_f32_planes_kernel): behind the slabs, [A image | B image | column-sum / column-max parts],
// every region a multiple of 16 bytes.
PlanesPlan planes_plan(int mode, int math, int M, int N, int K) {
    PlanesPlan p = {false, 0, 0, 0, 0};
    if (math != ACR_MATH_BF16X3 && math != ACR_MATH_FP16X2) return p;
    p.on = true; p.nkb = (K + P_BK - 1) / P_BK;
    if (math == ACR_MATH_FP16X2) {                          // TN: column-scaled images of a[K][M], b[K][N]; NT / NN: row-scaled of a, b (resp. b^T)
        const size_t nrb = (size_t)(K + 127) / 128;
        p.a_fl = mode == ACR_GEMM_TN ? h2_floats(K, M) : h2_floats(M, K);
        p.b_fl = mode == ACR_GEMM_TN ? h2_floats(K, N) : h2_floats(N, K);
        p.cs_fl = mode == ACR_GEMM_NT ? 0 : (nrb * (mode == ACR_GEMM_TN ? max(M, N) : N) + 3) / 4 * 4;
        return p;
    }
    if (mode == ACR_GEMM_TN) {                              // images of a[K][M] and b[K][N] as stored: rows = the K tokens
        p.a_fl = img_floats(K, M); p.b_fl = img_floats(K, N);
        p.cs_fl = ((size_t)(K + 127) / 128 * M + 3) / 4 * 4;
        return p;
    }
    p.a_fl = img_floats(M, K); p.b_fl = img_floats(N, K);
    return p;
}
// out[c] = sum over the nparts row-block parts of planes_tile_t_kernel, 16 columns per workgroup, 16 threads per column each
// summing every 16th part (independent loads in flight), combined through LDS in a fixed order (deterministic)
__global__ __launch_bounds__(256) void planes_colsum_kernel(const float* __restrict__ parts, int nparts, int C, float* __restrict__ out) {
    __shared__ float red[256];
    const int c = blockIdx.x * 16 + (threadIdx.x & 15), q = threadIdx.x >> 4;
    float s = 0.f;
    if (c < C) {
#pragma unroll 8
        for (int k = q; k < nparts; k += 16) s += parts[(int64_t)k * C + c];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < 16 && c < C) {
        float t = red[threadIdx.x];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += red[k * 16 + threadIdx.x];
        out[c] = t;
    }
}
// operand rows = x's rows
template <int FMT = 0>
static void launch_planes_tile(const float* x, int64_t ld, int rows, int K, int nkb, float* img, float* colpart, hipStream_t st, const int* ex = nullptr) {
    const int64_t nb = (int64_t)((rows + F_BM - 1) / F_BM) * ((nkb + 3) / 4);
    hipLaunchKernelGGL(planes_tile_kernel<FMT>, dim3((unsigned)nb), dim3(256), 0, st, x, ld, rows, K, nkb, reinterpret_cast<char*>(img), colpart, ex);
}
// operand rows = x's C columns, contraction = x's R rows; the row blocks of x cover whole stages up to nkb * 16
template <int FMT = 0>
static void launch_planes_tile_t(const float* x, int64_t ld, int R, int C, int nkb, float* img, float* colpart, hipStream_t st, const int* ex = nullptr) {
    const int cpad = (C + F_BM - 1) / F_BM * F_BM;            // all 128 rows of the last row block are written (zeros past C)
    const int64_t nb = (int64_t)((nkb * P_BK + 63) / 64) * (cpad / 64);
    hipLaunchKernelGGL(planes_tile_t_kernel<FMT>, dim3((unsigned)nb), dim3(256), 0, st, x, ld, R, C, nkb, reinterpret_cast<char*>(img), colpart, ex);
}

// ---- the image API: split-product operands made once, used by several products (include/acr_hip.h "split-product images") ------
extern "C" size_t acr_x3_image_floats(int32_t rows, int32_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return img_floats(rows, cols);
}
extern "C" size_t acr_x3_colsum_ws_floats(int32_t rows, int32_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (size_t)((rows + F_BM - 1) / F_BM) * cols;
}
extern "C" int acr_x3_image(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, float* colsum, float* colsum_ws, void* stream) {
    ACR_CHECK_ARG(x && image, "acr_x3_image: null pointer");
    ACR_CHECK_ARG(rows > 0 && cols > 0 && ld >= cols, "acr_x3_image: bad shape (rows=%d cols=%d ld=%lld)", rows, cols, (long long)ld);
    ACR_CHECK_ARG(al16(x) && al16(image) && (ld % 4) == 0, "acr_x3_image: x and image must be 16-byte aligned, ld %% 4 == 0");
    ACR_CHECK_ARG(!colsum || colsum_ws, "acr_x3_image: colsum needs colsum_ws (acr_x3_colsum_ws_floats)");
    hipStream_t st = (hipStream_t)stream;
    launch_planes_tile(x, ld, rows, cols, (cols + P_BK - 1) / P_BK, image, colsum ? colsum_ws : nullptr, st);
    if (colsum)
        hipLaunchKernelGGL(planes_colsum_kernel, dim3((cols + 15) / 16), dim3(256), 0, st, (const float*)colsum_ws, (rows + F_BM - 1) / F_BM, cols, colsum);
    return acr_check_launch("acr_x3_image");
}
extern "C" int acr_x3_image_t(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, void* stream) {
    ACR_CHECK_ARG(x && image, "acr_x3_image_t: null pointer");
    ACR_CHECK_ARG(rows > 0 && cols > 0 && ld >= cols, "acr_x3_image_t: bad shape (rows=%d cols=%d ld=%lld)", rows, cols, (long long)ld);
    ACR_CHECK_ARG(al16(x) && al16(image) && (ld % 4) == 0, "acr_x3_image_t: x and image must be 16-byte aligned, ld %% 4 == 0");
    launch_planes_tile_t(x, ld, rows, cols, (rows + P_BK - 1) / P_BK, image, nullptr, (hipStream_t)stream);
    return acr_check_launch("acr_x3_image_t");
}
extern "C" size_t acr_gemm_x3_ws_floats(int32_t mode, int32_t act, int32_t M, int32_t N, int32_t K) {
    if (mode == ACR_GEMM_NN) return 0;
    const size_t base = (gemm_ws_base_floats(mode, M, N, K, true) + 3) / 4 * 4;
    return base + (act == 4 ? ((size_t)((M + F_BM - 1) / F_BM) * N + 3) / 4 * 4 : 0);        // act 4: column-sum parts per tile row
}
template <int FMT>
int gemm_planes(int32_t mode, int32_t act, const float* a_img, const float* b_img, const float* bias, const float* aux, int64_t ldaux,
                       float* c, int64_t ldc, float* c2, float* colsum, int32_t M, int32_t N, int32_t K, float* ws, const int* ea, const int* eb,
                       hipStream_t st) {
    GemmF32Args g;
    g.a = a_img; g.lda = 0; g.b = b_img; g.ldb = 0; g.bias = bias; g.aux = aux; g.ldaux = ldaux; g.c = c; g.ldc = ldc; g.c2 = c2;
    g.cs = nullptr; g.M = M; g.N = N; g.ea = ea; g.eb = eb;
    g.K = (K + P_BK - 1) / P_BK * P_BK;                     // the images are zero past K
    g.tiles_m = (M + F_BM - 1) / F_BM; g.tiles_n = (N + F_BN - 1) / F_BN; g.nsplit = 1; g.kps = g.K;
    g.a_zs = g.b_zs = g.c_zs = g.aux_zs = 0; g.k_zs = g.kps; g.ksplit = 1 << 30;
    g.tile0 = 0; g.tiles_launch = g.tiles_m * g.tiles_n;
    g.nkb_a = (M + P_BK - 1) / P_BK; g.nkb_b = (N + P_BK - 1) / P_BK;
    if (mode == ACR_GEMM_TN) {                              // a_img = image of a[K][M], b_img = image of b[K][N] (rows = the K tokens)
        const TnPlan p = tn_plan(M, N, K);
        g.nsplit = p.nsplit; g.kps = p.kps; g.k_zs = p.kps;
        g.c = ws; g.ldc = N;
        hipLaunchKernelGGL(gemm_f32_planes_tn_kernel<FMT>, dim3((unsigned)(g.tiles_m * g.tiles_n * p.nsplit)), dim3(256), 0, st, g);
        gemm_f32_reduce(ws, p.nsplit, (int64_t)M * N / 4, c, st);
        return acr_check_launch(FMT == 0 ? "acr_gemm_x3(TN)" : "acr_gemm_h2(TN)");
    }
    TailPlan tp = gemm_tail_plan(M, N, K, true);
    if (!ws) tp.ntail = 0;
    float* parts = (act == 4 && colsum) ? ws + (gemm_ws_base_floats(mode, M, N, K, true) + 3) / 4 * 4 : nullptr;
    g.cs = parts; g.img_nkb = (N + P_BK - 1) / P_BK;
    g.tiles_launch -= tp.ntail;
    if (g.tiles_launch > 0) {
        const dim3 grid((unsigned)g.tiles_launch);
        if (act == 0) hipLaunchKernelGGL((gemm_f32_planes_kernel<0, FMT>), grid, dim3(256), 0, st, g);
        else if (act == 1) hipLaunchKernelGGL((gemm_f32_planes_kernel<1, FMT>), grid, dim3(256), 0, st, g);
        else if (act == 2) hipLaunchKernelGGL((gemm_f32_planes_kernel<2, FMT>), grid, dim3(256), 0, st, g);
        else if constexpr (FMT == 0) {
            if (act == 3) hipLaunchKernelGGL((gemm_f32_planes_kernel<5>), grid, dim3(256), 0, st, g);
            else hipLaunchKernelGGL((gemm_f32_planes_kernel<6>), grid, dim3(256), 0, st, g);
        }
    }
    if (tp.ntail) {                                         // the tail tiles, K-split into slabs, and their epilogue (gemm_tail_plan)
        GemmF32Args gt = g;
        gt.tile0 = g.tiles_launch; gt.tiles_launch = tp.ntail; gt.nsplit = tp.nsplit; gt.kps = tp.kps; gt.k_zs = tp.kps; gt.c = ws;
        hipLaunchKernelGGL((gemm_f32_planes_kernel<4, FMT>), dim3((unsigned)(tp.ntail * tp.nsplit)), dim3(256), 0, st, gt);
        GemmF32Args ge = g;
        ge.tile0 = gt.tile0;
        if (act <= 2) gemm_f32_tail_epilogue(act, ge, ws, tp.ntail, tp.nsplit, st);
        else if (act == 3) hipLaunchKernelGGL((gemm_x3_tail_image_kernel<5>), dim3((unsigned)tp.ntail), dim3(256), 0, st, ge, (const float*)ws, tp.ntail, tp.nsplit);
        else hipLaunchKernelGGL((gemm_x3_tail_image_kernel<6>), dim3((unsigned)tp.ntail), dim3(256), 0, st, ge, (const float*)ws, tp.ntail, tp.nsplit);
    }
    if (parts) hipLaunchKernelGGL(planes_colsum_kernel, dim3((N + 15) / 16), dim3(256), 0, st, (const float*)parts, g.tiles_m, N, colsum);
    return acr_check_launch(FMT == 0 ? "acr_gemm_x3" : "acr_gemm_h2");
}
template int gemm_planes<1>(int32_t, int32_t, const float*, const float*, const float*, const float*, int64_t, float*, int64_t, float*, float*, int32_t,
                            int32_t, int32_t, float*, const int*, const int*, hipStream_t);      // acr_gemm_f32 (gemm_f32.hip) calls it
extern "C" int acr_gemm_x3(int32_t mode, int32_t act, const float* a_img, const float* b_img, const float* bias, const float* aux, int64_t ldaux,
                           float* c, int64_t ldc, float* c2, float* colsum, int32_t M, int32_t N, int32_t K, float* ws, void* stream) {
    ACR_CHECK_ARG(a_img && b_img && (c || act == 4), "acr_gemm_x3: null pointer");
    ACR_CHECK_ARG(M > 0 && N > 0 && K > 0, "acr_gemm_x3: empty problem (M=%d N=%d K=%d)", M, N, K);
    ACR_CHECK_ARG((mode == ACR_GEMM_NT || mode == ACR_GEMM_TN) && act >= 0 && act <= 4, "acr_gemm_x3: mode must be ACR_GEMM_NT or ACR_GEMM_TN (got %d), act 0..4 (got %d)", mode, act);
    ACR_CHECK_ARG(!colsum || act == 4, "acr_gemm_x3: colsum comes with act 4 only (the image passes give it otherwise)");
    ACR_CHECK_ARG(al16(a_img) && al16(b_img) && al16(c) && (ldc % 4) == 0 && (!bias || al16(bias)) && (!aux || (al16(aux) && (ldaux % 4) == 0)) && (!c2 || al16(c2)),
                  "acr_gemm_x3: pointers must be 16-byte aligned, pitches %% 4 == 0");
    ACR_CHECK_ARG(!ws || al16(ws), "acr_gemm_x3: ws must be 16-byte aligned");
    if (mode == ACR_GEMM_TN) {
        ACR_CHECK_ARG(act == 0 && !bias && !aux, "acr_gemm_x3: TN takes no epilogue");
        ACR_CHECK_ARG(ws, "acr_gemm_x3: TN needs the acr_gemm_x3_ws_floats workspace");
        ACR_CHECK_ARG((M % 4) == 0 && (N % 4) == 0 && ldc == N, "acr_gemm_x3: TN needs M, N %% 4 == 0 and a dense output (ldc == N)");
    } else {
        ACR_CHECK_ARG((act != 1 && act != 3 && act != 4) || c2, "acr_gemm_x3: act 1 / 3 / 4 need c2");
        ACR_CHECK_ARG((act != 2 && act != 4) || aux, "acr_gemm_x3: act 2 / 4 (GELU') need the saved derivative in aux");
        ACR_CHECK_ARG(act < 3 || ((N % 8) == 0 && (!aux || (ldaux % 4) == 0)), "acr_gemm_x3: image epilogues need N %% 8 == 0");
        ACR_CHECK_ARG(act != 4 || !colsum || ws, "acr_gemm_x3: act 4 with colsum needs ws");
    }
    return gemm_planes<0>(mode, act, a_img, b_img, bias, aux, ldaux, c, ldc, c2, colsum, M, N, K, ws, nullptr, nullptr, (hipStream_t)stream);
}

// ---- fp16x2 images ------------------------------------------------------------------------------------------------------------------
extern "C" size_t acr_h2_image_floats(int32_t rows, int32_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return h2_floats(rows, cols);
}
extern "C" size_t acr_h2_ws_floats(int32_t rows, int32_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (size_t)((rows + F_BM - 1) / F_BM) * cols;
}
// image -> scale direction (ACR_H2_ROWS / ACR_H2_COLS) of the last acr_h2_image* call that wrote it: acr_gemm_h2 checks an image's
// direction against its mode without reading the device-side flag (no host synchronisation)
static std::mutex h2_reg_mu;
static std::unordered_map<const void*, int> h2_reg;
static void h2_record(const void* img, int dir) {
    std::lock_guard<std::mutex> lk(h2_reg_mu);
    h2_reg[img] = dir;
}
static int h2_recorded(const void* img) {
    std::lock_guard<std::mutex> lk(h2_reg_mu);
    const auto it = h2_reg.find(img);
    return it == h2_reg.end() ? -1 : it->second;
}
// row-scaled image of x (rows x cols): one exponent per row; colsum (or null) = x's column sums, parts in ws
void h2_image_rows(const float* x, int64_t ld, int rows, int cols, float* img, float* colsum, float* ws, hipStream_t st) {
    const int nexp = h2_nexp(rows, cols);
    int* ex = h2_exps(img, rows, cols);
    hipLaunchKernelGGL(h2_rowexp_kernel, dim3((unsigned)((nexp + 3) / 4)), dim3(256), 0, st, x, ld, rows, cols, nexp, ex, ex + nexp, (int)ACR_H2_ROWS);
    launch_planes_tile<1>(x, ld, rows, cols, (cols + P_BK - 1) / P_BK, img, colsum ? ws : nullptr, st, ex);
    if (colsum)
        hipLaunchKernelGGL(planes_colsum_kernel, dim3((cols + 15) / 16), dim3(256), 0, st, (const float*)ws, (rows + F_BM - 1) / F_BM, cols, colsum);
}
// column-scaled image of x (rows x cols, the contraction over rows: a TN operand): one exponent per column.  ws holds the
// per-row-block column maxima, then (colsum) the column-sum parts
void h2_image_cols(const float* x, int64_t ld, int rows, int cols, float* img, float* colsum, float* ws, hipStream_t st) {
    const int nexp = h2_nexp(rows, cols), nrb = (rows + F_BM - 1) / F_BM;
    int* ex = h2_exps(img, rows, cols);
    hipLaunchKernelGGL(h2_colmax_kernel, dim3((unsigned)nrb, (unsigned)((cols + 255) / 256)), dim3(256), 0, st, x, ld, rows, cols, ws);
    hipLaunchKernelGGL(h2_colexp_kernel, dim3((unsigned)((nexp + 63) / 64)), dim3(256), 0, st, (const float*)ws, nrb, cols, nexp, ex, ex + nexp,
                       (int)ACR_H2_COLS);
    launch_planes_tile<2>(x, ld, rows, cols, (cols + P_BK - 1) / P_BK, img, colsum ? ws : nullptr, st, ex);
    if (colsum)
        hipLaunchKernelGGL(planes_colsum_kernel, dim3((cols + 15) / 16), dim3(256), 0, st, (const float*)ws, nrb, cols, colsum);
}
// row-scaled image of x^T (x: rows x cols; operand rows = x's columns): one exponent per column of x; ws: the column maxima parts
void h2_image_t(const float* x, int64_t ld, int rows, int cols, float* img, float* ws, hipStream_t st) {
    const int nexp = h2_nexp(cols, rows), nrb = (rows + F_BM - 1) / F_BM;
    int* ex = h2_exps(img, cols, rows);
    hipLaunchKernelGGL(h2_colmax_kernel, dim3((unsigned)nrb, (unsigned)((cols + 255) / 256)), dim3(256), 0, st, x, ld, rows, cols, ws);
    hipLaunchKernelGGL(h2_colexp_kernel, dim3((unsigned)((nexp + 63) / 64)), dim3(256), 0, st, (const float*)ws, nrb, cols, nexp, ex, ex + nexp,
                       (int)ACR_H2_ROWS);
    launch_planes_tile_t<1>(x, ld, rows, cols, (rows + P_BK - 1) / P_BK, img, nullptr, st, ex);
}
#define H2_IMAGE_ARGS(what)                                                                                                                  \
    ACR_CHECK_ARG(x && image, what ": null pointer");                                                                                        \
    ACR_CHECK_ARG(rows > 0 && cols > 0 && ld >= cols, what ": bad shape (rows=%d cols=%d ld=%lld)", rows, cols, (long long)ld);               \
    ACR_CHECK_ARG(al16(x) && al16(image) && (ld % 4) == 0 && (!ws || al16(ws)), what ": x, image and ws must be 16-byte aligned, ld %% 4 == 0")
extern "C" int acr_h2_image(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, float* colsum, float* ws, void* stream) {
    H2_IMAGE_ARGS("acr_h2_image");
    ACR_CHECK_ARG(!colsum || ws, "acr_h2_image: colsum needs ws (acr_h2_ws_floats)");
    h2_image_rows(x, ld, rows, cols, image, colsum, ws, (hipStream_t)stream);
    h2_record(image, ACR_H2_ROWS);
    return acr_check_launch("acr_h2_image");
}
extern "C" int acr_h2_image_cols(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, float* colsum, float* ws, void* stream) {
    H2_IMAGE_ARGS("acr_h2_image_cols");
    ACR_CHECK_ARG(ws, "acr_h2_image_cols: needs ws (acr_h2_ws_floats)");
    h2_image_cols(x, ld, rows, cols, image, colsum, ws, (hipStream_t)stream);
    h2_record(image, ACR_H2_COLS);
    return acr_check_launch("acr_h2_image_cols");
}
extern "C" int acr_h2_image_t(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, float* ws, void* stream) {
    H2_IMAGE_ARGS("acr_h2_image_t");
    ACR_CHECK_ARG(ws, "acr_h2_image_t: needs ws (acr_h2_ws_floats)");
    h2_image_t(x, ld, rows, cols, image, ws, (hipStream_t)stream);
    h2_record(image, ACR_H2_ROWS);
    return acr_check_launch("acr_h2_image_t");
}
#undef H2_IMAGE_ARGS
extern "C" size_t acr_gemm_h2_ws_floats(int32_t mode, int32_t act, int32_t M, int32_t N, int32_t K) {
    (void)act;
    if (mode != ACR_GEMM_NT && mode != ACR_GEMM_TN) return 0;
    return (gemm_ws_base_floats(mode, M, N, K, true) + 3) / 4 * 4;
}
extern "C" int acr_gemm_h2(int32_t mode, int32_t act, const float* a_img, const float* b_img, const float* bias, const float* aux, int64_t ldaux,
                           float* c, int64_t ldc, float* c2, int32_t M, int32_t N, int32_t K, float* ws, void* stream) {
    ACR_CHECK_ARG(a_img && b_img && c, "acr_gemm_h2: null pointer");
    ACR_CHECK_ARG(M > 0 && N > 0 && K > 0, "acr_gemm_h2: empty problem (M=%d N=%d K=%d)", M, N, K);
    ACR_CHECK_ARG((mode == ACR_GEMM_NT || mode == ACR_GEMM_TN) && act >= 0 && act <= 2, "acr_gemm_h2: mode must be ACR_GEMM_NT or ACR_GEMM_TN (got %d), act 0..2 (got %d)", mode, act);
    ACR_CHECK_ARG(al16(a_img) && al16(b_img) && al16(c) && (ldc % 4) == 0 && (!bias || al16(bias)) && (!aux || (al16(aux) && (ldaux % 4) == 0)) && (!c2 || al16(c2)) && (!ws || al16(ws)),
                  "acr_gemm_h2: pointers must be 16-byte aligned, pitches %% 4 == 0");
    const int want = mode == ACR_GEMM_NT ? ACR_H2_ROWS : ACR_H2_COLS;
    ACR_CHECK_ARG(h2_recorded(a_img) == want && h2_recorded(b_img) == want,
                  "acr_gemm_h2: %s needs %s-scaled images (acr_h2_image%s)", mode == ACR_GEMM_NT ? "NT" : "TN", want == ACR_H2_ROWS ? "row" : "column",
                  want == ACR_H2_ROWS ? " / acr_h2_image_t" : "_cols");
    if (mode == ACR_GEMM_TN) {
        ACR_CHECK_ARG(act == 0 && !bias && !aux && !c2, "acr_gemm_h2: TN takes no epilogue");
        ACR_CHECK_ARG(ws, "acr_gemm_h2: TN needs the acr_gemm_h2_ws_floats workspace");
        ACR_CHECK_ARG((M % 4) == 0 && (N % 4) == 0 && ldc == N, "acr_gemm_h2: TN needs M, N %% 4 == 0 and a dense output (ldc == N)");
        return gemm_planes<1>(mode, 0, a_img, b_img, nullptr, nullptr, 0, c, ldc, nullptr, nullptr, M, N, K, ws, h2_exps(a_img, K, M), h2_exps(b_img, K, N),
                              (hipStream_t)stream);
    }
    ACR_CHECK_ARG(act != 1 || c2, "acr_gemm_h2: act 1 needs c2");
    ACR_CHECK_ARG(act != 2 || aux, "acr_gemm_h2: act 2 (GELU') needs the saved derivative in aux");
    return gemm_planes<1>(mode, act, a_img, b_img, bias, aux, ldaux, c, ldc, c2, nullptr, M, N, K, ws, h2_exps(a_img, M, K), h2_exps(b_img, N, K),
                          (hipStream_t)stream);
}
