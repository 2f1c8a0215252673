// Split products: the one place where the operand split, the order of the product's terms and the geometry of an operand image
// are written.  The image FORMAT is stated in include/acr_hip.h ("split-product images", "fp16x2 images"); this header is its
// implementation for every kernel that writes an image (image passes, image epilogues, LayerNorm, the attention forward) or
// reads one (plane GEMMs, 1x1 / 3x3 weight-image convolutions).
#pragma once
#include "acr_common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- bf16x3: x = h0 + h1 + h2 (3 x 8 = 24 mantissa bits) -------------------------------------------------------------------------
__device__ __forceinline__ void split3_bf16(float x, __bf16& h0, __bf16& h1, __bf16& h2) {
    h0 = (__bf16)x;
    const float r1 = x - (float)h0;
    h1 = (__bf16)r1;
    const float r2 = r1 - (float)h1;
    h2 = (__bf16)r2;
}
// 8 elements -> one fragment (or one 16-byte image chunk) per piece: from two f32x4, from float[8], from accumulator registers 8S .. 8S+7
__device__ __forceinline__ void split3_bf16(const f32x4& lo4, const f32x4& hi4, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        __bf16 h0, h1, h2;
        split3_bf16(e < 4 ? lo4[e] : hi4[e - 4], h0, h1, h2);
        p0[e] = h0; p1[e] = h1; p2[e] = h2;
    }
}
__device__ __forceinline__ void split3_bf16(const float (&x)[8], bf16x8& p0, bf16x8& p1, bf16x8& p2) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        __bf16 h0, h1, h2;
        split3_bf16(x[e], h0, h1, h2);
        p0[e] = h0; p1[e] = h1; p2[e] = h2;
    }
}
template <int S>
__device__ __forceinline__ void split3_bf16_acc(const f32x16& z, bf16x8 (&p)[3]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        __bf16 h0, h1, h2;
        split3_bf16(z[8 * S + e], h0, h1, h2);
        p[0][e] = h0; p[1][e] = h1; p[2][e] = h2;
    }
}

// ---- fp16x2: xs = x 2^e (exact), p0 = fp16(xs), p1 = fp16(xs - p0) (the difference is exact) --------------------------------------
__device__ __forceinline__ void h2_split8(const float (&x)[8], const int (&e)[8], bf16x8& p0, bf16x8& p1) {
    f16x8 q0, q1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float xs = ldexpf(x[i], e[i]);
        const _Float16 h0 = (_Float16)xs;
        q0[i] = h0; q1[i] = (_Float16)(xs - (float)h0);
    }
    p0 = __builtin_bit_cast(bf16x8, q0); p1 = __builtin_bit_cast(bf16x8, q1);
}
// scale exponent e with max|x| 2^e in [2^14, 2^15) for the largest FINITE |x| of a group; 0 for a group without a finite non-zero value
__device__ __forceinline__ float h2_absmax(float m, float v) { const float a = fabsf(v); return a <= 3.402823466e38f ? fmaxf(m, a) : m; }
__device__ __forceinline__ int h2_exp(float m) {
    if (!(m > 0.f)) return 0;
    int ex;
    frexpf(m, &ex);                                         // m = f 2^ex, f in [0.5, 1): m 2^(15 - ex) = f 2^15
    return 15 - ex;
}

// ---- the terms of a product, smallest first ------------------------------------------------------------------------------------------
// bf16x3: (0,2) (2,0) (1,1) (0,1) (1,0) (0,0); the dropped terms are <= 2^-24 |a b|.  A, Bv: the three pieces of a fragment.
#define ACR_MFMA6(ACC, A, Bv)                                                        \
    {                                                                                \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], Bv[2], ACC, 0, 0, 0);    \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2], Bv[0], ACC, 0, 0, 0);    \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], Bv[1], ACC, 0, 0, 0);    \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], Bv[1], ACC, 0, 0, 0);    \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], Bv[0], ACC, 0, 0, 0);    \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], Bv[0], ACC, 0, 0, 0);    \
    }
// The same order as a table, for the kernels that issue a stage's terms in ranges between their LDS reads: piece of a / of b in
// term t of image format fmt (0 bf16x3: the six above; 1 fp16x2: (0,1) (1,0) (0,0))
__host__ __device__ constexpr int pl_ta(int fmt, int t) { return fmt == 0 ? (t == 1 ? 2 : (t == 2 || t == 4) ? 1 : 0) : (t == 1 ? 1 : 0); }
__host__ __device__ constexpr int pl_tb(int fmt, int t) { return fmt == 0 ? (t == 0 ? 2 : (t == 2 || t == 3) ? 1 : 0) : (t == 0 ? 1 : 0); }

// ---- image geometry ---------------------------------------------------------------------------------------------------------------
// Stage (row block rb of IMG_ROWS rows, kb of IMG_BK contraction elements) = NP planes of IMG_PLANE_B bytes, [row][IMG_ROW_B bytes]
// with the two 16-byte halves of a row swapped where bit 3 of the row is set.  Every writer leaves rows past the operand's end, up
// to the end of its last row block, and contraction elements past K as ZEROS: readers neither clamp nor mask.
#define IMG_ROWS 128
#define IMG_BK 16
#define IMG_ROW_B 32                  // IMG_BK x 2 bytes
#define IMG_PLANE_B 4096              // IMG_ROWS x IMG_ROW_B
template <int FMT> struct PlanesFmt { static constexpr int NP = FMT == 0 ? 3 : 2, NT = FMT == 0 ? 6 : 3; };      // planes, terms
__host__ __device__ constexpr size_t img_floats(int rows, int cols, int np = 3) {
    return (size_t)((rows + IMG_ROWS - 1) / IMG_ROWS) * ((cols + IMG_BK - 1) / IMG_BK) * (np * IMG_PLANE_B / 4);
}
// Address arithmetic is kept as macros: as functions the compiler orders it differently, and a refactor of these kernels is checked
// by comparing their machine code byte for byte (scripts/device_code_diff.py).
// byte offset of stage (rb, kb) of an image with nkb stages per row block and np planes
#define IMG_STAGE_OFF(rb, nkb, kb, np) (((int64_t)(rb) * (nkb) + (kb)) * ((np) * IMG_PLANE_B))
// rows whose two 16-byte halves are swapped; byte offset inside a plane of the 16-byte chunk (row rr of the block, contraction half kh)
#define IMG_ROW_SWZ(row) (((row) >> 3) & 1)
__device__ __forceinline__ int planes_chunk_off(int rr, int kh) { return rr * IMG_ROW_B + ((kh ^ IMG_ROW_SWZ(rr)) << 4); }
// LDS byte address of lane (r, h)'s fragment read in a plane copied as is to `base`: row `row` of the block, row & 31 == r
#define IMG_FRAG_SWZ(r, h) (((h) ^ IMG_ROW_SWZ(r)) * 16)
#define IMG_FRAG_ADDR(base, row, r, h) ((base) + (row) * IMG_ROW_B + IMG_FRAG_SWZ(r, h))
// stage of a weight-image convolution in LDS: the weight's three planes, then the fp32 activation tile
#define IMG_W_STAGE_B(tile_floats) (3 * IMG_PLANE_B + (tile_floats) * 4)
