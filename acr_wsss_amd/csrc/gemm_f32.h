// What the fp32 GEMM translation units share (gemm_f32.hip: exact-fp32 / in-register-split loops and the acr_gemm_f32 dispatch;
// gemm_planes.hip: products on operand images; conv1x1.hip: the stem's 1x1 convolutions on both): the kernel argument block, the
// tile constants, the epilogues every loop ends in, the launch plans and the host functions called across the file boundaries.
#pragma once
#include "acr_split.h"

#define F_BM 128
#define F_BN 128
#define F_BK 32
#define F_PKC 36                 // [i][k] pitch (floats)
#define F_PKS 128                // [k][i] pitch (floats)
#define F_STAGE (F_BM * F_PKC)   // floats per operand per stage (>= F_BK * F_PKS = 4096)

struct GemmF32Args {
    const float* a; int64_t lda;
    const float* b; int64_t ldb;
    const float* bias;             // (N) or null
    const float* aux; int64_t ldaux;   // resid (ACT 0) / saved pre-activation h (ACT 2), (M,N) or null
    float* c; int64_t ldc;
    float* c2;                     // ACT 1: GELU(c), same pitch
    float* cs;                     // TN: per-split column sums of A (bias gradient slabs) or null
    int M, N, K;
    int tiles_m, tiles_n, nsplit, kps;   // kps: contraction elements per split (multiple of F_BK)
    int tile0, tiles_launch;             // this launch covers tiles tile0 .. tile0 + tiles_launch - 1 (each nsplit times)
    int nkb_a, nkb_b;                    // gemm_f32_planes_tn_kernel: stages (16 features) per token block of the a / b image
    int img_nkb;                         // image epilogues (ACT 5, 6): stages per row block of the OUTPUT image c2 points at (ceil(N / 16))
    const int* ea; const int* eb;        // fp16x2 images: scale exponents per output row (of a) / column (of b)
    // z-slices: workgroup slice z = split index.  K-split (weight gradient of a Linear): operands shared, k range z*k_zs..;
    // batch (1x1 convolutions per sample): operands / outputs advance by *_zs per slice, k range the whole contraction
    int64_t a_zs, b_zs, c_zs, aux_zs;
    int k_zs, ksplit;                    // slice z = split / ksplit (operand / output offsets), contraction part split % ksplit
};

// Tile order of the NT / NN products: bands of 8 tile rows, column-major inside a band, so that the 64 workgroups an XCD
// holds at a time (it walks one contiguous range of this order, acr_xcd_remap) form an 8 x 8 block of tiles: 8 + 8 operand
// panels (6.3 MB at K = 768) per 64 tiles instead of one A panel + ALL B panels per tile row (N = 3072: the 9.4 MB weight
// exceeds one XCD's 4 MB L2 and was re-fetched for every tile row: 1.04 GB fetched for 86 MB of operands).
#define F_BAND 8
__device__ __forceinline__ void tile_coords(int tt, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int per_band = F_BAND * tiles_n;
    const int band = tt / per_band, in_band = tt - band * per_band;
    const int first = band * F_BAND;
    const int rows = min(tiles_m - first, F_BAND);
    tn = in_band / rows;
    tm = first + (in_band - tn * rows);
}

// epilogue of one wave's 64x64 block (rows mb.., columns nb..): lane (r, h), register e of a 32x32 accumulator = row
// krow(e, h), column r.  EDGE = false: the tile is interior, every access is unconditional (loads batch, no branches).
template <int ACT, bool EDGE>
__device__ __forceinline__ void epilogue_f32(const GemmF32Args& g, f32x16 (&acc)[2][2], int mb, int nb, int r, int h) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = nb + j * 32 + r;
        const bool cok = !EDGE || col < g.N;
        const float bj = (ACT != 2 && g.bias && cok) ? g.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float x[16];
            if (ACT == 2 || (ACT == 0 && g.aux)) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = mb + i * 32 + acr_krow(e, h);
                    x[e] = (!EDGE || (row < g.M && cok)) ? g.aux[(int64_t)row * g.ldaux + col] : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = mb + i * 32 + acr_krow(e, h);
                if (EDGE && !(row < g.M && cok)) continue;
                float v = acc[i][j][e] + bj;
                float* cp = g.c + (int64_t)row * g.ldc + col;
                if (ACT == 0) {
                    *cp = g.aux ? v + x[e] : v;
                } else if (ACT == 1) {                          // one erff serves GELU and GELU'
                    const float er = erff(v * 0.70710678118654752440f);
                    g.c2[(int64_t)row * g.ldc + col] = v * 0.5f * (1.0f + er);
                    *cp = 0.5f * (1.0f + er) + v * (expf(-0.5f * v * v) * 0.39894228040143267794f);
                } else {
                    *cp = v * x[e];
                }
            }
        }
    }
}

// everything after the K loop of a DMA-ring kernel: tail slab (ACT 4), split slab + bias-gradient column sums (ACT 3) or the
// epilogue.  `smem` must be free (all fragment reads behind a barrier).
template <bool A_KC, int ACT>
__device__ __forceinline__ void gemm_f32_finish(const GemmF32Args& g, f32x16 (&acc)[2][2], float* smem, int split, int tt, int tn, int m0,
                                                int n0, int zs, int wm, int wn, int r, int h, int tid, float csum, bool want_cs) {
    if (ACT == 4) {                                         // K-split tail tile: raw accumulators into a compact slab
        float* slab = g.c + ((int64_t)split * g.tiles_launch + (tt - g.tile0)) * (F_BM * F_BN);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = wn * 64 + j * 32 + r;
#pragma unroll
                for (int e = 0; e < 16; ++e) slab[(wm * 64 + i * 32 + acr_krow(e, h)) * F_BN + col] = acc[i][j][e];
            }
        return;
    }
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
        if (want_cs) {
            float* red = smem;                              // behind the loop's last barrier
            red[tid] = csum;
            __syncthreads();
            if (tid < 128 && m0 + tid < g.M) g.cs[(int64_t)split * g.M + m0 + tid] = red[tid] + red[tid + 128];
        }
        return;
    }
    GemmF32Args gz = g;
    gz.c += (int64_t)zs * g.c_zs;
    if (gz.aux) gz.aux += (int64_t)zs * g.aux_zs;
    if (m0 + F_BM <= g.M && n0 + F_BN <= g.N)
        epilogue_f32<ACT, false>(gz, acc, m0 + wm * 64, n0 + wn * 64, r, h);
    else
        epilogue_f32<ACT, true>(gz, acc, m0 + wm * 64, n0 + wn * 64, r, h);
}

#define S_BK 16                      // stage depth of the split-product loops (one bf16 MFMA k-step)
#define S_TILE (F_BM * S_BK)         // floats per operand per stage (8 KiB)
#define P_BK IMG_BK                  // ... and of the loops on images
#define P_SLOTS 3

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- gemm_f32.hip
struct TailPlan { int ntail, nsplit, kps; };
struct TnPlan { int nsplit, kps; };
TailPlan gemm_tail_plan(int M, int N, int K, bool x3 = false);
TnPlan tn_plan(int M, int N, int K);
size_t gemm_ws_base_floats(int mode, int M, int N, int K, bool x3 = false);
// gemm_f32_reduce_kernel / gemm_f32_tail_epilogue_kernel<act>
void gemm_f32_reduce(const float* ws, int nsplit, int64_t n4, float* out, hipStream_t st);
void gemm_f32_tail_epilogue(int act, const GemmF32Args& ge, const float* ws, int ntail, int nsplit, hipStream_t st);
// the loops a 1x1 convolution runs on: <a_kc, b_kc, act> of gemm_f32_split_kernel (loop 2), gemm_f32_dma_kernel (1), gemm_f32_kernel (0)
enum { GEMM_LOOP_STAGED = 0, GEMM_LOOP_DMA = 1, GEMM_LOOP_SPLIT = 2 };
void gemm_f32_conv_launch(int loop, bool a_kc, bool b_kc, int act, dim3 grid, const GemmF32Args& g, hipStream_t st);

// ---- gemm_planes.hip
struct PlanesPlan { bool on; int nkb; size_t a_fl, b_fl, cs_fl; };
PlanesPlan planes_plan(int mode, int math, int M, int N, int K);
int* h2_exps(const float* img, int rows, int cols);
void h2_image_rows(const float* x, int64_t ld, int rows, int cols, float* img, float* colsum, float* ws, hipStream_t st);
void h2_image_cols(const float* x, int64_t ld, int rows, int cols, float* img, float* colsum, float* ws, hipStream_t st);
void h2_image_t(const float* x, int64_t ld, int rows, int cols, float* img, float* ws, hipStream_t st);
template <int FMT>
int gemm_planes(int32_t mode, int32_t act, const float* a_img, const float* b_img, const float* bias, const float* aux, int64_t ldaux,
                float* c, int64_t ldc, float* c2, float* colsum, int32_t M, int32_t N, int32_t K, float* ws, const int* ea, const int* eb,
                hipStream_t st);
