/*
 * acr_hip.h -- C ABI of libacr_hip.so, the MI355X (gfx950) implementation of the ACR_WSSS hot path.
 *
 * The reference (OpenNLPLab/ACR_WSSS) has no FFI layer: its hot path is stock PyTorch ops called from
 * Python.  This header is the boundary the replacement defines underneath the reference's Python
 * surface.  Each entry point names the reference code it replaces (file:line under
 * the reference root).  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - plain C, no torch types; device pointers are raw `void*` / `float*` owned by the caller
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); no hidden synchronisation,
 *     no allocation -> safe to capture into a hipGraph, re-entrant.  The ONLY process-wide state is
 *     the explicit option table below (acr_set_option): a kernel-variant selector for an A/B measurement,
 *     atomically readable, never read from the environment by the library itself
 *   - returns 0 on success, a negative acr_status on failure; acr_last_error() gives a
 *     thread-local message for the last failure on the calling thread
 *   - tensors are row-major; "stride" arguments are in ELEMENTS of the tensor's dtype
 */
#ifndef ACR_HIP_H
#define ACR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACR_ABI_VERSION 2      /* 2: per-call `math` argument of the fp32 GEMM / 1x1-convolution entries, ACR_F32_BF16X3, acr_attn_bwd_ws_floats, acr_split3_bf16 */

typedef enum acr_status {
    ACR_OK = 0,
    ACR_ERR_INVALID = -1,      /* bad argument (null pointer, unsupported head_dim, ...) */
    ACR_ERR_LAUNCH = -2,       /* hipLaunch / hipGetLastError failure */
    ACR_ERR_UNSUPPORTED = -3   /* dtype / shape not built into this library */
} acr_status;

/* ACR_F32: fp32 tensors, exact-fp32 MFMA (parity / inference precision).
 * ACR_BF16: bf16 tensors, bf16 MFMA with fp32 accumulate and fp32 softmax (training throughput precision).
 * ACR_BF16_F32MATH: bf16 tensors, every product in exact fp32 (debug / reference for the bf16 kernels).
 * ACR_F32_BF16X3: fp32 tensors; every matrix product is evaluated on the bf16 MFMA as six exact terms of a three-way
 *   operand split (acr_math below), fp32 accumulate, fp32 softmax / lse / delta / head mean -- fp32-accurate results at the
 *   bf16 matrix rate.  Accepted by acr_attn_fwd_scores / acr_attn_bwd_scores (training attention). */
typedef enum acr_dtype { ACR_F32 = 0, ACR_BF16 = 1, ACR_BF16_F32MATH = 2, ACR_F32_BF16X3 = 3 } acr_dtype;

/* How an fp32 entry point multiplies (a PER-CALL argument: two models, or two calls of one model, may differ).
 * ACR_MATH_F32: v_mfma_f32_32x32x2_f32, exact fp32 products (157 TF peak).
 * ACR_MATH_BF16X3: a = a0 + a1 + a2 with a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1) (3 x 8 = 24 mantissa
 *   bits = all of an fp32 mantissa), a.b ~ a0b0 + a0b1 + a1b0 + a1b1 + a0b2 + a2b0 on v_mfma_f32_32x32x16_bf16 (the dropped
 *   terms are <= 2^-24 |a.b|); every bf16 x bf16 product is exact in fp32 and the sums accumulate in fp32.  Same tensors,
 *   layouts, epilogues and determinism as ACR_MATH_F32; as accurate against float64 as the fp32 FMA chain
 *   (tests/test_kernels_gpu.py::test_split_math_adversarial_operands).  Peak: bf16 MFMA peak / 6 = 417 TF-equivalent.
 * ACR_MATH_FP16X2 (opt-in, narrower: 22 significand bits per operand instead of 24): every operand group -- a row of an NT / NN
 *   operand, a column of a TN operand, i.e. one NON-contracted index -- gets an exact power-of-two scale 2^e with
 *   max|finite x| 2^e in [2^14, 2^15) (e = 0 for an all-zero group), and x 2^e = p0 + p1 with p0 = fp16(x 2^e),
 *   p1 = fp16(x 2^e - p0) (ldexp scaling, never a float factor); a.b = ldexp(sum(a0b0 + a0b1 + a1b0), -(e_a + e_b)) on
 *   v_mfma_f32_32x32x16_f16 (same rate and lane maps as the bf16 form), products exact in fp32, fp32 accumulate.  Per element
 *   |x - (p0 + p1) 2^-e| <= ACR_FP16X2_REL |x| + ACR_FP16X2_FLOOR max|group| (the floor: half of fp16's smallest subnormal
 *   2^-24 in units where the group maximum is >= 2^14).  A NaN operand element stays NaN; an inf element becomes NaN (its
 *   second piece is inf - inf) -- never a finite result; groups without a non-finite element are unaffected.  No atomics,
 *   fixed-order reductions, no host synchronisation.  Accepted by acr_gemm_f32 only (and the fp16x2 image calls below); the
 *   1x1 / 3x3 convolution entries return ACR_ERR_UNSUPPORTED for it, and attention has no fp16x2 dtype. */
typedef enum acr_math { ACR_MATH_F32 = 0, ACR_MATH_BF16X3 = 1, ACR_MATH_FP16X2 = 2 } acr_math;
#define ACR_FP16X2_REL 2.384185791015625e-07      /* 2^-22 */
#define ACR_FP16X2_FLOOR 1.8189894035458565e-12   /* 2^-39 */

typedef enum acr_getam_func {   /* DPT/ACR.py:189-205 */
    ACR_GETAM_GRAD = 0, ACR_GETAM_CAM_GRAD = 1, ACR_GETAM_GRAD_S = 2, ACR_GETAM_CAM_GRAD_S = 3
} acr_getam_func;

/* Geometry of one multi-head attention problem.  q, k, v share one stride triple so that they can
 * alias slices of the packed output of the qkv Linear, (B, T, 3, H, d): sb = 3*H*d*T, st = 3*H*d,
 * sh = d (no permute copy, models/vision_transformer.py:200-201).  o / do use (o_sb, o_st, o_sh);
 * for the reference's (B, T, H*d) activation layout: o_sb = T*H*d, o_st = H*d, o_sh = d
 * (the transpose(1,2).reshape of vision_transformer.py:211 is folded into the store).
 * head_dim must be 64 (every ViT the reference's backbone_dict reaches: tiny/small/base/large). */
typedef struct acr_attn_desc {
    int32_t B, H, T, head_dim;
    int32_t dtype;              /* acr_dtype of q/k/v/o/do/dq/dk/dv */
    float   scale;              /* head_dim^-0.5, vision_transformer.py:173 */
    int64_t qkv_sb, qkv_st, qkv_sh;
    int64_t o_sb, o_st, o_sh;
} acr_attn_desc;

int         acr_version(void);
const char* acr_last_error(void);

/* Kernel-variant selector (A/B measurement switch; the default = the measured-fastest setting).
 * Process-wide, set explicitly by the host (acr_wsss_amd/_lib.py set_option); results are identical under every setting.
 * Codes 0-6 and 8-12 named variants that were retired once their A/B was settled; they are unknown options now.
 * acr_set_option returns ACR_ERR_INVALID for an unknown option; acr_get_option returns INT32_MIN for one. */
typedef enum acr_option {
    ACR_OPT_ATTN_DELTA_1HEAD = 7, /* 1: the delta pass of the resident-score backward keeps one wave per (query block, head) reading the gradient block from HBM itself (A/B of the 4-head LDS-staged kernel) */
} acr_option;
int     acr_set_option(int32_t option, int32_t value);
int32_t acr_get_option(int32_t option);

/* ---- attention (models/vision_transformer.py:198-214 `Attention.forward`, minus the two Linears) ----
 * O = softmax(q k^T * scale) v without materialising P.  lse2 (B,H,T) fp32 receives the row
 * log-sum-exp in base-2 units of the scaled logits: P[b,h,i,j] = exp2(s2 - lse2), s2 = q.k*scale*log2(e).
 * If pmean != NULL it receives mean_h P (B,T,T) fp32 with batch stride pmean_sb and row pitch pmean_st
 * (>= T): the per-layer slice of the (B,L,T,T) stack DPT/ACR.py:107-112 builds with 12 mean kernels + stack. */
int acr_attn_fwd(const acr_attn_desc* desc, const void* q, const void* k, const void* v,
                 void* o, float* lse2, float* pmean, int64_t pmean_sb, int64_t pmean_st, void* stream);

/* Backward of acr_attn_fwd.  gmean (nullable) is dLoss/d(mean_h P), (B,T,T) fp32, batch stride
 * gmean_sb, row pitch gmean_st >= T (what autograd delivers to the `torch.mean(attn, dim=1)` node of
 * DPT/ACR.py:109; a pitch that is a multiple of 4 floats lets the bf16 kernels pull it in 16-byte groups).  dP_h = dO_h V_h^T + gmean/H.  delta_ws: caller-owned (B,H,T) fp32 scratch.
 * dq/dk/dv use the q/k/v strides (they may alias slices of one packed (B,T,3,H,d) buffer). */
int acr_attn_bwd(const acr_attn_desc* desc, const void* q, const void* k, const void* v,
                 const void* o, const void* d_o, const float* lse2,
                 const float* gmean, int64_t gmean_sb, int64_t gmean_st,
                 void* dq, void* dk, void* dv, float* delta_ws, void* stream);

/* ---- the same attention with RESIDENT SCORES (fp32 tensors only; acr_wsss_amd/csrc/attn_f32_sres.hip) ----
 * The exact-fp32 MFMA runs at the fp32 vector rate (157 TF) while HBM moves 6+ TB/s: recomputing a logit (128 FLOP per 4
 * bytes) costs more than reading it back.  acr_attn_fwd_scores computes exactly what acr_attn_fwd computes and additionally
 * stores the scaled base-2 logits s2 of every (b, h) ONCE into `scores` (caller-owned, acr_attn_scores_floats(desc) floats,
 * 16-byte aligned; opaque blocked layout: 32 x 32 tiles in MFMA accumulator order, keys >= T hold -inf).  The head mean
 * (pmean, as in acr_attn_fwd) is then a stream over `scores`, and acr_attn_bwd_scores -- same contract as acr_attn_bwd plus
 * the `scores` of the matching forward call -- runs 5 matrix products instead of 8.  gmean additionally has to be 16-byte
 * aligned with row pitch and batch stride multiples of 4 floats.  Replaces the same reference lines as acr_attn_fwd /
 * acr_attn_bwd (models/vision_transformer.py:203-211 and its autograd backward; there P itself, (B,H,T,T), is what stays
 * resident between forward and backward).
 *
 * desc->dtype = ACR_F32_BF16X3 (csrc/attn_f32_x3.hip): the same contract on the same fp32 tensors, with S, PV, dP, dQ, dK, dV
 * as split products on the bf16 MFMA (acr_math ACR_MATH_BF16X3); softmax, lse2, delta and the head mean stay fp32.  The
 * forward splits q, k, v once into bf16 planes kept BEHIND the score blocks (acr_attn_scores_floats(desc) accounts for them:
 * nine bf16 planes of B*T*H*64 elements), the backward reads them from there (its q / k / v arguments must still be the
 * forward's tensors: when T leaves exactly ONE 32-row block beyond a whole number of workgroups -- T = 785, 1025, 2305 -- that
 * block's rows are computed by the exact-fp32 split-tail workgroups of the ACR_F32 kernels from the fp32 operands) and splits
 * d_o into planes behind delta: delta_ws must hold acr_attn_bwd_ws_floats(desc) floats
 * (B*H*T for ACR_F32) and be 16-byte aligned.  head strides must be >= 64. */
int64_t acr_attn_scores_floats(const acr_attn_desc* desc);
int64_t acr_attn_bwd_ws_floats(const acr_attn_desc* desc);
/* x (rows, cols) fp32 with row pitch ld -> three dense bf16 (rows, cols) planes p0, p1, p2 at planes + i * plane_stride
 * (elements) with x = p0 + p1 + p2 exactly (barring bf16 underflow): p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1).
 * The operand form of acr_math ACR_MATH_BF16X3.  cols %% 8 == 0, 16-byte aligned pointers. */
int acr_split3_bf16(const float* x, int64_t rows, int64_t cols, int64_t ld, void* planes, int64_t plane_stride, void* stream);
int acr_attn_fwd_scores(const acr_attn_desc* desc, const void* q, const void* k, const void* v,
                        void* o, float* lse2, float* scores, float* pmean, int64_t pmean_sb, int64_t pmean_st, void* stream);
/* acr_attn_fwd_scores (desc->dtype = ACR_F32_BF16X3 only) whose output additionally leaves as the split-product image of the
 * (B*T) x (H*64) matrix o (o dense: o_sh = 64, o_st = H*64, o_sb = T*o_st) -- what acr_x3_image(o, H*64, B*T, H*64, o_image, ...) would
 * write, bit for bit, for every row < B*T: the operand of the Linear behind the attention (models/vision_transformer.py:211-212).
 * o_image: acr_x3_image_floats(B*T, H*64) floats; the rows past B*T of the last 128-row block are written as zeros by the call
 * (the image contract; round 6 -- the caller used to zero them).  The leftover 32-row block of T = 1025, 2305, ... stays on an
 * ordinary workgroup in this call: acr_attn_fwd_oimg_offered(desc) = 1 where this entry point is the faster forward, 0 where
 * acr_attn_fwd_scores (split-tail workgroups) + acr_x3_image(o) is. */
int acr_attn_fwd_scores_oimg(const acr_attn_desc* desc, const void* q, const void* k, const void* v,
                             void* o, float* lse2, float* scores, float* pmean, int64_t pmean_sb, int64_t pmean_st, float* o_image,
                             void* stream);
int acr_attn_fwd_oimg_offered(const acr_attn_desc* desc);
int acr_attn_bwd_scores(const acr_attn_desc* desc, const void* q, const void* k, const void* v,
                        const void* o, const void* d_o, const float* lse2, const float* scores,
                        const float* gmean, int64_t gmean_sb, int64_t gmean_st,
                        void* dq, void* dk, void* dv, float* delta_ws, void* stream);

/* Materialise per-head maps for API compatibility with `Attention.get_attn()` /
 * `get_attn_gradients()` (vision_transformer.py:186-196): probs -> P (B,H,T,T) fp32 contiguous,
 * dprobs -> dO V^T (B,H,T,T) fp32 contiguous.  Not used by the fused training / GETAM paths. */
int acr_attn_probs(const acr_attn_desc* desc, const void* q, const void* k, const float* lse2,
                   float* probs, void* stream);
int acr_attn_dprobs(const acr_attn_desc* desc, const void* d_o, const void* v,
                    float* dprobs, void* stream);

/* ---- projections of the attention block (models/vision_transformer.py:200 `self.qkv(x)`, :212 `self.proj(x)`) ----
 * y[M,N] = a[M,K] . b[N,K]^T (+ bias[N]) (+ resid[M,N]); bf16 tensors, fp32 accumulate, hand-written MFMA GEMM.
 * a = activations (rows = tokens), b = nn.Linear weight as stored (N,K).  Also computes the input gradient
 * dX = dY . W when given b = W^T.  ld* are row pitches in elements (multiples of 8), K %% 64 == 0.
 * bias / resid may be NULL.  With y = the packed (B*T, 3*H*64) buffer this is the projection half of the
 * "fused qkv-projection + attention" path: acr_linear_bf16 -> acr_attn_fwd read it in place, no permute. */
int acr_linear_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, const void* bias,
                    const void* resid, int64_t ldr, void* y, int64_t ldy, int32_t M, int32_t N, int32_t K,
                    void* stream);
/* The MLP of a block with its GELU folded into the GEMM epilogues (models/vision_transformer.py:158-164):
 * acr_linear_gelu_bf16: with h = bf16(a w^T + bias) (M,N): act = GELU(h) (exact erf form) and, written to `h`, GELU'(h)
 * -- fc1 forward keeps the derivative its backward needs in place of the pre-activation (nothing else reads it);
 * acr_linear_dgelu_bf16: y = (a w^T) * h -- the input gradient of fc2 taken through the activation
 * (a = dY (M,K), w = W2^T (N,K), h = the GELU'(h) saved by acr_linear_gelu_bf16 (M,N)).  Same operand rules as
 * acr_linear_bf16. */
int acr_linear_gelu_bf16(const void* a, int64_t lda, const void* w, int64_t ldw, const void* bias, void* h, void* act,
                         int64_t ldy, int32_t M, int32_t N, int32_t K, void* stream);
int acr_linear_dgelu_bf16(const void* a, int64_t lda, const void* w, int64_t ldw, const void* h, int64_t ldh, void* y,
                          int64_t ldy, int32_t M, int32_t N, int32_t K, void* stream);


/* ---- the same Linears at the REFERENCE precision: fp32 tensors, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) ----
 * One entry point, three operand arrangements (models/vision_transformer.py:158-164,200,212 and their autograd backward):
 *   ACR_GEMM_NT  c[M,N] = a[M,K] . b[N,K]^T      Linear forward  (a = x, b = W as stored)
 *   ACR_GEMM_NN  c[M,N] = a[M,K] . b[K,N]        input gradient  (a = dy, b = W as stored -- no transposed weight copies)
 *   ACR_GEMM_TN  c[M,N] = a[K,M]^T . b[K,N]      weight gradient (a = dy, b = x, K = tokens), contraction split over
 *                workgroups into fp32 slabs summed in split order (deterministic); colsum (nullable, (M)) receives
 *                sum_k a[k][m] -- the bias gradient -- from the same sweep over dy
 * Epilogues of NT / NN (act): 0: c = acc (+ bias[N]) (+ aux[M,N] = the block's residual);
 *   1: with h = acc + bias: c2 = GELU(h) (exact erf form) and c = GELU'(h) -- fc1 forward writes the activation and, in
 *      place of the pre-activation, the derivative its backward needs (one erff serves both; h itself is used nowhere else);
 *   2: c = acc * aux with aux = the saved GELU'(h) (fc2's input gradient taken through the activation).
 * Pitches in elements, multiples of 4; pointers 16-byte aligned; K %% 4 == 0 (NT/NN), M, N %% 4 == 0 and ldc == N (TN).
 * math: acr_math (how the products are evaluated; everything else is identical).
 * ws: caller-owned scratch of acr_gemm_f32_ws_floats(mode, math, M, N, K) floats (TN: the split slabs; NT / NN: slabs for the
 * K-split tail tiles, 0 when the tile count needs none -- ws may then be NULL; without ws the product runs unsplit.
 * math = ACR_MATH_BF16X3 adds the bf16 planes both operands are split into once per call (csrc/gemm_planes.hip
 * gemm_f32_planes_kernel); with ws == NULL the operand tiles are split inside the GEMM kernel instead, same results).
 * math = ACR_MATH_FP16X2 adds the fp16x2 images of both operands (row-scaled for NT / NN, column-scaled for TN) and requires ws;
 * it has no other way to run (ACR_ERR_INVALID without ws). */
typedef enum acr_gemm_mode { ACR_GEMM_NT = 0, ACR_GEMM_NN = 1, ACR_GEMM_TN = 2 } acr_gemm_mode;
size_t acr_gemm_f32_ws_floats(int32_t mode, int32_t math, int32_t M, int32_t N, int32_t K);
int acr_gemm_f32(int32_t mode, int32_t math, int32_t act, const float* a, int64_t lda, const float* b, int64_t ldb, const float* bias,
                 const float* aux, int64_t ldaux, float* c, int64_t ldc, float* c2, float* colsum, int32_t M, int32_t N,
                 int32_t K, float* ws, void* stream);

/* Weight gradient of a projection: dw[N,K] = dy[M,N]^T . x[M,K] (bf16, fp32 accumulate), contraction over the M tokens
 * split over workgroups with fp32 partial slabs summed in a fixed order (deterministic).  N, K multiples of 128.
 * ws: caller-owned fp32 scratch of acr_wgrad_ws_floats(M, N, K) floats (0 = shape not supported). */
size_t acr_wgrad_ws_floats(int32_t M, int32_t N, int32_t K);
int acr_wgrad_bf16(const void* dy, int64_t ldy, const void* x, int64_t ldx, int32_t M, int32_t N, int32_t K,
                   float* ws, void* dw, void* stream);
/* Weight and bias gradient in one sweep over dy: dbias[n] = sum_m dy[m][n] is accumulated from the dy fragments inside
 * the weight-gradient kernel (no second pass over dy).  ws: acr_wgrad_bias_ws_floats(M, N, K) floats. */
size_t acr_wgrad_bias_ws_floats(int32_t M, int32_t N, int32_t K);
int acr_wgrad_bias_bf16(const void* dy, int64_t ldy, const void* x, int64_t ldx, int32_t M, int32_t N, int32_t K, float* ws,
                        void* dw, void* dbias, void* stream);


/* Bias gradient of a projection: out[n] = sum_m dy[m, n], bf16 in/out, fp32 two-stage deterministic accumulation.
 * ws: caller-owned fp32 scratch of acr_colsum_ws_floats(M, N) floats.  N and ld multiples of 8. */
size_t acr_colsum_ws_floats(int32_t M, int32_t N);
int acr_colsum_bf16(const void* dy, int64_t ld, int32_t M, int32_t N, float* ws, void* out, void* stream);

/* ---- 1x1 convolutions of the ResNetV2 stem, NCHW bf16, stride 1 (models/resnetv2.py:186-190 conv1/conv3/downsample) ----
 * y[n][co][p] = sum_ci w[co][ci] x[n][ci][p] as one MFMA GEMM per sample without any layout change; the same entry
 * point gives the input gradient with w = W^T (cin/cout swapped).  cin %% 64 == 0, hw = H*W %% 8 == 0.
 * addend (nullable, shaped like y): added to the result in fp32 -- the gradient arriving over the block's shortcut.
 * acr_conv1x1_wgrad_bf16: dw[co][ci] = sum_n sum_p dy[n][co][p] x[n][ci][p] (fp32 slabs in ws, fixed-order reduction). */
int acr_conv1x1_bf16(const void* w, int64_t ldw, const void* x, const void* addend, void* y, int32_t nsamp, int32_t cout,
                     int32_t cin, int32_t hw, void* stream);
size_t acr_conv1x1_wgrad_ws_floats(int32_t nsamp, int32_t cout, int32_t cin, int32_t hw);
int acr_conv1x1_wgrad_bf16(const void* dy, const void* x, int32_t nsamp, int32_t cout, int32_t cin, int32_t hw,
                           float* ws, void* dw, void* stream);

/* The same 1x1 convolutions at the reference precision (fp32 NCHW) on the fp32 GEMM kernels, one slice per sample.
 * acr_conv1x1_f32: y[n] = W . x[n] (+ addend[n]); w_transposed = 0: w is (cout, cin); w_transposed = 1: w is stored (cin, cout),
 * i.e. the forward weight handed over as is for the input gradient (no transposed copy).  cout / cin / hw multiples of 4.
 * acr_conv1x1_wgrad_f32: dw (cout, cin) = sum_n dy[n] . x[n]^T through one fp32 slab per sample (ws: nsamp*cout*cin floats).
 * math: acr_math, as for acr_gemm_f32. */
size_t acr_conv1x1_ws_floats(int32_t math, int32_t nsamp, int32_t cout, int32_t cin, int32_t hw);
int acr_conv1x1_f32(int32_t math, const float* w, int32_t w_transposed, const float* x, const float* addend, float* y, int32_t nsamp,
                    int32_t cout, int32_t cin, int32_t hw, float* ws, void* stream);
/* acr_conv1x1_x3: the same product under ACR_MATH_BF16X3 with the weight given as a split-product image -- acr_x3_image of W
 * (cout, cin) for the forward, acr_x3_image_t of the forward's weight for the input gradient -- so that only the activation tile
 * is split inside the kernel (half the vector work per MFMA).  cin %% 16 == 0; ws as acr_conv1x1_f32 (acr_conv1x1_ws_floats). */
int acr_conv1x1_x3(const float* w_img, const float* x, const float* addend, float* y, int32_t nsamp, int32_t cout, int32_t cin, int32_t hw,
                   float* ws, void* stream);
size_t acr_conv1x1_wgrad_f32_ws_floats(int32_t nsamp, int32_t cout, int32_t cin, int32_t hw);
int acr_conv1x1_wgrad_f32(int32_t math, const float* dy, const float* x, int32_t nsamp, int32_t cout, int32_t cin, int32_t hw, float* ws,
                          float* dw, void* stream);

/* ---- split-product images: operands of acr_math ACR_MATH_BF16X3 products made ONCE and used by several products -------------
 * (a Linear's input serves its forward and its weight gradient, its output gradient the input and the weight gradient:
 * models/vision_transformer.py:158-164,200,212 and their autograd backward).  An image holds the three bf16 planes of a
 * row-major fp32 matrix x[rows][cols], tiled [128 rows][16 cols] exactly as the GEMM kernels copy them to LDS
 * (csrc/gemm_planes.hip "PRE-TILED"; the geometry as code: csrc/acr_split.h); zero outside the matrix, so no shape conditions beyond the alignment ones.
 *   acr_x3_image_floats(rows, cols): size of an image in floats.
 *   acr_x3_image: image of x (pitch ld floats).  colsum (nullable, (cols)) receives the column sums of x from the same pass
 *                 -- the bias gradient when x = dy -- through colsum_ws (acr_x3_colsum_ws_floats(rows, cols) floats).
 *   acr_x3_image_t: image of x^T (an image of a (cols) x (rows) matrix): what ACR_GEMM_NT needs of a weight W[out][in] to form
 *                 dx = dy . W without a transposed copy.
 *   acr_gemm_x3: c[M,N] from images, epilogues / workspace / determinism exactly as acr_gemm_f32:
 *     ACR_GEMM_NT  c = A[M,K] . B[N,K]^T   a_img = image of A (M x K), b_img = image of B (N x K)
 *     ACR_GEMM_TN  c = A[K,M]^T . B[K,N]   a_img = image of A (K x M), b_img = image of B (K x N) -- the SAME images of dy and x
 *                  the other two products read (fragments are read transposed from LDS).
 *     act (NT): 0, 1, 2 as acr_gemm_f32; and two epilogues whose output leaves the kernel AS the image the next product reads
 *       (an MLP's 4x-wide tensors never exist in fp32; N %% 8 == 0):
 *       3: with h = acc + bias: c = GELU'(h) (fp32, as act 1) and c2 = IMAGE of GELU(h) (acr_x3_image_floats(M, N) floats);
 *       4: c2 = IMAGE of acc * aux, c unused (may be NULL), colsum (nullable, (N)) = its column sums (the bias gradient of
 *          the Linear whose dy this is), deterministic.
 *   ws: acr_gemm_x3_ws_floats(mode, act, M, N, K) floats (TN: required; NT: K-split tail slabs (+ act 4: column-sum parts), may be
 *       NULL when colsum is NULL).
 * acr_gemm_f32(math = ACR_MATH_BF16X3) is these calls on images it makes in its own workspace. */
size_t acr_x3_image_floats(int32_t rows, int32_t cols);
size_t acr_x3_colsum_ws_floats(int32_t rows, int32_t cols);
int acr_x3_image(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, float* colsum, float* colsum_ws, void* stream);
int acr_x3_image_t(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, void* stream);
size_t acr_gemm_x3_ws_floats(int32_t mode, int32_t act, int32_t M, int32_t N, int32_t K);
/* Many small images in ONE launch (the stem's standardised convolution weights: W, W^T and the packed 3x3 forms).  `descs`: device
 * array of acr_x3_many_desc records: image `dst` (acr_x3_image_floats(rows, K) floats) of the rows x K operand whose element
 * (r, k) is src[r*sr + (k/kin)*sko + (k%kin)*ski] (K, kin multiples of 8; nkb = ceil(K / 16)); record i owns workgroups
 * wg0 .. wg0 + ceil(rows/128) * ceil(nkb/4) - 1 and `blk` (device, nwg int32) maps every workgroup to its record. */
typedef struct acr_x3_many_desc {
    const float* src;
    void* dst;
    int32_t rows, K, sr, kin, sko, ski, wg0, nkb;
} acr_x3_many_desc;
int acr_x3_image_many(const void* descs, const int32_t* blk, int32_t nwg, void* stream);
int acr_gemm_x3(int32_t mode, int32_t act, const float* a_img, const float* b_img, const float* bias, const float* aux, int64_t ldaux, float* c,
                int64_t ldc, float* c2, float* colsum, int32_t M, int32_t N, int32_t K, float* ws, void* stream);

/* ---- fp16x2 images: operands of acr_math ACR_MATH_FP16X2 products, made once and used by several products ---------------------
 * Layout, in floats: the two fp16 planes of x[rows][cols] (x 2^e), tiled [128 rows][16 cols] as the split-product images above
 * (zero outside the matrix); then nexp = 128 max(ceil(rows / 128), ceil(cols / 128)) int32 exponents e along the scaled
 * dimension (0 past its end); then 4 int32, the first of which is the scale direction (acr_h2_dir).
 *   acr_h2_image_floats(rows, cols): size of an image in floats.
 *   acr_h2_ws_floats(rows, cols): scratch of the calls below (per-128-row-block column maxima / column-sum parts).
 *   acr_h2_image: ROW-scaled image of x (pitch ld): the operand of ACR_GEMM_NT.  colsum (nullable, (cols)) = x's column sums
 *                 (through ws, required with colsum).
 *   acr_h2_image_cols: COLUMN-scaled image of x (rows = the contraction): the operand of ACR_GEMM_TN.  ws required; colsum as above.
 *   acr_h2_image_t: ROW-scaled image of x^T (a (cols) x (rows) matrix, one exponent per column of x): a weight's image for dx.
 *                 ws required.
 *   acr_gemm_h2: c[M,N] from images as acr_gemm_x3 (NT: act 0, 1 (c2 = GELU(h)), 2; TN: act 0), K-split tails and workspace
 *                (acr_gemm_h2_ws_floats) as there.  An image whose scale direction does not match the mode (NT: rows, TN:
 *                columns) -- as recorded on the host when an acr_h2_image* call last wrote that address -- is refused with
 *                ACR_ERR_INVALID. */
typedef enum acr_h2_dir { ACR_H2_ROWS = 0, ACR_H2_COLS = 1 } acr_h2_dir;
size_t acr_h2_image_floats(int32_t rows, int32_t cols);
size_t acr_h2_ws_floats(int32_t rows, int32_t cols);
int acr_h2_image(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, float* colsum, float* ws, void* stream);
int acr_h2_image_cols(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, float* colsum, float* ws, void* stream);
int acr_h2_image_t(const float* x, int64_t ld, int32_t rows, int32_t cols, float* image, float* ws, void* stream);
size_t acr_gemm_h2_ws_floats(int32_t mode, int32_t act, int32_t M, int32_t N, int32_t K);
int acr_gemm_h2(int32_t mode, int32_t act, const float* a_img, const float* b_img, const float* bias, const float* aux, int64_t ldaux, float* c,
                int64_t ldc, float* c2, int32_t M, int32_t N, int32_t K, float* ws, void* stream);

/* ---- 3x3 stride-1 SAME convolutions of the stem's bottlenecks (models/resnetv2.py:171-216 `conv2`; std_conv.py:40-65) in NCHW fp32
 * as implicit GEMMs with split products on the bf16 MFMA (math = ACR_MATH_BF16X3 only: ACR_ERR_UNSUPPORTED otherwise -- the
 * exact-fp32 arithmetic keeps the library's Winograd kernels).  No im2col buffer, no layout change.
 * acr_conv3x3_f32: y[n][co][p] = sum_t sum_ci w_packed[co][t*cin + ci] * x[n][ci][p + off_t] (zero outside the image), with
 * w_packed (cout, 9*cin) = w.permute(0,2,3,1) of the (cout, cin, 3, 3) weight.  The input gradient is the same call on dy with
 * w_packed = w.flip(2,3).permute(1,2,3,0) as (cin, 9*cout).  cin %% 16 == 0, H*W %% 4 == 0, 16-byte aligned pointers.
 * ws: acr_conv3x3_ws_floats(...) floats or NULL (0 for launches that fill the chip: only small ones -- CAM generation on one image --
 * are split along the contraction into slabs, summed in a fixed order).
 * No byte outside [x, x + nsamp*cin*H*W) is addressed: the workgroups whose shifted tap windows touch the tensor's two ends clamp
 * their reads into it (ABI 2 rounds 3-4 asked the caller for ACR_CONV3X3_PAD floats of readable slack there; that contract is gone).
 * acr_conv3x3_wgrad_f32: dw_packed (cout, 9*cin) = sum_n sum_p dy[n][co][p] * x[n][ci][p + off_t]; ws: fp32 slabs of
 * acr_conv3x3_wgrad_ws_floats(...) floats, summed in a fixed order (deterministic). */
size_t acr_conv3x3_ws_floats(int32_t nsamp, int32_t cout, int32_t cin, int32_t H, int32_t W);
int acr_conv3x3_f32(int32_t math, const float* w_packed, const float* x, float* y, int32_t nsamp, int32_t cout, int32_t cin,
                    int32_t H, int32_t W, float* ws, void* stream);
/* acr_conv3x3_f32 (math = ACR_MATH_BF16X3) with the packed weight given as a split-product image -- w_img = acr_x3_image of w_packed
 * (rows = cout, cols = 9*cin; for the input gradient of the flipped / role-swapped pack) --: only the activation tile is split in
 * registers, half the vector work per MFMA.  Same shapes, same ws (acr_conv3x3_ws_floats). */
int acr_conv3x3_x3(const float* w_img, const float* x, float* y, int32_t nsamp, int32_t cout, int32_t cin, int32_t H, int32_t W, float* ws,
                   void* stream);
size_t acr_conv3x3_wgrad_ws_floats(int32_t nsamp, int32_t cout, int32_t cin, int32_t H, int32_t W);
int acr_conv3x3_wgrad_f32(int32_t math, const float* dy, const float* x, int32_t nsamp, int32_t cout, int32_t cin, int32_t H, int32_t W,
                          float* ws, float* dw_packed, void* stream);

/* ---- strided SAME convolutions of the stem under split products: the 7x7 stride-2 stem convolution (models/resnetv2.py:337-340 via
 * models/layers/std_conv.py:40-65) and conv2 of the first bottleneck of stages 1 and 2 (3x3 stride 2, resnetv2.py:196-199), which the
 * reference hands to cuDNN through F.conv2d on a padded copy.  Here: one space-to-depth pass, then the 3x3 kernels driven by a TAP TABLE.
 * acr_space_to_depth2_f32: xs[n][(py*2+px)*C + c][y][x] = x[n][c][2y+py][2x+px] (zero past the image), a half-resolution grid of
 *   H2 = ceil(H/2) x W2 = ceil(W/2) with `xrows` >= 4C channel rows per sample, rows 4C.. zeroed.  acr_depth_to_space2_f32: the inverse
 *   (xrows = 4C; H even, W % 8 == 0).
 * acr_conv_taps_x3: y[n][co][p] = sum_t sum_c W[co][t*cin + c] * x[n][tcb[t] + c][p + tdy[t]*W + tdx[t]], zero where (py + tdy[t], px + tdx[t])
 *   leaves the H x W grid; w_img = acr_x3_image of W (rows = cout, cols = ntap*cin); x has xrows channel rows per sample, y has yrows
 *   (>= cout: y may point at a channel slice of a larger tensor -- the input gradient writes one pixel phase per launch);
 *   tdy / tdx / tcb: HOST arrays of ntap <= 16 entries, |tdy|, |tdx| <= 7.  cin % 16 == 0, H*W % 4 == 0.  ws as acr_conv3x3_x3
 *   (acr_conv_taps_ws_floats; ignored when yrows != cout).  No byte outside [x, x + nsamp*xrows*H*W) is addressed.
 * acr_conv_taps_wgrad_f32: dw_packed[co][t*cin + c] = sum_n sum_p dy[n][co][p] * x[n][tcb[t] + c][p + tdy[t]*W + tdx[t]] (same zeros);
 *   W % 4 == 0, W >= 16, H*W % 16 == 0; ws = acr_conv_taps_wgrad_ws_floats floats (slabs, summed in a fixed order). */
int acr_space_to_depth2_f32(const float* x, float* xs, int32_t nsamp, int32_t C, int32_t H, int32_t W, int32_t xrows, void* stream);
int acr_depth_to_space2_f32(const float* xs, float* x, int32_t nsamp, int32_t C, int32_t H, int32_t W, void* stream);
size_t acr_conv_taps_ws_floats(int32_t nsamp, int32_t cout, int32_t cin, int32_t H, int32_t W, int32_t ntap);
int acr_conv_taps_x3(const float* w_img, const float* x, float* y, int32_t nsamp, int32_t cout, int32_t cin, int32_t H, int32_t W, int32_t ntap,
                     const int32_t* tdy, const int32_t* tdx, const int32_t* tcb, int32_t xrows, int32_t yrows, float* ws, void* stream);
size_t acr_conv_taps_wgrad_ws_floats(int32_t nsamp, int32_t cout, int32_t cin, int32_t H, int32_t W, int32_t ntap);
int acr_conv_taps_wgrad_f32(int32_t math, const float* dy, const float* x, int32_t nsamp, int32_t cout, int32_t cin, int32_t H, int32_t W,
                            int32_t ntap, const int32_t* tdy, const int32_t* tdx, const int32_t* tcb, int32_t xrows, float* ws, float* dw_packed,
                            void* stream);

/* ---- 3x3 stride-2 max-pool of the stem with TF-SAME -inf padding folded in (models/resnetv2.py:322-328) ----
 * x (nc, h, w) -> y (nc, ho, wo); amax = 1-byte window argmax (i*3+j, first maximum like ATen) kept for the backward,
 * which gathers (no atomics).  Window (ho, wo) starts at (2 ho - pad_top, 2 wo - pad_left). */
int acr_maxpool3x3s2_fwd_bf16(const void* x, void* y, uint8_t* amax, int64_t nc, int32_t h, int32_t w, int32_t ho,
                              int32_t wo, int32_t pad_top, int32_t pad_left, void* stream);
int acr_maxpool3x3s2_bwd_bf16(const void* dy, const uint8_t* amax, void* dx, int64_t nc, int32_t h, int32_t w,
                              int32_t ho, int32_t wo, int32_t pad_top, int32_t pad_left, void* stream);
/* the same for fp32 maps (the reference's precision) */
int acr_maxpool3x3s2_fwd_f32(const void* x, void* y, uint8_t* amax, int64_t nc, int32_t h, int32_t w, int32_t ho,
                             int32_t wo, int32_t pad_top, int32_t pad_left, void* stream);
int acr_maxpool3x3s2_bwd_f32(const void* dy, const uint8_t* amax, void* dx, int64_t nc, int32_t h, int32_t w,
                             int32_t ho, int32_t wo, int32_t pad_top, int32_t pad_left, void* stream);
/* y[nc][i][j] = x[nc][2i][2j] (Ho = ceil(h/2), Wo = ceil(w/2)): the input of a stride-2 1x1 convolution (DownsampleConv, resnetv2.py:232-249),
 * and its backward dx = dy on the even pixels, zero elsewhere.  fp32. */
int acr_subsample2_fwd_f32(const float* x, float* y, int64_t nc, int32_t h, int32_t w, void* stream);
int acr_subsample2_bwd_f32(const float* dy, float* dx, int64_t nc, int32_t h, int32_t w, void* stream);

/* ---- Fused optimizer step, bf16 weights + fp32 masters (tool/torchutils.py:10-31 PolyOptimizer = SGD with
 * momentum slot = wt_dec, weight decay 0):  mom = momentum*mom + g;  master -= lr*mom;  param = bf16(master).
 * table: device array of acr_sgd_tensor; block b of the launch updates chunk blk_chunk[b] (acr_sgd_chunk_elems()
 * elements) of tensor blk_tensor[b].  Entries with grad == NULL are skipped (parameter without gradient). */
typedef struct acr_sgd_tensor {
    const void* grad;   /* bf16 (n) or NULL */
    float* master;      /* fp32 (n) */
    float* mom;         /* fp32 (n) momentum buffer */
    void* param;        /* bf16 (n) working copy */
    int64_t n;
} acr_sgd_tensor;
int32_t acr_sgd_chunk_elems(void);
int acr_sgd_step_bf16(const void* table, const int32_t* blk_tensor, const int32_t* blk_chunk, int32_t nblocks, float lr,
                      float momentum, void* stream);
/* the same for an all-fp32 model: grad fp32, `master` is the parameter itself, `param` unused (NULL) */
int acr_sgd_step_f32(const void* table, const int32_t* blk_tensor, const int32_t* blk_chunk, int32_t nblocks, float lr,
                     float momentum, void* stream);

/* ---- Batched transpose: dst_i (cols, rows) = src_i (rows, cols)^T for a table of bf16 matrices in one launch (the
 * (in, out) copies of the block weights that the input-gradient GEMMs read; refreshed once per optimizer step).
 * rows and cols multiples of 8; block b transposes 64x64 tile (b - tile0) of tensor blk_tensor[b]. */
typedef struct acr_tr_tensor {
    const void* src;
    void* dst;
    int32_t rows, cols;
    int32_t tile0;      /* index of the tensor's first tile in the launch */
    int32_t tiles_c;    /* ceil(cols / 64) */
} acr_tr_tensor;
int acr_transpose_many_bf16(const void* table, const int32_t* blk_tensor, int32_t nblocks, void* stream);
/* the same for fp32 matrices (rows and cols multiples of 4) */
int acr_transpose_many_f32(const void* table, const int32_t* blk_tensor, int32_t nblocks, void* stream);

/* ---- LayerNorm of the transformer blocks (models/vision_transformer.py:219-222,299), bf16 (M, C) rows ----
 * C a multiple of 256, <= 1024.  stats: (M*2) fp32 [mean, rstd].  Backward writes dx, dgamma, dbeta in one pass over
 * x and dy; ws: fp32 scratch of acr_layernorm_ws_floats(M, C) floats (per-wave partials, summed in wave order).
 * dskip (nullable, (M, C) bf16): gradient arriving over the residual connection x -> x + f(LN(x)); it is added to dx
 * in fp32 before the single bf16 rounding, which replaces autograd's separate accumulation pass. */
size_t acr_layernorm_ws_floats(int32_t M, int32_t C);
int acr_layernorm_fwd_bf16(const void* x, const void* gamma, const void* beta, void* y, float* stats, int32_t M,
                           int32_t C, float eps, void* stream);
int acr_layernorm_bwd_bf16(const void* dy, const void* x, const void* gamma, const float* stats, const void* dskip,
                           void* dx, float* ws, void* dgamma, void* dbeta, int32_t M, int32_t C, void* stream);

/* fp32 rows (reference precision), same contract with float tensors. */
int acr_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* stats, int32_t M, int32_t C,
                          float eps, void* stream);
int acr_layernorm_bwd_f32(const float* dy, const float* x, const float* gamma, const float* stats, const float* dskip, float* dx,
                          float* ws, float* dgamma, float* dbeta, int32_t M, int32_t C, void* stream);
/* LayerNorm whose output leaves as a split-product image (acr_x3_image layout, rows = M, cols = C: the operand of the Linear that
 * follows -- norm1 -> attn.qkv, norm2 -> mlp.fc1, vision_transformer.py:219-226): no fp32 y is written.  stats as acr_layernorm_fwd_f32
 * (the backward is acr_layernorm_bwd_f32 on x and stats).  C in {256, 512, 768, 1024}. */
int acr_layernorm_image_f32(const float* x, const float* gamma, const float* beta, float* image, float* stats, int32_t M, int32_t C, float eps,
                            void* stream);

/* ---- token assembly of the hybrid ViT (vision_transformer.py:449-467: flatten(2).transpose(1, 2), cat(cls[, dist], x), + pos_embed) ----
 * acr_tokens_fwd_f32: tok[b][P+t][d] = y[b][d][t] + bias[d] + pos[P+t][d], tok[b][p][d] = prefix[p][d] + pos[p][d] for p < P;
 *   y (B, D, T) = the patch projection's output WITHOUT its bias, prefix (P, D) = class (+ distillation) token, pos (P+T, D), P <= 8.
 * acr_tokens_bwd_f32: dy[b][d][t] = dtok[b][P+t][d], dpos[r][d] = sum_b dtok[b][r][d] in batch order (the bias gradient is the sum of
 *   dpos rows >= P, the prefix gradient its first P rows). */
int acr_tokens_fwd_f32(const float* y, const float* bias, const float* prefix, const float* pos, float* tok, int32_t B, int32_t D, int32_t T,
                       int32_t P, void* stream);
int acr_tokens_bwd_f32(const float* dtok, float* dy, float* dpos, int32_t B, int32_t D, int32_t T, int32_t P, void* stream);

/* ---- ResNetV2 stem: fused GroupNorm(32) [+ residual] [+ ReLU], bf16 NCHW ----
 * models/layers/norm_act.py:69-85 (GroupNormAct), models/resnetv2.py:205-215 (norm3 -> act3(x + shortcut)).
 * act: 0 = none, 1 = ReLU, 2 = ReLU(gn(x) + resid).  x/resid/y: (N,C,H,W) contiguous, HW = H*W (multiple of 8),
 * C a multiple of 32; stats: (N*32*2) fp32 [mean, rstd] written by forward, read by backward.
 * Backward writes dx (and dresid for act 2) plus per-sample partials dgamma_part/dbeta_part (N,C) fp32; with
 * dgamma/dbeta (bf16 (C), nullable as a pair) it also sums them over the samples, in sample order. */
int acr_groupnorm_fwd_bf16(const void* x, const void* resid, const void* gamma, const void* beta, void* y,
                           float* stats, int32_t N, int32_t C, int32_t HW, float eps, int32_t act, void* stream);
int acr_groupnorm_bwd_bf16(const void* dy, const void* x, const void* resid, const void* gamma, const void* beta,
                           const float* stats, void* dx, void* dresid, float* dgamma_part, float* dbeta_part,
                           void* dgamma, void* dbeta, int32_t N, int32_t C, int32_t HW, int32_t act, void* stream);

/* The same at the reference precision (fp32 NCHW tensors, fp32 gamma / beta / gradients): a group of up to 100 352 floats (every
 * group of the 448^2 step; 50 176 in the backward, which holds x and dy) is read ONCE into the registers of a 1024-thread workgroup
 * (round 6), larger ones are streamed twice; HW a multiple of 4; deterministic (fixed-order block reductions, no atomics).
 * _mask_ variants (act 2 only): the forward also writes the ReLU mask of relu(gn(x) + resid), ONE BYTE per 16-byte vector of y
 * (relu_mask: N*C*HW/4 bytes, bit e = element e of the vector was positive), and the backward reads those bytes INSTEAD of the
 * residual -- it needs the residual for nothing else (same expression in both directions: the mask is the one the forward applied).
 * ws (forward; nullable): acr_groupnorm_fwd_ws_floats(N, C, HW) floats -- non-zero only for launches of a few samples (CAM
 * generation on one image), whose (sample, group) pairs are then cut into parts over two launches. */
size_t acr_groupnorm_fwd_ws_floats(int32_t N, int32_t C, int32_t HW);
int acr_groupnorm_fwd_f32(const float* x, const float* resid, const float* gamma, const float* beta, float* y, float* stats,
                          int32_t N, int32_t C, int32_t HW, float eps, int32_t act, float* ws, void* stream);
int acr_groupnorm_bwd_f32(const float* dy, const float* x, const float* resid, const float* gamma, const float* beta,
                          const float* stats, float* dx, float* dresid, float* dgamma_part, float* dbeta_part, float* dgamma,
                          float* dbeta, int32_t N, int32_t C, int32_t HW, int32_t act, void* stream);
int acr_groupnorm_fwd_mask_f32(const float* x, const float* resid, const float* gamma, const float* beta, float* y, float* stats,
                               int32_t N, int32_t C, int32_t HW, float eps, uint8_t* relu_mask, void* stream);
int acr_groupnorm_bwd_mask_f32(const float* dy, const float* x, const uint8_t* relu_mask, const float* gamma, const float* beta,
                               const float* stats, float* dx, float* dresid, float* dgamma_part, float* dbeta_part, float* dgamma,
                               float* dbeta, int32_t N, int32_t C, int32_t HW, void* stream);

/* Weight standardisation of all StdConv2dSame weights of the stem in one launch (models/layers/std_conv.py:56-59).
 * desc_dev: device array of n_conv acr_wstd_desc records sorted by ch_start (first global output-channel index of the
 * conv), n = fan-in, p0 .. p3 device addresses.  forward (backward = 0): p0 = w, p1 = w_hat out, p3 (nullable) = w_hat^T
 * (n, cout) out -- the copy a 1x1 convolution's input-gradient GEMM reads;
 * backward: p0 = w, p1 = dL/dw_hat, p2 = dL/dw out.  bf16 tensors, fp32 statistics. */
typedef struct acr_wstd_desc {
    uint64_t p0, p1, p2, p3;
    int32_t cout, n, ch_start, pad;
} acr_wstd_desc;
int acr_weight_std_bf16(const void* desc_dev, int32_t n_conv, int32_t total_channels, float eps, int32_t backward,
                        void* stream);
int acr_weight_std_f32(const void* desc_dev, int32_t n_conv, int32_t total_channels, float eps, int32_t backward,
                       void* stream);                /* fp32 tensors, same descriptor table */

/* ---- multilabel soft-margin loss of the class logits (train_acr.py:160-161: F.multilabel_soft_margin_loss(x, label) per view) ----
 * x, y: (N, C) fp32 with row pitches ldx, ldy (elements); loss[0] = mean_n (1/C) sum_c -(y ls(x) + (1 - y) ls(-x)), ls = log-sigmoid.
 * Backward: dx (N, C) dense = g[0] * (sigmoid(x) - y) / (N C), g = the upstream gradient of the scalar loss, in DEVICE memory.
 * One launch each way (the stock op: ~20 launches per view and direction); deterministic. */
int acr_mlsm_fwd_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, int32_t N, int32_t C, float* loss, void* stream);
int acr_mlsm_bwd_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* g, int32_t N, int32_t C, float* dx, void* stream);

/* ---- attention-consistency regulariser (train_acr.py:143-161, inline in train()) ----
 * a1, a2: (B,L,T,T) fp32 head-mean stacks of view 1 / view 2 (T = p*p + 1), batch stride a_sb each
 * (so both may live in one (2B,L,T,T) buffer).  With pi(i*p+j) = i*p+(p-1-j):
 *   out[0] = mean_{b,l,c}   |a1[b,l,0,1+c]   - a2[b,l,0,1+pi(c)]|          (cls_align_loss, :160)
 *   out[1] = mean_{b,l,r,c} |a1[b,l,1+r,1+c] - a2[b,l,1+pi(r),1+pi(c)]|    (aff_align_loss, :161)
 * equal to the reference's 3*p in-place block flips (:151-158) followed by two F.l1_loss.
 * partial_ws: caller-owned fp32 scratch of acr_consistency_ws_floats(B,L,T) floats.  Deterministic
 * (fixed-order two-stage reduction, no float atomics). */
size_t acr_consistency_ws_floats(int32_t B, int32_t L, int32_t T);
int acr_consistency_fwd(const float* a1, const float* a2, int64_t a_sb, int32_t B, int32_t L,
                        int32_t T, int32_t p, float* partial_ws, float* out2, void* stream);
/* gout2: device pointer to the two upstream gradients (d/d out[0], d/d out[1]).  Writes
 * g1, g2: (B,L,T,g_st) with row pitch g_st >= T and batch stride g_sb >= L*T*g_st; every element of
 * the T x T maps is written (zeros where the loss does not look); pad columns are left untouched. */
int acr_consistency_bwd(const float* a1, const float* a2, int64_t a_sb, int32_t B, int32_t L,
                        int32_t T, int32_t p, const float* gout2, float* g1, float* g2,
                        int64_t g_sb, int64_t g_st, void* stream);

/* ---- GETAM (DPT/ACR.py:177-215 `ACR.getam`) ----
 * Adds one layer's contribution to cam_row (T fp32, caller zero-initialised):
 *   cam_row[j] += f_h( dP_h[batch,0,j], P_h[batch,0,j] ),  dP_h = dO_h V_h^T (row 0 only)
 * for `func` in acr_getam_func.  Only row 0 of the layer-summed map is consumed by the reference
 * (:213), so nothing else is computed.  The final relu and the [1:] / [2:] slice are the caller's. */
int acr_getam_row_accum(const acr_attn_desc* desc, const void* q, const void* k, const void* v,
                        const void* d_o, const float* lse2, int32_t batch, int32_t func,
                        float* cam_row, void* stream);
/* The same for every sample of the batch in ONE launch (CAM generation batches the flipped and the plain pass and several
 * images: infer_cam.py:147-153 runs them one by one): cam_rows[b*row_stride + j] += f_h(...) of sample b, b = 0 .. desc->B-1. */
int acr_getam_rows_accum(const acr_attn_desc* desc, const void* q, const void* k, const void* v, const void* d_o,
                         const float* lse2, int32_t func, float* cam_rows, int64_t row_stride, void* stream);

/* Affinity refinement (infer_cam.py:164-165,183-184): out[c][r] = sum_l sum_k a[l][1+r][1+k] cam[c][k]
 * for one sample's (L,T,T) head-mean stack `a`, n_cam row vectors cam (n_cam, T-1) -> out (n_cam, T-1). */
int acr_aff_refine(const float* a, int32_t L, int32_t T, const float* cam, int32_t n_cam,
                   float* out, void* stream);
/* nbatch samples in one launch: a[s] = a + s * a_sb, cam / out (nbatch, n_cam, T-1) contiguous. */
int acr_aff_refine_batch(const float* a, int64_t a_sb, int32_t L, int32_t T, const float* cam, int32_t n_cam,
                         int32_t nbatch, float* out, void* stream);

/* ---- input pipeline (myTool.py:1158-1199 get_data_from_chunk_v2, :1364-1403 get_data_from_chunk_val) ----
 * One launch turns a batch of decoded uint8 HWC RGB images into the (B,3,S,S) network input: bilinear resize with
 * cv2.resize's float-path INTER_LINEAR rule (RandomResizeLong :995-1008 / cv2.resize(S,S)), optional horizontal flip
 * (:895-899), (x/255 - mean)/std (:1180-1182) and the zero-padded RandomCrop (:923-955).  The HOST decodes and draws the
 * geometry (the reference uses the unseeded `random` module); packed_u8 holds the images back to back, `table` is a
 * device array of `batch` acr_pre_image records.  Validation batches: rh = rw = S, flip 0, boxes = the whole image.
 * mean3 / std3: HOST pointers to 3 floats.  out_dtype: ACR_F32 or ACR_BF16. */
typedef struct acr_pre_image {
    int64_t offset;        /* byte offset of this image inside packed_u8 */
    int32_t h, w;          /* decoded height, width */
    int32_t rh, rw;        /* height, width after the resize step */
    int32_t flip;          /* 1 = flip horizontally after resizing */
    int32_t cont_top, cont_left, img_top, img_left, ch, cw;   /* RandomCrop: container / image corners, copied extent */
} acr_pre_image;
int acr_preprocess_batch(const void* packed_u8, const void* table, int32_t batch, int32_t S, const float* mean3,
                         const float* std3, int32_t out_dtype, void* out, void* stream);

/* ---- segmentation-training loaders (myTool.py:1257-1310 get_data_from_chunk_v4: image + target map; :1202-1253
 * get_data_from_chunk_v3: image + saliency map, the same code with another resize range; both on RandomResizeLong2 :1010-1023,
 * flip2 :901-905 and RandomCrop2 :957-993) ----
 * A sibling of acr_preprocess_batch: ONE launch writes the four tensors a chunk yields, all from the image's acr_pre_image
 * record.  packed_u8 holds the RGB images AND the single-channel uint8 maps (one H2D copy); map_offsets[b] is the byte offset of
 * image b's (h, w) map inside packed_u8 (a device array next to `table`; read only when map_u8 is given).  With (y, x) an output
 * pixel, "inside" means cont_top <= y < cont_top + ch and cont_left <= x < cont_left + cw; an inside pixel is pixel
 * (ry, rx) = (img_top + y - cont_top, img_left + x - cont_left) of the resized and flipped image, i.e. column rw - 1 - rx of the
 * resized one when flip is set.
 *   images    (B,3,S,S) out_dtype: exactly what acr_preprocess_batch writes for the same table -- same integer sample positions,
 *             same arithmetic, bit for bit (0 outside).
 *   ori_u8    (B,3,S,S) uint8 (:1293-1297): a pure function of the fp32 value x computed for `images` (before any bf16 rounding),
 *             trunc((x * std_c + mean_c) * 255) evaluated as fp32 multiply, add, multiply WITHOUT contraction (numpy on the
 *             reference's float32 container) and clamped to 0..255 before the conversion.  Outside: (123, 116, 103).
 *   croppings (B,S,S) fp32 (:984,991): 1 inside, 0 outside.
 *   map_u8    (B,S,S) uint8: the map through resize-nearest -> flip -> crop with the image's geometry.  Resized pixel (ry, rx)
 *             reads source (min(ry * h / rh, h - 1), min(rx * w / rw, w - 1)) in integer division: OpenCV's published
 *             INTER_NEAREST rule floor(d * src / dst).  cv2 is not part of the reference tree, so this step is UNPINNED in the
 *             same sense as the bilinear rule above; OpenCV evaluates the product d * (src / dst) in double, which can differ from
 *             the exact quotient where d * src / dst is an integer.  Outside the crop box the map holds map_fill (0..255): 0 is
 *             the reference's zero container (:982); 255, the cross-entropy's ignore value, is this project's extension.
 * ori_u8, croppings and map_u8 may each be NULL and are then skipped.  With S % 4 == 0 every output is written with 4-pixel
 * vector stores, so all four buffers must be 16-byte aligned.  The kernel trusts table and map_offsets: the caller validates them. */
int acr_preprocess_seg_batch(const void* packed_u8, const void* table, const int64_t* map_offsets, int32_t batch, int32_t S,
                             const float* mean3, const float* std3, int32_t out_dtype, int32_t map_fill, void* images,
                             void* ori_u8, void* croppings, void* map_u8, void* stream);

/* ---- dense-CRF refinement of CAMs (tool/imutils.py:345-362 crf_inference = pydensecrf DenseCRF2D with
 * addPairwiseGaussian + addPairwiseBilateral + inference(t), called by infer_cam.py:27-40,218-225) ----
 * The permutohedral lattice follows wrapper/bilateralfilter/permutohedral.cpp:112-283 (init) and :441-520 (compute).
 * acr_lattice_build: lattice over the H x W pixels with features (x / sxy, y / sxy) when rgb is NULL (d = 2,
 * addPairwiseGaussian) or (x / sxy, y / sxy, r / srgb, g / srgb, b / srgb) for rgb = (H, W, 3) uint8 (d = 5,
 * addPairwiseBilateral; bilateralfilter.cpp:4-20).  ws = acr_lattice_ws_bytes(H * W, d) bytes of device memory (opaque).
 * acr_lattice_info synchronises the stream and returns the number of lattice points (ACR_ERR_INVALID if a key did not
 * fit the 12-bit-per-coordinate packing).  acr_lattice_tables returns device pointers INTO ws: offsets (n, d+1) int32,
 * weights (n, d+1) float, point_keys (n_points) uint64 (coordinate c of a key = ((k >> 12 (d-1-c)) & 4095) - 2048).
 * acr_lattice_filter: out[k][p] = post_scale * post[p] * sum_q kernel(p, q) * pre[q] * in[k][q] for K planes of n pixels
 * (Permutohedral::compute; pre / post nullable, post_scale applied when apply_scale != 0); vals = scratch of
 * 2 * K * (n_points + 2) floats.  Sums run in the CPU code's order: results equal the reference lattice bit for bit. */
int64_t acr_lattice_ws_bytes(int32_t n_pixels, int32_t d);
int acr_lattice_build(const void* rgb, int32_t H, int32_t W, float sxy, float srgb, void* ws, int64_t ws_bytes, void* stream);
int acr_lattice_info(const void* ws, int32_t* n_points, int32_t* key_overflow, void* stream);
int acr_lattice_tables(void* ws, int32_t n_pixels, int32_t d, void** offsets, void** weights, void** point_keys);
int acr_lattice_filter(const void* ws, int32_t n_pixels, int32_t d, int32_t n_points, const void* in, const void* pre, void* out,
                       const void* post, float post_scale, int32_t apply_scale, int32_t K, void* vals, void* stream);
/* mean field (densecrf v2: unary_from_softmax, DenseKernel NORMALIZE_SYMMETRIC, DenseCRF::inference + expAndNormalize):
 * unary = -log(clamp(probs, clip, 1)); norm = 1 / sqrt(norm + 1e-20) in place; q[:, p] = softmax_k(-unary + msg0 + msg1)
 * over K planes of n pixels (msg0 / msg1 nullable). */
int acr_crf_unary(const void* probs, void* unary, int64_t n, float clip, void* stream);
int acr_crf_norm(void* norm, int32_t n_pixels, void* stream);
int acr_crf_update(const void* unary, const void* msg0, const void* msg1, void* q, int32_t n_pixels, int32_t K, void* stream);
/* Several score stacks through one mean field (crf.crf_with_alphas_device) and the label-map CRF (tool/imutils.py:387-400
 * crf_inference_label).  Planes of a lattice filter call are independent, so G groups of K planes filtered in one call and
 * normalised by acr_crf_update_groups hold, plane for plane, the bits of G separate runs.  All buffers are the caller's, on the
 * device, fp32 unless named _u8; nothing allocates or synchronises.
 * acr_crf_alpha_unary: cams = n_cls planes of n_pixels, alphas = n_alpha floats on the device.  With n = 1 + n_cls, group a is
 *   planes [a n, (a + 1) n) of scores (nullable), unary and q (each n_alpha * n planes):
 *     scores[a n] = powf(1.0f - max_c cams[c], alphas[a]) (the subtraction in fp32, infer_cam.py:31-33);  scores[a n + 1 + c] = cams[c]
 *     unary = -logf(clamp(scores, clip, 1))  (acr_crf_unary's expression);  q = softmax over the group's planes of -unary (what
 *     acr_crf_update gives with null messages).  Each CAM element is read once; scores and unary are stored once, q by its
 *     owning thread as in acr_crf_update (it holds the softmax's intermediate values).  Requires n_alpha * n * n_pixels < 2^31.
 * acr_crf_update_groups: acr_crf_update on each of G groups of K consecutive planes (unary, msg0, msg1, q: G * K planes; the
 *   messages nullable), one launch; per group the operation order is acr_crf_update's, so the result equals G calls on the
 *   sub-stacks bit for bit.  1 <= G <= 65535.
 * acr_crf_label_unary: pydensecrf's unary_from_labels(labels, n_labels, gt_prob, zero_unsure=False) with the energies evaluated by
 *   the caller (in double, rounded to float, so the unary has numpy's bits and the device takes no log): unary[k][p] = e_label
 *   where k == labels_u8[p] and e_other elsewhere, e_label = -log(gt_prob), e_other = -log((1 - gt_prob) / (n_labels - 1)).
 *   THIS PROJECT'S EXTENSION: a label >= n_labels (255 included) is "unsure" and gets e_unsure = -log(1 / n_labels) on all
 *   planes; the reference raises an IndexError there.  q = softmax over the n_labels planes of -unary.  2 <= n_labels <= 255.
 * acr_crf_update_argmax: the last update of a run that only returns labels: label_u8[p] = the FIRST k with the largest
 *   -unary[k][p] + msg0[k][p] + msg1[k][p] (additions in acr_crf_update's order; messages nullable), no exp, no Q.  1 <= K <= 256.
 *   It equals np.argmax of acr_crf_update's Q except where two DISTINCT logits give probabilities that round to the same float:
 *   np.argmax(Q) then takes the lower index, this the larger logit. */
int acr_crf_alpha_unary(const void* cams, int32_t n_cls, int32_t n_pixels, const void* alphas, int32_t n_alpha, float clip, void* scores,
                        void* unary, void* q, void* stream);
int acr_crf_update_groups(const void* unary, const void* msg0, const void* msg1, void* q, int32_t n_pixels, int32_t K, int32_t G, void* stream);
int acr_crf_label_unary(const uint8_t* labels_u8, int32_t n_pixels, int32_t n_labels, float e_label, float e_other, float e_unsure, void* unary,
                        void* q, void* stream);
int acr_crf_update_argmax(const void* unary, const void* msg0, const void* msg1, int32_t n_pixels, int32_t K, uint8_t* label_u8, void* stream);

/* ---- CAM read-outs ----
 * Patch-token -> class activation (DPT/ACR.py:133-134): out[n][c] = relu(x[n,:] . w[c,:] + bias[c]),
 * x (N, D) with row stride x_st, w (C, D) contiguous, out (N, C) contiguous; dtype of x/w/bias. */
int acr_patch_cam(const void* x, int64_t x_st, const void* w, const void* bias, int32_t N, int32_t D,
                  int32_t C, int32_t dtype, float* out, void* stream);
/* Bilinear resize of a (C, ih, iw) fp32 map given as src[(y*iw + x)*src_sp + c*src_sc] to (C, oh, ow)
 * contiguous, torch semantics (infer_cam.py:157 align_corners=0; :187 align_corners=1), then optional
 * per-channel multiply (label mask, :158; chan_mul nullable) and horizontal flip (:159-160,195-196).
 * If accumulate != 0 the result is added to dst (sum over flips/scales, :201,208). */
int acr_bilinear_resize(const float* src, int64_t src_sc, int64_t src_sp, int32_t C, int32_t ih,
                        int32_t iw, float* dst, int32_t oh, int32_t ow, int32_t align_corners,
                        const float* chan_mul, int32_t hflip, int32_t accumulate, void* stream);

/* ---- pixel-adaptive mask refinement of CAMs (pamr.py:115-144 PAMR.forward, with LocalAffinityAbs / LocalStDev /
 * LocalAffinityCopy :10-110; imported by infer_cam.py:14 and train_acr_coco.py:15) ----
 * fp32, planar, contiguous tensors; `dilations` is a HOST array of n_dil (1..8) values >= 1, read during the call.
 * P = 8 * n_dil neighbours per pixel: neighbour 8 * i + j of dilation d_i sits at (y + dy * d_i, x + dx * d_i), clamped to the
 * image (replicate padding), j walking (dy, dx) over {-1, 0, 1}^2 row-major without the centre.
 * acr_pamr_affinity (pamr.py:133-137): x (B, K, H, W) -> w_out (B, P, H, W),
 *   w[p] = softmax_p( mean_k -|x_k - x_k(neighbour p)| / (1e-8 + 0.1 * std_k) ), std_k the unbiased deviation of the
 *   9 * n_dil samples of channel k (the centre counted once per dilation).  A flat neighbourhood gives exactly uniform weights.
 * acr_pamr_propagate (pamr.py:140-141), one iteration: mask_out[c] = sum_p w[p] * mask_in[c](neighbour p) for (B, C, H, W)
 *   masks; mask_in and mask_out must not alias (iterate by ping-pong between two buffers).
 * No atomics, fixed summation order: bit-reproducible, and independent of the batch a sample rides in. */
int acr_pamr_affinity(const float* x, int32_t B, int32_t K, int32_t H, int32_t W, const int32_t* dilations, int32_t n_dil,
                      float* w_out, void* stream);
int acr_pamr_propagate(const float* w, const float* mask_in, float* mask_out, int32_t B, int32_t C, int32_t H, int32_t W,
                       const int32_t* dilations, int32_t n_dil, void* stream);

/* ---- CAM evaluation on the device (evaluation.py:19-52: the TP / P / T counters behind the mIoU of every background threshold;
 * --type png mode and tool/metrics.py:36-41 Evaluator._generate_matrix: the confusion matrix of a label map) ----
 * All counters are int64 and exact: integer sums, bit-identical run to run.  2 <= num_cls <= 128 (background included).
 * acr_eval_sweep_f32 (evaluation.py:27-49, for all thresholds in one pass): cams (n, h, w) fp32 contiguous on the device;
 *   `classes` is a HOST array of n strictly ascending 0-based class indices in [0, num_cls - 1), read during the call,
 *   1 <= n <= num_cls - 1; gt (h, w) uint8 on the device; thresholds (nt) fp32 on the device, strictly ascending (the CALLER's
 *   contract, not checked here), 1 <= nt <= 256.  Per pixel with gt < num_cls (255 = ignore; a gt in num_cls..254 is ignored
 *   too -- a deviation: the reference counts such a pixel in P only, VOC and COCO hold none): v_c = the value of class c's plane,
 *   exactly 0.0f for a class without one; m = max_c v_c; a = 1 + the smallest c with v_c == m (np.argmax: the first maximum);
 *   kfg = #{k : thresholds[k] < m} compared in fp32.  Then, ACCUMULATED into raw:
 *     NVALID += 1;  T[gt] += 1;  FG[kfg][a] += 1;  HIT[kfg][a] += 1 if a == gt;  BG[kfg] += 1 if gt == 0
 *   raw = FG (nt + 1, num_cls) | HIT (nt + 1, num_cls) | BG (nt + 1) | T (num_cls) | NVALID (1), 2 (nt + 1) num_cls + nt + num_cls + 2
 *   values.  Inputs are finite: NaN is outside the contract.
 * acr_eval_sweep_finish (evaluation.py:37-52): a pure function of raw that WRITES TP and P, both (nt, num_cls):
 *   c >= 1: P[k][c] = sum_{j > k} FG[j][c], TP[k][c] = sum_{j > k} HIT[j][c];
 *   P[k][0] = NVALID - sum_{c >= 1} P[k][c];  TP[k][0] = sum_{j <= k} BG[j].
 * acr_eval_confusion_u8: pred, gt (n_pixels) uint8 on the device; conf (num_cls, num_cls + 1), ACCUMULATED into:
 *   conf[gt][min(pred, num_cls)] += 1 for gt < num_cls (1 <= num_cls <= 128); the last column collects predictions outside
 *   the label range, every other gt is ignored.  T = row sums, P = sums of the first num_cls columns, TP = diagonal. */
#define ACR_EVAL_MAX_CLS 128           /* num_cls <= 128: labels and class indices travel as bytes */
#define ACR_EVAL_MAX_NT 256            /* thresholds per sweep */
int acr_eval_sweep_f32(const float* cams, const int32_t* classes, int32_t n, const uint8_t* gt, int32_t h, int32_t w,
                       const float* thresholds, int32_t nt, int32_t num_cls, int64_t* raw, void* stream);
int acr_eval_sweep_finish(const int64_t* raw, int32_t nt, int32_t num_cls, int64_t* TP, int64_t* P, void* stream);
int acr_eval_confusion_u8(const uint8_t* pred, const uint8_t* gt, int64_t n_pixels, int32_t num_cls, int64_t* conf, void* stream);

/* ---- pseudo-label composition from refined CAMs (myTool.py:674-744 compute_seg_label_rrm) ----
 * All outputs are uint8 label maps, exact functions of their inputs (no float sums, integer atomics only): bit-identical run to
 * run.  num_classes = C (background excluded), C + 1 <= 128.  `classes` is a HOST array of K strictly ascending 0-based class
 * indices in [0, C), 1 <= K <= C, read during the call.  A score stack is (K + 1, h, w) fp32 contiguous on the device: plane 0 is
 * label 0 (background), plane j + 1 label classes[j] + 1.  Inputs are finite: NaN is outside the contract.
 * acr_pseudo_label_f32 (myTool.py:705-706, np.argmax over the dense (C + 1, h, w) array): out (h, w) = the smallest label among
 *   the maxima over the labels 0..C, a label without a plane counting as 0.0f (the convention of acr_eval_sweep_f32).
 * acr_pseudo_compose (myTool.py:694-735 and the line kept commented at :737): cams (K, h, w) fp32, plane j the CAM of classes[j];
 *   la / ha the score stacks refined at the low / high background alpha.  With L_la, L_ha their label maps as above:
 *     out = L_la;  out = 255 where L_la == 0;  out = 0 where L_ha == 0                                        (:707-708, :732)
 *   and, if ignore_uncertain != 0, out = 255 wherever  max(ha[0], la[1..K]) < crf_sure  or the pixel is not sure  (:733-737):
 *     m = max_j cams[j] (and 0.0f if K < C);  bg = (float)pow((double)(1.0f - m), bg_alpha);  M = the label map of {0: bg,
 *     classes[j] + 1: cams[j]} as above                                                                        (:694-701)
 *     for every label l that occurs in L_la, and only those                                                    (:710-712)
 *       l == 0: sure where M == 0 and bg > bg_sure                                                             (:724-728)
 *       l > 0:  S = the values cams[l] where M == l and the value > cam_floor, n = |S|; n == 0 (always so for a label without
 *               a plane): no pixel of l is sure -- the reference raises IndexError there; otherwise v = sort(S)[(int)(n *
 *               fg_quantile)], the product in double, and sure where M == l and cams[l] > v                    (:714-722)
 *   All comparisons are fp32.  v is an exact selection on the fp32 bit patterns (a fixed four radix passes over all classes at
 *   once; nothing depends on the data, nothing is read back).  Requires cam_floor >= 0, 0 <= fg_quantile < 1, crf_sure > 0.
 *   ws: acr_pseudo_ws_bytes(K, h, w) bytes on the device, 4-byte aligned, contents arbitrary (cleared here by a kernel on the stream); used
 *   only if ignore_uncertain != 0 (else it may be null).
 * acr_pseudo_ws_bytes: host only; negative for arguments outside the supported range.
 * The entry points allocate nothing and do not synchronise; they capture into a hipGraph. */
#define ACR_PSEUDO_MAX_LABELS 128      /* C + 1 <= 128: labels and plane indices travel as bytes */
int64_t acr_pseudo_ws_bytes(int32_t K, int32_t h, int32_t w);
int acr_pseudo_label_f32(const float* scores, const int32_t* classes, int32_t K, int32_t h, int32_t w, int32_t num_classes,
                         uint8_t* out, void* stream);
int acr_pseudo_compose(const float* cams, const int32_t* classes, int32_t K, const float* la, const float* ha, int32_t h, int32_t w,
                       int32_t num_classes, int32_t ignore_uncertain, double bg_alpha, float cam_floor, double fg_quantile,
                       float bg_sure, float crf_sure, void* ws, int64_t ws_bytes, uint8_t* out, void* stream);

/* ---- saliency-guided pseudo-labels (myTool.py:188-264 compute_seg_label_3; its twin :313-367 compute_seg_label_two_step is the
 * same rule with another background exponent -- bg_alpha: _3 uses 12, two_step uses 32) ----
 * The entry points are acr_sal_pseudo_*, not acr_pseudo_sal_*: tests/test_pseudo_cpu.py counts the symbols that begin with
 * acr_pseudo_ as the three of the rule above and leaves room for one more.
 * For a batch of B images and C classes, 1 <= B <= 65535, 1 <= C <= 127, h * w < 2^31, all arrays contiguous on the device:
 *   cams (B, C, h, w) fp32, finite, in [0, 1];  present (B, C) uint8, nonzero = the image has the class (the reference's
 *   cam_label.astype(uint8) > 1e-5, :190,195) -- the plane of an absent class is never read;  saliency (B, h, w) uint8.
 * Per image, with P = its present classes and v_c = cams[c] at the pixel, every comparison in fp32:
 *   1. m = max(0, max_{c in P} v_c);  bg = (float)pow((double)(1.0f - m), bg_alpha);  L = 0 if bg >= m, else 1 + the smallest
 *      c in P with v_c == m  (np.argmax over [bg, the planes with zeros for absent classes]: the first maximum wins, :217-223)
 *   2. label = 255 where L == 0, else L;  then label = 0 where saliency == 0                                     (:229-230)
 *   3. per c in P: n_c = #{v_c > 0} over the plane, pos_c = (int)(n_c * cut), the product in double; thr_c = the pos_c-th
 *      smallest (0-based) of those values if pos_c > 0, else +inf (:239-243).  A pixel with label == 0 after step 2 takes
 *      label = 1 + the smallest c in P with v_c > thr_c, and its saliency byte becomes 255, if there is such a c (:244-246).
 *      (The reference walks the classes in ascending order and a grabbed pixel is no longer 0, so the lowest class keeps it;
 *      its conflict branch :247-248 asks for a pixel grabbed twice and never fires.)
 *   4. if open_size = k > 0 (:253-255):  F = label != 0 (the 255 pixels count);  with a = k / 2 and D = {-a .. k - 1 - a},
 *        E(y, x) = AND of F(y + dy, x + dx) over dy, dx in D, positions outside the image left out;
 *        O(y, x) = OR of E(y + dy, x + dx) over the SAME offsets (not reflected), positions outside the image left out;
 *      label = 0 where O is false.  This is OpenCV's documented erode / dilate with a k x k box, its default anchor (k / 2,
 *      k / 2) and default borders (+max for the minimum, 0 for the maximum) -- the definition here; cv2 itself is not at hand to
 *      compare with.  For an even k the pair is an opening shifted by one pixel: O can hold where F does not; label is 0 there
 *      anyway.
 *   label (B, h, w) uint8: 0, 1..C, 255.  saliency_out (B, h, w) uint8: the map the reference returns, changed by step 3 only;
 *   it may be `saliency` itself.  label shares its buffer with neither.
 * thr_c is an exact selection on the fp32 bit patterns, for all B * C planes at once (a fixed four radix passes; nothing depends
 * on the data, nothing is read back, integer atomics only): the outputs are bit-identical run to run.
 * Requires bg_alpha > 0, 0 <= cut < 1, 0 <= open_size <= 32.
 *   ws: acr_sal_pseudo_ws_bytes(B, C, h, w) bytes on the device, 4-byte aligned, contents arbitrary (cleared here by a kernel on
 *   the stream).
 * acr_sal_pseudo_ws_bytes: host only; negative for arguments outside the supported range.
 * acr_morph_open_u8 (:254, cv2.morphologyEx(frg, cv2.MORPH_OPEN, np.ones((k, k)))): step 4 alone on B masks (h, w): F = src != 0,
 *   dst = 255 where O else 0 -- for a mask of 0 and 255 the grey-scale opening.  1 <= k <= 32; dst is not src.
 * The entry points allocate nothing and do not synchronise; they capture into a hipGraph. */
#define ACR_SAL_PSEUDO_MAX_CLASSES 127 /* labels c + 1 travel as bytes next to 255 */
int64_t acr_sal_pseudo_ws_bytes(int32_t B, int32_t C, int32_t h, int32_t w);
int acr_sal_pseudo_compose(const float* cams, const uint8_t* present, int32_t B, int32_t C, int32_t h, int32_t w, const uint8_t* saliency,
                           double bg_alpha, double cut, int32_t open_size, void* ws, int64_t ws_bytes, uint8_t* label,
                           uint8_t* saliency_out, void* stream);
int acr_morph_open_u8(const uint8_t* src, int32_t B, int32_t h, int32_t w, int32_t k, uint8_t* dst, void* stream);

/* ---- pseudo-label segmentation loss (myTool.py:825-857 compute_joint_loss: the bilinear upsampling of the logits :831, the
 * background-only / foreground-only cross-entropies with ignore :845-855 -- nn.CrossEntropyLoss(ignore_index=255), or
 * SegmentationLosses.CrossEntropyLoss tool/loss.py:21-33 with batch_average -- and the softmax probabilities :832-833) ----
 * "h, w" / "W, H" are the first and second spatial axis (the reference swaps the names itself, :829-831).
 * logits (B, K, h, w) fp32 contiguous; label (B, W, H) uint8 on the device, 0..K-1 or ignore: 255, and any value in K..254 too.
 * Requires 1 <= B <= 65535, 2 <= K <= 128, 1 <= h <= W, 1 <= w <= H, W * H < 2^31; anything else returns ACR_ERR_INVALID.
 * acr_segloss_fwd: per label pixel pred = bilinear(logits) by torch's align_corners=False rule in fp32 (the rule of
 *   acr_bilinear_resize: src = max(scale * (dst + 0.5) - 0.5, 0), scale = in / out), log-softmax over K, and per image
 *     sum_bg = sum_{label == 0} -log p_0,  n_bg,  sum_fg = sum_{1 <= label < K} -log p_label,  n_fg
 *   written to sums (B, 2) fp32 and counts (B + 1, 2) int64 (row B: the totals over the batch).  Then, over the whole batch,
 *     bg = sum_bg / n_bg,  fg = sum_fg / n_fg  (each also / B if batch_average != 0),  loss (3) = { bg + fg, bg, fg }.
 *   A count of 0 gives NaN for that term (0 / 0), as torch's mean over no pixel does.
 *   probs (B, K, W, H), nullable: the softmax of pred (pred_probs, :832-833).  rowstat (B, W, H, 2), nullable, 8-byte aligned:
 *   the row maximum and the sum of exp(pred - max) per pixel -- what acr_segloss_bwd takes.
 * acr_segloss_bwd: d_logits (B, K, h, w), WRITTEN:
 *     d_logits[b,k,y,x] = sum_pixels bilinear_weight * ( coef(pixel) * (p_k - [k == label]) + p_k * (d_probs_k - sum_j p_j d_probs_j) )
 *   coef = (g[0] + g[1]) / n_bg for label 0, (g[0] + g[2]) / n_fg for 1 <= label < K, 0 for an ignored pixel (each / B under
 *   batch_average); g (3) fp32 ON THE DEVICE: the gradients of { celoss, bg, fg }.  An ignored pixel contributes exactly 0, so a
 *   count of 0 puts no Inf or NaN into d_logits.  d_probs (B, K, W, H) nullable (the energy term's gradient enters there) and
 *   then requires the probs the forward wrote.  A gather per low-resolution logit in a fixed order: bit-identical run to run.
 * ws: acr_segloss_ws_bytes(...) bytes on the device, 8-byte aligned, contents arbitrary; the backward uses it only with d_probs.
 * acr_segloss_ws_bytes: host only; negative for arguments outside the supported range.
 * All sums over pixels run in double in a fixed order (no float atomics); counts are integers.
 *
 * Dense energy on the lattice (the --densecrfloss / --rloss-scale / --sigma-rgb / --sigma-xy flags of infer_cam.py:58-65).  The
 * reference passes its DenseEnergyLosslayer in as an argument and does not contain the class -- only its filter,
 * bilateralfilter_batch (wrapper/bilateralfilter/bilateralfilter.cpp:42-55) -- so THE DEFINITION IS THIS PROJECT'S OWN.  For image
 * b with probabilities S (K, n), roi (n) in [0, 1] and F_b the bilateral lattice filter of acr_lattice_filter on the features
 * (x / sigma_xy, y / sigma_xy, rgb / sigma_rgb) (bilateralfilter.cpp:4-20):
 *     AS = roi * F_b[roi * S],   E = -(weight / B) * sum_b sum_k sum_i S[k,i] * AS[k,i],   dE/dS := -(2 * weight / B) * AS
 *   The gradient treats the filter as symmetric, as the regularised-loss layer does; it is a definition, not a derivative of the
 *   lattice's arithmetic.
 * acr_dense_energy_dot: out[0] = sum_i s[i] * as[i] over count = K * n values (products and sum in double, fixed order, one
 *   rounding to fp32); grad (count), nullable: grad[i] = grad_scale * as[i].  ws: ACR_DENSE_ENERGY_WS_BYTES on the device,
 *   8-byte aligned.
 * The entry points allocate nothing and do not synchronise; they capture into a hipGraph. */
#define ACR_DENSE_ENERGY_WS_BYTES 2048
#define ACR_SEG_MAX_K 128              /* 2 <= K <= 128: the logits acr_segloss_* train on and acr_segpred_f32 predicts from */
int64_t acr_segloss_ws_bytes(int32_t B, int32_t K, int32_t h, int32_t w, int32_t W, int32_t H);
int acr_segloss_fwd(const float* logits, const uint8_t* label, int32_t B, int32_t K, int32_t h, int32_t w, int32_t W, int32_t H,
                    int32_t batch_average, void* ws, int64_t ws_bytes, float* probs, float* rowstat, float* sums, int64_t* counts,
                    float* loss, void* stream);
int acr_segloss_bwd(const float* logits, const uint8_t* label, const float* rowstat, const int64_t* counts, const float* g,
                    const float* probs, const float* d_probs, int32_t B, int32_t K, int32_t h, int32_t w, int32_t W, int32_t H,
                    int32_t batch_average, void* ws, int64_t ws_bytes, float* d_logits, void* stream);
int acr_dense_energy_dot(const float* s, const float* as, int64_t count, float grad_scale, float* grad, void* ws, int64_t ws_bytes,
                         float* out, void* stream);

/* ---- DPT decoder (ACR(..., seg=True), DPT/ACR.py:51,78-85: the fusion blocks DPT/blocks.py:277-413 and the head
 * DPT/DPT.py:376-383): BatchNorm2d, the x2 bilinear upsampling and the leading ReLU of a residual unit ----
 * All tensors fp32, NCHW, contiguous, 16-byte aligned bases; HW = H * W; n = N * HW values per channel, n < 2^31.
 * acr_bn2d_fwd (nn.BatchNorm2d of blocks.py:312-338):
 *   training != 0: per channel mu = mean over N, H, W and the biased variance var = mean (x - mu)^2, accumulated in double as
 *     a shifted sum (the shift is the channel's first value), so a large mean costs no digits; n >= 2 or ACR_ERR_INVALID, as
 *     torch refuses one value per channel.  running_mean / running_var (C, nullable together) are UPDATED in place:
 *       running_mean = (1 - momentum) * running_mean + momentum * mu
 *       running_var  = (1 - momentum) * running_var  + momentum * var * n / (n - 1)        (the unbiased variance)
 *   training == 0: mu = running_mean, var = running_var (required); nothing is updated.
 *   invstd = 1 / sqrt(var + eps);   y = act( gamma * (x - mu) * invstd + beta [+ resid] [+ resid2] )
 *   act = ReLU for relu != 0, else the identity.  resid is the residual unit's `out + x` (blocks.py:343), resid2 the fusion
 *   block's `output + res` (:402); both nullable, resid2 only with resid.  The expression is evaluated in double per value and
 *   rounded to fp32 once.  stats (C, 2) double, WRITTEN: mu and invstd -- what acr_bn2d_bwd takes.
 * acr_bn2d_bwd: with g = dy where the saved output y > 0 (relu != 0; y is then required) and g = dy otherwise,
 *   xhat = (x - mu) * invstd:
 *       dbeta = sum g,   dgamma = sum g * xhat                                             (each nullable)
 *       dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat))      training != 0
 *       dx = gamma * invstd * g                                          training == 0 (the statistics are constants)
 *   dres (nullable, only with relu != 0): g, the gradient of either addend; without a fused ReLU that gradient is dy itself
 *   and nothing is written.  dx nullable.
 * ws: acr_bn2d_ws_bytes(N, C, HW) bytes on the device, 8-byte aligned, contents arbitrary (host only; negative for arguments
 *   outside the supported range).  Every sum runs in double in a fixed order (thread, LDS tree, slabs ascending): no float
 *   atomics, bit-identical run to run.  Nothing outside a plane is read or written.
 * acr_relu_fwd_f32 / acr_relu_bwd_f32: y = max(x, 0) over n values (the `activation(x)` of blocks.py:330; the raw x stays with
 *   the caller for the skip, :343) and dx = dy where y > 0, else 0.
 * acr_upsample2x_fwd (F.interpolate(scale_factor=2, mode="bilinear", align_corners=True), blocks.py:407-409 and the head's
 *   Interpolate): x (planes, H, W) -> y (planes, OH, OW), y 8-byte aligned.  Only OH = 2 H and OW = 2 W are built: anything else
 *   returns ACR_ERR_UNSUPPORTED.  Per axis, in fp32 (torch's rule, aten/src/ATen/native/UpSample.h):
 *       scale = (in - 1) / (out - 1)  (0 when out == 1),  src = scale * dst,  i0 = min((int)src, in - 1),
 *       lambda = src - i0,  i1 = i0 + (i0 < in - 1),  value = (1 - lambda) * v[i0] + lambda * v[i1]
 *   rows outside, columns inside: y = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11).
 * acr_upsample2x_bwd: dx (planes, H, W), WRITTEN: the adjoint, as a gather per input pixel over exactly the output rows and
 *   columns whose first tap is i - 1 or i (found with the forward's own fp32 index function), summed in ascending order in
 *   double: bit-identical run to run.
 * Cross-rank statistics (nn.SyncBatchNorm: every rank normalises with the statistics of all ranks' values).  Each direction is
 *   two entry points with the CALLER'S exchange between them; what is exchanged is a fixed-size double tensor per layer --
 *   (C, 3) forward, (C, 2) backward -- gathered into W rows in rank order, so the merge order is this library's, the same on
 *   every rank whatever the collective's algorithm, and every rank computes the same bits.  Ranks may hold different N >= 1 (an empty
 *   shard is refused like any N < 1); H * W is the same on all.  No pass over a tensor is added: forward x twice, backward x, y, dy twice, as the fused entry points.
 * acr_bn2d_moments: moments (C, 3) double, WRITTEN: count n = N * HW, mean, M2 = sum (x - mean)^2 of the local tensor, from the
 *   shifted slab sums a = sum d, b = sum d^2: mean = shift + a / n, M2 = max(b - a^2 / n, 0).  n = 1 is legal (M2 = 0).
 * acr_bn2d_fwd_merged: gathered (W, C, 3) double, the moments of ranks 0 .. W - 1.  Per channel they are merged in ascending
 *   rank order by the pairwise update, the only formula used (no difference of sums of squares):
 *       n = n_a + n_b,  delta = mean_b - mean_a,  mean = mean_a + delta * n_b / n,  M2 = M2_a + M2_b + delta^2 * n_a * n_b / n
 *   var = M2 / n; the running statistics are updated as acr_bn2d_fwd updates them, with the merged mean and M2 / (n - 1); y as
 *   acr_bn2d_fwd.  A merged count below 2 returns ACR_ERR_INVALID -- decided on the host from its lower bound N * HW +
 *   (W - 1) * HW (every rank holds at least one plane), nothing is read back.  stats, 3 C doubles, WRITTEN: (C, 2) mu and invstd
 *   as acr_bn2d_fwd writes them, then the C merged counts.  1 <= W <= 65536.
 * acr_bn2d_bwd_sums: stats as acr_bn2d_fwd_merged wrote it.  sums (C, 2) double, WRITTEN: sum g and sum g * xhat of the LOCAL
 *   tensor under the merged mu / invstd.  dgamma / dbeta (each nullable) are these local sums: the caller averages parameter
 *   gradients over the ranks afterwards, as it does for every other parameter.
 * acr_bn2d_bwd_merged: gathered_sums (W, C, 2) double.  The rows are added in ascending rank order and divided by the merged
 *   count: mean(g), mean(g * xhat) over all ranks; dx and dres as acr_bn2d_bwd with training != 0.
 * The entry points allocate nothing, launch on `stream` and read nothing back; they capture into a hipGraph. */
int64_t acr_bn2d_ws_bytes(int32_t N, int32_t C, int32_t HW);
int acr_bn2d_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, const float* resid,
                 const float* resid2, int32_t N, int32_t C, int32_t HW, int32_t training, double eps, double momentum, int32_t relu,
                 void* ws, int64_t ws_bytes, double* stats, float* y, void* stream);
int acr_bn2d_bwd(const float* x, const float* y, const float* dy, const float* gamma, const double* stats, int32_t N, int32_t C,
                 int32_t HW, int32_t training, int32_t relu, void* ws, int64_t ws_bytes, float* dx, float* dgamma, float* dbeta,
                 float* dres, void* stream);
int acr_bn2d_moments(const float* x, int32_t N, int32_t C, int32_t HW, void* ws, int64_t ws_bytes, double* moments, void* stream);
int acr_bn2d_fwd_merged(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                        const float* resid, const float* resid2, int32_t N, int32_t C, int32_t HW, const double* gathered, int32_t W,
                        double eps, double momentum, int32_t relu, void* ws, int64_t ws_bytes, double* stats, float* y, void* stream);
int acr_bn2d_bwd_sums(const float* x, const float* y, const float* dy, const double* stats, int32_t N, int32_t C, int32_t HW,
                      int32_t relu, void* ws, int64_t ws_bytes, double* sums, float* dgamma, float* dbeta, void* stream);
int acr_bn2d_bwd_merged(const float* x, const float* y, const float* dy, const float* gamma, const double* stats,
                        const double* gathered_sums, int32_t W, int32_t N, int32_t C, int32_t HW, int32_t relu, void* ws,
                        int64_t ws_bytes, float* dx, float* dres, void* stream);
int acr_relu_fwd_f32(const float* x, int64_t n, float* y, void* stream);
int acr_relu_bwd_f32(const float* y, const float* dy, int64_t n, float* dx, void* stream);
int acr_upsample2x_fwd(const float* x, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, float* y, void* stream);
int acr_upsample2x_bwd(const float* dy, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, float* dx, void* stream);

/* ---- the same ten entry points on bf16 STORAGE (the decoder under math "bf16") ----
 * The argument lists are the fp32 ones; x, y, resid, resid2, dy, dx, dres, gamma and beta are bf16 (spelled void*, as every bf16
 * pointer of this header), running_mean / running_var / dgamma / dbeta stay float, stats / moments / gathered / sums /
 * gathered_sums stay double, ws is sized by acr_bn2d_ws_bytes.  Bases 16-byte aligned as above (acr_upsample2x_fwd_bf16: y
 * 4-byte aligned); any HW >= 1.
 * Definition.  A bf16 input stands for its exact fp32 value.  Every bf16 output is the fp32 value that the fp32 entry point of
 * the same name defines for those inputs, rounded to bf16 by round-to-nearest-even.  That fp32 value is the double expression
 * rounded to fp32 once, so the chain is double -> fp32 -> bf16, deliberately: the fp32 entry point on the upcast inputs is the
 * yardstick, y_bf16 == bf16(y_fp32) at every element.  Every float and double output is defined exactly as for fp32.
 * The kernels are the fp32 kernels instantiated on the storage type with the SAME assignment of values to lanes (a lane takes 4
 * consecutive values: 8-byte loads here, 16-byte there), so every double sum adds the same numbers in the same order and
 * stats, moments, sums, dgamma, dbeta and the running statistics equal the fp32 entry point's bit for bit.
 * The ReLU mask of the backward is y > 0 on the STORED bf16 y; it equals the fp32 mask, because a positive normal fp32 never
 * rounds to a bf16 zero (the two formats share the exponent range).  dres is the masked dy, a copy of bf16 values.
 * As above: all sums in double in a fixed order (thread, LDS tree, slabs ascending), no float atomics, bit-identical run to run,
 * nothing outside a plane read or written, nothing allocated or read back, capturable; the same error codes (n < 2 in training
 * mode, a merged count < 2: ACR_ERR_INVALID; OH != 2 H or OW != 2 W: ACR_ERR_UNSUPPORTED). */
int acr_bn2d_fwd_bf16(const void* x, const void* gamma, const void* beta, float* running_mean, float* running_var, const void* resid,
                      const void* resid2, int32_t N, int32_t C, int32_t HW, int32_t training, double eps, double momentum, int32_t relu,
                      void* ws, int64_t ws_bytes, double* stats, void* y, void* stream);
int acr_bn2d_bwd_bf16(const void* x, const void* y, const void* dy, const void* gamma, const double* stats, int32_t N, int32_t C,
                      int32_t HW, int32_t training, int32_t relu, void* ws, int64_t ws_bytes, void* dx, float* dgamma, float* dbeta,
                      void* dres, void* stream);
int acr_bn2d_moments_bf16(const void* x, int32_t N, int32_t C, int32_t HW, void* ws, int64_t ws_bytes, double* moments, void* stream);
int acr_bn2d_fwd_merged_bf16(const void* x, const void* gamma, const void* beta, float* running_mean, float* running_var,
                             const void* resid, const void* resid2, int32_t N, int32_t C, int32_t HW, const double* gathered, int32_t W,
                             double eps, double momentum, int32_t relu, void* ws, int64_t ws_bytes, double* stats, void* y,
                             void* stream);
int acr_bn2d_bwd_sums_bf16(const void* x, const void* y, const void* dy, const double* stats, int32_t N, int32_t C, int32_t HW,
                           int32_t relu, void* ws, int64_t ws_bytes, double* sums, float* dgamma, float* dbeta, void* stream);
int acr_bn2d_bwd_merged_bf16(const void* x, const void* y, const void* dy, const void* gamma, const double* stats,
                             const double* gathered_sums, int32_t W, int32_t N, int32_t C, int32_t HW, int32_t relu, void* ws,
                             int64_t ws_bytes, void* dx, void* dres, void* stream);
int acr_relu_fwd_bf16(const void* x, int64_t n, void* y, void* stream);
int acr_relu_bwd_bf16(const void* y, const void* dy, int64_t n, void* dx, void* stream);
int acr_upsample2x_fwd_bf16(const void* x, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, void* y, void* stream);
int acr_upsample2x_bwd_bf16(const void* dy, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, void* dx, void* stream);

/* ---- read-out reassembly of the plain ViT backbones under seg=True (vitb, deit, deit_distilled, vitl) ----
 * The read-out of tap i (DPT/vit.py:263-341, run by forward_vit :117-146; start_index = 2 for the distilled DeiT, :617-632) is
 * Slice(start) -> Transpose -> Unflatten -> Conv2d(D, f, 1) -> ConvTranspose2d(f, f, s, stride = s) (s = 4, 2; tap 3 has none:
 * s = 1).  With kernel == stride no two outputs overlap: the transposed convolution is the product
 *   y2 (B T, C s^2) = z (B T, C) . Wt.view(C, C s^2)          (acr_gemm_f32 'nn', the weight (ci, co, s, s) as stored)
 * on ALL tokens, followed by what these entry points replace -- :117-146's slice / transpose / unflatten and the scatter of
 * nn.ConvTranspose2d with its bias:
 * acr_reassemble_fwd:  out[b][co][i s + di][j s + dj] = y[(b T + start + i gw + j) ldy + (co s + di) s + dj] (+ bias[co]),
 *   0 <= i < gh, 0 <= j < gw; one fp32 add per element (none for bias == NULL: a copy).  out (B, C, gh s, gw s) contiguous.
 * acr_reassemble_bwd (their autograd backward): dy[(b T + start + i gw + j) lddy + (co s + di) s + dj] = dout[b][co][i s + di][j s + dj];
 *   the `start` skipped rows of every sample are WRITTEN with zeros in columns < C s^2; columns >= C s^2 of any row are not
 *   touched.  dbias (C, nullable) = sum_b sum_pixels dout[b][co]: every tile's sum in a fixed order in fp32, the tiles of a
 *   channel in a fixed order in double, rounded once; no atomics, bit-identical run to run.  dbias needs ws:
 *   acr_reassemble_ws_bytes(B, gh, gw, C, s) bytes on the device, 4-byte aligned, contents arbitrary (0 for arguments outside
 *   the contract).
 * Contract: s in {1, 2, 4}; T == start + gh gw; 0 <= start <= 8; ldy, lddy >= C s^2 (any value: no alignment is assumed); B, C, gh,
 *   gw any positive value with gh gw < 2^26, C s^2 < 2^30 and fewer than 2^31 tiles (a tile: 64 columns of y by 32 grid columns of
 *   one grid row; s = 1: by 64 grid positions).  Anything else returns ACR_ERR_INVALID and launches nothing.
 * Both directions move contiguous runs on both sides through an LDS tile (csrc/reassemble.hip); edge tiles are masked per element,
 * nothing outside the tensors is addressed.  The entry points allocate nothing and do not synchronise; they capture into a hipGraph. */
size_t acr_reassemble_ws_bytes(int32_t B, int32_t gh, int32_t gw, int32_t C, int32_t s);
int acr_reassemble_fwd(const float* y, int64_t ldy, const float* bias, int32_t B, int32_t T, int32_t start, int32_t gh, int32_t gw,
                       int32_t C, int32_t s, float* out, void* stream);
int acr_reassemble_bwd(const float* dout, int32_t B, int32_t T, int32_t start, int32_t gh, int32_t gw, int32_t C, int32_t s, float* dy,
                       int64_t lddy, float* dbias, void* ws, int64_t ws_bytes, void* stream);

/* ---- segmentation prediction (myTool.py:1826-1895 validation: the resize of the logits to the image's own size :1881, the softmax
 * :1883 and the argmax :1891, or the probabilities _crf_with_alpha_2 :1819-1823 hands to the CRF) in one pass ----
 * logits (B, K, h, w) fp32 contiguous; label (B, H, W) uint8, nullable; probs (B, K, H, W) fp32, nullable; at least one output.
 * Requires 1 <= B <= 65535, 2 <= K <= 128, h, w, H, W >= 1, K * h * w < 2^31, K * H * W < 2^31; anything else returns
 * ACR_ERR_INVALID.  Inputs are finite: NaN is outside the contract.
 * Interpolation: per output pixel (Y, X), v_k = the bilinear interpolation of plane k by torch's align_corners=False rule in fp32
 *   (the rule of acr_bilinear_resize and acr_segloss_fwd), for any h, w, H, W -- enlarging, shrinking, the identity, h = w = 1.
 *   Per axis (aten/src/ATen/native/UpSample.h), computed once per pixel and used for all K planes:
 *       scale = in / out,  src = max(scale * (dst + 0.5) - 0.5, 0),  i0 = min((int)src, in - 1),
 *       lambda = src - i0,  i1 = i0 + (i0 < in - 1)
 *   rows outside, columns inside, with hy = 1 - ly, hx = 1 - lx and no fused multiply-add:
 *       v = hy * (hx * p[y0][x0] + lx * p[y0][x1]) + ly * (hx * p[y1][x0] + lx * p[y1][x1])
 * Flip: hflip != 0 says the pass ran on the mirrored image: columns x0, x1 are read at w - 1 - x0, w - 1 - x1 with the same
 *   weights, so the result equals, bit for bit, that of hflip = 0 on the logits flipped along w.
 * Softmax: m = max_k v_k;  p_k = exp(v_k - m) / sum_j exp(v_j - m), in fp32, the sum in ascending j.
 * accumulate == 0: probs, if given, is WRITTEN with p; label, if given, is the smallest k among the maxima of v (the argmax of the
 *   logits, :1891; the first-maximum convention of acr_pseudo_label_f32).
 * accumulate != 0 (probs required): probs += p, one fp32 add per value; label, if given, is the smallest k among the maxima of the
 *   UPDATED probs -- test-time augmentation over scales and flips: the last pass leaves the final label map, with no extra launch.
 * No atomics, a fixed order, nothing outside the tensors is read or written: bit-identical run to run.  The entry point allocates
 * nothing and does not synchronise; it captures into a hipGraph. */
int acr_segpred_f32(const float* logits, int32_t B, int32_t K, int32_t h, int32_t w, int32_t H, int32_t W, int32_t hflip,
                    int32_t accumulate, float* probs, uint8_t* label, void* stream);

/* ---- training-time CAM targets (compute_cam_up, myTool.py:860-864: the patch CAMs of forward_cam upsampled to the crop and
 * multiplied by the image-level label; with normalize, the two-view sum and min-max normalisation infer_cam.py:156-162, 201-202
 * applies to patch CAMs) -- the (B, C, oh, ow) tensor acr_sal_pseudo_compose takes as `cams`, made while training runs ----
 * cam1 fp32 patch CAMs of view 1, token-major (B, gh * gw, C): element (b, t, c) lies at cam1[b * batch_stride + t * tok_stride +
 *   c] (strides in elements, >= 0; the class stride is 1), so a slice of a (B, T, C) tensor that skips the class / distillation
 *   tokens is passed as it lies.  cam2, nullable: the CAMs of the H-FLIPPED view, same geometry and strides.  label (B, C) fp32
 *   contiguous: the multipliers.  out (B, C, oh, ow) fp32 contiguous; every element is WRITTEN exactly once.
 * Rule, all in fp32, the operations and their order as written (the build has -ffp-contract=off):
 *   up(src)[y, x]: torch's upsample_bilinear2d with align_corners=False, the rule of acr_bilinear_resize (csrc/acr_resample.h:
 *     scale = in / out, src = max(scale * (dst + 0.5) - 0.5, 0), i0 = min((int)src, in - 1), lambda = src - i0, i1 = i0 + (i0 < in - 1),
 *     v = hy * (hx * p[y0][x0] + lx * p[y0][x1]) + ly * (hx * p[y1][x0] + lx * p[y1][x1])) for any gh, gw, oh, ow >= 1;
 *   l = label[b][c];
 *   s[y, x] = up(cam1)[y, x] * l                                       without cam2,
 *   s[y, x] = up(cam1)[y, x] * l + up(cam2)[y, ow - 1 - x] * l         with cam2: view 2 enters at the mirrored OUTPUT column, as
 *     acr_bilinear_resize's hflip + accumulate does it (np.flip of the upsampled map, infer_cam.py:159-160) -- not at mirrored
 *     taps, which differ in the last bit;
 *   normalize == 0: out = s (compute_cam_up for the whole batch);
 *   normalize == 1: out = (s - mn) / ((mx - mn) + eps), mn and mx the minimum and maximum of s over the UPSAMPLED plane
 *     (infer_cam.py:202), not of the source: with half-pixel sampling an enlargement never hits an interior texel centre, so the
 *     plane's maximum lies below the source's.  min / max are exact in any order: the result does not depend on the launch geometry.
 *   A plane with l == 0 is written as +0 WITHOUT READING ITS SOURCE -- the one deviation from v * 0, which a non-finite source
 *   value would turn into NaN (and the normalisation of a plane of zeros gives 0 / eps = +0 anyway).
 * Requires B, C, gh, gw, oh, ow >= 1, B * C <= 2^22, gh * gw < 2^31, oh * ow < 2^31, eps > 0, normalize 0 or 1; anything else
 *   returns ACR_ERR_INVALID and launches nothing.  Present planes hold finite values (NaN is outside the contract).
 * ws: acr_train_cam_ws_bytes(B, C, oh, ow) bytes on the device, 4-byte aligned, contents arbitrary; used (and required) with
 *   normalize == 1 only.  acr_train_cam_ws_bytes: host only; negative for arguments outside the supported range.
 * 16-byte stores where ow is a multiple of 4 and out is 16-byte aligned, 4-byte stores otherwise.  No atomics, nothing outside the
 * tensors is read or written: bit-identical run to run.  The entry point allocates nothing and does not synchronise; it captures
 * into a hipGraph. */
int64_t acr_train_cam_ws_bytes(int32_t B, int32_t C, int32_t oh, int32_t ow);
int acr_train_cam_f32(const float* cam1, const float* cam2, int64_t tok_stride, int64_t batch_stride, const float* label, int32_t B,
                      int32_t C, int32_t gh, int32_t gw, int32_t oh, int32_t ow, float eps, int32_t normalize, void* ws,
                      int64_t ws_bytes, float* out, void* stream);

/* ---- affinity stage (PSA, Ahn & Kwak CVPR 2018): pair labels (tool/torchutils.py:107-157 ExtractAffinityLabelInRadius, fed by
 * AffinityFromMaskDataset :159-173 and voc12/data.py:222-278 VOC12AffDataset), pair geometry (tool/pyutils.py:125-159
 * get_indices_of_pairs), and -- this project's own statement of PSA's definitions, which the reference expects around them -- the
 * pair affinity, its loss with gradient, and the random walk ----
 * Geometry: radius R (2..5; the reference's default 5), r = R - 1.  Offsets (dy, dx) in the reference's order: (0, x) for
 *   x = 1 .. r, then for y = 1 .. r, x = -r .. r: (y, x) where x^2 + y^2 < R^2; P = acr_aff_pairs(R) of them (34 for R = 5; -1 for
 *   a radius outside 2..5; host only).  On an h x w grid the from-pixels are rows [0, h - r) and columns [r, w - r):
 *   N = (h - r)(w - 2 r); from-index n = yy (w - 2 r) + xx is pixel (yy, r + xx), its partner under offset p is
 *   (yy + dy, r + xx + dx) -- flat index to = from + dy w + dx.  Requires h > r, w > 2 r, h, w <= 4096, 1 <= B <= 65535;
 *   anything else returns ACR_ERR_INVALID and launches nothing.
 * acr_aff_pair_codes: label_map (B, S0, S1) uint8 on the device: class ids, 255 = ignore.  The grid is the map subsampled by
 *   `stride` -- g[y][x] = map[stride y][stride x], h = S0 / stride, w = S1 / stride; this rule IS the definition of the
 *   reference's RescaleNearest(0.125) here (stride 8); S0 and S1 must be multiples of stride; stride 1 takes a grid-sized map.
 *   The subsampled map never exists.  With lf = g(from), lt = g(to), codes (B, P, N) uint8, WRITTEN:
 *       1  bg-pos  lf == lt == 0
 *       2  fg-pos  lf == lt, lf != 0, both < 255
 *       3  neg     lf != lt, both < 255
 *       0  none    otherwise
 *   so that (codes == k) are the three float masks of ExtractAffinityLabelInRadius.  counts int64[3] on the device, WRITTEN
 *   (cleared on the stream first): the batch totals of codes 1, 2, 3 -- 64-bit integer atomics, exact in any order.
 * acr_aff_loss_fwd: feat (B, C, h, w) fp32 contiguous.  With eps = 1e-5:
 *       d[b,p,n] = (1 / C) sum_c |feat[b,c,from] - feat[b,c,to]|,   aff = exp(-d)
 *       bg  = sum_{code 1} -log(aff + eps)     / (counts[0] + eps)
 *       fg  = sum_{code 2} -log(aff + eps)     / (counts[1] + eps)
 *       neg = sum_{code 3} -log(1 + eps - aff) / (counts[2] + eps)
 *       loss = bg / 4 + fg / 4 + neg / 2
 *   the counts those of the whole batch, as acr_aff_pair_codes left them on the device.  aff (B, P, N) fp32, nullable, WRITTEN;
 *   g (B, P, N) fp32, WRITTEN: d loss / d d -- (1/4) aff / (aff + eps) / (counts[k-1] + eps) for codes k = 1, 2,
 *   -(1/2) aff / (1 + eps - aff) / (counts[2] + eps) for code 3, 0 for code 0; loss4 = (loss, bg, fg, neg) fp32, WRITTEN.  A term
 *   without a pair is exactly 0.  codes == NULL is the inference forward: only aff is written (counts, g, ws, loss4 unused).
 *   Every value is evaluated in double -- the differences, the channel sum (channels ascending), exp, log -- and rounded to
 *   fp32 once; the three sums are double: a thread's pairs in offset order, the LDS tree of its 16 x 16 tile, the tiles
 *   ascending.  ws: acr_aff_loss_ws_bytes(B, h, w, R) bytes on the device, 8-byte aligned, contents arbitrary (host only;
 *   negative for arguments outside the contract).  1 <= C <= 2^20.
 * acr_aff_loss_bwd: dfeat (B, C, h, w), WRITTEN (every element) = gscale[0] * d loss / d feat, gscale one fp32 value on the
 *   device (the upstream gradient).  Gather form, no atomics: a pixel sums, offsets ascending, g * sign(f_me - f_partner) / C
 *   over the pairs it starts (partner at +offset) and the pairs that end in it (partner at -offset, where that pixel is a
 *   from-pixel), in double; sign(0) = 0, as torch's abs has it.
 *   Both directions stage 8 channels of a 16 x 16 tile's rows and columns (with the halo of r) in LDS per round and keep the P
 *   (forward) or 2 P (backward) per-pixel values in registers; nothing with a C x P extent exists.
 * acr_aff_walk_weights: the symmetric A has A[i][j] = A[j][i] = aff^beta for every listed pair (i, j), A[i][i] = 1, 0 otherwise;
 *   T[i][j] = A[i][j] / sum_k A[k][j].  wt (B, 2 P + 1, h w) fp32, WRITTEN: for pixel j tap 0 = T[j][j], tap 1 + 2 p = T[i][j]
 *   with i = j + offset p (the pair j starts), tap 2 + 2 p = T[i][j] with i = j - offset p (the pair that ends in j); 0 where
 *   there is no such pair.  pow, the column sum (1, then the taps ascending) and the division in double.  beta > 0.
 * acr_aff_walk: scores (B, K, h, w) fp32 -> out = scores . T^steps (out is not scores), as `steps` gathers
 *       new[j] = sum_t wt[t][j] * old[i_t(j)]          (taps ascending, in double, rounded to fp32 once per step)
 *   the K planes of an image independent under its T.  resident = 1: one launch, one workgroup per (image, plane), the plane
 *   ping-ponged in LDS -- needs acr_aff_walk_resident(h, w, R) == 1 (two planes of h w + 2 (r w + r) floats within 64 KiB; host
 *   only); resident = 0: one launch per step on planes in ws through the same step function -- the two forms agree bit for
 *   bit; resident = -1 chooses, and chooses the stepwise form: it spreads every plane over all CUs and was the faster one at
 *   every plane count measured, the resident form runs on request.  ws (used by the stepwise form only):
 *   acr_aff_walk_ws_bytes(B, K, h, w, R) bytes on the device, 4-byte aligned, cleared here on the stream (host only; negative
 *   for arguments outside the contract).  B * K <= 65535, 0 <= steps <= 2^20; steps = 0 copies.  Scores are finite: a tap of
 *   weight 0 is multiplied, not skipped.
 * No float atomics, fixed orders, nothing outside the tensors is read or written: bit-identical run to run, and a sample's result
 * does not depend on its batch.  The entry points allocate nothing and do not synchronise; they capture into a hipGraph. */
int32_t acr_aff_pairs(int32_t R);
int acr_aff_pair_codes(const uint8_t* label_map, int32_t B, int32_t S0, int32_t S1, int32_t stride, int32_t R, uint8_t* codes,
                       int64_t* counts, void* stream);
int64_t acr_aff_loss_ws_bytes(int32_t B, int32_t h, int32_t w, int32_t R);
int acr_aff_loss_fwd(const float* feat, int32_t B, int32_t C, int32_t h, int32_t w, int32_t R, const uint8_t* codes,
                     const int64_t* counts, float* aff, float* g, void* ws, int64_t ws_bytes, float* loss4, void* stream);
int acr_aff_loss_bwd(const float* feat, const float* g, const float* gscale, int32_t B, int32_t C, int32_t h, int32_t w, int32_t R,
                     float* dfeat, void* stream);
int acr_aff_walk_weights(const float* aff, int32_t B, int32_t h, int32_t w, int32_t R, double beta, float* wt, void* stream);
int32_t acr_aff_walk_resident(int32_t h, int32_t w, int32_t R);
int64_t acr_aff_walk_ws_bytes(int32_t B, int32_t K, int32_t h, int32_t w, int32_t R);
int acr_aff_walk(const float* wt, const float* scores, float* out, int32_t B, int32_t K, int32_t h, int32_t w, int32_t R,
                 int32_t steps, int32_t resident, void* ws, int64_t ws_bytes, void* stream);

/* ---- affinity-stage input (voc12/data.py:241-278 VOC12AffDataset.__getitem__ under PSA's transforms: the joint RandomCrop(S) --
 * tool/imutils.py:167-190 get_random_crop_box, :201-225 random_crop -- and RandomHorizontalFlip :239-246, then AvgPool2d(8)
 * :228-236 on the scores): the label grid the pair masks are cut from, out of the two CRF score dumps ----
 * Per image, with n planes per dump (n_planes[b], 2..81; plane 0 the background, then class + 1 in the dicts' own key order):
 *   1. stack    the n low-alpha planes, then the n high-alpha planes: 2 n planes of (h, w) fp32.
 *   2. crop     into a zero container of SH x SW: container pixel (y, x) is "inside" when cont_top <= y < cont_top + ch and
 *               cont_left <= x < cont_left + cw, and then holds pixel (ry, rx) = (img_top + y - cont_top, img_left + x - cont_left)
 *               of the FLIPPED planes, i.e. column w - 1 - rx of the stored ones when flip is set; every other pixel is 0.  This is
 *               the acr_pre_image record's own meaning (flip, then crop) with rh = h and rw = w: no resize.  The reference crops and
 *               then flips the container (np.fliplr); that equals this form with the box mirrored, cont_left' = S - cont_left - cw
 *               and img_left' = w - img_left - cw, which is what the caller writes into the record when it draws a flip.
 *   3. pool     the mean over each 8 x 8 block of the container, per plane: the exact sum of the 64 values times 1 / 64, rounded to
 *               fp32 once.  Summed in double in a fixed order: a column's rows ascending, then the 8 columns by a butterfly (xor 1,
 *               2, 4).  For values that are 0 or in [2^-20, 1] that sum is exact in any order.
 *   4. no score where the maximum over all 2 n pooled planes < 1e-5f, compared in fp32.
 *   5. argmax   la over the first n pooled planes, ha over the last n; the first maximum wins; a plane INDEX 0 .. n - 1, not a class
 *               id (the pair masks test only equality, 0 and 255).  Scores are finite.
 *   6. label    = la; 255 where la == 0; then 0 where ha == 0; then 255 where there is no score (data.py:268-275).
 * label_u8 (batch, SH / 8, SW / 8) uint8, WRITTEN, every element: the grid ExtractAffinityLabelInRadius(cropsize // 8) takes, i.e.
 * acr_aff_pair_codes' label_map at stride 1.
 * scores: one device buffer; image b's low-alpha stack, n_planes[b] contiguous (h, w) fp32 planes, starts at BYTE offset la_off[b],
 * its high-alpha stack at ha_off[b] (both multiples of 4).  table: `batch` acr_pre_image records on the device, unchanged (their
 * offset field is not read); la_off, ha_off (int64) and n_planes (int32): device arrays of `batch` entries.  SH and SW are separate
 * so that a whole uncropped image is the record cont = img = (0, 0), ch = h, cw = w in a container of its size rounded up to
 * multiples of 8: the zero padding of skimage's block_reduce.
 * One launch per batch.  Every score element inside the crop box is read exactly once, in wave-wide runs of 256 contiguous bytes
 * along x (4-byte loads: an image row starts at any 4-byte boundary); nothing outside the box is addressed.  The kernel trusts the
 * table and the offsets: the caller validates them.  Contract: 1 <= batch <= 65535, SH and SW multiples of 8 up to 32768; anything
 * else returns ACR_ERR_INVALID and launches nothing.  No atomics, no workspace, plain stores: bit-identical run to run.  The entry
 * point allocates nothing and does not synchronise; it captures into a hipGraph. */
int acr_aff_label_batch(const void* scores, const void* table, const int64_t* la_off, const int64_t* ha_off, const int32_t* n_planes,
                        int32_t batch, int32_t SH, int32_t SW, uint8_t* label_u8, void* stream);

/* ---- colour jitter (the affinity stage reads VOC12AffDataset, voc12/data.py:241-278, through PSA's transform list, which begins
 * with torchvision's ColorJitter(brightness=0.3, contrast=0.3, saturation=0.3, hue=0.1) on the PIL image, before np.asarray,
 * Normalize and the joint crop) ----
 * torchvision's ColorJitter on a PIL image is Pillow's ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color and an
 * HSV round trip: uint8 in, uint8 out, so the result is defined bit for bit.  Images are (h, w, 3) uint8 RGB.  Every operation
 * below is of the type written, with no contraction and IEEE division.
 *   gray(r, g, b) = (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16, in integers.
 *   blend(deg, img, a), a an fp32 value:  t = (float)deg + a * (float)(img - deg) -- an fp32 product, then an fp32 sum; img - deg is
 *     formed as an int.  For 0 <= a <= 1: out = (uint8)(int)t.  Otherwise: out = 0 if t <= 0, 255 if t >= 255, else (uint8)(int)t.
 *     a == 0 gives deg, a == 1 gives img.
 *   brightness(f) = blend(0, img, f) per channel.        saturation(f) = blend(gray(pixel), channel, f).
 *   contrast(f)   = blend(m, channel, f), m = int(sum of gray / (h w) + 0.5) over the WHOLE image as it is when the contrast
 *     operation is reached (operations earlier in the order change m).  The sum is an exact integer and
 *     m = (2 sum + n) / (2 n) in integers, n = h w.
 *   hue(shift): RGB -> HSV, H = (H + shift) mod 256, HSV -> RGB; shift = trunc(hue_factor * 255) mod 256 with the product in double
 *     (-0.05 gives 244).  Always the round trip, also at shift 0: it is lossy.
 *     RGB -> HSV (Pillow's rgb2hsv_row): maxc, minc uint8, V = maxc.  minc == maxc: H = S = 0.  Otherwise cr = (float)(maxc - minc),
 *       s = cr / (float)maxc, rc, gc, bc = (float)(maxc - x) / cr;  h = bc - gc if r == maxc (an fp32 difference), else
 *       h = 2.0 + rc - bc if g == maxc, else h = 4.0 + gc - rc (double literals: double arithmetic); h is stored as float;
 *       h = (float)fmod((double)h / 6.0 + 1.0, 1.0);  H = clip((int)((double)h * 255.0), 0, 255),
 *       S = clip((int)((double)s * 255.0), 0, 255).
 *     HSV -> RGB (hsv2rgb_row): S == 0: r = g = b = V.  Otherwise hf = (double)(float)H * 6.0 / 255.0, i = (float)floor(hf),
 *       f = (float)(hf - (double)i), fs = (float)((double)(float)S / 255.0);  p = round((double)V * (1.0 - (double)fs)),
 *       q = round((double)V * (1.0 - (double)(fs * f))) with fs * f an fp32 product,
 *       t = round((double)V * (1.0 - (double)fs * (1.0 - (double)f))); round is C's (half away from zero), clipped to 0..255;
 *       (r, g, b) by (int)i % 6: 0 (V, t, p), 1 (q, V, p), 2 (p, V, t), 3 (p, q, V), 4 (t, p, V), 5 (V, p, q); H = 255 gives
 *       i = 6, which is case 0.
 *   The jitter applies an image's operations in its own order to the whole image.
 * acr_color_jitter_batch works IN PLACE on packed_u8, the packed uint8 batch acr_preprocess_batch reads: image b is h w 3 bytes
 * at BYTE offset offsets[b], a multiple of 16 (packed_u8 itself 16-byte aligned); the bytes between images are neither read nor
 * written.  Device arrays: offsets (batch) int64; hw (batch, 2) int32 = (h, w), h w >= 1; order (batch, 4) int32 operation codes,
 * executed slot 0 first, ACR_JITTER_NONE = slot unused, no code twice; factors (batch, 3) fp32 indexed by the operation code
 * (brightness, contrast, saturation; an unused one is not read); hue_shift (batch) int32 in 0..255.  The kernels trust these tables:
 * the caller validates them.
 * Two launches for the whole batch, whatever the image sizes: a mean pass (only images whose order names contrast: every pixel
 * through the operations in front of contrast, then gray, then an exact 64-bit integer sum per image, merged from per-workgroup
 * partials in ws) and an apply pass (every pixel through its whole sequence, stored once).  ws: acr_color_jitter_ws_bytes(batch)
 * bytes on the device, 8-byte aligned, contents arbitrary (host only; negative for a batch outside the contract); it may be null
 * when NO order names contrast, and then the mean pass is not launched.  Contract: 1 <= batch <= 65535; anything else returns
 * ACR_ERR_INVALID and launches nothing.  No atomics, integer sums: bit-identical run to run.  The entry point allocates nothing and
 * does not synchronise; it captures into a hipGraph. */
#define ACR_JITTER_NONE -1
#define ACR_JITTER_BRIGHTNESS 0
#define ACR_JITTER_CONTRAST 1
#define ACR_JITTER_SATURATION 2
#define ACR_JITTER_HUE 3
int64_t acr_color_jitter_ws_bytes(int32_t batch);
int acr_color_jitter_batch(uint8_t* packed_u8, const int64_t* offsets, const int32_t* hw, const int32_t* order, const float* factors,
                           const int32_t* hue_shift, int32_t batch, void* ws, void* stream);

/* ---- class-centre feature-distance loss (myTool.py:1616-1710 compute_dis_no_batch with compute_cos: the feature-clustering term
 * of the single-stage recipe) ----
 * seg (B, K, h, w) fp32 logits and feat (B, C, h, w) fp32, both contiguous; N = h w, eps = 1e-7.  The reference hard-codes the
 * classes 1..20; here they are 1..K-1, K = 21 reproduces it.
 *   lab[b,n] = the first index of the maximum of seg[b,:,n], a NaN counting as the maximum (torch.argmax).  The loss is not
 *     differentiable in seg.  n_b = #{n : lab[b,n] = 0} per image, m_i = #{(b,n) : lab[b,n] = i} over the batch, i >= 1.
 *   background centre per image   c_b = sum_{n in bg(b)} f_n / (n_b + eps)   (the zero vector when n_b = 0);
 *   foreground centre over the batch   g_i = sum_{n in i} f_n / (m_i + eps)   for the classes with m_i >= 1: F of them, ordered
 *     by class;   cos(x, y) = x . y / (|x| |y| + eps).
 *   pixel_dis = [ sum_b T_b + sum_{i present} (sum_{n in i} (1 - cos(f_n, g_i))) / (m_i + eps) ] / (F + B),
 *     T_b = (sum_{n in bg(b)} (1 - cos(f_n, c_b))) / (n_b + eps) when n_b >= 1, T_b = 2 when n_b = 0.
 *   ff = [sum_{i != j} (1 + cos(g_i, g_j))] / (F (F - 1)) when F > 1, else 0;  fb = the mean over the F x B matrix of
 *     1 + cos(g_i, c_b), an image without background contributing 1 per entry.
 *   dis = ff / 2 + fb / 2 with at least one foreground and one background pixel in the batch; ff / 2 + 1 with no background
 *     pixel at all; 0 with no foreground pixel.
 *   loss = dis + pixel_dis.  Its gradient in feat is that of this expression with d|x|/dx := 0 at x = 0 (torch's rule for norm).
 *     At an all-zero feature vector the denominator is eps, so that pixel's gradient is of order 1 / eps: the reference's
 *     behaviour, kept.  The divisors n + eps are formed in double (the reference forms them in fp32, where 1 + 1e-7 rounds to
 *     1 + 2^-23).
 * In closed form, with k the centre of pixel n (centre r < B: the background of image r; centre B + i - 1: class i; NC = B + K - 1),
 * D_n = |f_n| |c_k| + eps, Z = F + B and cnt' = count_k + eps:
 *     d_feat[b,:,n] = g_out (a_n c_k + b_n f_n + G_k / cnt'),   a_n = -1 / (Z cnt' D_n),
 *     b_n = (f_n . c_k) |c_k| / (Z cnt' |f_n| D_n^2)   (0 at |f_n| = 0),   G_k = d loss / d c_k.
 * acr_featdis_fwd: loss (3) fp32 = (dis + pixel_dis, dis, pixel_dis); labels (B, h, w) uint8; counts (B + K - 1) int64: n_b per
 *   image, then m_i per class i = 1..K-1; pix (B, N, 2) double: (a_n, b_n); cst (2, NC, C) double: the centres c_k, then
 *   G_k / cnt' (0 for a centre without a pixel).  All WRITTEN, every element; labels, pix and cst are what acr_featdis_bwd takes.
 *   Every value is evaluated in double and rounded once.  Sums: per slab of 2048 ceil(K / 32) pixels of an image, per class and
 *   channel, the pixels ascending; then the slabs in (image, slab) order, as eight consecutive runs whose sums are added in order; channel
 *   sums in channel order, by fixed quarters or by a fixed butterfly.
 *   The forward reads feat three times (class sums; dot products; the class sums weighted by 1 / D_n that G_k needs -- the
 *   re-read form, the weight of a pixel being known only after its dot product), the backward once.
 *   ws: acr_featdis_ws_bytes(B, K, C, h, w) bytes on the device, 16-byte aligned, contents arbitrary (host only; negative for
 *   arguments outside the contract).  The slab partials in it are [slabs][K][C] doubles: 2 K / (2048 ceil(K / 32)) <= 1/32 of feat.
 * acr_featdis_bwd: dfeat (B, C, h, w), WRITTEN (every element) = gscale[0] * d loss / d feat, gscale one fp32 value on the device.
 * Contract: 1 <= B <= 65535, 2 <= K <= 128, 1 <= C <= 2^20, h, w >= 1, B h w < 2^31; anything else returns ACR_ERR_INVALID and
 * launches nothing.  No float atomics, fixed orders: bit-identical run to run.  The entry points allocate nothing and do not
 * synchronise. */
#define ACR_FEATDIS_MAX_K 128
int64_t acr_featdis_ws_bytes(int32_t B, int32_t K, int32_t C, int32_t h, int32_t w);
int acr_featdis_fwd(const float* seg, const float* feat, int32_t B, int32_t K, int32_t C, int32_t h, int32_t w, void* ws,
                    int64_t ws_bytes, float* loss, uint8_t* labels, int64_t* counts, double* pix, double* cst, void* stream);
int acr_featdis_bwd(const float* feat, const uint8_t* labels, const double* pix, const double* cst, const float* gscale, int32_t B,
                    int32_t K, int32_t C, int32_t h, int32_t w, float* dfeat, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACR_HIP_H */
