// Segmentation prediction on the device (the reference's validation, myTool.py:1826-1895): the bilinear resize of the
// segmentation logits to the image's own size (:1881), the softmax over the classes (:1883) and the argmax (:1891) in ONE pass, so
// that the (K, H, W) fp32 tensor F.interpolate would write (15.75 MB at 21 x 375 x 500, for 187 KB of labels) never exists; with
// `accumulate` the probabilities of several passes (scales, flips) are summed in place and the last pass leaves the label map.
//
// Mapping: ONE THREAD PER OUTPUT PIXEL, pixels numbered row-major so that the 64 lanes of a wave hold 64 consecutive values of the
// contiguous axis: every store of a class plane is one 256-byte segment and the four source texels of neighbouring lanes are the
// same or adjacent (the source, 12.4 MB at 21 x 384 x 384, is read through the caches).  Indices and weights are computed once per
// pixel and reused for the K planes.  The label-only mode is a single sweep over the planes in registers.  The modes that need
// the probabilities keep the K interpolated logits of a pixel in a private LDS column ([k][thread]: conflict free, the layout of
// segloss_fwd_kernel), so the maximum, the sum and the quotients read them without touching the source again; the exponentials
// overwrite the column, so each is evaluated once.  No thread reads another thread's column: no barrier, no atomics, nothing
// depends on the launch geometry -- bit-identical run to run.
#include "acr_resample.h"

#define SEGPRED_MAX_K ACR_SEG_MAX_K
#define SEGPRED_MAX_B 65535
#define SEGPRED_UNROLL 8                  // planes whose texels are in flight together (K = 21: three batches)

enum { SEGPRED_LABEL = 0, SEGPRED_PROBS = 1, SEGPRED_ACCUM = 2 };

// grid = (ceil(H * W / 256), B); K * h * w and K * H * W are below 2^31, so offsets inside one image are int
template <int MODE>
__global__ __launch_bounds__(256) void segpred_kernel(const float* __restrict__ logits, int K, int h, int w, int H, int W, float sh,
                                                      float sw, int hflip, float* __restrict__ probs, uint8_t* __restrict__ label) {
    extern __shared__ __attribute__((aligned(16))) float segpred_smem[];
    const int HW = H * W, hw = h * w;
    const int pix = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (pix >= HW) return;                               // no barrier below: a thread past the image simply leaves
    const int b = blockIdx.y;
    // the taps of acr_resample.h, which acr_segloss_fwd takes too (and acr_bilinear_resize's source index)
    const acr_taps t = acr_taps_of<true>(pix / W, pix % W, h, w, sh, sw, hflip);
    const float* lg = logits + (int64_t)b * K * hw;
    float* col = segpred_smem + threadIdx.x;             // v_k, then exp(v_k - m), of this thread's pixel at col[k * 256]
    float m = -INFINITY;
    int lab = 0;
    auto take = [&](int k, float v) {
        if (MODE != SEGPRED_LABEL) col[k * 256] = v;
        if (v > m) {                                     // strict: the smallest k among the maxima stays
            m = v;
            lab = k;
        }
    };
    // The planes are independent, but left to itself the compiler waits for the four texels of one plane before it asks for the
    // next (seen in the ISA): a wave then pays one memory latency per class.  So the texels of SEGPRED_UNROLL planes are requested
    // first and interpolated afterwards.  The last batch re-reads plane K - 1 in its unused slots (in bounds, never taken).
    for (int k = 0; k < K; k += SEGPRED_UNROLL) {
        float tex[SEGPRED_UNROLL][4];
#pragma unroll
        for (int u = 0; u < SEGPRED_UNROLL; ++u) {
            const float* p = lg + min(k + u, K - 1) * hw;
            tex[u][0] = p[t.o00];
            tex[u][1] = p[t.o01];
            tex[u][2] = p[t.o10];
            tex[u][3] = p[t.o11];
        }
#pragma unroll
        for (int u = 0; u < SEGPRED_UNROLL; ++u)
            if (k + u < K) take(k + u, acr_bilerp(t.hy, t.ly, t.hx, t.lx, tex[u][0], tex[u][1], tex[u][2], tex[u][3]));
    }
    if (MODE != SEGPRED_LABEL) {
        float s = 0.f;
        for (int k = 0; k < K; ++k) {
            const float e = expf(col[k * 256] - m);
            col[k * 256] = e;
            s += e;
        }
        float* pp = probs + (int64_t)b * K * HW + pix;
        if (MODE == SEGPRED_ACCUM) {
            float best = -INFINITY;
            lab = 0;
            auto add = [&](int k, float old) {
                const float q = old + col[k * 256] / s;
                pp[k * HW] = q;
                if (q > best) {
                    best = q;
                    lab = k;
                }
            };
            for (int k = 0; k < K; k += SEGPRED_UNROLL) {                     // the same staging for the values added to
                float old[SEGPRED_UNROLL];
#pragma unroll
                for (int u = 0; u < SEGPRED_UNROLL; ++u) old[u] = pp[min(k + u, K - 1) * HW];
#pragma unroll
                for (int u = 0; u < SEGPRED_UNROLL; ++u)
                    if (k + u < K) add(k + u, old[u]);
            }
        } else {
            for (int k = 0; k < K; ++k) pp[k * HW] = col[k * 256] / s;
        }
    }
    if (label) label[(int64_t)b * HW + pix] = (uint8_t)lab;
}

extern "C" int acr_segpred_f32(const float* logits, int32_t B, int32_t K, int32_t h, int32_t w, int32_t H, int32_t W, int32_t hflip,
                               int32_t accumulate, float* probs, uint8_t* label, void* stream) {
    ACR_CHECK_ARG(B >= 1 && B <= SEGPRED_MAX_B, "acr_segpred_f32: B=%d outside 1..%d", B, SEGPRED_MAX_B);
    ACR_CHECK_ARG(K >= 2 && K <= SEGPRED_MAX_K, "acr_segpred_f32: K=%d outside 2..%d", K, SEGPRED_MAX_K);
    ACR_CHECK_ARG(h >= 1 && w >= 1 && H >= 1 && W >= 1, "acr_segpred_f32: empty size (logits %d x %d, output %d x %d)", h, w, H, W);
    ACR_CHECK_ARG((int64_t)K * h * w < (1ll << 31), "acr_segpred_f32: logits too large (%d x %d x %d)", K, h, w);
    ACR_CHECK_ARG((int64_t)K * H * W < (1ll << 31), "acr_segpred_f32: output too large (%d x %d x %d)", K, H, W);
    ACR_CHECK_ARG(logits, "acr_segpred_f32: null pointer (logits)");
    ACR_CHECK_ARG(probs || label, "acr_segpred_f32: no output (probs and label both null)");
    ACR_CHECK_ARG(!accumulate || probs, "acr_segpred_f32: accumulate needs the probs buffer it adds to");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(((int64_t)H * W + 255) / 256), (unsigned)B);
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    const size_t lds = (size_t)K * 256 * sizeof(float);
    const int flip = hflip ? 1 : 0;
    if (!probs)
        hipLaunchKernelGGL(segpred_kernel<SEGPRED_LABEL>, grid, dim3(256), 0, st, logits, K, h, w, H, W, sh, sw, flip, probs, label);
    else if (accumulate)
        hipLaunchKernelGGL(segpred_kernel<SEGPRED_ACCUM>, grid, dim3(256), lds, st, logits, K, h, w, H, W, sh, sw, flip, probs, label);
    else
        hipLaunchKernelGGL(segpred_kernel<SEGPRED_PROBS>, grid, dim3(256), lds, st, logits, K, h, w, H, W, sh, sw, flip, probs, label);
    return acr_check_launch("acr_segpred_f32");
}
