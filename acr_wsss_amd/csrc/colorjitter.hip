// Colour jitter of the affinity stage's input (voc12/data.py:241-278 reads it through PSA's transform list, which begins with
// torchvision's ColorJitter on the PIL image): Pillow's ImageEnhance.Brightness / Contrast / Color and an HSV round trip, uint8 in and
// uint8 out, on the packed batch in place.  include/acr_hip.h, "colour jitter", states every operation with its types; this file
// executes them as typed (-ffp-contract=off, IEEE division), so the result is Pillow's bit for bit.
//
// Two launches for the whole batch: blockIdx.y is the image, so the operation order, the factors and the contrast mean are uniform
// in a workgroup and the switch over the operations never diverges.
//   mean pass   only the images whose order names contrast: every pixel through the operations in front of contrast, then gray, then
//               an exact integer sum.  A thread sums in 64 bits, a wave by a butterfly, a workgroup through LDS; workgroup x of
//               image b stores its partial at ws[b * gridDim.x + x] (0 when it had no pixel).  No atomics and nothing to clear.
//   apply pass  adds the image's partials (integers: any order is exact), forms m = (2 sum + n) / (2 n), puts every pixel through the
//               whole sequence and stores it once.
// Both walk an image in groups of 4 pixels = 12 bytes = three aligned dwords per lane (an image starts at a 16-byte aligned offset),
// 768 contiguous bytes per wave; the last group of an image with h w % 4 != 0 is read and written byte by byte, so the alignment
// padding between images is never touched.  The arithmetic is a few dozen VALU operations per pixel with double-precision divisions
// in the hue round trip: ALU-bound, not bandwidth-bound (6 bytes of traffic per pixel).
#include "acr_common.h"

namespace {

struct JitterOps {
    int32_t op[4];
    float factor[3];
    int32_t shift;
};

__device__ __forceinline__ int jitter_gray(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Pillow's ImagingBlend: a float32 product, then a float32 sum; clipped only for a outside [0, 1]
__device__ __forceinline__ int jitter_blend(int deg, int img, float a, bool inside) {
    const float t = (float)deg + a * (float)(img - deg);
    if (inside) return (int)t & 255;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int jitter_clip(int v) { return min(max(v, 0), 255); }

// Pillow's rgb2hsv_row, H shifted, hsv2rgb_row
__device__ __forceinline__ void jitter_hue(int& r, int& g, int& b, int shift) {
    const int maxc = max(max(r, g), b), minc = min(min(r, g), b);
    int H = 0, S = 0;
    const int V = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc)
            h = bc - gc;
        else if (g == maxc)
            h = (float)(2.0 + (double)rc - (double)bc);
        else
            h = (float)(4.0 + (double)gc - (double)rc);
        const double x = (double)h / 6.0 + 1.0;               // in (0.8, 2): fmod(x, 1.0) = x - floor(x), exactly
        h = (float)(x - floor(x));
        H = jitter_clip((int)((double)h * 255.0));
        S = jitter_clip((int)((double)s * 255.0));
    }
    H = (H + shift) & 255;
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const double hf = (double)(float)H * 6.0 / 255.0;
    const float i = (float)floor(hf);
    const float f = (float)(hf - (double)i);
    const float fs = (float)((double)(float)S / 255.0);
    const double Vd = (double)V;
    const int p = jitter_clip((int)round(Vd * (1.0 - (double)fs)));
    const int q = jitter_clip((int)round(Vd * (1.0 - (double)(fs * f))));
    const int t = jitter_clip((int)round(Vd * (1.0 - (double)fs * (1.0 - (double)f))));
    const int k = (int)i % 6;                                    // selects, not a switch: r, g, b stay in registers
    r = (k == 0 || k == 5) ? V : (k == 1 ? q : (k == 4 ? t : p));
    g = (k == 1 || k == 2) ? V : (k == 0 ? t : (k == 3 ? q : p));
    b = (k == 3 || k == 4) ? V : (k == 2 ? t : (k == 5 ? q : p));
}

// One pixel through the operations of slots 0 .. n_ops - 1: the mean pass stops in front of contrast, the apply pass runs all four
__device__ __forceinline__ void jitter_pixel(int& r, int& g, int& b, const JitterOps& J, int n_ops, int mean) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = J.op[k];                                  // uniform over the workgroup
        if (k >= n_ops) break;
        if (op == ACR_JITTER_HUE) {
            jitter_hue(r, g, b, J.shift);
        } else if (op >= 0) {
            const float a = op == ACR_JITTER_BRIGHTNESS ? J.factor[0] : (op == ACR_JITTER_CONTRAST ? J.factor[1] : J.factor[2]);
            const bool inside = a >= 0.f && a <= 1.f;
            int dr = 0, dg = 0, db = 0;
            if (op == ACR_JITTER_CONTRAST) dr = dg = db = mean;
            if (op == ACR_JITTER_SATURATION) dr = dg = db = jitter_gray(r, g, b);
            r = jitter_blend(dr, r, a, inside), g = jitter_blend(dg, g, a, inside), b = jitter_blend(db, b, a, inside);
        }
    }
}

__device__ __forceinline__ JitterOps jitter_load(const int32_t* order, const float* factors, const int32_t* hue_shift, int b) {
    JitterOps J;
#pragma unroll
    for (int k = 0; k < 4; ++k) J.op[k] = order[4 * b + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) J.factor[k] = factors[3 * b + k];
    J.shift = hue_shift[b];
    return J;
}

// The 12 bytes of pixel group `grp` (4 pixels; the image's last group may hold 1..3) -> px[12]; `cnt` pixels are valid
__device__ __forceinline__ void jitter_read(const uint8_t* img, int64_t grp, int cnt, int px[12]) {
    uint32_t w[3] = {0, 0, 0};
    if (cnt == 4) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(img + 12 * grp);
        w[0] = p[0], w[1] = p[1], w[2] = p[2];
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (k < 3 * cnt) w[k >> 2] |= (uint32_t)img[12 * grp + k] << (8 * (k & 3));
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) px[k] = (w[k >> 2] >> (8 * (k & 3))) & 255;
}

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void color_jitter_mean_kernel(const uint8_t* __restrict__ packed, const int64_t* __restrict__ offsets,
                                                                     const int32_t* __restrict__ hw, const int32_t* __restrict__ order,
                                                                     const float* __restrict__ factors,
                                                                     const int32_t* __restrict__ hue_shift,
                                                                     unsigned long long* __restrict__ ws) {
    const int b = blockIdx.y;
    const JitterOps J = jitter_load(order, factors, hue_shift, b);
    int n_ops = -1;                                              // the slot of contrast
#pragma unroll
    for (int k = 3; k >= 0; --k)
        if (J.op[k] == ACR_JITTER_CONTRAST) n_ops = k;
    if (n_ops < 0) return;                                       // no contrast in this image: the whole workgroup leaves
    const uint8_t* img = packed + offsets[b];
    const int64_t n = (int64_t)hw[2 * b] * hw[2 * b + 1], groups = (n + 3) >> 2;
    unsigned long long sum = 0;
    for (int64_t grp = (int64_t)blockIdx.x * kThreads + threadIdx.x; grp < groups; grp += (int64_t)gridDim.x * kThreads) {
        const int cnt = (int)min((int64_t)4, n - 4 * grp);
        int px[12];
        jitter_read(img, grp, cnt, px);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int r = px[3 * k], g = px[3 * k + 1], bl = px[3 * k + 2];
            jitter_pixel(r, g, bl, J, n_ops, 0);
            if (k < cnt) sum += (unsigned)jitter_gray(r, g, bl);
        }
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    __shared__ unsigned long long part[kThreads / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) ws[(int64_t)b * gridDim.x + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(kThreads) void color_jitter_apply_kernel(uint8_t* __restrict__ packed, const int64_t* __restrict__ offsets,
                                                                      const int32_t* __restrict__ hw, const int32_t* __restrict__ order,
                                                                      const float* __restrict__ factors,
                                                                      const int32_t* __restrict__ hue_shift,
                                                                      const unsigned long long* __restrict__ ws, int n_part) {
    const int b = blockIdx.y;
    const JitterOps J = jitter_load(order, factors, hue_shift, b);
    uint8_t* img = packed + offsets[b];
    const int64_t n = (int64_t)hw[2 * b] * hw[2 * b + 1], groups = (n + 3) >> 2;
    if ((int64_t)blockIdx.x * kThreads >= groups) return;        // nothing for this workgroup: it leaves before the barrier
    bool has_contrast = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) has_contrast |= J.op[k] == ACR_JITTER_CONTRAST;
    int mean = 0;
    if (has_contrast && ws) {                                    // uniform over the workgroup
        unsigned long long sum = 0;
        for (int k = threadIdx.x; k < n_part; k += kThreads) sum += ws[(int64_t)b * n_part + k];
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        __shared__ unsigned long long part[kThreads / 64];
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
        __syncthreads();
        sum = part[0] + part[1] + part[2] + part[3];
        mean = (int)((2 * sum + (unsigned long long)n) / (2 * (unsigned long long)n));      // int(sum / n + 0.5)
    }
    for (int64_t grp = (int64_t)blockIdx.x * kThreads + threadIdx.x; grp < groups; grp += (int64_t)gridDim.x * kThreads) {
        const int cnt = (int)min((int64_t)4, n - 4 * grp);
        int px[12];
        jitter_read(img, grp, cnt, px);
#pragma unroll
        for (int k = 0; k < 4; ++k) jitter_pixel(px[3 * k], px[3 * k + 1], px[3 * k + 2], J, 4, mean);
        if (cnt == 4) {
            uint32_t* p = reinterpret_cast<uint32_t*>(img + 12 * grp);
            p[0] = (uint32_t)px[0] | (uint32_t)px[1] << 8 | (uint32_t)px[2] << 16 | (uint32_t)px[3] << 24;
            p[1] = (uint32_t)px[4] | (uint32_t)px[5] << 8 | (uint32_t)px[6] << 16 | (uint32_t)px[7] << 24;
            p[2] = (uint32_t)px[8] | (uint32_t)px[9] << 8 | (uint32_t)px[10] << 16 | (uint32_t)px[11] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (k < 3 * cnt) img[12 * grp + k] = (uint8_t)px[k];
        }
    }
}

// workgroups per image: about 2048 in all, between 8 and 256 per image; a workgroup strides over its image's pixel groups
int jitter_blocks(int batch) { return batch >= 256 ? 8 : (batch <= 8 ? 256 : (2048 + batch - 1) / batch); }

}  // namespace

extern "C" int64_t acr_color_jitter_ws_bytes(int32_t batch) {
    if (batch <= 0 || batch > 65535) {
        acr_set_error("acr_color_jitter_ws_bytes: batch=%d outside 1..65535", batch);
        return ACR_ERR_INVALID;
    }
    return (int64_t)batch * jitter_blocks(batch) * 8;
}

extern "C" int acr_color_jitter_batch(uint8_t* packed_u8, const int64_t* offsets, const int32_t* hw, const int32_t* order,
                                      const float* factors, const int32_t* hue_shift, int32_t batch, void* ws, void* stream) {
    ACR_CHECK_ARG(packed_u8 && offsets && hw && order && factors && hue_shift, "acr_color_jitter_batch: null pointer");
    ACR_CHECK_ARG(batch > 0 && batch <= 65535, "acr_color_jitter_batch: batch=%d outside 1..65535", batch);
    ACR_CHECK_ARG(((uintptr_t)packed_u8 & 15) == 0 && ((uintptr_t)ws & 7) == 0, "acr_color_jitter_batch: packed_u8 not aligned to 16 or ws not to 8 bytes");
    const int nb = jitter_blocks(batch);
    const dim3 grid((unsigned)nb, (unsigned)batch);
    if (ws) {                                                    // a null workspace: no order names contrast, no mean pass
        hipLaunchKernelGGL(color_jitter_mean_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, (const uint8_t*)packed_u8, offsets, hw, order,
                           factors, hue_shift, (unsigned long long*)ws);
        const int rc = acr_check_launch("acr_color_jitter_batch (mean)");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(color_jitter_apply_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, packed_u8, offsets, hw, order, factors, hue_shift,
                       (const unsigned long long*)ws, nb);
    return acr_check_launch("acr_color_jitter_batch");
}
