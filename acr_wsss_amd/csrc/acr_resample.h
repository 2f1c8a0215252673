// The fp32 bilinear resampling rules of the post-processing kernels, stated once: torch's upsample_bilinear2d as cam.hip
// (acr_bilinear_resize), segpred.hip, segloss.hip and decoder.hip (upsample2x) apply it.  Several tests pin these kernels to each
// other bit for bit, which holds because they share this text (the build has -ffp-contract=off: an expression keeps its operations
// and their order wherever it is inlined).  preprocess.hip's cv2 sample is a different rule (exact integer positions) and stays there.
#pragma once
#include "acr_common.h"

// torch upsample_bilinear2d source index (aten/src/ATen/native/UpSample.h area_pixel_compute_source_index), in fp32
__device__ __forceinline__ float acr_src_half_pixel(float scale, int dst) {        // align_corners=False
    const float s = scale * ((float)dst + 0.5f) - 0.5f;
    return s < 0.f ? 0.f : s;
}
__device__ __forceinline__ float acr_src_corners(float scale, int dst) { return scale * (float)dst; }      // align_corners=True

// hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11): the four texels in ATen's order of operations
__device__ __forceinline__ float acr_bilerp(float hy, float ly, float hx, float lx, float v00, float v01, float v10, float v11) {
    return hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

// the taps of destination pixel (Y, X) in an (h, w) source plane, align_corners=False.  MIRROR: the caller may pass hflip (the
// switch is compile time because a never-taken runtime branch here reordered the code of the callers that do not mirror)
struct acr_taps {
    int y0, y1, x0, x1;                   // the four source texels ...
    int o00, o01, o10, o11;               // ... and their offsets into the plane
    float hy, ly, hx, lx;
};

template <bool MIRROR = false>
__device__ __forceinline__ acr_taps acr_taps_of(int Y, int X, int h, int w, float sh, float sw, int hflip = 0) {
    acr_taps t;
    const float fy = acr_src_half_pixel(sh, Y), fx = acr_src_half_pixel(sw, X);
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 < h - 1 ? y0 : h - 1;         // fy < h always; the clamp keeps a rounding at the edge inside the plane
    x0 = x0 < w - 1 ? x0 : w - 1;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0);
    int x1 = x0 + (x0 < w - 1 ? 1 : 0);
    t.ly = fy - (float)y0;
    t.lx = fx - (float)x0;
    t.hy = 1.f - t.ly;
    t.hx = 1.f - t.lx;
    if (MIRROR && hflip) {                          // the source is the mirrored scene: its column x is column w - 1 - x of the scene
        x0 = w - 1 - x0;
        x1 = w - 1 - x1;
    }
    t.y0 = y0;
    t.y1 = y1;
    t.x0 = x0;
    t.x1 = x1;
    t.o00 = y0 * w + x0;
    t.o01 = y0 * w + x1;
    t.o10 = y1 * w + x0;
    t.o11 = y1 * w + x1;
    return t;
}

__device__ __forceinline__ float acr_interp(const float* __restrict__ p, const acr_taps& t) {
    return acr_bilerp(t.hy, t.ly, t.hx, t.lx, p[t.o00], p[t.o01], p[t.o10], p[t.o11]);
}

// Range search of a gather-form resize backward: the smallest destination index in [0, n_out] whose first source tap
// first_tap(d) is >= t.  first_tap is monotone in d and never passes n_in - 1; start(t) is the caller's estimate of the answer (the
// inverse of its source-index rule, asked for t >= 1 only), from which the search walks to the exact one.
template <typename S, typename F>
__device__ __forceinline__ int acr_first_dst(int t, int n_out, int n_in, S start, F first_tap) {
    if (t <= 0) return 0;
    if (t > n_in - 1) return n_out;
    float e = start(t);
    e = e < 0.f ? 0.f : (e > (float)n_out ? (float)n_out : e);
    int d = (int)e;
    while (d > 0 && first_tap(d - 1) >= t) --d;
    while (d < n_out && first_tap(d) < t) ++d;
    return d;
}
