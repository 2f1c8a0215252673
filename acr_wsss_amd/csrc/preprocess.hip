// Batched input pipeline of the ACR training / CAM steps:
//   myTool.py:1158-1199 get_data_from_chunk_v2   decode -> RandomResizeLong (cv2.resize, bilinear) -> flip ->
//                                                (x/255 - mean)/std -> zero-padded RandomCrop to S x S
//   myTool.py:1364-1403 get_data_from_chunk_val  decode -> cv2.resize(S, S) -> (x/255 - mean)/std
// The host decodes (any decoder) and draws the geometry; this kernel does everything else for the WHOLE batch in one
// launch, reading the decoded uint8 HWC RGB images once and writing the (B,3,S,S) network input once: resize, flip,
// normalisation and crop are an index map plus a pointwise affine, so they fuse into one gather per output pixel.
// HBM-bound: 4 source pixels (L2-resident neighbours) + 12 or 6 bytes written per output pixel.
//
// cv2.resize(float image, INTER_LINEAR) semantics (the reference converts to float64 BEFORE resizing, so it is the
// float path, not the 11-bit fixed-point uint8 path): sample position (d + 0.5) * in/out - 0.5, clamped to the border
// -- identical to F.interpolate(bilinear, align_corners=False) without antialiasing.
#include "acr_common.h"

struct PreImg : acr_pre_image {};   // the header's record under the name the kernels' symbols carry

// The normalised image value at pixel (ry, rx) of the resized image: cv2.resize's float INTER_LINEAR sample, then (v / 255 - mean) /
// std.  Not the fp32 rule of acr_resample.h: the sample position (d + 0.5) * in/out - 0.5 = ((2d + 1) * in - out) / (2 * out) is
// taken in exact integer arithmetic, because the reference computes it in float64, and an fp32 product loses ~3e-5 of a pixel at
// x ~ 500, i.e. 2e-4 of the output.  Both kernels below take their image from here, so their images agree bit for bit.
struct PreRgb { float r0, r1, r2; };
__device__ __forceinline__ PreRgb pre_sample(const uint8_t* __restrict__ p, const PreImg& im, int ry, int rx, float m0, float m1,
                                             float m2, float s0, float s1, float s2) {
    const int ny = (2 * ry + 1) * im.h - im.rh, dy = 2 * im.rh;
    const int nx = (2 * rx + 1) * im.w - im.rw, dx = 2 * im.rw;
    const int y0 = ny < 0 ? 0 : min(ny / dy, im.h - 1), x0 = nx < 0 ? 0 : min(nx / dx, im.w - 1);
    const int y1 = min(y0 + 1, im.h - 1), x1 = min(x0 + 1, im.w - 1);
    const float ly = (ny < 0 || y0 >= im.h - 1) ? 0.f : (float)(ny - y0 * dy) / (float)dy;
    const float lx = (nx < 0 || x0 >= im.w - 1) ? 0.f : (float)(nx - x0 * dx) / (float)dx;
    const uint8_t* p00 = p + ((int64_t)y0 * im.w + x0) * 3;
    const uint8_t* p01 = p + ((int64_t)y0 * im.w + x1) * 3;
    const uint8_t* p10 = p + ((int64_t)y1 * im.w + x0) * 3;
    const uint8_t* p11 = p + ((int64_t)y1 * im.w + x1) * 3;
    const float w00 = (1.f - ly) * (1.f - lx), w01 = (1.f - ly) * lx, w10 = ly * (1.f - lx), w11 = ly * lx;
    const float v0 = w00 * p00[0] + w01 * p01[0] + w10 * p10[0] + w11 * p11[0];
    const float v1 = w00 * p00[1] + w01 * p01[1] + w10 * p10[1] + w11 * p11[1];
    const float v2 = w00 * p00[2] + w01 * p01[2] + w10 * p10[2] + w11 * p11[2];
    return {(v0 / 255.f - m0) / s0, (v1 / 255.f - m1) / s1, (v2 / 255.f - m2) / s2};
}

template <typename T>
__global__ __launch_bounds__(256) void preprocess_kernel(const uint8_t* __restrict__ packed, const PreImg* __restrict__ tab,
                                                         T* __restrict__ out, int S, float m0, float m1, float m2, float s0,
                                                         float s1, float s2) {
    const int b = blockIdx.y;
    const PreImg im = tab[b];
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= S * S) return;
    const int y = pix / S, x = pix - y * S;
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    const int cy = y - im.cont_top, cx = x - im.cont_left;
    if (cy >= 0 && cy < im.ch && cx >= 0 && cx < im.cw) {
        const int ry = im.img_top + cy;                       // pixel of the resized (and flipped) image
        int rx = im.img_left + cx;
        if (im.flip) rx = im.rw - 1 - rx;
        const PreRgb q = pre_sample(packed + im.offset, im, ry, rx, m0, m1, m2, s0, s1, s2);
        r0 = q.r0;
        r1 = q.r1;
        r2 = q.r2;
    }
    T* o = out + (int64_t)b * 3 * S * S + pix;
    acr_store1<T>(o, r0);
    acr_store1<T>(o + (int64_t)S * S, r1);
    acr_store1<T>(o + 2 * (int64_t)S * S, r2);
}

extern "C" int acr_preprocess_batch(const void* packed_u8, const void* table, int32_t batch, int32_t S, const float* mean3,
                                    const float* std3, int32_t out_dtype, void* out, void* stream) {
    ACR_CHECK_ARG(packed_u8 && table && out && mean3 && std3, "acr_preprocess_batch: null pointer");
    ACR_CHECK_ARG(batch > 0 && S > 0, "acr_preprocess_batch: bad geometry batch=%d S=%d", batch, S);
    const dim3 grid((unsigned)((S * S + 255) / 256), (unsigned)batch);
    if (out_dtype == ACR_F32)
        hipLaunchKernelGGL((preprocess_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)packed_u8,
                           (const PreImg*)table, (float*)out, S, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    else if (out_dtype == ACR_BF16)
        hipLaunchKernelGGL((preprocess_kernel<__bf16>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)packed_u8,
                           (const PreImg*)table, (__bf16*)out, S, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    else {
        acr_set_error("acr_preprocess_batch: unknown output dtype %d", out_dtype);
        return ACR_ERR_UNSUPPORTED;
    }
    return acr_check_launch("acr_preprocess_batch");
}

// ---- segmentation-training loaders: myTool.py:1257-1310 get_data_from_chunk_v4 (image + target map) and :1202-1253
// get_data_from_chunk_v3 (image + saliency map) on RandomResizeLong2 (:1010-1023), flip2 (:901-905), RandomCrop2 (:957-993) ----
// One launch writes the four outputs of a chunk from the same geometry record (include/acr_hip.h states the rule in full).  The
// image value is pre_sample's, as in preprocess_kernel above (the build has -ffp-contract=off), so `images` equals
// acr_preprocess_batch's output bit for bit.  A bandwidth-bound gather, ~20 bytes written per output pixel: with
// S % 4 == 0 a thread owns 4 consecutive x of one row and stores 16 bytes (fp32 planes, croppings), 8 (bf16) or 4 (the uint8
// planes) at a time; any other S takes one pixel per thread.  No atomics, no LDS.
__device__ __forceinline__ uint8_t seg_ori_byte(float x, float sd, float mn) {
    // :1293-1297 on the float32 container: separate multiply, add, multiply (numpy does not contract), then astype(uint8)
    const float v = __fmul_rn(__fadd_rn(__fmul_rn(x, sd), mn), 255.f);
    return (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f);
}

template <typename T, int V>
__global__ __launch_bounds__(256) void preprocess_seg_kernel(const uint8_t* __restrict__ packed, const PreImg* __restrict__ tab,
                                                             const int64_t* __restrict__ map_offs, T* __restrict__ out,
                                                             uint8_t* __restrict__ ori, float* __restrict__ crop,
                                                             uint8_t* __restrict__ omap, int S, float m0, float m1, float m2,
                                                             float s0, float s1, float s2, int map_fill) {
    const int b = blockIdx.y;
    const PreImg im = tab[b];
    const int pix = (blockIdx.x * 256 + threadIdx.x) * V;     // V == 4 only with S % 4 == 0: the V pixels share a row
    if (pix >= S * S) return;
    const int y = pix / S, xb = pix - y * S;
    const int cy = y - im.cont_top;
    const bool row_in = cy >= 0 && cy < im.ch;
    const int ry = im.img_top + cy;                           // row of the resized image (used only when row_in)
    const uint8_t* p = packed + im.offset;
    const uint8_t* mp = omap ? packed + map_offs[b] : nullptr;
    const int my = row_in ? min((int)((int64_t)ry * im.h / im.rh), im.h - 1) : 0;      // INTER_NEAREST: floor(d * src / dst)
    float r[3][V], in[V];
    uint8_t mv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        const int cx = xb + v - im.cont_left;
        const bool inside = row_in && cx >= 0 && cx < im.cw;
        uint8_t mval = (uint8_t)map_fill;
        if (inside) {
            int rx = im.img_left + cx;
            if (im.flip) rx = im.rw - 1 - rx;
            const PreRgb q = pre_sample(p, im, ry, rx, m0, m1, m2, s0, s1, s2);
            r0 = q.r0;
            r1 = q.r1;
            r2 = q.r2;
            if (mp) {
                const int mx = min((int)((int64_t)rx * im.w / im.rw), im.w - 1);
                mval = mp[(int64_t)my * im.w + mx];
            }
        }
        r[0][v] = r0;
        r[1][v] = r1;
        r[2][v] = r2;
        in[v] = inside ? 1.f : 0.f;
        mv[v] = mval;
    }
    const int64_t plane = (int64_t)S * S;
    T* o = out + (int64_t)b * 3 * plane + pix;
    if constexpr (V == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 q = {r[c][0], r[c][1], r[c][2], r[c][3]};
            acr_store4<T>(o + c * plane, q);
        }
        if (ori) {
            const float sd[3] = {s0, s1, s2}, mn[3] = {m0, m1, m2};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                uint32_t w = 0;
#pragma unroll
                for (int v = 0; v < 4; ++v) w |= (uint32_t)seg_ori_byte(r[c][v], sd[c], mn[c]) << (8 * v);
                *reinterpret_cast<uint32_t*>(ori + ((int64_t)b * 3 + c) * plane + pix) = w;
            }
        }
        if (crop) {
            const f32x4 q = {in[0], in[1], in[2], in[3]};
            *reinterpret_cast<f32x4*>(crop + (int64_t)b * plane + pix) = q;
        }
        if (omap)
            *reinterpret_cast<uint32_t*>(omap + (int64_t)b * plane + pix) =
                (uint32_t)mv[0] | (uint32_t)mv[1] << 8 | (uint32_t)mv[2] << 16 | (uint32_t)mv[3] << 24;
    } else {
        acr_store1<T>(o, r[0][0]);
        acr_store1<T>(o + plane, r[1][0]);
        acr_store1<T>(o + 2 * plane, r[2][0]);
        if (ori) {
            uint8_t* oo = ori + (int64_t)b * 3 * plane + pix;
            oo[0] = seg_ori_byte(r[0][0], s0, m0);
            oo[plane] = seg_ori_byte(r[1][0], s1, m1);
            oo[2 * plane] = seg_ori_byte(r[2][0], s2, m2);
        }
        if (crop) crop[(int64_t)b * plane + pix] = in[0];
        if (omap) omap[(int64_t)b * plane + pix] = mv[0];
    }
}

template <typename T>
static void launch_seg(bool vec, dim3 grid, hipStream_t st, const void* packed_u8, const void* table, const int64_t* map_offsets,
                       void* images, void* ori, void* crop, void* omap, int S, const float* mean3, const float* std3, int map_fill) {
    if (vec)
        hipLaunchKernelGGL((preprocess_seg_kernel<T, 4>), grid, dim3(256), 0, st, (const uint8_t*)packed_u8, (const PreImg*)table,
                           map_offsets, (T*)images, (uint8_t*)ori, (float*)crop, (uint8_t*)omap, S, mean3[0], mean3[1], mean3[2],
                           std3[0], std3[1], std3[2], map_fill);
    else
        hipLaunchKernelGGL((preprocess_seg_kernel<T, 1>), grid, dim3(256), 0, st, (const uint8_t*)packed_u8, (const PreImg*)table,
                           map_offsets, (T*)images, (uint8_t*)ori, (float*)crop, (uint8_t*)omap, S, mean3[0], mean3[1], mean3[2],
                           std3[0], std3[1], std3[2], map_fill);
}

extern "C" int acr_preprocess_seg_batch(const void* packed_u8, const void* table, const int64_t* map_offsets, int32_t batch,
                                        int32_t S, const float* mean3, const float* std3, int32_t out_dtype, int32_t map_fill,
                                        void* images, void* ori_u8, void* croppings, void* map_u8, void* stream) {
    ACR_CHECK_ARG(packed_u8 && table && images && mean3 && std3, "acr_preprocess_seg_batch: null pointer");
    ACR_CHECK_ARG(batch > 0 && batch <= 65535 && S > 0 && S <= 32768, "acr_preprocess_seg_batch: bad geometry batch=%d S=%d", batch, S);
    ACR_CHECK_ARG(!map_u8 || map_offsets, "acr_preprocess_seg_batch: a map output needs the map offsets");
    ACR_CHECK_ARG(map_fill >= 0 && map_fill <= 255, "acr_preprocess_seg_batch: map_fill=%d outside 0..255", map_fill);
    const bool vec = S % 4 == 0;
    const int items = vec ? S * S / 4 : S * S;
    const dim3 grid((unsigned)((items + 255) / 256), (unsigned)batch);
    if (out_dtype == ACR_F32)
        launch_seg<float>(vec, grid, (hipStream_t)stream, packed_u8, table, map_offsets, images, ori_u8, croppings, map_u8, S, mean3,
                          std3, map_fill);
    else if (out_dtype == ACR_BF16)
        launch_seg<__bf16>(vec, grid, (hipStream_t)stream, packed_u8, table, map_offsets, images, ori_u8, croppings, map_u8, S, mean3,
                           std3, map_fill);
    else {
        acr_set_error("acr_preprocess_seg_batch: unknown output dtype %d", out_dtype);
        return ACR_ERR_UNSUPPORTED;
    }
    return acr_check_launch("acr_preprocess_seg_batch");
}
