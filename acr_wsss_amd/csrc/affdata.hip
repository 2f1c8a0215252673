// Training input of the affinity stage: the label grid VOC12AffDataset.__getitem__ (voc12/data.py:241-278) cuts its pair masks from,
// for a whole batch in one launch.  Per image the reference stacks the low- and the high-alpha score planes, crops them into a
// zero container (tool/imutils.py:167-190 get_random_crop_box, :201-225 random_crop), flips the container (:239-246), pools it
// 8 x 8 (:228-236 AvgPool2d) and takes two argmaxes; include/acr_hip.h, "affinity-stage input", states the rule in full.
//
// Crop, flip and pool are an index map plus a block mean, so nothing but the label is ever written: the stacked (h, w, 2n) array,
// the container and the pooled planes never exist.  Purely bandwidth-bound -- 2 n ch cw 4 bytes read per image, SH SW / 64 written.
//
// Mapping: a wave owns 8 neighbouring cells of one cell row, lane l the container column 64 u + l of all 8 container rows of that
// cell row; a cell is 8 consecutive lanes.  Per plane a lane issues up to 8 independent 4-byte loads (one per row), each a wave-wide
// run of 256 contiguous bytes along x (descending addresses under a flip, the same run), so every score element inside the crop box
// is read exactly once and nothing outside it is addressed: those container cells are 0 by definition.  Image rows start at any
// 4-byte boundary (w is arbitrary), hence 4-byte loads and no vector form with a head and a tail.  A lane sums its column's rows
// ascending in double, the 8 column sums of a cell meet in a fixed butterfly (xor 1, 2, 4): a fixed order, no atomics, no LDS.
// The planes are walked with a running best per half because n differs from image to image.
#include "acr_common.h"

struct AffPreImg : acr_pre_image {};   // the header's record (rh = h, rw = w here) under the name the kernel's symbol carries

__global__ __launch_bounds__(256) void aff_label_kernel(const uint8_t* __restrict__ scores, const AffPreImg* __restrict__ tab,
                                                        const int64_t* __restrict__ la_off, const int64_t* __restrict__ ha_off,
                                                        const int32_t* __restrict__ n_planes, int SH, int SW,
                                                        uint8_t* __restrict__ label) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int strips = (SW + 63) >> 6;                           // 64-column strips of a cell row
    const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);        // wave-uniform: (cell row, strip)
    const int gh = SH >> 3, gw = SW >> 3;
    if (unit >= gh * strips) return;                             // the whole wave leaves; no barrier below
    const int gy = unit / strips, x = (unit - gy * strips) * 64 + lane;
    const AffPreImg im = tab[b];
    const int n = n_planes[b];
    // container rows [8 gy, 8 gy + 8) that lie in the crop box, as rows r0 .. r1 - 1 of the cell row: wave-uniform
    const int r0 = max(im.cont_top - 8 * gy, 0), r1 = min(im.cont_top + im.ch - 8 * gy, 8);
    const int cx = x - im.cont_left;
    const bool col_in = cx >= 0 && cx < im.cw;                   // x >= SW lies outside as well: cont_left + cw <= SW
    int sx = im.img_left + cx;                                   // column of the flipped image ...
    if (im.flip) sx = im.w - 1 - sx;                             // ... and of the stored one
    const int64_t plane = (int64_t)im.h * im.w;
    const int64_t first = (int64_t)(im.img_top + 8 * gy - im.cont_top) * im.w + sx;     // row r of the cell row: first + r w
    float best[2] = {0.f, 0.f};
    int arg[2] = {0, 0};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const float* p = reinterpret_cast<const float*>(scores + (half ? ha_off[b] : la_off[b]));
        for (int k = 0; k < n; ++k, p += plane) {
            float v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = (col_in && r >= r0 && r < r1) ? p[first + (int64_t)r * im.w] : 0.f;
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < 8; ++r) s += (double)v[r];
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) s += __shfl_xor(s, off);
            const float m = (float)(s * 0.015625);               // the exact sum of the 64 values / 64, rounded once
            if (k == 0 || m > best[half]) {                      // the first maximum wins
                best[half] = m;
                arg[half] = k;
            }
        }
    }
    if ((lane & 7) == 0 && x < SW) {
        int lab = arg[0] == 0 ? 255 : arg[0];
        if (arg[1] == 0) lab = 0;
        if (fmaxf(best[0], best[1]) < 1e-5f) lab = 255;          // no score: mostly outside the crop box
        label[((int64_t)b * gh + gy) * gw + (x >> 3)] = (uint8_t)lab;
    }
}

extern "C" int acr_aff_label_batch(const void* scores, const void* table, const int64_t* la_off, const int64_t* ha_off,
                                   const int32_t* n_planes, int32_t batch, int32_t SH, int32_t SW, uint8_t* label_u8, void* stream) {
    ACR_CHECK_ARG(scores && table && la_off && ha_off && n_planes && label_u8, "acr_aff_label_batch: null pointer");
    ACR_CHECK_ARG(batch > 0 && batch <= 65535 && SH > 0 && SW > 0 && SH <= 32768 && SW <= 32768 && SH % 8 == 0 && SW % 8 == 0,
                  "acr_aff_label_batch: bad geometry batch=%d SH=%d SW=%d (multiples of 8 up to 32768)", batch, SH, SW);
    const int units = (SH / 8) * ((SW + 63) / 64);
    hipLaunchKernelGGL(aff_label_kernel, dim3((unsigned)((units + 3) / 4), (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)scores, (const AffPreImg*)table, la_off, ha_off, n_planes, SH, SW, label_u8);
    return acr_check_launch("acr_aff_label_batch");
}
