// Saliency-guided pseudo-labels on the device (the reference's compute_seg_label_3, myTool.py:188-264, and its save-to-disk twin
// compute_seg_label_two_step, :313-367, which differ in the background exponent only): the CAM label map with its background as
// "ignore" (:217-229), zero where the saliency map is zero (:230), the grab rule that hands the most confident part of every
// present class back to such pixels (:236-250) and the 10 x 10 morphological opening of the labelled area (:253-255).  Per-pixel
// work on integers and comparisons, one exact order statistic per (image, class) plane and a binary opening: the outputs are pure
// functions of the inputs, bit-identical run to run.  include/acr_hip.h states the rule in full.
//
// Launches of one call, none of them data dependent: clear | 4 x (histogram, pick) | per-pixel | opening.
//   thresholds  the radix selection of pseudo_select.h over all B * C planes at once; absent planes and planes whose rank
//               int(n * cut) is 0 get +inf.
//   per-pixel   one thread per pixel reads every present plane once: the running maximum gives the label, the first plane above
//               its threshold the grab.
//   opening     one workgroup per 64 x 64 output tile.  A wave loads 64 bytes of a row and its ballot IS the bit-packed row, so
//               the tile and its halo of 2 (k - 1) are <= 126 rows of 128 bits in LDS.  Erosion is an AND of the k shifts of a
//               row, then of k rows; dilation the same with OR; positions outside the image enter the erosion as 1 and the
//               dilation as 0.
#include "acr_common.h"
#include "pseudo_select.h"

#define PSAL_MAX_CLASSES ACR_SAL_PSEUDO_MAX_CLASSES
#define PSAL_MAX_BATCH 65535
#define PSAL_TILE 64                     // opening: edge of a workgroup's output tile = the lanes of one ballot
#define PSAL_MAX_K 32
#define PSAL_BATCH 8                     // opening: loads a wave keeps in flight
#define PSAL_SETS 16                     // histogram: counter sets per workgroup (a power of two)
#define PSAL_ROWS (PSAL_TILE + 2 * (PSAL_MAX_K - 1))     // rows (and columns, within 128 bits) of a tile with its halo
// workspace, in 32-bit words, P = B * C planes: PREFIX (P: bits of the threshold) | RANK (P) | HIST (4 passes, P planes, 256 bins);
// then the label map before the opening, one byte per pixel

static size_t psal_head_words(int64_t P) { return (size_t)P * (2 + PSEUDO_PASSES * PSEUDO_BINS); }

// histogram pass 0..3 of plane blockIdx.x: the byte at `shift` of every value > 0 that agrees with the plane's prefix above it.
// V values per thread and load (4: hw is a multiple of 4 and the planes are 16-byte aligned).  CAM values crowd into three or
// four bins of the first pass, so the counters are kept PSAL_SETS times, lane l adding to set l % PSAL_SETS of a bin (neighbouring
// banks): a wave's 64 adds to one bin collide 4-fold, not 64-fold.
template <int V>
__global__ __launch_bounds__(256) void psal_hist_kernel(const float* __restrict__ cams, const uint8_t* __restrict__ present, int64_t hw,
                                                        int64_t P, int pass, uint32_t* __restrict__ ws) {
    __shared__ uint32_t hist[PSEUDO_BINS * PSAL_SETS];
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x;
    if (!present[plane]) return;                         // the whole workgroup
    const uint32_t prefix = pass ? ws[plane] : 0u;
    if (pass && ws[P + plane] == PSEUDO_EMPTY) return;   // nothing is selected from this plane
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < PSEUDO_BINS * PSAL_SETS; i += 256) hist[i] = 0;
    __syncthreads();
    uint32_t* mine = hist + (tid & (PSAL_SETS - 1));
    const float* p = cams + plane * hw;
    const int64_t n = hw / V;
    for (int64_t i = (int64_t)blockIdx.y * 256 + tid; i < n; i += (int64_t)gridDim.y * 256) {
        float v[V];
        if (V == 4) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(p + 4 * i);
#pragma unroll
            for (int u = 0; u < V; ++u) v[u] = q[u];
        } else {
            v[0] = p[i];
        }
#pragma unroll
        for (int u = 0; u < V; ++u)
            if (v[u] > 0.f) {
                const uint32_t bits = __float_as_uint(v[u]);
                if (pass == 0 || (bits >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&mine[((bits >> shift) & 255u) * PSAL_SETS], 1u);
            }
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int u = 0; u < PSAL_SETS; ++u) sum += hist[tid * PSAL_SETS + u];
    __syncthreads();
    hist[tid] = sum;
    __syncthreads();
    pseudo_hist_merge(hist, ws + 2 * P + ((size_t)pass * P + plane) * PSEUDO_BINS, PSEUDO_BINS);
}

// the head of the workspace (PREFIX, RANK, HIST) starts every call at zero: a kernel, so that a captured call holds kernel nodes only
__global__ __launch_bounds__(256) void psal_clear_kernel(uint32_t* __restrict__ ws, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) ws[i] = 0u;
}

// one workgroup per plane: pass 0 knows n = #{v > 0} and the rank pos = int(n * cut) (:241); pos == 0 selects nothing (:242)
__global__ __launch_bounds__(256) void psal_pick_kernel(uint32_t* __restrict__ ws, int64_t P, int pass, double cut) {
    __shared__ uint32_t incl[PSEUDO_BINS];
    const int64_t j = blockIdx.x;
    pseudo_pick_bin(ws + 2 * P + ((size_t)pass * P + j) * PSEUDO_BINS, ws + j, ws + P + j, pass, cut, true, incl);
}

// steps 1-3 for image blockIdx.x: the label before the opening and the saliency map the reference returns.  V pixels per thread
// (4: hw is a multiple of 4, the planes are 16-byte and the byte maps 4-byte aligned: one load per plane, one store per map).
template <int V>
__global__ __launch_bounds__(256) void psal_pixel_kernel(const float* __restrict__ cams, const uint8_t* __restrict__ present,
                                                         const uint8_t* sal, int C, int64_t hw, double bg_alpha,
                                                         const uint32_t* __restrict__ ws, uint8_t* __restrict__ label, uint8_t* sal_out) {
    __shared__ float thr[PSAL_MAX_CLASSES + 1];
    __shared__ int cls[PSAL_MAX_CLASSES + 1];
    __shared__ int K_s;
    const int64_t b = blockIdx.x;
    if (threadIdx.x == 0) {                              // the present classes of this image, ascending, and their thresholds
        int K = 0;
        for (int c = 0; c < C; ++c)
            if (present[b * C + c]) {
                cls[K] = c;
                thr[K] = __uint_as_float(ws[b * C + c]);
                ++K;
            }
        K_s = K;
    }
    __syncthreads();
    const int K = K_s;
    const float* img = cams + b * C * hw;
    const int64_t n = hw / V;
    for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.y * 256) {
        const int64_t pix = i * V;
        float m[V];                                      // max over the present planes and 0: values lie in [0, 1]
        int am[V], grab[V], s[V];
#pragma unroll
        for (int u = 0; u < V; ++u) m[u] = 0.f, am[u] = 0, grab[u] = 0;
        if (V == 4) {
            const uint32_t q = *reinterpret_cast<const uint32_t*>(sal + b * hw + pix);
#pragma unroll
            for (int u = 0; u < V; ++u) s[u] = (q >> (8 * u)) & 255u;
        } else {
            s[0] = sal[b * hw + pix];
        }
#pragma unroll 2
        for (int j = 0; j < K; ++j) {
            const int c1 = cls[j] + 1;
            const float t = thr[j];
            float v[V];
            if (V == 4) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(img + (int64_t)cls[j] * hw + pix);
#pragma unroll
                for (int u = 0; u < V; ++u) v[u] = q[u];
            } else {
                v[0] = img[(int64_t)cls[j] * hw + pix];
            }
#pragma unroll
            for (int u = 0; u < V; ++u) {
                if (v[u] > m[u]) {                       // first maximum wins (np.argmax, :223)
                    m[u] = v[u];
                    am[u] = c1;
                }
                if (!grab[u] && v[u] > t) grab[u] = c1;  // the lowest class above its threshold (:244-245)
            }
        }
        uint32_t o4 = 0, so4 = 0;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            int o, so;
            if (s[u] == 0) {                             // :230, then the grab
                o = grab[u];
                so = grab[u] ? 255 : 0;                  // :246
            } else {
                const float bg = (float)pow((double)(1.0f - m[u]), bg_alpha);        // :217
                o = m[u] > bg ? am[u] : 255;             // :223, :229: the background (it wins ties, being first) is "ignore"
                so = s[u];
            }
            o4 |= (uint32_t)o << (8 * u);
            so4 |= (uint32_t)so << (8 * u);
        }
        if (V == 4) {
            *reinterpret_cast<uint32_t*>(label + b * hw + pix) = o4;
            *reinterpret_cast<uint32_t*>(sal_out + b * hw + pix) = so4;
        } else {
            label[b * hw + pix] = (uint8_t)o4;
            sal_out[b * hw + pix] = (uint8_t)so4;
        }
    }
}

// bits [first, first + 64) of the 128-bit row (lo, hi) shifted right by j, 1 <= j < 64
__device__ __forceinline__ uint64_t psal_shr_lo(uint64_t lo, uint64_t hi, int j) { return (lo >> j) | (hi << (64 - j)); }

// O = dilate(erode(F)), F = src != 0, over the offsets -(k / 2) .. k - 1 - k / 2 on both axes in both passes.
// MASK: dst = src where O else 0 (:255); else dst = 255 where O else 0.
template <bool MASK>
__global__ __launch_bounds__(256) void psal_open_kernel(const uint8_t* __restrict__ src, int h, int w, int k, int tiles_x, int tiles_y,
                                                        uint8_t* __restrict__ dst) {
    __shared__ uint64_t A[PSAL_ROWS][2];                 // F, later the eroded tile
    __shared__ uint64_t R[PSAL_ROWS][2];                 // rows eroded, later rows dilated
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y;
    const int64_t b = t / tiles_y;
    const uint8_t* img = src + b * h * w;
    const int a = k / 2;
    const int x0 = tx * PSAL_TILE, y0 = ty * PSAL_TILE;
    const int rows_f = PSAL_TILE + 2 * (k - 1);          // F: rows y0 - 2a + r, bit i of a row is column x0 - 2a + i
    const int rows_e = PSAL_TILE + (k - 1);              // eroded: rows y0 - a + r, bit i is column x0 - a + i

    // F, bit-packed by ballot; outside the image 1 (ignored by the erosion's minimum).  A wave takes every fourth (row, word) and
    // issues PSAL_BATCH loads before the first ballot waits for one; columns beyond the halo are not read.
    for (int base = wave; base < 2 * rows_f; base += 4 * PSAL_BATCH) {
        uint8_t v[PSAL_BATCH];
#pragma unroll
        for (int u = 0; u < PSAL_BATCH; ++u) {
            const int idx = base + 4 * u;
            const int r = idx >> 1, wd = idx & 1;
            const int y = y0 - 2 * a + r, col = wd * 64 + lane, x = x0 - 2 * a + col;
            v[u] = 1;
            if (idx < 2 * rows_f && col < rows_f && y >= 0 && y < h && x >= 0 && x < w) v[u] = img[(int64_t)y * w + x];
        }
#pragma unroll
        for (int u = 0; u < PSAL_BATCH; ++u) {
            const int idx = base + 4 * u;
            if (idx < 2 * rows_f) {                      // the whole wave
                const uint64_t bits = __ballot(v[u] != 0);
                if (lane == 0) A[idx >> 1][idx & 1] = bits;
            }
        }
    }
    __syncthreads();
    // rows eroded: bit i = AND of F's bits i .. i + k - 1
    if (tid < rows_f) {
        const uint64_t lo = A[tid][0], hi = A[tid][1];
        uint64_t elo = lo, ehi = hi;
        for (int j = 1; j < k; ++j) {
            elo &= psal_shr_lo(lo, hi, j);
            ehi &= hi >> j;
        }
        R[tid][0] = elo;
        R[tid][1] = ehi;
    }
    __syncthreads();
    // columns eroded: row r = AND of rows r .. r + k - 1; then 0 outside the image (ignored by the dilation's maximum)
    if (tid < 2 * rows_e) {
        const int r = tid >> 1, wd = tid & 1;
        uint64_t e = ~0ull;
        for (int j = 0; j < k; ++j) e &= R[r + j][wd];
        const int y = y0 - a + r;
        const int xa = x0 - a + wd * 64;                 // column of bit 0
        const int first = xa < 0 ? -xa : 0, end = w - xa < 64 ? w - xa : 64;
        uint64_t inside = 0;
        if (y >= 0 && y < h && first < end) inside = (end - first == 64 ? ~0ull : ((1ull << (end - first)) - 1)) << first;
        A[r][wd] = e & inside;
    }
    __syncthreads();
    // rows dilated: bit i = OR of the eroded bits i .. i + k - 1; 64 bits are left: column x0 + i
    if (tid < rows_e) {
        const uint64_t lo = A[tid][0], hi = A[tid][1];
        uint64_t d = lo;
        for (int j = 1; j < k; ++j) d |= psal_shr_lo(lo, hi, j);
        R[tid][0] = d;
    }
    __syncthreads();
    // columns dilated, a wave per row: every lane forms the row's word and keeps its own bit
#pragma unroll 4
    for (int r = wave; r < PSAL_TILE; r += 4) {
        const int y = y0 + r, x = x0 + lane;
        uint64_t o = 0;
        for (int j = 0; j < k; ++j) o |= R[r + j][0];
        if (y < h && x < w) {
            const int64_t at = b * h * w + (int64_t)y * w + x;
            const bool on = (o >> lane) & 1;
            dst[at] = MASK ? (on ? src[at] : (uint8_t)0) : (on ? (uint8_t)255 : (uint8_t)0);
        }
    }
}

static int64_t psal_tiles(int32_t n) { return (n + PSAL_TILE - 1) / PSAL_TILE; }

static int psal_geometry(const char* who, int32_t B, int32_t h, int32_t w) {
    ACR_CHECK_ARG(B >= 1 && B <= PSAL_MAX_BATCH, "%s: B=%d outside 1..%d", who, B, PSAL_MAX_BATCH);
    ACR_CHECK_ARG(h >= 1 && w >= 1, "%s: bad geometry h=%d w=%d", who, h, w);
    ACR_CHECK_ARG((int64_t)h * w < (1ll << 31), "%s: image too large (%d x %d)", who, h, w);
    ACR_CHECK_ARG(B * psal_tiles(h) * psal_tiles(w) < (1ll << 31), "%s: %d images of %d x %d are too many tiles for one launch", who, B, h, w);
    return ACR_OK;
}

// the caller has checked the geometry
static void psal_open(bool mask, const uint8_t* src, int32_t B, int32_t h, int32_t w, int32_t k, uint8_t* dst, hipStream_t st) {
    const int tiles_x = (int)psal_tiles(w), tiles_y = (int)psal_tiles(h);
    const dim3 grid((unsigned)((int64_t)B * tiles_x * tiles_y));
    if (mask)
        hipLaunchKernelGGL(psal_open_kernel<true>, grid, dim3(256), 0, st, src, h, w, k, tiles_x, tiles_y, dst);
    else
        hipLaunchKernelGGL(psal_open_kernel<false>, grid, dim3(256), 0, st, src, h, w, k, tiles_x, tiles_y, dst);
}

extern "C" int64_t acr_sal_pseudo_ws_bytes(int32_t B, int32_t C, int32_t h, int32_t w) {
    if (B < 1 || B > PSAL_MAX_BATCH || C < 1 || C > PSAL_MAX_CLASSES || h < 1 || w < 1 || (int64_t)h * w >= (1ll << 31)) {
        acr_set_error("acr_sal_pseudo_ws_bytes: B=%d C=%d h=%d w=%d outside the supported range", B, C, h, w);
        return ACR_ERR_INVALID;
    }
    return (int64_t)(4 * psal_head_words((int64_t)B * C)) + (((int64_t)B * h * w + 15) & ~15ll);
}

extern "C" int acr_morph_open_u8(const uint8_t* src, int32_t B, int32_t h, int32_t w, int32_t k, uint8_t* dst, void* stream) {
    ACR_CHECK_ARG(src && dst, "acr_morph_open_u8: null pointer");
    ACR_CHECK_ARG(src != dst, "acr_morph_open_u8: dst must not be src (tiles read their neighbours' pixels)");
    const int rc = psal_geometry("acr_morph_open_u8", B, h, w);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(k >= 1 && k <= PSAL_MAX_K, "acr_morph_open_u8: k=%d outside 1..%d", k, PSAL_MAX_K);
    psal_open(false, src, B, h, w, k, dst, (hipStream_t)stream);
    return acr_check_launch("acr_morph_open_u8");
}

extern "C" int acr_sal_pseudo_compose(const float* cams, const uint8_t* present, int32_t B, int32_t C, int32_t h, int32_t w,
                                      const uint8_t* saliency, double bg_alpha, double cut, int32_t open_size, void* ws, int64_t ws_bytes,
                                      uint8_t* label, uint8_t* saliency_out, void* stream) {
    ACR_CHECK_ARG(cams && present && saliency && label && saliency_out, "acr_sal_pseudo_compose: null pointer");
    ACR_CHECK_ARG(label != saliency && label != saliency_out, "acr_sal_pseudo_compose: label must not share its buffer with a saliency map");
    const int rc = psal_geometry("acr_sal_pseudo_compose", B, h, w);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(C >= 1 && C <= PSAL_MAX_CLASSES, "acr_sal_pseudo_compose: C=%d outside 1..%d", C, PSAL_MAX_CLASSES);
    ACR_CHECK_ARG(bg_alpha > 0.0, "acr_sal_pseudo_compose: bg_alpha=%g <= 0", bg_alpha);
    ACR_CHECK_ARG(cut >= 0.0 && cut < 1.0, "acr_sal_pseudo_compose: cut=%g outside [0, 1)", cut);
    ACR_CHECK_ARG(open_size >= 0 && open_size <= PSAL_MAX_K, "acr_sal_pseudo_compose: open_size=%d outside 0..%d", open_size, PSAL_MAX_K);
    ACR_CHECK_WS("acr_sal_pseudo_compose", ws, 4, ws_bytes, acr_sal_pseudo_ws_bytes(B, C, h, w));
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)h * w, P = (int64_t)B * C;
    uint32_t* words = reinterpret_cast<uint32_t*>(ws);
    const int64_t head = (int64_t)psal_head_words(P);
    uint8_t* pre = reinterpret_cast<uint8_t*>(words + head);     // the label before the opening
    hipLaunchKernelGGL(psal_clear_kernel, dim3(pseudo_blocks(head)), dim3(256), 0, st, words, head);
    // four values / pixels per thread where the rows of four are aligned
    const bool vec = hw % 4 == 0 && ((uintptr_t)cams & 15) == 0 && (((uintptr_t)saliency | (uintptr_t)saliency_out | (uintptr_t)label) & 3) == 0;
    const unsigned blocks = pseudo_blocks(vec ? hw / 4 : hw);
    const dim3 hist_grid((unsigned)P, blocks < 64 ? blocks : 64);                     // B * C planes share the device
    for (int pass = 0; pass < PSEUDO_PASSES; ++pass) {
        if (vec)
            hipLaunchKernelGGL(psal_hist_kernel<4>, hist_grid, dim3(256), 0, st, cams, present, hw, P, pass, words);
        else
            hipLaunchKernelGGL(psal_hist_kernel<1>, hist_grid, dim3(256), 0, st, cams, present, hw, P, pass, words);
        hipLaunchKernelGGL(psal_pick_kernel, dim3((unsigned)P), dim3(256), 0, st, words, P, pass, cut);
    }
    uint8_t* first = open_size ? pre : label;
    if (vec)
        hipLaunchKernelGGL(psal_pixel_kernel<4>, dim3((unsigned)B, blocks), dim3(256), 0, st, cams, present, saliency, C, hw, bg_alpha,
                           (const uint32_t*)words, first, saliency_out);
    else
        hipLaunchKernelGGL(psal_pixel_kernel<1>, dim3((unsigned)B, blocks), dim3(256), 0, st, cams, present, saliency, C, hw, bg_alpha,
                           (const uint32_t*)words, first, saliency_out);
    if (open_size) psal_open(true, pre, B, h, w, open_size, label, st);
    return acr_check_launch("acr_sal_pseudo_compose");
}
