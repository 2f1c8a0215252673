// CAM evaluation on the device (the counters of the reference's evaluation.py:19-52 for every background threshold at once, and the
// confusion matrix of its --type png mode / tool/metrics.py:36-41): one streaming pass per image that turns each pixel into one
// histogram bin and counts bins in integers.  Integer sums do not depend on their order, so results are bit-identical run to run.
//
// Counting: a workgroup keeps the whole histogram as 32-bit counters in LDS and adds its nonzero bins to the 64-bit global
// counters once, at its end.  CAMs are mostly exact zeros (threshold bin 0) and labels form blobs, so the 64 pixels of a wave
// mostly fall into one or two bins: the wave first groups its lanes by bin (EVAL_PEEL rounds of "take the first open lane's
// bin, ballot who shares it") and issues ONE add per group; lanes still open after those rounds add on their own, which bounds
// the cost on inputs without structure.  A histogram too large for LDS is counted the same way straight into the global counters.
#include "acr_common.h"

#define EVAL_MAX_CLS ACR_EVAL_MAX_CLS
#define EVAL_MAX_NT ACR_EVAL_MAX_NT
#define EVAL_PEEL 4
#define EVAL_LDS_BYTES (128 * 1024)      // histograms up to this size live in LDS
#define EVAL_MAX_BLOCKS 512

struct eval_classes {
    int32_t first_absent;                // 1 + the smallest class index without a plane, 0: every class has one
    uint32_t packed[(EVAL_MAX_CLS - 1 + 3) / 4];      // label (class index + 1) of plane j in byte j
};

template <bool LDS>
__device__ __forceinline__ void eval_add(uint32_t* hist, unsigned long long* raw, int idx, uint32_t v) {
    if (LDS)
        atomicAdd(&hist[idx], v);
    else
        atomicAdd(&raw[idx], (unsigned long long)v);
}

// One add per group of lanes that share `key`, for the first EVAL_PEEL groups of the wave; the rest add alone.  `open`: the lane
// takes part.  f1 / f2: per-lane flags counted into bins i1 / i2 of the group's first lane (i1 = i2 = -1: no such bins).
// Must be reached by all lanes of the wave.
template <bool LDS>
__device__ __forceinline__ void eval_count(uint32_t* hist, unsigned long long* raw, int lane, bool open, int key, bool f1, int i1,
                                           bool f2, int i2) {
    unsigned long long rest = __ballot(open);
    for (int r = 0; r < EVAL_PEEL && rest; ++r) {
        const int leader = __ffsll((long long)rest) - 1;
        const int k = __shfl(key, leader);
        const bool mine = ((rest >> lane) & 1) && key == k;
        const unsigned long long grp = __ballot(mine);
        const unsigned long long m1 = __ballot(mine && f1), m2 = __ballot(mine && f2);
        if (lane == leader) {
            eval_add<LDS>(hist, raw, key, (uint32_t)__popcll(grp));
            if (m1) eval_add<LDS>(hist, raw, i1, (uint32_t)__popcll(m1));
            if (m2) eval_add<LDS>(hist, raw, i2, (uint32_t)__popcll(m2));
        }
        rest &= ~grp;
    }
    if ((rest >> lane) & 1) {
        eval_add<LDS>(hist, raw, key, 1u);
        if (f1) eval_add<LDS>(hist, raw, i1, 1u);
        if (f2) eval_add<LDS>(hist, raw, i2, 1u);
    }
}

template <bool LDS>
__device__ __forceinline__ void eval_flush(const uint32_t* hist, unsigned long long* raw, int total) {
    if (!LDS) return;
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += 256) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(&raw[i], (unsigned long long)v);
    }
}

// raw = FG (nt + 1, num_cls) | HIT (nt + 1, num_cls) | BG (nt + 1) | T (num_cls) | NVALID; one thread per pixel and pass of the
// grid-stride loop, consecutive lanes on consecutive pixels of every plane (coalesced 256-byte rows).
template <bool LDS>
__global__ __launch_bounds__(256) void eval_sweep_kernel(const float* __restrict__ cams, eval_classes cls, int n,
                                                         const uint8_t* __restrict__ gt, int64_t hw,
                                                         const float* __restrict__ thresholds, int nt, int num_cls,
                                                         unsigned long long* __restrict__ raw) {
    extern __shared__ uint32_t hist[];
    __shared__ float th[EVAL_MAX_NT];
    __shared__ uint32_t labels[sizeof(cls.packed) / 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nfg = (nt + 1) * num_cls;
    const int o_hit = nfg, o_bg = 2 * nfg, o_t = o_bg + nt + 1, o_nv = o_t + num_cls, total = o_nv + 1;
    for (int i = tid; i < nt; i += 256) th[i] = thresholds[i];
#pragma unroll
    for (int i = 0; i < (int)(sizeof(cls.packed) / 4); ++i)
        if (tid == i) labels[i] = cls.packed[i];
    if (LDS)
        for (int i = tid; i < total; i += 256) hist[i] = 0;
    __syncthreads();
    const uint8_t* label_of = reinterpret_cast<const uint8_t*>(labels);

    for (int64_t base = (int64_t)blockIdx.x * 256; base < hw; base += (int64_t)gridDim.x * 256) {     // wave-uniform
        const int64_t pix = base + tid;
        bool valid = false, hit = false;
        int g = 0, kfg = 0, key = 0;
        if (pix < hw) {
            g = gt[pix];
            valid = g < num_cls;                         // 255 = ignore; labels in num_cls..254 are ignored like it
        }
        if (valid) {
            const float* p = cams + pix;
            float m = -INFINITY;
            int jb = 0;
            int j = 0;
            for (; j + 4 <= n; j += 4) {                 // four planes in flight; first maximum wins (strict >, ascending j)
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = p[(int64_t)(j + u) * hw];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (v[u] > m) {
                        m = v[u];
                        jb = j + u;
                    }
            }
            for (; j < n; ++j) {
                const float v = p[(int64_t)j * hw];
                if (v > m) {
                    m = v;
                    jb = j;
                }
            }
            int a = label_of[jb];
            // the zero plane of an absent class: it wins below 0 and, at exactly 0, when its index is the smaller one
            if (cls.first_absent && (m < 0.f || (m == 0.f && cls.first_absent < a))) {
                m = 0.f;
                a = cls.first_absent;
            }
            int lo = 0, hi = nt;                         // kfg = #{k : th[k] < m}, th ascending
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (th[mid] < m)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            kfg = lo;
            key = kfg * num_cls + a;
            hit = a == g;
        }
        eval_count<LDS>(hist, raw, lane, valid, key, hit, o_hit + key, g == 0, o_bg + kfg);          // FG, HIT, BG
        eval_count<LDS>(hist, raw, lane, valid, o_t + g, true, o_nv, false, -1);                     // T, NVALID
    }
    eval_flush<LDS>(hist, raw, total);
}

// TP / P of every threshold from the raw histograms, one workgroup: column c >= 1 is a suffix sum over the threshold bins, column
// 0 (background) follows from BG's prefix sum and from NVALID minus the foreground predictions.
__global__ __launch_bounds__(256) void eval_finish_kernel(const long long* __restrict__ raw, int nt, int num_cls,
                                                          long long* __restrict__ TP, long long* __restrict__ P) {
    __shared__ long long rowsum[EVAL_MAX_NT + 1];
    const int tid = threadIdx.x;
    const int nfg = (nt + 1) * num_cls;
    const long long *FG = raw, *HIT = raw + nfg, *BG = raw + 2 * nfg;
    const long long nvalid = raw[2 * nfg + nt + 1 + num_cls];
    for (int j = tid; j <= nt; j += 256) {
        long long s = 0;
        for (int c = 1; c < num_cls; ++c) s += FG[j * num_cls + c];
        rowsum[j] = s;
    }
    __syncthreads();
    if (tid >= 1 && tid < num_cls) {
        long long p = 0, tp = 0;
        for (int k = nt - 1; k >= 0; --k) {
            p += FG[(k + 1) * num_cls + tid];
            tp += HIT[(k + 1) * num_cls + tid];
            P[k * num_cls + tid] = p;
            TP[k * num_cls + tid] = tp;
        }
    } else if (tid == 0) {
        long long s = 0;
        for (int k = nt - 1; k >= 0; --k) {
            s += rowsum[k + 1];
            P[k * num_cls] = nvalid - s;
        }
        long long b = 0;
        for (int k = 0; k < nt; ++k) {
            b += BG[k];
            TP[k * num_cls] = b;
        }
    }
}

// conf[gt][min(pred, num_cls)] += 1 for gt < num_cls; the matrix (at most 128 x 129 counters, 65 KB) always fits in LDS
__global__ __launch_bounds__(256) void eval_confusion_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                             int64_t n_pixels, int num_cls, unsigned long long* __restrict__ conf) {
    extern __shared__ uint32_t hist[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int total = num_cls * (num_cls + 1);
    for (int i = tid; i < total; i += 256) hist[i] = 0;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n_pixels; base += (int64_t)gridDim.x * 256) {  // wave-uniform
        const int64_t pix = base + tid;
        bool valid = false;
        int key = 0;
        if (pix < n_pixels) {
            const int g = gt[pix];
            valid = g < num_cls;
            key = g * (num_cls + 1) + min((int)pred[pix], num_cls);
        }
        eval_count<true>(hist, conf, lane, valid, key, false, -1, false, -1);
    }
    eval_flush<true>(hist, conf, total);
}

static unsigned eval_blocks(int64_t pixels) {
    const int64_t b = (pixels + 255) / 256;
    return (unsigned)(b < EVAL_MAX_BLOCKS ? b : EVAL_MAX_BLOCKS);
}

extern "C" int acr_eval_sweep_f32(const float* cams, const int32_t* classes, int32_t n, const uint8_t* gt, int32_t h, int32_t w,
                                  const float* thresholds, int32_t nt, int32_t num_cls, int64_t* raw, void* stream) {
    ACR_CHECK_ARG(cams && classes && gt && thresholds && raw, "acr_eval_sweep_f32: null pointer");
    ACR_CHECK_ARG(num_cls >= 2 && num_cls <= EVAL_MAX_CLS, "acr_eval_sweep_f32: num_cls=%d outside 2..%d", num_cls, EVAL_MAX_CLS);
    ACR_CHECK_ARG(n >= 1 && n <= num_cls - 1, "acr_eval_sweep_f32: n=%d outside 1..num_cls-1=%d", n, num_cls - 1);
    ACR_CHECK_ARG(nt >= 1 && nt <= EVAL_MAX_NT, "acr_eval_sweep_f32: nt=%d outside 1..%d", nt, EVAL_MAX_NT);
    ACR_CHECK_ARG(h >= 1 && w >= 1, "acr_eval_sweep_f32: bad geometry h=%d w=%d", h, w);
    ACR_CHECK_ARG((int64_t)h * w < (1ll << 31), "acr_eval_sweep_f32: image too large (%d x %d)", h, w);
    eval_classes cls;
    for (size_t i = 0; i < sizeof(cls.packed) / 4; ++i) cls.packed[i] = 0;
    cls.first_absent = 0;
    for (int j = 0; j < n; ++j) {
        ACR_CHECK_ARG(classes[j] >= 0 && classes[j] < num_cls - 1, "acr_eval_sweep_f32: classes[%d]=%d outside 0..%d", j, classes[j],
                      num_cls - 2);
        ACR_CHECK_ARG(j == 0 || classes[j] > classes[j - 1], "acr_eval_sweep_f32: classes must be strictly ascending (classes[%d]=%d)", j,
                      classes[j]);
        cls.packed[j >> 2] |= (uint32_t)(classes[j] + 1) << (8 * (j & 3));
    }
    if (n < num_cls - 1) {                               // strictly ascending: the first j with classes[j] != j marks the gap
        int c = 0;
        while (c < n && classes[c] == c) ++c;
        cls.first_absent = c + 1;
    }
    const size_t words = 2 * (size_t)(nt + 1) * num_cls + (nt + 1) + num_cls + 1;
    const dim3 grid(eval_blocks((int64_t)h * w));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(raw);
    if (words * 4 <= EVAL_LDS_BYTES)
        hipLaunchKernelGGL(eval_sweep_kernel<true>, grid, dim3(256), words * 4, st, cams, cls, n, gt, (int64_t)h * w, thresholds, nt,
                           num_cls, out);
    else
        hipLaunchKernelGGL(eval_sweep_kernel<false>, grid, dim3(256), 0, st, cams, cls, n, gt, (int64_t)h * w, thresholds, nt, num_cls,
                           out);
    return acr_check_launch("acr_eval_sweep_f32");
}

extern "C" int acr_eval_sweep_finish(const int64_t* raw, int32_t nt, int32_t num_cls, int64_t* TP, int64_t* P, void* stream) {
    ACR_CHECK_ARG(raw && TP && P, "acr_eval_sweep_finish: null pointer");
    ACR_CHECK_ARG(num_cls >= 2 && num_cls <= EVAL_MAX_CLS, "acr_eval_sweep_finish: num_cls=%d outside 2..%d", num_cls, EVAL_MAX_CLS);
    ACR_CHECK_ARG(nt >= 1 && nt <= EVAL_MAX_NT, "acr_eval_sweep_finish: nt=%d outside 1..%d", nt, EVAL_MAX_NT);
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(raw), nt,
                       num_cls, reinterpret_cast<long long*>(TP), reinterpret_cast<long long*>(P));
    return acr_check_launch("acr_eval_sweep_finish");
}

extern "C" int acr_eval_confusion_u8(const uint8_t* pred, const uint8_t* gt, int64_t n_pixels, int32_t num_cls, int64_t* conf,
                                     void* stream) {
    ACR_CHECK_ARG(pred && gt && conf, "acr_eval_confusion_u8: null pointer");
    ACR_CHECK_ARG(num_cls >= 1 && num_cls <= EVAL_MAX_CLS, "acr_eval_confusion_u8: num_cls=%d outside 1..%d", num_cls, EVAL_MAX_CLS);
    ACR_CHECK_ARG(n_pixels >= 1, "acr_eval_confusion_u8: n_pixels=%lld < 1", (long long)n_pixels);
    const size_t bytes = 4 * (size_t)num_cls * (num_cls + 1);
    const dim3 grid(eval_blocks(n_pixels));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(conf);
    hipLaunchKernelGGL(eval_confusion_kernel, grid, dim3(256), bytes, st, pred, gt, n_pixels, num_cls, out);
    return acr_check_launch("acr_eval_confusion_u8");
}
