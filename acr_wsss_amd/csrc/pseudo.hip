// Pseudo-label composition from refined CAMs on the device (the reference's compute_seg_label_rrm, myTool.py:674-744: the label
// maps of the low- and high-alpha refinements :705-706, their combination :707-708,732, and the confidence rule :694-701,710-735
// with the line kept commented at :737).  Everything is per-pixel work on integers and comparisons, plus one exact order statistic
// per class: the output is a pure function of the inputs, bit-identical run to run.
//
// The order statistic (sort(S)[int(n * q)], :717-720) is a radix selection on the fp32 bit pattern -- the values of S are above
// cam_floor >= 0, and positive floats order as their unsigned bit patterns: four passes of eight bits, most significant first.
// A pass counts, for every class at once, the values that agree with the class's prefix so far in a 256-bin histogram per class
// (32-bit counters in LDS per workgroup, nonzero bins merged with integer adds into the caller's workspace); one small workgroup
// per class then picks the bin that holds the wanted rank and extends the prefix.  The first pass rides in the per-pixel kernel
// that also writes the combined label map, so uncertainty costs 1 + 3 + 4 + 1 further small launches, none of them data dependent.
#include "acr_common.h"
#include "pseudo_select.h"                   // the radix selection shared with pseudo_sal.hip

#define PSEUDO_MAX_LABELS ACR_PSEUDO_MAX_LABELS
#define PSEUDO_SEL_NONE 255              // sel map: the pixel is in no selection set and can never be sure
#define PSEUDO_SEL_BG 254                // sel map: M == 0 and bg > bg_sure (sure iff label 0 occurs in L_la)
// workspace, in 32-bit words: OCC (128: label l occurs in L_la) | PREFIX (128: bits of v per plane) | RANK (128) |
// HIST (4 passes, K planes, 256 bins) | then the sel map, one byte per pixel
#define PSEUDO_O_PREFIX 128
#define PSEUDO_O_RANK 256
#define PSEUDO_O_HIST 384

struct pseudo_classes {
    int32_t first_absent;                // 1 + the smallest class index without a plane, 0: every class has one
    uint32_t packed[(PSEUDO_MAX_LABELS - 1 + 3) / 4];     // label (class index + 1) of class plane j in byte j
};

static size_t pseudo_head_words(int K) { return PSEUDO_O_HIST + (size_t)PSEUDO_PASSES * K * PSEUDO_BINS; }

// np.argmax over the dense (C + 1)-plane array: label 0 holds m0, label classes[j] + 1 holds planes[j], every other label 0.0;
// the smallest label among the maxima wins.  Returns the label; *jb: the class plane that won, -1 if none did.
__device__ __forceinline__ int pseudo_argmax(float m0, const float* __restrict__ p, int64_t hw, int K, const uint8_t* label_of,
                                             int first_absent, int* jb_out, float* m_out) {
    float m = m0;
    int jb = -1;
    int j = 0;
    for (; j + 4 <= K; j += 4) {                         // four planes in flight; first maximum wins (strict >, ascending j)
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
    for (; j < K; ++j) {
        const float v = p[(int64_t)j * hw];
        if (v > m) {
            m = v;
            jb = j;
        }
    }
    int a = jb < 0 ? 0 : label_of[jb];
    // the zero plane of an absent class: it wins below 0 and, at exactly 0, when its label is the smaller one
    if (first_absent && (m < 0.f || (m == 0.f && first_absent < a))) {
        m = 0.f;
        a = first_absent;
        jb = -1;
    }
    *jb_out = jb;
    *m_out = m;
    return a;
}

__device__ __forceinline__ void pseudo_load_labels(const pseudo_classes& cls, uint32_t* labels) {
#pragma unroll
    for (int i = 0; i < (int)(sizeof(cls.packed) / 4); ++i)
        if ((int)threadIdx.x == i) labels[i] = cls.packed[i];
}

// step A for one score stack (K + 1, hw): one thread per pixel and pass of the grid-stride loop
__global__ __launch_bounds__(256) void pseudo_label_kernel(const float* __restrict__ scores, pseudo_classes cls, int K, int64_t hw,
                                                           uint8_t* __restrict__ out) {
    __shared__ uint32_t labels[sizeof(cls.packed) / 4];
    pseudo_load_labels(cls, labels);
    __syncthreads();
    const uint8_t* label_of = reinterpret_cast<const uint8_t*>(labels);
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < hw; pix += (int64_t)gridDim.x * 256) {
        int jb;
        float m;
        out[pix] = (uint8_t)pseudo_argmax(scores[pix], scores + hw + pix, hw, K, label_of, cls.first_absent, &jb, &m);
    }
}

struct pseudo_params {
    double bg_alpha;
    float cam_floor, bg_sure, crf_sure;
};

// Steps A and B per pixel, and with UNC what step C needs of it: out = the combined label, 255 already where the refined scores
// are unsure; sel = the class plane whose selection set S the pixel belongs to (or BG / NONE); OCC; and the first histogram pass.
template <bool UNC>
__global__ __launch_bounds__(256) void pseudo_pixel_kernel(const float* __restrict__ cams, const float* __restrict__ la,
                                                           const float* __restrict__ ha, pseudo_classes cls, int K, int64_t hw,
                                                           pseudo_params prm, uint32_t* __restrict__ ws, uint8_t* __restrict__ sel,
                                                           uint8_t* __restrict__ out) {
    extern __shared__ uint32_t hist[];                   // UNC: K * 256 counters
    __shared__ uint32_t labels[sizeof(cls.packed) / 4];
    __shared__ uint32_t occ[PSEUDO_MAX_LABELS];
    const int tid = threadIdx.x;
    pseudo_load_labels(cls, labels);
    if (UNC) {
        for (int i = tid; i < K * PSEUDO_BINS; i += 256) hist[i] = 0;
        if (tid < PSEUDO_MAX_LABELS) occ[tid] = 0;
    }
    __syncthreads();
    const uint8_t* label_of = reinterpret_cast<const uint8_t*>(labels);

    for (int64_t pix = (int64_t)blockIdx.x * 256 + tid; pix < hw; pix += (int64_t)gridDim.x * 256) {
        int jb;
        float mla, mha;
        const float ha0 = ha[pix];
        const int l_la = pseudo_argmax(la[pix], la + hw + pix, hw, K, label_of, cls.first_absent, &jb, &mla);
        const int l_ha = pseudo_argmax(ha0, ha + hw + pix, hw, K, label_of, cls.first_absent, &jb, &mha);
        int o = l_la == 0 ? 255 : l_la;                  // myTool.py:707-708
        if (l_ha == 0) o = 0;                            // :732
        if (UNC) {
            occ[l_la] = 1;                               // every writer stores the same value
            // max(ha[0], la[1..K]) < crf_sure (:733-734; the zero planes of absent classes cannot matter: crf_sure > 0)
            float top = ha0;
            for (int j = 0; j < K; ++j) top = fmaxf(top, la[(int64_t)(j + 1) * hw + pix]);
            if (top < prm.crf_sure) o = 255;
            // :694-701: bg = (1 - max cam)^bg_alpha over the dense planes, M = their argmax
            float m = cls.first_absent ? 0.f : -INFINITY;
            for (int j = 0; j < K; ++j) m = fmaxf(m, cams[(int64_t)j * hw + pix]);
            const float bg = (float)pow((double)(1.0f - m), prm.bg_alpha);
            float mm;
            const int M = pseudo_argmax(bg, cams + pix, hw, K, label_of, cls.first_absent, &jb, &mm);
            int s = PSEUDO_SEL_NONE;
            if (M == 0) {
                if (bg > prm.bg_sure) s = PSEUDO_SEL_BG; // :724-728
            } else if (jb >= 0 && mm > prm.cam_floor) {  // :714-717; an absent label's zero plane holds nothing above the floor
                s = jb;
                atomicAdd(&hist[jb * PSEUDO_BINS + (__float_as_uint(mm) >> 24)], 1u);
            }
            sel[pix] = (uint8_t)s;
        }
        out[pix] = (uint8_t)o;
    }
    if (UNC) {
        __syncthreads();
        pseudo_hist_merge(hist, ws + PSEUDO_O_HIST, K * PSEUDO_BINS);
        if (tid < PSEUDO_MAX_LABELS && occ[tid]) atomicOr(&ws[tid], 1u);
    }
}

// histogram pass 1..3: the byte at `shift` of every value of S that agrees with its plane's prefix above that byte
__global__ __launch_bounds__(256) void pseudo_hist_kernel(const float* __restrict__ cams, const uint8_t* __restrict__ sel, int K,
                                                          int64_t hw, int pass, uint32_t* __restrict__ ws) {
    extern __shared__ uint32_t hist[];
    const int tid = threadIdx.x;
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < K * PSEUDO_BINS; i += 256) hist[i] = 0;
    __syncthreads();
    for (int64_t pix = (int64_t)blockIdx.x * 256 + tid; pix < hw; pix += (int64_t)gridDim.x * 256) {
        const int s = sel[pix];
        if (s < K) {
            const uint32_t bits = __float_as_uint(cams[(int64_t)s * hw + pix]);
            if ((bits >> (shift + 8)) == (ws[PSEUDO_O_PREFIX + s] >> (shift + 8)))
                atomicAdd(&hist[s * PSEUDO_BINS + ((bits >> shift) & 255u)], 1u);
        }
    }
    __syncthreads();
    pseudo_hist_merge(hist, ws + PSEUDO_O_HIST + (size_t)pass * K * PSEUDO_BINS, K * PSEUDO_BINS);
}

// one workgroup per class plane, one thread per bin: the bin of this pass that holds the wanted rank.  Pass 0 knows n = |S| and
// sets the rank int(n * fg_quantile), the product in double (:719); an empty S gets v = +inf.
__global__ __launch_bounds__(256) void pseudo_pick_kernel(uint32_t* __restrict__ ws, int K, int pass, double fg_quantile) {
    __shared__ uint32_t incl[PSEUDO_BINS];
    const int j = blockIdx.x;
    pseudo_pick_bin(ws + PSEUDO_O_HIST + ((size_t)pass * K + j) * PSEUDO_BINS, ws + PSEUDO_O_PREFIX + j, ws + PSEUDO_O_RANK + j, pass,
                    fg_quantile, false, incl);
}

// :721-722,730,735,737: a pixel that is not sure becomes 255
__global__ __launch_bounds__(256) void pseudo_finish_kernel(const float* __restrict__ cams, const uint8_t* __restrict__ sel,
                                                            pseudo_classes cls, int K, int64_t hw, const uint32_t* __restrict__ ws,
                                                            uint8_t* __restrict__ out) {
    __shared__ uint32_t labels[sizeof(cls.packed) / 4];
    pseudo_load_labels(cls, labels);
    __syncthreads();
    const uint8_t* label_of = reinterpret_cast<const uint8_t*>(labels);
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < hw; pix += (int64_t)gridDim.x * 256) {
        const int s = sel[pix];
        bool sure = false;
        if (s < K)
            sure = ws[label_of[s]] && cams[(int64_t)s * hw + pix] > __uint_as_float(ws[PSEUDO_O_PREFIX + s]);
        else if (s == PSEUDO_SEL_BG)
            sure = ws[0] != 0;
        if (!sure) out[pix] = 255;
    }
}

// the head of the workspace (OCC, PREFIX, RANK, HIST) starts every call at zero: a kernel, so that a captured call holds kernel
// nodes only
__global__ __launch_bounds__(256) void pseudo_clear_kernel(uint32_t* __restrict__ ws, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) ws[i] = 0u;
}

// shared argument checks; fills cls
static int pseudo_classes_of(const char* who, const int32_t* classes, int32_t K, int32_t h, int32_t w, int32_t num_classes,
                             pseudo_classes* cls) {
    ACR_CHECK_ARG(classes, "%s: null pointer", who);
    ACR_CHECK_ARG(num_classes >= 1 && num_classes + 1 <= PSEUDO_MAX_LABELS, "%s: num_classes=%d outside 1..%d", who, num_classes,
                  PSEUDO_MAX_LABELS - 1);
    ACR_CHECK_ARG(K >= 1 && K <= num_classes, "%s: K=%d outside 1..num_classes=%d", who, K, num_classes);
    ACR_CHECK_ARG(h >= 1 && w >= 1, "%s: bad geometry h=%d w=%d", who, h, w);
    ACR_CHECK_ARG((int64_t)h * w < (1ll << 31), "%s: image too large (%d x %d)", who, h, w);
    for (size_t i = 0; i < sizeof(cls->packed) / 4; ++i) cls->packed[i] = 0;
    cls->first_absent = 0;
    for (int j = 0; j < K; ++j) {
        ACR_CHECK_ARG(classes[j] >= 0 && classes[j] < num_classes, "%s: classes[%d]=%d outside 0..%d", who, j, classes[j], num_classes - 1);
        ACR_CHECK_ARG(j == 0 || classes[j] > classes[j - 1], "%s: classes must be strictly ascending (classes[%d]=%d)", who, j, classes[j]);
        cls->packed[j >> 2] |= (uint32_t)(classes[j] + 1) << (8 * (j & 3));
    }
    if (K < num_classes) {                               // strictly ascending: the first j with classes[j] != j marks the gap
        int c = 0;
        while (c < K && classes[c] == c) ++c;
        cls->first_absent = c + 1;
    }
    return ACR_OK;
}

extern "C" int64_t acr_pseudo_ws_bytes(int32_t K, int32_t h, int32_t w) {
    if (K < 1 || K > PSEUDO_MAX_LABELS - 1 || h < 1 || w < 1 || (int64_t)h * w >= (1ll << 31)) {
        acr_set_error("acr_pseudo_ws_bytes: K=%d h=%d w=%d outside the supported range", K, h, w);
        return ACR_ERR_INVALID;
    }
    return (int64_t)(4 * pseudo_head_words(K)) + (((int64_t)h * w + 15) & ~15ll);
}

extern "C" int acr_pseudo_label_f32(const float* scores, const int32_t* classes, int32_t K, int32_t h, int32_t w, int32_t num_classes,
                                    uint8_t* out, void* stream) {
    ACR_CHECK_ARG(scores && out, "acr_pseudo_label_f32: null pointer");
    pseudo_classes cls;
    const int rc = pseudo_classes_of("acr_pseudo_label_f32", classes, K, h, w, num_classes, &cls);
    if (rc != ACR_OK) return rc;
    const int64_t hw = (int64_t)h * w;
    hipLaunchKernelGGL(pseudo_label_kernel, dim3(pseudo_blocks(hw)), dim3(256), 0, (hipStream_t)stream, scores, cls, K, hw, out);
    return acr_check_launch("acr_pseudo_label_f32");
}

extern "C" int acr_pseudo_compose(const float* cams, const int32_t* classes, int32_t K, const float* la, const float* ha, int32_t h,
                                  int32_t w, int32_t num_classes, int32_t ignore_uncertain, double bg_alpha, float cam_floor,
                                  double fg_quantile, float bg_sure, float crf_sure, void* ws, int64_t ws_bytes, uint8_t* out,
                                  void* stream) {
    ACR_CHECK_ARG(cams && la && ha && out, "acr_pseudo_compose: null pointer");
    pseudo_classes cls;
    const int rc = pseudo_classes_of("acr_pseudo_compose", classes, K, h, w, num_classes, &cls);
    if (rc != ACR_OK) return rc;
    const int64_t hw = (int64_t)h * w;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(pseudo_blocks(hw));
    pseudo_params prm = {bg_alpha, cam_floor, bg_sure, crf_sure};
    if (!ignore_uncertain) {
        hipLaunchKernelGGL(pseudo_pixel_kernel<false>, grid, dim3(256), 0, st, cams, la, ha, cls, K, hw, prm, (uint32_t*)nullptr,
                           (uint8_t*)nullptr, out);
        return acr_check_launch("acr_pseudo_compose");
    }
    ACR_CHECK_ARG(cam_floor >= 0.f, "acr_pseudo_compose: cam_floor=%g < 0", (double)cam_floor);
    ACR_CHECK_ARG(fg_quantile >= 0.0 && fg_quantile < 1.0, "acr_pseudo_compose: fg_quantile=%g outside [0, 1)", fg_quantile);
    ACR_CHECK_ARG(crf_sure > 0.f, "acr_pseudo_compose: crf_sure=%g <= 0", (double)crf_sure);
    ACR_CHECK_WS("acr_pseudo_compose", ws, 4, ws_bytes, acr_pseudo_ws_bytes(K, h, w));
    uint32_t* words = reinterpret_cast<uint32_t*>(ws);
    uint8_t* sel = reinterpret_cast<uint8_t*>(words + pseudo_head_words(K));
    const size_t lds = (size_t)K * PSEUDO_BINS * 4;      // at most 127 KB
    const int64_t head = (int64_t)pseudo_head_words(K);
    hipLaunchKernelGGL(pseudo_clear_kernel, dim3(pseudo_blocks(head)), dim3(256), 0, st, words, head);
    hipLaunchKernelGGL(pseudo_pixel_kernel<true>, grid, dim3(256), lds, st, cams, la, ha, cls, K, hw, prm, words, sel, out);
    for (int pass = 0; pass < PSEUDO_PASSES; ++pass) {
        if (pass)
            hipLaunchKernelGGL(pseudo_hist_kernel, grid, dim3(256), lds, st, cams, (const uint8_t*)sel, K, hw, pass, words);
        hipLaunchKernelGGL(pseudo_pick_kernel, dim3(K), dim3(256), 0, st, words, K, pass, fg_quantile);
    }
    hipLaunchKernelGGL(pseudo_finish_kernel, grid, dim3(256), 0, st, cams, (const uint8_t*)sel, cls, K, hw, (const uint32_t*)words, out);
    return acr_check_launch("acr_pseudo_compose");
}
