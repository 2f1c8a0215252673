// Pseudo-label segmentation loss on the device (the reference's compute_joint_loss, myTool.py:825-857): the bilinear upsampling of
// the segmentation logits to label size (:831), the two cross-entropies with ignore against the background-only and the
// foreground-only label (:845-855, tool/loss.py:21-33), the softmax probabilities the dense-energy term takes (:832-833), and the
// dot product of that term over the lattice filter (wrapper/bilateralfilter/bilateralfilter.cpp:42-55 feeds it).
//
// Mapping: ONE THREAD PER LABEL-SIZE PIXEL, the K classes walked in a loop, lanes along the contiguous second spatial axis.
// K = 21 or 81 values per pixel fill no wave evenly; a pixel per lane keeps all 64 lanes busy for any K, makes the softmax a loop
// in registers (no cross-lane step) and every load and store of a class plane a contiguous row segment.  The K upsampled logits of
// a pixel are kept in a private LDS column ([k][thread]: conflict free) so that the max, the sum and the probabilities each read
// them once and the source texels are fetched once.  The backward is a GATHER per low-resolution logit: a thread owns one
// (b, k, y, x), walks the label-size pixels whose footprint touches it in ascending order, recomputes p_k from the two saved row
// statistics (max, sum) and adds weight * d pred -- no scatter, no float atomics, bit-identical run to run.
// Every sum over pixels runs in double in a fixed order (thread, then an LDS tree, then the blocks in a finish kernel).
#include "acr_reduce.h"
#include "acr_resample.h"

#define SEGLOSS_MAX_K ACR_SEG_MAX_K
#define SEGLOSS_MAX_BLOCKS 256            // partial-sum workgroups per image (and of one energy dot)
#define SEGLOSS_MAX_B 65535
#define SEGLOSS_RED_BYTES (256 * (8 + 8 + 4 + 4))

struct segloss_part {                     // one workgroup's share of an image
    double sum_bg, sum_fg;
    int64_t n_bg, n_fg;
};

// sum the four per-thread numbers over the workgroup in a fixed order; the result is valid in thread 0
__device__ __forceinline__ void segloss_block_sum(void* smem, double& a, double& b, int& na, int& nb) {
    double* rd = reinterpret_cast<double*>(smem);
    int* ri = reinterpret_cast<int*>(rd + 512);
    const int tid = threadIdx.x;
    __syncthreads();                                     // the caller's use of smem is over
    rd[tid] = a;
    rd[256 + tid] = b;
    ri[tid] = na;
    ri[256 + tid] = nb;
    acr_tree_sum256(tid, [&](int i, int j) {
        rd[i] += rd[j];
        rd[256 + i] += rd[256 + j];
        ri[i] += ri[j];
        ri[256 + i] += ri[256 + j];
    });
    a = rd[0];
    b = rd[256];
    na = ri[0];
    nb = ri[256];
}

// forward: grid = B * nblk workgroups, workgroup (b, blk) strides over the pixels of image b
template <bool PROBS>
__global__ __launch_bounds__(256) void segloss_fwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ label, int K,
                                                          int h, int w, int W, int H, float sh, float sw, int nblk,
                                                          float* __restrict__ probs, float2* __restrict__ rowstat,
                                                          segloss_part* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char segloss_smem[];
    float* col = reinterpret_cast<float*>(segloss_smem) + threadIdx.x;      // pred_k of this thread's pixel at col[k * 256]
    const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
    const int64_t hw = (int64_t)h * w, WH = (int64_t)W * H;
    const float* lg = logits + (int64_t)b * K * hw;
    double sum_bg = 0.0, sum_fg = 0.0;
    int n_bg = 0, n_fg = 0;
    for (int64_t pix = (int64_t)blk * 256 + threadIdx.x; pix < WH; pix += (int64_t)nblk * 256) {
        const acr_taps t = acr_taps_of((int)(pix / H), (int)(pix % H), h, w, sh, sw);
        const int lab = label[(int64_t)b * WH + pix];
        float m = -INFINITY, xl = 0.f;
        for (int k = 0; k < K; ++k) {
            const float v = acr_interp(lg + (int64_t)k * hw, t);
            col[k * 256] = v;
            m = fmaxf(m, v);
            xl = k == lab ? v : xl;
        }
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(col[k * 256] - m);
        if (PROBS) {
            float* pp = probs + (int64_t)b * K * WH + pix;
            for (int k = 0; k < K; ++k) pp[(int64_t)k * WH] = expf(col[k * 256] - m) / s;
        }
        if (rowstat) rowstat[(int64_t)b * WH + pix] = make_float2(m, s);
        const float nll = (m - xl) + logf(s);            // -log p_label
        if (lab == 0) {
            sum_bg += (double)nll;
            ++n_bg;
        } else if (lab < K) {
            sum_fg += (double)nll;
            ++n_fg;
        }
    }
    segloss_block_sum(segloss_smem, sum_bg, sum_fg, n_bg, n_fg);
    if (threadIdx.x == 0) {
        segloss_part p = {sum_bg, sum_fg, (int64_t)n_bg, (int64_t)n_fg};
        part[blockIdx.x] = p;
    }
}

// one workgroup: the blocks of every image in a fixed order, then the batch.  sums (B, 2) fp32, counts (B + 1, 2) int64 (row B:
// the batch totals), loss (3) = celoss, bg, fg
__global__ __launch_bounds__(256) void segloss_finish_kernel(const segloss_part* __restrict__ part, int B, int nblk, int batch_average,
                                                             float* __restrict__ sums, int64_t* __restrict__ counts,
                                                             float* __restrict__ loss) {
    __shared__ double rd[512];
    __shared__ int64_t rn[512];
    const int tid = threadIdx.x;
    double tot_bg = 0.0, tot_fg = 0.0;
    int64_t cnt_bg = 0, cnt_fg = 0;
    for (int b = 0; b < B; ++b) {
        __syncthreads();
        if (tid < nblk) {
            const segloss_part p = part[(int64_t)b * nblk + tid];
            rd[tid] = p.sum_bg;
            rd[256 + tid] = p.sum_fg;
            rn[tid] = p.n_bg;
            rn[256 + tid] = p.n_fg;
        } else {
            rd[tid] = rd[256 + tid] = 0.0;
            rn[tid] = rn[256 + tid] = 0;
        }
        acr_tree_sum256(tid, [&](int i, int j) {
            rd[i] += rd[j];
            rd[256 + i] += rd[256 + j];
            rn[i] += rn[j];
            rn[256 + i] += rn[256 + j];
        });
        if (tid == 0) {
            sums[2 * b] = (float)rd[0];
            sums[2 * b + 1] = (float)rd[256];
            counts[2 * b] = rn[0];
            counts[2 * b + 1] = rn[256];
            tot_bg += rd[0];
            tot_fg += rd[256];
            cnt_bg += rn[0];
            cnt_fg += rn[256];
        }
    }
    if (tid == 0) {
        counts[2 * B] = cnt_bg;
        counts[2 * B + 1] = cnt_fg;
        double bg = tot_bg / (double)cnt_bg, fg = tot_fg / (double)cnt_fg;      // a count of 0: 0 / 0 = NaN, as torch's mean gives
        if (batch_average) {
            bg /= (double)B;
            fg /= (double)B;
        }
        const float bgf = (float)bg, fgf = (float)fg;
        loss[0] = bgf + fgf;
        loss[1] = bgf;
        loss[2] = fgf;
    }
}

// backward, d_probs path: dot[b][pix] = sum_k probs[b][k][pix] * d_probs[b][k][pix], one thread per pixel
__global__ __launch_bounds__(256) void segloss_pdot_kernel(const float* __restrict__ probs, const float* __restrict__ d_probs, int K,
                                                           int64_t WH, int64_t total, float* __restrict__ dot) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / WH, pix = i % WH;
        const float* p = probs + b * K * WH + pix;
        const float* d = d_probs + b * K * WH + pix;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc += (double)p[(int64_t)k * WH] * (double)d[(int64_t)k * WH];
        dot[i] = (float)acc;
    }
}

// the gather range of acr_resample.h for the half-pixel rule: the estimate inverts it, the first tap is clamped like acr_taps_of's
__device__ __forceinline__ int segloss_first_dst(int t, int n_out, int n_in, float scale, float inv) {
    return acr_first_dst(
        t, n_out, n_in, [&](int tap) { return ((float)tap + 0.5f) * inv - 0.5f; },
        [&](int d) { return min((int)acr_src_half_pixel(scale, d), n_in - 1); });
}

// backward: one thread per low-resolution logit (b, k, y, x), lanes along x.  g (3): the gradients of celoss, bg, fg.
__global__ __launch_bounds__(256) void segloss_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ label,
                                                          const float2* __restrict__ rowstat, const int64_t* __restrict__ counts,
                                                          const float* __restrict__ g, const float* __restrict__ d_probs,
                                                          const float* __restrict__ dot, int B, int K, int h, int w, int W, int H,
                                                          float sh, float sw, float ish, float isw, int batch_average,
                                                          float* __restrict__ d_logits) {
    const int64_t hw = (int64_t)h * w, WH = (int64_t)W * H;
    const int64_t total = (int64_t)B * K * hw;
    float c_bg = g[0] + g[1], c_fg = g[0] + g[2];
    if (batch_average) {
        c_bg /= (float)B;
        c_fg /= (float)B;
    }
    c_bg /= (float)counts[2 * B];                        // a count of 0: never used, no pixel carries that label
    c_fg /= (float)counts[2 * B + 1];
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int x = (int)(idx % w), y = (int)((idx / w) % h);
        const int k = (int)((idx / hw) % K), b = (int)(idx / (hw * K));
        const float* plane = logits + ((int64_t)b * K + k) * hw;
        const int Ya = segloss_first_dst(y - 1, W, h, sh, ish), Yb = segloss_first_dst(y + 1, W, h, sh, ish);
        const int Xa = segloss_first_dst(x - 1, H, w, sw, isw), Xb = segloss_first_dst(x + 1, H, w, sw, isw);
        double acc = 0.0;
        for (int Y = Ya; Y < Yb; ++Y) {
            for (int X = Xa; X < Xb; ++X) {
                const acr_taps t = acr_taps_of(Y, X, h, w, sh, sw);
                const float wy = (t.y0 == y ? t.hy : 0.f) + (t.y1 == y ? t.ly : 0.f);
                const float wx = (t.x0 == x ? t.hx : 0.f) + (t.x1 == x ? t.lx : 0.f);
                const int64_t pix = (int64_t)Y * H + X;
                const int lab = label[(int64_t)b * WH + pix];
                const float2 ms = rowstat[(int64_t)b * WH + pix];
                const float p = expf(acr_interp(plane, t) - ms.x) / ms.y;
                float dpred = 0.f;
                if (lab == 0)
                    dpred = c_bg * (p - (k == 0 ? 1.f : 0.f));
                else if (lab < K)
                    dpred = c_fg * (p - (k == lab ? 1.f : 0.f));
                if (d_probs) dpred += p * (d_probs[((int64_t)b * K + k) * WH + pix] - dot[(int64_t)b * WH + pix]);
                acc += (double)wy * (double)wx * (double)dpred;
            }
        }
        d_logits[idx] = (float)acc;
    }
}

// dense energy: part[blk] = sum over the workgroup's elements of s * as (double); grad = scale * as when asked for
__global__ __launch_bounds__(256) void energy_dot_kernel(const float* __restrict__ s, const float* __restrict__ as, int64_t count,
                                                         float scale, float* __restrict__ grad, double* __restrict__ part) {
    __shared__ double rd[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < count; i += (int64_t)gridDim.x * 256) {
        const float a = as[i];
        acc += (double)s[i] * (double)a;
        if (grad) grad[i] = scale * a;
    }
    rd[tid] = acc;
    acr_tree_sum256(tid, [&](int i, int j) { rd[i] += rd[j]; });
    if (tid == 0) part[blockIdx.x] = rd[0];
}

__global__ __launch_bounds__(256) void energy_finish_kernel(const double* __restrict__ part, int nblk, float* __restrict__ out) {
    __shared__ double rd[256];
    const int tid = threadIdx.x;
    rd[tid] = tid < nblk ? part[tid] : 0.0;
    acr_tree_sum256(tid, [&](int i, int j) { rd[i] += rd[j]; });
    if (tid == 0) out[0] = (float)rd[0];
}

static int segloss_nblk(int64_t WH) {
    const int64_t n = (WH + 255) / 256;
    return (int)(n < SEGLOSS_MAX_BLOCKS ? n : SEGLOSS_MAX_BLOCKS);
}

static int segloss_check(const char* who, int32_t B, int32_t K, int32_t h, int32_t w, int32_t W, int32_t H) {
    ACR_CHECK_ARG(B >= 1 && B <= SEGLOSS_MAX_B, "%s: B=%d outside 1..%d", who, B, SEGLOSS_MAX_B);
    ACR_CHECK_ARG(K >= 2 && K <= SEGLOSS_MAX_K, "%s: K=%d outside 2..%d", who, K, SEGLOSS_MAX_K);
    ACR_CHECK_ARG(h >= 1 && w >= 1 && h <= W && w <= H, "%s: logits %d x %d must be no larger than the label %d x %d", who, h, w, W, H);
    ACR_CHECK_ARG((int64_t)W * H < (1ll << 31), "%s: label too large (%d x %d)", who, W, H);
    return ACR_OK;
}

static size_t segloss_part_bytes(int32_t B, int32_t W, int32_t H) {
    return (size_t)B * segloss_nblk((int64_t)W * H) * sizeof(segloss_part);
}

extern "C" int64_t acr_segloss_ws_bytes(int32_t B, int32_t K, int32_t h, int32_t w, int32_t W, int32_t H) {
    if (segloss_check("acr_segloss_ws_bytes", B, K, h, w, W, H) != ACR_OK) return ACR_ERR_INVALID;
    return (int64_t)segloss_part_bytes(B, W, H) + 4 * (int64_t)B * W * H;
}

extern "C" int acr_segloss_fwd(const float* logits, const uint8_t* label, int32_t B, int32_t K, int32_t h, int32_t w, int32_t W,
                               int32_t H, int32_t batch_average, void* ws, int64_t ws_bytes, float* probs, float* rowstat,
                               float* sums, int64_t* counts, float* loss, void* stream) {
    const int rc = segloss_check("acr_segloss_fwd", B, K, h, w, W, H);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(logits && label && sums && counts && loss, "acr_segloss_fwd: null pointer");
    ACR_CHECK_WS("acr_segloss_fwd", ws, 8, ws_bytes, acr_segloss_ws_bytes(B, K, h, w, W, H));
    ACR_CHECK_ARG(!rowstat || ((uintptr_t)rowstat & 7) == 0, "acr_segloss_fwd: rowstat not aligned to 8 bytes");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = segloss_nblk((int64_t)W * H);
    const float sh = (float)h / (float)W, sw = (float)w / (float)H;
    size_t lds = (size_t)K * 256 * 4;
    if (lds < SEGLOSS_RED_BYTES) lds = SEGLOSS_RED_BYTES;
    segloss_part* part = reinterpret_cast<segloss_part*>(ws);
    if (probs)
        hipLaunchKernelGGL(segloss_fwd_kernel<true>, dim3((unsigned)B * nblk), dim3(256), lds, st, logits, label, K, h, w, W, H, sh, sw,
                           nblk, probs, reinterpret_cast<float2*>(rowstat), part);
    else
        hipLaunchKernelGGL(segloss_fwd_kernel<false>, dim3((unsigned)B * nblk), dim3(256), lds, st, logits, label, K, h, w, W, H, sh, sw,
                           nblk, (float*)nullptr, reinterpret_cast<float2*>(rowstat), part);
    hipLaunchKernelGGL(segloss_finish_kernel, dim3(1), dim3(256), 0, st, (const segloss_part*)part, B, nblk, batch_average ? 1 : 0, sums,
                       counts, loss);
    return acr_check_launch("acr_segloss_fwd");
}

extern "C" int acr_segloss_bwd(const float* logits, const uint8_t* label, const float* rowstat, const int64_t* counts, const float* g,
                               const float* probs, const float* d_probs, int32_t B, int32_t K, int32_t h, int32_t w, int32_t W,
                               int32_t H, int32_t batch_average, void* ws, int64_t ws_bytes, float* d_logits, void* stream) {
    const int rc = segloss_check("acr_segloss_bwd", B, K, h, w, W, H);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(logits && label && rowstat && counts && g && d_logits, "acr_segloss_bwd: null pointer");
    ACR_CHECK_ARG(((uintptr_t)rowstat & 7) == 0, "acr_segloss_bwd: rowstat not aligned to 8 bytes");
    ACR_CHECK_ARG(!d_probs || probs, "acr_segloss_bwd: d_probs given without the probs the forward wrote");
    hipStream_t st = (hipStream_t)stream;
    const int64_t WH = (int64_t)W * H;
    float* dot = nullptr;
    if (d_probs) {
        ACR_CHECK_WS("acr_segloss_bwd", ws, 8, ws_bytes, acr_segloss_ws_bytes(B, K, h, w, W, H));
        dot = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(ws) + segloss_part_bytes(B, W, H));
        int64_t nb = (B * WH + 255) / 256;
        if (nb > 2048) nb = 2048;
        hipLaunchKernelGGL(segloss_pdot_kernel, dim3((unsigned)nb), dim3(256), 0, st, probs, d_probs, K, WH, B * WH, dot);
    }
    const float sh = (float)h / (float)W, sw = (float)w / (float)H;
    const float ish = (float)W / (float)h, isw = (float)H / (float)w;
    int64_t nb = ((int64_t)B * K * h * w + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(segloss_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, st, logits, label, reinterpret_cast<const float2*>(rowstat),
                       counts, g, d_probs, (const float*)dot, B, K, h, w, W, H, sh, sw, ish, isw, batch_average ? 1 : 0, d_logits);
    return acr_check_launch("acr_segloss_bwd");
}

extern "C" int acr_dense_energy_dot(const float* s, const float* as, int64_t count, float grad_scale, float* grad, void* ws,
                                    int64_t ws_bytes, float* out, void* stream) {
    ACR_CHECK_ARG(s && as && out, "acr_dense_energy_dot: null pointer");
    ACR_CHECK_ARG(count >= 1, "acr_dense_energy_dot: count=%lld < 1", (long long)count);
    ACR_CHECK_WS("acr_dense_energy_dot", ws, 8, ws_bytes, ACR_DENSE_ENERGY_WS_BYTES);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = segloss_nblk(count);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(energy_dot_kernel, dim3(nblk), dim3(256), 0, st, s, as, count, grad_scale, grad, part);
    hipLaunchKernelGGL(energy_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nblk, out);
    return acr_check_launch("acr_dense_energy_dot");
}
