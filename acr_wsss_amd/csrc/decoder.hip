// DPT decoder kernels (the reference's fusion blocks, DPT/blocks.py:277-413, and its head, DPT/DPT.py:376-383): BatchNorm2d with
// batch or running statistics, an optional ReLU and up to two residual addends in the same pass (blocks.py:312-343,402), its
// backward, the x2 bilinear upsampling with align_corners=True (blocks.py:407-409) and its backward, and the leading ReLU of a
// residual unit (blocks.py:330).  NCHW contiguous tensors, stored as fp32 or as bf16: every kernel that touches a tensor is a
// template on the storage type T with the SAME assignment of values to lanes (a lane takes 4 consecutive values: a 16-byte load of
// fp32, an 8-byte load of bf16), all arithmetic after the load in fp32 / double as before, and the result rounded to T on the store.
// So the double sums of the two instantiations add the same numbers in the same order, and a bf16 output is the fp32 kernel's output
// rounded to nearest even (double -> fp32 -> bf16, include/acr_hip.h).  "float" / "16-byte vector" below read "T" / "4 values".
//
// Mapping of the norm: a channel's data are N separate rows of H*W floats.  A launch is C * S workgroups, workgroup (c, s) owning
// slab s of channel c: a contiguous range of the channel's N*H*W values in (n, i) order, so a slab is a few whole rows (small
// levels) or a piece of one (large levels).  Inside a slab a wave takes a row when there are at least four, otherwise all 256
// threads share a row; a row piece is walked as an unaligned head of at most 3 floats, 16-byte vectors, and a tail of at most 3 --
// nothing outside the piece is touched.  Every tensor of a call has the same shape and a 16-byte aligned base, so one head / tail
// split serves all of them.  Sums: a thread adds its values in double in a fixed order, an LDS tree adds the threads, a finish
// kernel adds the slabs in ascending order.  No atomics; bit-identical run to run.  The variance is the shifted sum
// (sum d^2 - (sum d)^2 / n) / n with d = x - x[first value of the channel] in double: a large mean costs nothing.
// The normalisation itself is one double FMA per value, y = fp32(a_c * x + b_c (+ r1 + r2)), rounded once.
// The ReLU mask of the backward is recomputed from the saved output (y > 0); no mask bytes are kept.
//
// Cross-rank statistics (nn.SyncBatchNorm): each direction is slab sums -> a per-channel kernel that writes a small double row
// ((C, 3) count / mean / M2 forward, (C, 2) sum g / sum g xhat backward) -> the CALLER's gather of the ranks' rows -> a per-channel
// kernel that merges the rows in ascending rank order and writes what the apply pass takes.  The slab walk, the block sum and the
// apply passes are the fused entry points' own; no pass over a tensor is added.
//
// Upsampling: forward one thread per pair of output pixels (8-byte stores: an output row has 2 W floats); backward a GATHER per
// input pixel over the exact range of output rows / columns whose first tap is i - 1 or i, found with the forward's own fp32
// source-index function, summed in ascending order in double.
#include "acr_reduce.h"
#include "acr_resample.h"

#define BN_MAX_SLABS 64

static int bn_slabs(int64_t M, int C) {
    const int64_t by_size = (M + 1023) / 1024;            // no slab below 1024 values ...
    const int64_t fill = (1024 + C - 1) / C;              // ... about 1024 workgroups (256 CUs x 4) where the level is small ...
    int64_t s = by_size < fill ? by_size : fill;
    const int64_t big = (M + 16383) / 16384;              // ... and no slab above 16384 values where it is large
    if (big > s) s = big;
    return (int)(s < 1 ? 1 : (s > BN_MAX_SLABS ? BN_MAX_SLABS : s));
}

// the values [start, end) of channel c in (n, i) order: f1(offset) per single float, f4(offset) per 16-byte aligned group of 4
template <typename F1, typename F4>
__device__ __forceinline__ void bn_walk(int64_t start, int64_t end, int HW, int C, int c, F1 f1, F4 f4) {
    if (start >= end) return;
    const int n0 = (int)(start / HW), n1 = (int)((end - 1) / HW);
    const int gsz = (n1 - n0 + 1) >= 4 ? 64 : 256;
    const int grp = threadIdx.x / gsz, ngrp = 256 / gsz, lane = threadIdx.x % gsz;
    for (int n = n0 + grp; n <= n1; n += ngrp) {
        const int64_t base = ((int64_t)n * C + c) * HW;
        const int lo = n == n0 ? (int)(start - (int64_t)n0 * HW) : 0;
        const int hi = n == n1 ? (int)(end - (int64_t)n1 * HW) : HW;
        int head = (int)((4 - ((base + lo) & 3)) & 3);
        if (head > hi - lo) head = hi - lo;
        const int nvec = (hi - lo - head) >> 2;
        const int tail0 = lo + head + 4 * nvec;
        if (lane < head) f1(base + lo + lane);
        for (int v = lane; v < nvec; v += gsz) f4(base + lo + head + 4 * v);
        if (lane < hi - tail0) f1(base + tail0 + lane);
    }
}

__device__ __forceinline__ void bn_slab_range(int64_t M, int S, int s, int64_t& start, int64_t& end) {
    const int64_t chunk = (M + S - 1) / S;
    start = (int64_t)s * chunk;
    end = start + chunk < M ? start + chunk : M;
}

// (a, b) summed over the workgroup in a fixed order; valid in thread 0
__device__ __forceinline__ void bn_block_sum(double& a, double& b) {
    __shared__ double rd[512];
    const int tid = threadIdx.x;
    rd[tid] = a;
    rd[256 + tid] = b;
    acr_tree_sum256(tid, [&](int i, int j) {
        rd[i] += rd[j];
        rd[256 + i] += rd[256 + j];
    });
    a = rd[0];
    b = rd[256];
}

// a channel's slab sums of a pass, added in ascending slab order
__device__ __forceinline__ void bn_slab_sum(const double* __restrict__ part, int c, int S, double& a, double& b) {
    a = 0.0;
    b = 0.0;
    for (int s = 0; s < S; ++s) {
        a += part[2 * ((int64_t)c * S + s)];
        b += part[2 * ((int64_t)c * S + s) + 1];
    }
}

// The merge rule of cross-rank statistics, stated once: (n, mean, M2 = sum (x - mean)^2) of a set A takes in those of a disjoint
// set B by the pairwise update (Chan, Golub, LeVeque 1979).  The spread between the two means enters as delta^2 n_a n_b / n, a
// sum of non-negative terms: no difference of sums of squares, so the digits the shifted slab sums keep are not lost here.
__device__ __forceinline__ void bn_merge_moments(double& n, double& mean, double& m2, double nb, double meanb, double m2b) {
    const double na = n, delta = meanb - mean;
    n = na + nb;
    mean = mean + delta * nb / n;
    m2 = m2 + m2b + delta * delta * na * nb / n;
}

// what a normalising pass and the backward take from the statistics: stats = (mean, invstd), coef of y = a x + b
template <typename T>
__device__ __forceinline__ void bn_write_coef(int c, double mean, double invstd, const T* __restrict__ gamma,
                                              const T* __restrict__ beta, double* __restrict__ stats, double* __restrict__ coef) {
    stats[2 * c] = mean;
    stats[2 * c + 1] = invstd;
    const double k = (double)acr_load1<T>(gamma + c) * invstd;
    coef[2 * c] = k;
    coef[2 * c + 1] = (double)acr_load1<T>(beta + c) - mean * k;
}

// the running update of nn.BatchNorm2d: the mean and the UNBIASED variance of the batch
__device__ __forceinline__ void bn_running_update(int c, float* __restrict__ running_mean, float* __restrict__ running_var,
                                                  double momentum, double mean, double unbiased) {
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
    if (running_var) running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
}

template <typename T>
__global__ __launch_bounds__(256) void bn_stats_kernel(const T* __restrict__ x, int C, int HW, int64_t M, int S,
                                                       double* __restrict__ part) {
    const int c = blockIdx.x / S, s = blockIdx.x % S;
    int64_t start, end;
    bn_slab_range(M, S, s, start, end);
    const double shift = (double)acr_load1<T>(x + (int64_t)c * HW);
    double a = 0.0, b = 0.0;
    bn_walk(
        start, end, HW, C, c,
        [&](int64_t o) {
            const double d = (double)acr_load1<T>(x + o) - shift;
            a += d;
            b += d * d;
        },
        [&](int64_t o) {
            const f32x4 v = acr_load4<T>(x + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d = (double)v[j] - shift;
                a += d;
                b += d * d;
            }
        });
    bn_block_sum(a, b);
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = a;
        part[2 * (int64_t)blockIdx.x + 1] = b;
    }
}

// one thread per channel: the slabs in ascending order, the statistics, the running update, the coefficients of y = a x + b
template <typename T>
__global__ __launch_bounds__(256) void bn_fwd_finish_kernel(const T* __restrict__ x, const double* __restrict__ part,
                                                            const T* __restrict__ gamma, const T* __restrict__ beta,
                                                            float* __restrict__ running_mean, float* __restrict__ running_var, int C,
                                                            int HW, int64_t M, int S, int training, double eps, double momentum,
                                                            double* __restrict__ stats, double* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double mean, invstd;
    if (training) {
        double a, b;
        bn_slab_sum(part, c, S, a, b);
        const double n = (double)M;
        mean = (double)acr_load1<T>(x + (int64_t)c * HW) + a / n;
        double var = (b - a * a / n) / n;
        var = var > 0.0 ? var : 0.0;
        invstd = 1.0 / sqrt(var + eps);
        bn_running_update(c, running_mean, running_var, momentum, mean, var * n / (n - 1.0));
    } else {
        mean = (double)running_mean[c];
        invstd = 1.0 / sqrt((double)running_var[c] + eps);
    }
    bn_write_coef(c, mean, invstd, gamma, beta, stats, coef);
}

// ---- cross-rank statistics: the forward's per-channel kernels on either side of the exchange ----------------------------------
// moments (C, 3) of the local tensor from its slab sums: count, mean, M2.  One value (n = 1) is legal: M2 = 0.
template <typename T>
__global__ __launch_bounds__(256) void bn_moments_kernel(const T* __restrict__ x, const double* __restrict__ part, int C, int HW,
                                                         int64_t M, int S, double* __restrict__ moments) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a, b;
    bn_slab_sum(part, c, S, a, b);
    const double n = (double)M;
    const double m2 = b - a * a / n;
    moments[3 * c] = n;
    moments[3 * c + 1] = (double)acr_load1<T>(x + (int64_t)c * HW) + a / n;
    moments[3 * c + 2] = m2 > 0.0 ? m2 : 0.0;
}

// one thread per channel: the W ranks' moments merged in ascending rank order, then what bn_fwd_finish_kernel writes; stats is
// (C, 2) mean / invstd followed by the C merged counts
template <typename T>
__global__ __launch_bounds__(256) void bn_fwd_merge_kernel(const double* __restrict__ gathered, int W, const T* __restrict__ gamma,
                                                           const T* __restrict__ beta, float* __restrict__ running_mean,
                                                           float* __restrict__ running_var, int C, double eps, double momentum,
                                                           double* __restrict__ stats, double* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double n = gathered[3 * c], mean = gathered[3 * c + 1], m2 = gathered[3 * c + 2];
    for (int r = 1; r < W; ++r) {
        const double* row = gathered + 3 * ((int64_t)r * C + c);
        bn_merge_moments(n, mean, m2, row[0], row[1], row[2]);
    }
    const double invstd = 1.0 / sqrt(m2 / n + eps);
    bn_running_update(c, running_mean, running_var, momentum, mean, m2 / (n - 1.0));
    bn_write_coef(c, mean, invstd, gamma, beta, stats, coef);
    stats[2 * (int64_t)C + c] = n;
}

template <typename T, bool RELU, int NRES>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, const double* __restrict__ coef,
                                                       const T* __restrict__ r1, const T* __restrict__ r2, int C, int HW,
                                                       int64_t M, int S, T* __restrict__ y) {
    const int c = blockIdx.x / S, s = blockIdx.x % S;
    int64_t start, end;
    bn_slab_range(M, S, s, start, end);
    const double ka = coef[2 * c], kb = coef[2 * c + 1];
    auto one = [&](float xv, float a1, float a2) {
        double v = (double)xv * ka + kb;
        if (NRES >= 1) v += (double)a1;
        if (NRES >= 2) v += (double)a2;
        const float f = (float)v;
        return RELU ? (f > 0.f ? f : 0.f) : f;
    };
    bn_walk(
        start, end, HW, C, c,
        [&](int64_t o) {
            acr_store1<T>(y + o, one(acr_load1<T>(x + o), NRES >= 1 ? acr_load1<T>(r1 + o) : 0.f, NRES >= 2 ? acr_load1<T>(r2 + o) : 0.f));
        },
        [&](int64_t o) {
            const f32x4 v = acr_load4<T>(x + o);
            f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f}, out;
            if (NRES >= 1) a1 = acr_load4<T>(r1 + o);
            if (NRES >= 2) a2 = acr_load4<T>(r2 + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = one(v[j], a1[j], a2[j]);
            acr_store4<T>(y + o, out);
        });
}

// backward, first pass: part = (sum g, sum g * xhat) per slab, g = dy through the ReLU mask of the saved output
template <typename T, bool RELU>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ x, const T* __restrict__ y,
                                                            const T* __restrict__ dy, const double* __restrict__ stats, int C,
                                                            int HW, int64_t M, int S, double* __restrict__ part) {
    const int c = blockIdx.x / S, s = blockIdx.x % S;
    int64_t start, end;
    bn_slab_range(M, S, s, start, end);
    const double mean = stats[2 * c], invstd = stats[2 * c + 1];
    double a = 0.0, b = 0.0;
    bn_walk(
        start, end, HW, C, c,
        [&](int64_t o) {
            const double g = (!RELU || acr_load1<T>(y + o) > 0.f) ? (double)acr_load1<T>(dy + o) : 0.0;
            a += g;
            b += g * (((double)acr_load1<T>(x + o) - mean) * invstd);
        },
        [&](int64_t o) {
            const f32x4 xv = acr_load4<T>(x + o), gv = acr_load4<T>(dy + o);
            f32x4 yv = {1.f, 1.f, 1.f, 1.f};
            if (RELU) yv = acr_load4<T>(y + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double g = yv[j] > 0.f ? (double)gv[j] : 0.0;
                a += g;
                b += g * (((double)xv[j] - mean) * invstd);
            }
        });
    bn_block_sum(a, b);
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = a;
        part[2 * (int64_t)blockIdx.x + 1] = b;
    }
}

// coef (C, 3): k = gamma * invstd, mean(g), mean(g * xhat) (the last two 0 in eval mode: the statistics are constants)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double* __restrict__ part, const T* __restrict__ gamma,
                                                            const double* __restrict__ stats, int C, int64_t M, int S, int training,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            double* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a, b;
    bn_slab_sum(part, c, S, a, b);
    if (dbeta) dbeta[c] = (float)a;
    if (dgamma) dgamma[c] = (float)b;
    coef[3 * c] = (double)acr_load1<T>(gamma + c) * stats[2 * c + 1];
    coef[3 * c + 1] = training ? a / (double)M : 0.0;
    coef[3 * c + 2] = training ? b / (double)M : 0.0;
}

// ---- cross-rank statistics: the backward's per-channel kernels on either side of the exchange ---------------------------------
// sums (C, 2) = (sum g, sum g * xhat) of the local tensor; the parameter gradients are the local sums
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const double* __restrict__ part, int C, int S, double* __restrict__ sums,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a, b;
    bn_slab_sum(part, c, S, a, b);
    sums[2 * c] = a;
    sums[2 * c + 1] = b;
    if (dbeta) dbeta[c] = (float)a;
    if (dgamma) dgamma[c] = (float)b;
}

// the W ranks' sums added in ascending rank order and divided by the merged count: the coef of bn_bwd_apply_kernel
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_merge_kernel(const double* __restrict__ gathered, int W, const T* __restrict__ gamma,
                                                           const double* __restrict__ stats, int C, double* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int r = 0; r < W; ++r) {
        a += gathered[2 * ((int64_t)r * C + c)];
        b += gathered[2 * ((int64_t)r * C + c) + 1];
    }
    const double n = stats[2 * (int64_t)C + c];
    coef[3 * c] = (double)acr_load1<T>(gamma + c) * stats[2 * c + 1];
    coef[3 * c + 1] = a / n;
    coef[3 * c + 2] = b / n;
}

template <typename T, bool RELU>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ y,
                                                           const T* __restrict__ dy, const double* __restrict__ stats,
                                                           const double* __restrict__ coef, int C, int HW, int64_t M, int S,
                                                           T* __restrict__ dx, T* __restrict__ dres) {
    const int c = blockIdx.x / S, s = blockIdx.x % S;
    int64_t start, end;
    bn_slab_range(M, S, s, start, end);
    const double mean = stats[2 * c], invstd = stats[2 * c + 1];
    const double k = coef[3 * c], mg = coef[3 * c + 1], mgx = coef[3 * c + 2];
    auto one = [&](float xv, float g) { return (float)(k * ((double)g - mg - (((double)xv - mean) * invstd) * mgx)); };
    bn_walk(
        start, end, HW, C, c,
        [&](int64_t o) {
            const float g = (!RELU || acr_load1<T>(y + o) > 0.f) ? acr_load1<T>(dy + o) : 0.f;
            if (dx) acr_store1<T>(dx + o, one(acr_load1<T>(x + o), g));
            if (RELU && dres) acr_store1<T>(dres + o, g);
        },
        [&](int64_t o) {
            const f32x4 xv = acr_load4<T>(x + o);
            f32x4 gv = acr_load4<T>(dy + o), out;
            if (RELU) {
                const f32x4 yv = acr_load4<T>(y + o);
#pragma unroll
                for (int j = 0; j < 4; ++j) gv[j] = yv[j] > 0.f ? gv[j] : 0.f;
            }
            if (dx) {
#pragma unroll
                for (int j = 0; j < 4; ++j) out[j] = one(xv[j], gv[j]);
                acr_store4<T>(dx + o, out);
            }
            if (RELU && dres) acr_store4<T>(dres + o, gv);
        });
}

// ---- ReLU of a residual unit's input (blocks.py:330) and its backward from the saved output ---------------------------------
template <typename T>
__global__ __launch_bounds__(256) void relu_fwd_kernel(const T* __restrict__ x, int64_t n, T* __restrict__ y) {
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        f32x4 v = acr_load4<T>(x + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : 0.f;
        acr_store4<T>(y + 4 * i, v);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float v = acr_load1<T>(x + 4 * n4 + threadIdx.x);
        acr_store1<T>(y + 4 * n4 + threadIdx.x, v > 0.f ? v : 0.f);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ y, const T* __restrict__ dy, int64_t n,
                                                       T* __restrict__ dx) {
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const f32x4 v = acr_load4<T>(y + 4 * i);
        f32x4 g = acr_load4<T>(dy + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = v[j] > 0.f ? g[j] : 0.f;
        acr_store4<T>(dx + 4 * i, g);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t o = 4 * n4 + threadIdx.x;
        acr_store1<T>(dx + o, acr_load1<T>(y + o) > 0.f ? acr_load1<T>(dy + o) : 0.f);
    }
}

// ---- x2 bilinear upsampling, align_corners=True (torch upsample_bilinear2d; aten/src/ATen/native/UpSample.h) -----------------
struct up_tap {
    int i0, i1;
    float l0, l1;                          // weights of i0 and i1
};

__device__ __forceinline__ up_tap up_tap_of(float scale, int dst, int n_in) {
    up_tap t;
    const float src = acr_src_corners(scale, dst);
    int i0 = (int)src;
    i0 = i0 < n_in - 1 ? i0 : n_in - 1;
    float l = src - (float)i0;
    l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
    t.i0 = i0;
    t.i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    t.l1 = l;
    t.l0 = 1.f - l;
    return t;
}

template <typename T>
__device__ __forceinline__ float up_interp(const T* __restrict__ p, int W, const up_tap& ty, const up_tap& tx) {
    return acr_bilerp(ty.l0, ty.l1, tx.l0, tx.l1, acr_load1<T>(p + ty.i0 * W + tx.i0), acr_load1<T>(p + ty.i0 * W + tx.i1),
                      acr_load1<T>(p + ty.i1 * W + tx.i0), acr_load1<T>(p + ty.i1 * W + tx.i1));
}

// a pair of neighbouring outputs as one store: 8 bytes of fp32, 4 bytes of bf16 (an output row holds 2 W values, so a pair never
// straddles an alignment boundary of a base aligned to that size)
__device__ __forceinline__ void up_store2(float* p, float a, float b) {
    float2 o;
    o.x = a;
    o.y = b;
    *reinterpret_cast<float2*>(p) = o;
}
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void up_store2(__bf16* p, float a, float b) {
    const bf16x2 o = {(__bf16)a, (__bf16)b};
    *reinterpret_cast<bf16x2*>(p) = o;
}

// one thread per pair of output pixels (Y, 2 xp), (Y, 2 xp + 1)
template <typename T>
__global__ __launch_bounds__(256) void upsample2x_fwd_kernel(const T* __restrict__ x, int64_t planes, int H, int W, float sh, float sw,
                                                             T* __restrict__ y) {
    const int OH = 2 * H, OW = 2 * W;
    const int64_t total = planes * OH * W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int xp = (int)(idx % W), Y = (int)((idx / W) % OH);
        const int64_t p = idx / ((int64_t)W * OH);
        const T* plane = x + p * H * W;
        const up_tap ty = up_tap_of(sh, Y, H);
        const up_tap ta = up_tap_of(sw, 2 * xp, W), tb = up_tap_of(sw, 2 * xp + 1, W);
        up_store2(y + (p * OH + Y) * OW + 2 * xp, up_interp(plane, W, ty, ta), up_interp(plane, W, ty, tb));
    }
}

// the gather range of acr_resample.h for the corners rule: the estimate inverts it
__device__ __forceinline__ int up_first_dst(int t, int n_out, int n_in, float scale, float inv) {
    return acr_first_dst(
        t, n_out, n_in, [&](int tap) { return (float)tap * inv; }, [&](int d) { return up_tap_of(scale, d, n_in).i0; });
}

// one thread per input pixel, lanes along x
template <typename T>
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const T* __restrict__ dy, int64_t planes, int H, int W, float sh, float sw,
                                                             float ish, float isw, T* __restrict__ dx) {
    const int OH = 2 * H, OW = 2 * W;
    const int64_t total = planes * H * W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int xx = (int)(idx % W), yy = (int)((idx / W) % H);
        const int64_t p = idx / ((int64_t)W * H);
        const T* g = dy + p * OH * OW;
        const int Ya = up_first_dst(yy - 1, OH, H, sh, ish), Yb = up_first_dst(yy + 1, OH, H, sh, ish);
        const int Xa = up_first_dst(xx - 1, OW, W, sw, isw), Xb = up_first_dst(xx + 1, OW, W, sw, isw);
        double acc = 0.0;
        for (int Y = Ya; Y < Yb; ++Y) {
            const up_tap ty = up_tap_of(sh, Y, H);
            const float wy = (ty.i0 == yy ? ty.l0 : 0.f) + (ty.i1 == yy ? ty.l1 : 0.f);
            for (int X = Xa; X < Xb; ++X) {
                const up_tap tx = up_tap_of(sw, X, W);
                const float wx = (tx.i0 == xx ? tx.l0 : 0.f) + (tx.i1 == xx ? tx.l1 : 0.f);
                acc += (double)wy * (double)wx * (double)acr_load1<T>(g + (int64_t)Y * OW + X);
            }
        }
        acr_store1<T>(dx + idx, (float)acc);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
#define BN_ALIGNED(p) ((((uintptr_t)(p)) & 15) == 0)

static int bn_check(const char* who, int32_t N, int32_t C, int32_t HW) {
    ACR_CHECK_ARG(N >= 1 && C >= 1 && HW >= 1, "%s: N=%d C=%d HW=%d must be positive", who, N, C, HW);
    ACR_CHECK_ARG((int64_t)N * HW < (1ll << 31), "%s: N * H * W = %lld values per channel, 2^31 - 1 at most", who, (long long)N * HW);
    ACR_CHECK_ARG((int64_t)C * BN_MAX_SLABS < (1ll << 31), "%s: C=%d too large", who, C);
    return ACR_OK;
}

extern "C" int64_t acr_bn2d_ws_bytes(int32_t N, int32_t C, int32_t HW) {
    if (bn_check("acr_bn2d_ws_bytes", N, C, HW) != ACR_OK) return ACR_ERR_INVALID;
    return 8 * ((int64_t)C * bn_slabs((int64_t)N * HW, C) * 2 + 3 * (int64_t)C);
}

// the passes over the tensors, launched for the fused entry points and for the cross-rank ones alike
template <typename T>
static void bn_launch_apply(hipStream_t st, dim3 grid, const T* x, const double* coef, const T* resid, const T* resid2, int C, int HW,
                            int64_t M, int S, int relu, T* y) {
#define BN_APPLY(R, K) hipLaunchKernelGGL((bn_apply_kernel<T, R, K>), grid, dim3(256), 0, st, x, coef, resid, resid2, C, HW, M, S, y)
    const int nres = resid2 ? 2 : (resid ? 1 : 0);
    if (relu) {
        if (nres == 0) BN_APPLY(true, 0);
        else if (nres == 1) BN_APPLY(true, 1);
        else BN_APPLY(true, 2);
    } else {
        if (nres == 0) BN_APPLY(false, 0);
        else if (nres == 1) BN_APPLY(false, 1);
        else BN_APPLY(false, 2);
    }
#undef BN_APPLY
}

template <typename T>
static void bn_launch_bwd_reduce(hipStream_t st, dim3 grid, const T* x, const T* y, const T* dy, const double* stats, int C, int HW,
                                 int64_t M, int S, int relu, double* part) {
    if (relu)
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, true>), grid, dim3(256), 0, st, x, y, dy, stats, C, HW, M, S, part);
    else
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, false>), grid, dim3(256), 0, st, x, y, dy, stats, C, HW, M, S, part);
}

template <typename T>
static void bn_launch_bwd_apply(hipStream_t st, dim3 grid, const T* x, const T* y, const T* dy, const double* stats, const double* coef,
                                int C, int HW, int64_t M, int S, int relu, T* dx, T* dres) {
    if (relu)
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T, true>), grid, dim3(256), 0, st, x, y, dy, stats, coef, C, HW, M, S, dx, dres);
    else
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T, false>), grid, dim3(256), 0, st, x, y, dy, stats, coef, C, HW, M, S, dx, dres);
}

// Every entry point exists once per storage type T (float: the plain names; __bf16: the _bf16 names): the same checks, launches
// and walk, so the double sums of the two are the same numbers.
template <typename T>
static int bn2d_fwd(const char* who, const T* x, const T* gamma, const T* beta, float* running_mean, float* running_var, const T* resid,
                    const T* resid2, int32_t N, int32_t C, int32_t HW, int32_t training, double eps, double momentum, int32_t relu,
                    void* ws, int64_t ws_bytes, double* stats, T* y, void* stream) {
    const int rc = bn_check(who, N, C, HW);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(x && gamma && beta && stats && y, "%s: null pointer", who);
    ACR_CHECK_ARG(resid || !resid2, "%s: resid2 given without resid", who);
    ACR_CHECK_ARG(BN_ALIGNED(x) && BN_ALIGNED(y) && BN_ALIGNED(resid) && BN_ALIGNED(resid2), "%s: a tensor is not 16-byte aligned", who);
    ACR_CHECK_ARG(((uintptr_t)stats & 7) == 0, "%s: stats not aligned to 8 bytes", who);
    ACR_CHECK_WS(who, ws, 8, ws_bytes, acr_bn2d_ws_bytes(N, C, HW));
    const int64_t M = (int64_t)N * HW;
    if (training)
        ACR_CHECK_ARG(M >= 2, "%s: %lld value per channel in training mode, 2 at least", who, (long long)M);
    else
        ACR_CHECK_ARG(running_mean && running_var, "%s: eval mode needs the running statistics", who);
    ACR_CHECK_ARG(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, "%s: eps=%g, momentum=%g", who, eps, momentum);
    hipStream_t st = (hipStream_t)stream;
    const int S = bn_slabs(M, C);
    double* part = reinterpret_cast<double*>(ws);
    double* coef = part + (int64_t)C * S * 2;
    const dim3 grid((unsigned)(C * S)), cgrid((unsigned)((C + 255) / 256));
    if (training) hipLaunchKernelGGL(bn_stats_kernel<T>, grid, dim3(256), 0, st, x, C, HW, M, S, part);
    hipLaunchKernelGGL(bn_fwd_finish_kernel<T>, cgrid, dim3(256), 0, st, x, (const double*)part, gamma, beta, running_mean, running_var, C,
                       HW, M, S, training ? 1 : 0, eps, momentum, stats, coef);
    bn_launch_apply<T>(st, grid, x, coef, resid, resid2, C, HW, M, S, relu, y);
    return acr_check_launch(who);
}

template <typename T>
static int bn2d_bwd(const char* who, const T* x, const T* y, const T* dy, const T* gamma, const double* stats, int32_t N, int32_t C,
                    int32_t HW, int32_t training, int32_t relu, void* ws, int64_t ws_bytes, T* dx, float* dgamma, float* dbeta, T* dres,
                    void* stream) {
    const int rc = bn_check(who, N, C, HW);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(x && dy && gamma && stats, "%s: null pointer", who);
    ACR_CHECK_ARG(!relu || y, "%s: a fused ReLU needs the saved output", who);
    ACR_CHECK_ARG(relu || !dres, "%s: without a fused ReLU the addends' gradient is dy itself; dres must be null", who);
    ACR_CHECK_ARG(BN_ALIGNED(x) && BN_ALIGNED(y) && BN_ALIGNED(dy) && BN_ALIGNED(dx) && BN_ALIGNED(dres),
                  "%s: a tensor is not 16-byte aligned", who);
    ACR_CHECK_ARG(((uintptr_t)stats & 7) == 0, "%s: stats not aligned to 8 bytes", who);
    ACR_CHECK_WS(who, ws, 8, ws_bytes, acr_bn2d_ws_bytes(N, C, HW));
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = (int64_t)N * HW;
    const int S = bn_slabs(M, C);
    double* part = reinterpret_cast<double*>(ws);
    double* coef = part + (int64_t)C * S * 2;
    const dim3 grid((unsigned)(C * S)), cgrid((unsigned)((C + 255) / 256));
    bn_launch_bwd_reduce<T>(st, grid, x, y, dy, stats, C, HW, M, S, relu, part);
    hipLaunchKernelGGL(bn_bwd_finish_kernel<T>, cgrid, dim3(256), 0, st, (const double*)part, gamma, stats, C, M, S, training ? 1 : 0,
                       dgamma, dbeta, coef);
    if (dx || dres) bn_launch_bwd_apply<T>(st, grid, x, y, dy, stats, coef, C, HW, M, S, relu, dx, dres);
    return acr_check_launch(who);
}

// ---- cross-rank statistics (nn.SyncBatchNorm): the two halves of each direction, the caller's gather between them -------------
#define BN_WORLD_MAX 65536

// the shape, the workspace and the 8-byte alignment of the double buffers, common to the four entry points
static int bn_sync_check(const char* who, int32_t N, int32_t C, int32_t HW, const void* ws, int64_t ws_bytes, const void* d1,
                         const void* d2) {
    const int rc = bn_check(who, N, C, HW);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(d1 && d2, "%s: null pointer", who);
    ACR_CHECK_ARG((((uintptr_t)d1 | (uintptr_t)d2) & 7) == 0, "%s: a double buffer not aligned to 8 bytes", who);
    ACR_CHECK_WS(who, ws, 8, ws_bytes, acr_bn2d_ws_bytes(N, C, HW));
    return ACR_OK;
}

template <typename T>
static int bn2d_moments(const char* who, const T* x, int32_t N, int32_t C, int32_t HW, void* ws, int64_t ws_bytes, double* moments,
                        void* stream) {
    const int rc = bn_sync_check(who, N, C, HW, ws, ws_bytes, moments, moments);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(x && BN_ALIGNED(x), "%s: x null or not 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = (int64_t)N * HW;
    const int S = bn_slabs(M, C);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(bn_stats_kernel<T>, dim3((unsigned)(C * S)), dim3(256), 0, st, x, C, HW, M, S, part);
    hipLaunchKernelGGL(bn_moments_kernel<T>, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, x, (const double*)part, C, HW, M, S,
                       moments);
    return acr_check_launch(who);
}

template <typename T>
static int bn2d_fwd_merged(const char* who, const T* x, const T* gamma, const T* beta, float* running_mean, float* running_var,
                           const T* resid, const T* resid2, int32_t N, int32_t C, int32_t HW, const double* gathered, int32_t W,
                           double eps, double momentum, int32_t relu, void* ws, int64_t ws_bytes, double* stats, T* y, void* stream) {
    const int rc = bn_sync_check(who, N, C, HW, ws, ws_bytes, gathered, stats);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(x && gamma && beta && y, "%s: null pointer", who);
    ACR_CHECK_ARG(resid || !resid2, "%s: resid2 given without resid", who);
    ACR_CHECK_ARG(BN_ALIGNED(x) && BN_ALIGNED(y) && BN_ALIGNED(resid) && BN_ALIGNED(resid2), "%s: a tensor is not 16-byte aligned", who);
    ACR_CHECK_ARG(W >= 1 && W <= BN_WORLD_MAX, "%s: W=%d ranks, 1 .. %d", who, W, BN_WORLD_MAX);
    ACR_CHECK_ARG(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, "%s: eps=%g, momentum=%g", who, eps, momentum);
    // every rank holds whole (H, W) planes of the same size, so the merged count is at least N * HW + (W - 1) * HW: known here
    // without reading the gathered counts back
    const int64_t M = (int64_t)N * HW;
    ACR_CHECK_ARG(M + (int64_t)(W - 1) * HW >= 2, "%s: 1 value per channel over all ranks, 2 at least", who);
    hipStream_t st = (hipStream_t)stream;
    const int S = bn_slabs(M, C);
    double* coef = reinterpret_cast<double*>(ws) + (int64_t)C * S * 2;
    hipLaunchKernelGGL(bn_fwd_merge_kernel<T>, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, gathered, W, gamma, beta, running_mean,
                       running_var, C, eps, momentum, stats, coef);
    bn_launch_apply<T>(st, dim3((unsigned)(C * S)), x, coef, resid, resid2, C, HW, M, S, relu, y);
    return acr_check_launch(who);
}

template <typename T>
static int bn2d_bwd_sums(const char* who, const T* x, const T* y, const T* dy, const double* stats, int32_t N, int32_t C, int32_t HW,
                         int32_t relu, void* ws, int64_t ws_bytes, double* sums, float* dgamma, float* dbeta, void* stream) {
    const int rc = bn_sync_check(who, N, C, HW, ws, ws_bytes, stats, sums);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(x && dy, "%s: null pointer", who);
    ACR_CHECK_ARG(!relu || y, "%s: a fused ReLU needs the saved output", who);
    ACR_CHECK_ARG(BN_ALIGNED(x) && BN_ALIGNED(y) && BN_ALIGNED(dy), "%s: a tensor is not 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = (int64_t)N * HW;
    const int S = bn_slabs(M, C);
    double* part = reinterpret_cast<double*>(ws);
    bn_launch_bwd_reduce<T>(st, dim3((unsigned)(C * S)), x, y, dy, stats, C, HW, M, S, relu, part);
    hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, (const double*)part, C, S, sums, dgamma,
                       dbeta);
    return acr_check_launch(who);
}

template <typename T>
static int bn2d_bwd_merged(const char* who, const T* x, const T* y, const T* dy, const T* gamma, const double* stats,
                           const double* gathered_sums, int32_t W, int32_t N, int32_t C, int32_t HW, int32_t relu, void* ws,
                           int64_t ws_bytes, T* dx, T* dres, void* stream) {
    const int rc = bn_sync_check(who, N, C, HW, ws, ws_bytes, stats, gathered_sums);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(x && dy && gamma, "%s: null pointer", who);
    ACR_CHECK_ARG(!relu || y, "%s: a fused ReLU needs the saved output", who);
    ACR_CHECK_ARG(relu || !dres, "%s: without a fused ReLU the addends' gradient is dy itself; dres must be null", who);
    ACR_CHECK_ARG(BN_ALIGNED(x) && BN_ALIGNED(y) && BN_ALIGNED(dy) && BN_ALIGNED(dx) && BN_ALIGNED(dres),
                  "%s: a tensor is not 16-byte aligned", who);
    ACR_CHECK_ARG(W >= 1 && W <= BN_WORLD_MAX, "%s: W=%d ranks, 1 .. %d", who, W, BN_WORLD_MAX);
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = (int64_t)N * HW;
    const int S = bn_slabs(M, C);
    double* coef = reinterpret_cast<double*>(ws) + (int64_t)C * S * 2;
    hipLaunchKernelGGL(bn_bwd_merge_kernel<T>, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, gathered_sums, W, gamma, stats, C,
                       coef);
    if (dx || dres) bn_launch_bwd_apply<T>(st, dim3((unsigned)(C * S)), x, y, dy, stats, coef, C, HW, M, S, relu, dx, dres);
    return acr_check_launch(who);
}

static int relu_grid(int64_t n) {
    const int64_t nb = ((n >> 2) + 255) / 256;
    return (int)(nb < 1 ? 1 : (nb > 8192 ? 8192 : nb));
}

template <typename T>
static int relu_fwd(const char* who, const T* x, int64_t n, T* y, void* stream) {
    ACR_CHECK_ARG(x && y && n >= 1, "%s: null pointer or n=%lld < 1", who, (long long)n);
    ACR_CHECK_ARG(BN_ALIGNED(x) && BN_ALIGNED(y), "%s: a tensor is not 16-byte aligned", who);
    hipLaunchKernelGGL(relu_fwd_kernel<T>, dim3(relu_grid(n)), dim3(256), 0, (hipStream_t)stream, x, n, y);
    return acr_check_launch(who);
}

template <typename T>
static int relu_bwd(const char* who, const T* y, const T* dy, int64_t n, T* dx, void* stream) {
    ACR_CHECK_ARG(y && dy && dx && n >= 1, "%s: null pointer or n=%lld < 1", who, (long long)n);
    ACR_CHECK_ARG(BN_ALIGNED(y) && BN_ALIGNED(dy) && BN_ALIGNED(dx), "%s: a tensor is not 16-byte aligned", who);
    hipLaunchKernelGGL(relu_bwd_kernel<T>, dim3(relu_grid(n)), dim3(256), 0, (hipStream_t)stream, y, dy, n, dx);
    return acr_check_launch(who);
}

static int up_check(const char* who, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW) {
    ACR_CHECK_ARG(planes >= 1 && H >= 1 && W >= 1, "%s: planes=%lld H=%d W=%d must be positive", who, (long long)planes, H, W);
    if (OH != 2 * H || OW != 2 * W) {
        acr_set_error("%s: only out = 2 * in per axis is built (%d x %d -> %d x %d)", who, H, W, OH, OW);
        return ACR_ERR_UNSUPPORTED;
    }
    ACR_CHECK_ARG((int64_t)OH * OW < (1ll << 31) && planes * OH * OW < (1ll << 40), "%s: tensor too large", who);
    return ACR_OK;
}

static int up_grid(int64_t total) {
    const int64_t nb = (total + 255) / 256;
    return (int)(nb > 16384 ? 16384 : nb);
}

template <typename T>
static int upsample2x_fwd(const char* who, const T* x, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, T* y, void* stream) {
    const int rc = up_check(who, planes, H, W, OH, OW);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(x && y && ((uintptr_t)y & (2 * sizeof(T) - 1)) == 0, "%s: null pointer, or y not aligned to %d bytes", who,
                  (int)(2 * sizeof(T)));
    const float sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f, sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
    hipLaunchKernelGGL(upsample2x_fwd_kernel<T>, dim3(up_grid(planes * OH * W)), dim3(256), 0, (hipStream_t)stream, x, planes, H, W, sh, sw,
                       y);
    return acr_check_launch(who);
}

template <typename T>
static int upsample2x_bwd(const char* who, const T* dy, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, T* dx, void* stream) {
    const int rc = up_check(who, planes, H, W, OH, OW);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(dy && dx, "%s: null pointer", who);
    const float sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f, sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
    const float ish = H > 1 ? (float)(OH - 1) / (float)(H - 1) : 0.f, isw = W > 1 ? (float)(OW - 1) / (float)(W - 1) : 0.f;
    hipLaunchKernelGGL(upsample2x_bwd_kernel<T>, dim3(up_grid(planes * H * W)), dim3(256), 0, (hipStream_t)stream, dy, planes, H, W, sh, sw,
                       ish, isw, dx);
    return acr_check_launch(who);
}

// ---- the C ABI: fp32 storage ---------------------------------------------------------------------------------------------------
extern "C" int acr_bn2d_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            const float* resid, const float* resid2, int32_t N, int32_t C, int32_t HW, int32_t training, double eps,
                            double momentum, int32_t relu, void* ws, int64_t ws_bytes, double* stats, float* y, void* stream) {
    return bn2d_fwd<float>("acr_bn2d_fwd", x, gamma, beta, running_mean, running_var, resid, resid2, N, C, HW, training, eps, momentum, relu,
                           ws, ws_bytes, stats, y, stream);
}

extern "C" int acr_bn2d_bwd(const float* x, const float* y, const float* dy, const float* gamma, const double* stats, int32_t N,
                            int32_t C, int32_t HW, int32_t training, int32_t relu, void* ws, int64_t ws_bytes, float* dx,
                            float* dgamma, float* dbeta, float* dres, void* stream) {
    return bn2d_bwd<float>("acr_bn2d_bwd", x, y, dy, gamma, stats, N, C, HW, training, relu, ws, ws_bytes, dx, dgamma, dbeta, dres, stream);
}

extern "C" int acr_bn2d_moments(const float* x, int32_t N, int32_t C, int32_t HW, void* ws, int64_t ws_bytes, double* moments,
                                void* stream) {
    return bn2d_moments<float>("acr_bn2d_moments", x, N, C, HW, ws, ws_bytes, moments, stream);
}

extern "C" int acr_bn2d_fwd_merged(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                   const float* resid, const float* resid2, int32_t N, int32_t C, int32_t HW, const double* gathered,
                                   int32_t W, double eps, double momentum, int32_t relu, void* ws, int64_t ws_bytes, double* stats,
                                   float* y, void* stream) {
    return bn2d_fwd_merged<float>("acr_bn2d_fwd_merged", x, gamma, beta, running_mean, running_var, resid, resid2, N, C, HW, gathered, W, eps,
                                  momentum, relu, ws, ws_bytes, stats, y, stream);
}

extern "C" int acr_bn2d_bwd_sums(const float* x, const float* y, const float* dy, const double* stats, int32_t N, int32_t C, int32_t HW,
                                 int32_t relu, void* ws, int64_t ws_bytes, double* sums, float* dgamma, float* dbeta, void* stream) {
    return bn2d_bwd_sums<float>("acr_bn2d_bwd_sums", x, y, dy, stats, N, C, HW, relu, ws, ws_bytes, sums, dgamma, dbeta, stream);
}

extern "C" int acr_bn2d_bwd_merged(const float* x, const float* y, const float* dy, const float* gamma, const double* stats,
                                   const double* gathered_sums, int32_t W, int32_t N, int32_t C, int32_t HW, int32_t relu, void* ws,
                                   int64_t ws_bytes, float* dx, float* dres, void* stream) {
    return bn2d_bwd_merged<float>("acr_bn2d_bwd_merged", x, y, dy, gamma, stats, gathered_sums, W, N, C, HW, relu, ws, ws_bytes, dx, dres,
                                  stream);
}

extern "C" int acr_relu_fwd_f32(const float* x, int64_t n, float* y, void* stream) { return relu_fwd<float>("acr_relu_fwd_f32", x, n, y, stream); }

extern "C" int acr_relu_bwd_f32(const float* y, const float* dy, int64_t n, float* dx, void* stream) {
    return relu_bwd<float>("acr_relu_bwd_f32", y, dy, n, dx, stream);
}

extern "C" int acr_upsample2x_fwd(const float* x, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, float* y, void* stream) {
    return upsample2x_fwd<float>("acr_upsample2x_fwd", x, planes, H, W, OH, OW, y, stream);
}

extern "C" int acr_upsample2x_bwd(const float* dy, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, float* dx, void* stream) {
    return upsample2x_bwd<float>("acr_upsample2x_bwd", dy, planes, H, W, OH, OW, dx, stream);
}

// ---- the C ABI: bf16 storage (the header spells a bf16 pointer void*) ------------------------------------------------------------
#define BF(p) reinterpret_cast<const __bf16*>(p)
#define BFW(p) reinterpret_cast<__bf16*>(p)

extern "C" int acr_bn2d_fwd_bf16(const void* x, const void* gamma, const void* beta, float* running_mean, float* running_var,
                                 const void* resid, const void* resid2, int32_t N, int32_t C, int32_t HW, int32_t training, double eps,
                                 double momentum, int32_t relu, void* ws, int64_t ws_bytes, double* stats, void* y, void* stream) {
    return bn2d_fwd<__bf16>("acr_bn2d_fwd_bf16", BF(x), BF(gamma), BF(beta), running_mean, running_var, BF(resid), BF(resid2), N, C, HW,
                            training, eps, momentum, relu, ws, ws_bytes, stats, BFW(y), stream);
}

extern "C" int acr_bn2d_bwd_bf16(const void* x, const void* y, const void* dy, const void* gamma, const double* stats, int32_t N,
                                 int32_t C, int32_t HW, int32_t training, int32_t relu, void* ws, int64_t ws_bytes, void* dx,
                                 float* dgamma, float* dbeta, void* dres, void* stream) {
    return bn2d_bwd<__bf16>("acr_bn2d_bwd_bf16", BF(x), BF(y), BF(dy), BF(gamma), stats, N, C, HW, training, relu, ws, ws_bytes, BFW(dx),
                            dgamma, dbeta, BFW(dres), stream);
}

extern "C" int acr_bn2d_moments_bf16(const void* x, int32_t N, int32_t C, int32_t HW, void* ws, int64_t ws_bytes, double* moments,
                                     void* stream) {
    return bn2d_moments<__bf16>("acr_bn2d_moments_bf16", BF(x), N, C, HW, ws, ws_bytes, moments, stream);
}

extern "C" int acr_bn2d_fwd_merged_bf16(const void* x, const void* gamma, const void* beta, float* running_mean, float* running_var,
                                        const void* resid, const void* resid2, int32_t N, int32_t C, int32_t HW,
                                        const double* gathered, int32_t W, double eps, double momentum, int32_t relu, void* ws,
                                        int64_t ws_bytes, double* stats, void* y, void* stream) {
    return bn2d_fwd_merged<__bf16>("acr_bn2d_fwd_merged_bf16", BF(x), BF(gamma), BF(beta), running_mean, running_var, BF(resid),
                                   BF(resid2), N, C, HW, gathered, W, eps, momentum, relu, ws, ws_bytes, stats, BFW(y), stream);
}

extern "C" int acr_bn2d_bwd_sums_bf16(const void* x, const void* y, const void* dy, const double* stats, int32_t N, int32_t C,
                                      int32_t HW, int32_t relu, void* ws, int64_t ws_bytes, double* sums, float* dgamma, float* dbeta,
                                      void* stream) {
    return bn2d_bwd_sums<__bf16>("acr_bn2d_bwd_sums_bf16", BF(x), BF(y), BF(dy), stats, N, C, HW, relu, ws, ws_bytes, sums, dgamma, dbeta,
                                 stream);
}

extern "C" int acr_bn2d_bwd_merged_bf16(const void* x, const void* y, const void* dy, const void* gamma, const double* stats,
                                        const double* gathered_sums, int32_t W, int32_t N, int32_t C, int32_t HW, int32_t relu,
                                        void* ws, int64_t ws_bytes, void* dx, void* dres, void* stream) {
    return bn2d_bwd_merged<__bf16>("acr_bn2d_bwd_merged_bf16", BF(x), BF(y), BF(dy), BF(gamma), stats, gathered_sums, W, N, C, HW, relu,
                                   ws, ws_bytes, BFW(dx), BFW(dres), stream);
}

extern "C" int acr_relu_fwd_bf16(const void* x, int64_t n, void* y, void* stream) {
    return relu_fwd<__bf16>("acr_relu_fwd_bf16", BF(x), n, BFW(y), stream);
}

extern "C" int acr_relu_bwd_bf16(const void* y, const void* dy, int64_t n, void* dx, void* stream) {
    return relu_bwd<__bf16>("acr_relu_bwd_bf16", BF(y), BF(dy), n, BFW(dx), stream);
}

extern "C" int acr_upsample2x_fwd_bf16(const void* x, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, void* y,
                                       void* stream) {
    return upsample2x_fwd<__bf16>("acr_upsample2x_fwd_bf16", BF(x), planes, H, W, OH, OW, BFW(y), stream);
}

extern "C" int acr_upsample2x_bwd_bf16(const void* dy, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, void* dx,
                                       void* stream) {
    return upsample2x_bwd<__bf16>("acr_upsample2x_bwd_bf16", BF(dy), planes, H, W, OH, OW, BFW(dx), stream);
}
#undef BF
#undef BFW
