// Class-centre feature-distance loss on the device (the reference's compute_dis_no_batch with compute_cos, myTool.py:1616-1710):
// every pixel's feature vector is pulled towards the centre of the class the head predicts for it, the foreground centres are
// pushed apart and away from each image's background centre.  include/acr_hip.h states the definition and the gradient in full.
//
// The features are read as they lie -- (B, C, N) with the pixels contiguous -- and no (B N, C) or per-class masked copy exists.
// Centres: centre r < B is the background centre of image r, centre B + i - 1 the foreground centre of class i (NC = B + K - 1).
// Passes over feat, lanes along the pixels in every one of them:
//   1. fd_classsum_kernel<false>  the class sums of a slab of pixels (one read)
//   2. fd_pixdot_kernel           per pixel f . c and |f|, from which 1 - cos, 1 / D and the two backward scalars follow (one read)
//   3. fd_classsum_kernel<true>   the class sums weighted by 1 / D_n, which d loss / d centre needs (one read: the re-read form of
//                                 the forward; the weight of a pixel is known only after its dot product)
//   4. fd_bwd_kernel              one read, one write
// Between them run small kernels over (centres x channels) or (slabs x classes): label and count, the merge of the slab partials, the
// centre-centre products, the per-slab sums of the pixel scalars, a single-workgroup finish that forms the loss and every
// coefficient of d loss / d centre, and the kernel that writes those gradients, so that the backward needs no reduction.
// Every sum runs in double in a fixed order (a thread's run of pixels, the slabs ascending, wave butterflies): no float atomics,
// bit-identical run to run.  The only atomics count labels in LDS as integers.
#include "acr_reduce.h"

#define FD_MAX_K ACR_FEATDIS_MAX_K
#define FD_MAX_B 65535
#define FD_MAX_C (1 << 20)
#define FD_SLAB 2048                      // pixels of a slab per 32 classes: a slab holds FD_SLAB * ceil(K / 32) pixels
#define FD_TAB_DOUBLES 6144               // the centre table of a workgroup in LDS: 48 KiB
#define FD_WIDE_MAX_K 90                  // up to here a class-sum workgroup owns 64 channels (bins + tile within 64 KiB), above 32
#define FD_WIDE_DOT_MIN_TILES 512         // from this many 256-pixel tiles on, a dot-product thread owns a whole pixel
#define FD_EPS 1e-7

// ---- 1. labels and counts --------------------------------------------------------------------------------------------------------
// one workgroup per slab: lab = first index of the maximum, a NaN the maximum (torch.argmax); slabcnt[slab][k] pixels of label k
__global__ __launch_bounds__(256) void fd_label_kernel(const float* __restrict__ seg, int K, int N, int slab, int S,
                                                       uint8_t* __restrict__ lab, int* __restrict__ slabcnt) {
    __shared__ int cnt[FD_MAX_K];
    const int tid = threadIdx.x;
    const int64_t sl = blockIdx.x, b = sl / S, s = sl % S;
    if (tid < FD_MAX_K) cnt[tid] = 0;
    __syncthreads();
    const int p1 = min(N, (int)(s + 1) * slab);
    const float* sg = seg + b * K * (int64_t)N;
    for (int p = (int)s * slab + tid; p < p1; p += 256) {
        float best = sg[p];
        int idx = 0;
#pragma unroll 4
        for (int k = 1; k < K; ++k) {
            const float v = sg[(int64_t)k * N + p];
            if (best == best && (v > best || v != v)) {
                best = v;
                idx = k;
            }
        }
        lab[b * N + p] = (uint8_t)idx;
        atomicAdd(&cnt[idx], 1);
    }
    __syncthreads();
    if (tid < K) slabcnt[sl * K + tid] = cnt[tid];
}

// the slabs a centre draws on: centre r < B the S slabs of image r with class 0, a foreground centre every slab with its class
struct fd_span {
    int64_t first, count;
    int cls;
};
__device__ __forceinline__ fd_span fd_span_of(int r, int B, int S) {
    fd_span sp;
    if (r < B) {
        sp.first = (int64_t)r * S;
        sp.count = S;
        sp.cls = 0;
    } else {
        sp.first = 0;
        sp.count = (int64_t)B * S;
        sp.cls = r - B + 1;
    }
    return sp;
}

// one wave per centre: counts[r] (n_b per image, then m_i per class), invcnt[r] = 1 / (count + eps) or 0 for an empty centre
__global__ __launch_bounds__(64) void fd_count_kernel(const int* __restrict__ slabcnt, int B, int K, int S, int64_t* __restrict__ counts,
                                                      double* __restrict__ invcnt) {
    const int r = blockIdx.x;
    const fd_span sp = fd_span_of(r, B, S);
    long long n = 0;
    for (int64_t j = threadIdx.x; j < sp.count; j += 64) n += slabcnt[(sp.first + j) * K + sp.cls];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (threadIdx.x == 0) {
        counts[r] = n;
        invcnt[r] = n >= 1 ? 1.0 / ((double)n + FD_EPS) : 0.0;
    }
}

// one workgroup: hdr = (Z = F + B, F, 1 when the batch has a background pixel)
__global__ __launch_bounds__(256) void fd_hdr_kernel(const int64_t* __restrict__ counts, int B, int K, double* __restrict__ hdr) {
    __shared__ int F, has_bg;
    if (threadIdx.x == 0) F = has_bg = 0;
    __syncthreads();
    for (int r = threadIdx.x; r < B + K - 1; r += 256) {
        if (counts[r] >= 1) {
            if (r < B)
                atomicOr(&has_bg, 1);
            else
                atomicAdd(&F, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        hdr[0] = (double)(F + B);
        hdr[1] = (double)F;
        hdr[2] = (double)has_bg;
    }
}

// ---- 2. class sums of a slab ---------------------------------------------------------------------------------------------------
// One wave per (slab, chunk of W channels).  A 64-pixel tile of the chunk goes to LDS with the lanes along the pixels; then lane c
// owns channel c and walks the pixels of the tile.  The label of a pixel is the same in every lane, so the wave keeps ONE register
// accumulator for the current run of equal labels and adds it to its LDS bin [label][c] when the label changes.
// partial[slab][k][c] = sum over the slab's pixels of label k of (weight *) feat, WRITTEN for every k.
template <bool WEIGHTED, int W>
__global__ __launch_bounds__(64) void fd_classsum_kernel(const float* __restrict__ feat, const uint8_t* __restrict__ lab,
                                                         const double* __restrict__ pixw, int K, int C, int N, int slab, int S,
                                                         double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fd_smem[];
    double* bins = reinterpret_cast<double*>(fd_smem);                   // [K][W]
    double* tw = bins + (size_t)K * W;                                   // [64] weights of the tile's pixels
    int* tl = reinterpret_cast<int*>(tw + 64);                           // [64] labels
    float* tile = reinterpret_cast<float*>(tl + 64);                     // [W][65]
    const int lane = threadIdx.x;
    const int64_t sl = blockIdx.x, b = sl / S, s = sl % S;
    const int c0 = blockIdx.y * W;
    const int p0 = (int)s * slab, p1 = min(N, p0 + slab);
    const float* fb = feat + b * C * (int64_t)N;
    if (lane < W)
        for (int k = 0; k < K; ++k) bins[k * W + lane] = 0.0;
    int cur = -1;
    double acc = 0.0;
    for (int t0 = p0; t0 < p1; t0 += 64) {
        const int np = min(64, p1 - t0);
        float v[W];                                                      // every row of the tile in flight before the first is stored
#pragma unroll
        for (int u = 0; u < W; ++u) v[u] = (c0 + u < C && lane < np) ? fb[(int64_t)(c0 + u) * N + t0 + lane] : 0.f;
        __syncthreads();                                                 // the previous tile has been read
#pragma unroll
        for (int u = 0; u < W; ++u) tile[u * 65 + lane] = v[u];
        if (lane < np) {
            tl[lane] = lab[b * N + t0 + lane];
            if (WEIGHTED) tw[lane] = pixw[b * N + t0 + lane];
        }
        __syncthreads();
        if (lane < W) {
            for (int j = 0; j < np; ++j) {
                const int l = tl[j];
                if (l != cur) {
                    if (cur >= 0) bins[cur * W + lane] += acc;
                    acc = 0.0;
                    cur = l;
                }
                const double x = (double)tile[lane * 65 + j];
                acc += WEIGHTED ? x * tw[j] : x;
            }
        }
    }
    if (lane < W) {
        if (cur >= 0) bins[cur * W + lane] += acc;
        if (c0 + lane < C)
            for (int k = 0; k < K; ++k) partial[(sl * K + k) * C + c0 + lane] = bins[k * W + lane];
    }
}

// out[r][c] = the slab partials [slab][K][C] of centre r added in (image, slab) order -- eight consecutive runs of slabs by eight
// threads, the eight added in order --; with `divide`, divided by count + eps: the centre.  A workgroup owns 32 channels of a centre.
__global__ __launch_bounds__(256) void fd_merge_kernel(const double* __restrict__ partial, const int64_t* __restrict__ counts, int B, int K,
                                                       int C, int S, int cblocks, int divide, double* __restrict__ out) {
    __shared__ double part[8][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int r = blockIdx.x / cblocks, c = (blockIdx.x % cblocks) * 32 + cl;
    const int64_t n = counts[r];
    double sum = 0.0;
    if (n >= 1 && c < C) {
        const fd_span sp = fd_span_of(r, B, S);
        const int64_t per = (sp.count + 7) / 8, j0 = g * per, j1 = min(sp.count, j0 + per);
#pragma unroll 4
        for (int64_t j = j0; j < j1; ++j) sum += partial[((sp.first + j) * K + sp.cls) * C + c];
    }
    part[g][cl] = sum;
    __syncthreads();
    if (g == 0 && c < C) {
        double t = 0.0;
        for (int i = 0; i < 8; ++i) t += part[i][cl];
        out[(int64_t)r * C + c] = divide ? t / ((double)n + FD_EPS) : t;
    }
}

// one wave per product: block r < NC |c_r| -> cnorm[r]; block NC + i NC + j: c_(B+i) . c_j -> M[i][j]
__global__ __launch_bounds__(64) void fd_dots_kernel(const double* __restrict__ cen, int B, int C, int NC, double* __restrict__ cnorm,
                                                     double* __restrict__ M) {
    const int64_t id = blockIdx.x;
    int x, y;
    if (id < NC) {
        x = y = (int)id;
    } else {
        x = B + (int)((id - NC) / NC);
        y = (int)((id - NC) % NC);
    }
    const double* cx = cen + (int64_t)x * C;
    const double* cy = cen + (int64_t)y * C;
    double acc = 0.0;
    for (int c = threadIdx.x; c < C; c += 64) acc += cx[c] * cy[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (threadIdx.x == 0) {
        if (id < NC)
            cnorm[id] = sqrt(acc);
        else
            M[id - NC] = acc;
    }
}

// ---- 3. per pixel: the dot product with its centre and |f| ---------------------------------------------------------------------------
// The centre table of an image (its background centre and the K - 1 foreground centres) lies in LDS by chunks of CC channels.
// SPLIT = false: a workgroup owns 256 pixels of one image and a thread one pixel, the channels ascending -- the form of the
// backward, 1 KiB of every channel row per workgroup.  SPLIT = true, for inputs with too few pixels to fill the device that way:
// a workgroup owns 64 pixels, thread (px, q) adds the channels q, q + 4, ... and the four quarters are added in order.
// Per pixel, with k its centre, D = |f| |c_k| + eps:
//   pix = (a, b) of the backward; pixw = 1 / D; pixe = 1 - cos; pixt = (f . c_k) |f| / D^2
template <bool SPLIT>
__global__ __launch_bounds__(256) void fd_pixdot_kernel(const float* __restrict__ feat, const uint8_t* __restrict__ lab,
                                                        const double* __restrict__ cen, const double* __restrict__ cnorm,
                                                        const double* __restrict__ invcnt, const double* __restrict__ hdr, int B, int K,
                                                        int C, int N, int CC, int tiles, double* __restrict__ pix,
                                                        double* __restrict__ pixw, double* __restrict__ pixe, double* __restrict__ pixt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fd_smem[];
    double* tab = reinterpret_cast<double*>(fd_smem);                    // [K][CC + 1]; SPLIT: afterwards the reduction's [2][256]
    constexpr int PX = SPLIT ? 64 : 256, STEP = SPLIT ? 4 : 1;
    const int tid = threadIdx.x, px = SPLIT ? tid & 63 : tid, q = SPLIT ? tid >> 6 : 0;
    const int64_t b = blockIdx.x / tiles;
    const int p = (blockIdx.x % tiles) * PX + px;
    const float* fb = feat + b * C * (int64_t)N;
    const int l = p < N ? lab[b * N + p] : 0;
    double dot = 0.0, nn = 0.0;
    const int ld = CC + 1;
    for (int ch0 = 0; ch0 < C; ch0 += CC) {
        const int cc = min(CC, C - ch0);
        __syncthreads();
        for (int i = tid; i < K * cc; i += 256) {
            const int row = i / cc, c = i % cc;
            const int64_t r = row == 0 ? b : B + row - 1;
            tab[row * ld + c] = cen[r * C + ch0 + c];
        }
        __syncthreads();
        if (p < N) {
            const double* row = tab + l * ld;
            const float* fp = fb + (int64_t)ch0 * N + p;
#pragma unroll 8
            for (int c = q; c < cc; c += STEP) {
                const double f = (double)fp[(int64_t)c * N];
                dot += f * row[c];
                nn += f * f;
            }
        }
    }
    if (SPLIT) {
        __syncthreads();
        tab[tid] = dot;
        tab[256 + tid] = nn;
        __syncthreads();
        if (q != 0) return;
        dot = nn = 0.0;
        for (int w = 0; w < 4; ++w) {
            dot += tab[w * 64 + px];
            nn += tab[256 + w * 64 + px];
        }
    }
    if (p >= N) return;
    const double Z = hdr[0];
    const int64_t r = l == 0 ? b : B + l - 1;
    const double nf = sqrt(nn), cn = cnorm[r], ic = invcnt[r];
    const double D = nf * cn + FD_EPS;
    const int64_t i = b * N + p;
    pix[2 * i] = -ic / (Z * D);
    pix[2 * i + 1] = nf > 0.0 ? dot * cn * ic / (Z * nf * D * D) : 0.0;
    pixw[i] = 1.0 / D;
    pixe[i] = 1.0 - dot / D;
    pixt[i] = dot * nf / (D * D);
}

// one workgroup per slab: slabsum[slab][k] = (sum of pixe, sum of pixt) over the slab's pixels of label k.  Thread (k, g) of
// K x G, G = 256 / K, scans the g-th of G runs of every 2048-pixel piece staged in LDS for label k, the pixels ascending; the G
// sums of a class are added in order.
__global__ __launch_bounds__(256) void fd_pixsum_kernel(const uint8_t* __restrict__ lab, const double* __restrict__ pixe,
                                                        const double* __restrict__ pixt, int K, int N, int slab, int S,
                                                        double* __restrict__ slabsum) {
    __shared__ double se[2048], st[2048];
    __shared__ uint8_t sl8[2048];
    const int tid = threadIdx.x, G = 256 / K, k = tid / G, g = tid % G;
    const int64_t sl = blockIdx.x, b = sl / S, s = sl % S;
    const int p0 = (int)s * slab, p1 = min(N, p0 + slab);
    double E = 0.0, T = 0.0;
    for (int t0 = p0; t0 < p1; t0 += 2048) {
        const int np = min(2048, p1 - t0);
        __syncthreads();
        for (int j = tid; j < np; j += 256) {
            se[j] = pixe[b * N + t0 + j];
            st[j] = pixt[b * N + t0 + j];
            sl8[j] = lab[b * N + t0 + j];
        }
        __syncthreads();
        if (k < K) {
            const int per = (np + G - 1) / G, j1 = min(np, (g + 1) * per);
            for (int j = g * per; j < j1; ++j) {
                if (sl8[j] == k) {
                    E += se[j];
                    T += st[j];
                }
            }
        }
    }
    __syncthreads();
    if (k < K) {
        se[k * G + g] = E;
        st[k * G + g] = T;
    }
    __syncthreads();
    if (k < K && g == 0) {
        E = T = 0.0;
        for (int i = 0; i < G; ++i) {
            E += se[k * G + i];
            T += st[k * G + i];
        }
        slabsum[(sl * K + k) * 2] = E;
        slabsum[(sl * K + k) * 2 + 1] = T;
    }
}

// ---- finish: the loss and the coefficients of d loss / d centre -----------------------------------------------------------------
// One workgroup.  With x = c_r, y = c_j, D = |x||y| + eps and the pair's weight w (1 / (F (F - 1)) between two foreground centres,
// 1 / (2 F B) between a foreground and a background centre, 0 where the case of `dis` has no such term):
//   d cos(x, y) / dx = y / D - (x . y) |y| x / (|x| D^2)        (the second term 0 at |x| = 0)
//   G_r = gamma_r W_r + beta_r c_r + sum_j alpha_rj c_j,   gamma_r = -1 / (Z cnt'_r),   alpha_rj = w / D,
//   beta_r = s_r / (Z cnt'_r |c_r|) - sum_j w (x . y) |y| / (|x| D^2)
// cvec, NC doubles each: [0] cnorm, [1] invcnt, [2] beta, [3] gamma, [4..5] the merged pairs (E_r, s_r) = (sum of 1 - cos, sum of
// (f . c)|f| / D^2 over the centre's pixels), [6] row sum of 1 + cos over foreground partners, [7] over background partners
__global__ __launch_bounds__(256) void fd_finish_kernel(const int64_t* __restrict__ counts, const double* __restrict__ M,
                                                        const double* __restrict__ hdr, int B, int K, double* __restrict__ cvec,
                                                        double* __restrict__ alpha, float* __restrict__ loss) {
    const int NC = B + K - 1, tid = threadIdx.x;
    const double* cnorm = cvec;
    const double* invcnt = cvec + NC;
    double* beta = cvec + 2 * (int64_t)NC;
    double* gamma = cvec + 3 * (int64_t)NC;
    const double* Es = cvec + 4 * (int64_t)NC;
    double* rff = cvec + 6 * (int64_t)NC;
    double* rfb = cvec + 7 * (int64_t)NC;
    const double Z = hdr[0], F = hdr[1];
    const bool has_bg = hdr[2] != 0.0;
    const double wff = F > 1.0 ? 1.0 / (F * (F - 1.0)) : 0.0;
    const double wfb = (F >= 1.0 && has_bg) ? 1.0 / (2.0 * F * (double)B) : 0.0;
    for (int r = tid; r < NC; r += 256) {
        const bool valid = counts[r] >= 1;
        const double s = Es[2 * r + 1];
        const double cn = cnorm[r], ic = invcnt[r];
        double bt = (valid && cn > 0.0) ? ic / Z * s / cn : 0.0;
        double sff = 0.0, sfb = 0.0;
        if (r >= B) {
            const int i = r - B;
            for (int j = 0; j < NC; ++j) {
                const double m = M[(int64_t)i * NC + j], cj = cnorm[j];
                const double D = cn * cj + FD_EPS;
                double w = 0.0;
                if (valid && j < B) {
                    w = wfb;
                    sfb += 1.0 + m / D;
                } else if (valid && j != r && counts[j] >= 1) {
                    w = wff;
                    sff += 1.0 + m / D;
                }
                alpha[(int64_t)i * NC + j] = w / D;
                if (cn > 0.0) bt -= w * m * cj / (cn * D * D);
            }
        } else if (valid && cn > 0.0) {
            for (int i = 0; i < K - 1; ++i) {
                if (counts[B + i] < 1) continue;
                const double m = M[(int64_t)i * NC + r], ci = cnorm[B + i];
                const double D = cn * ci + FD_EPS;
                bt -= wfb * m * ci / (cn * D * D);
            }
        }
        beta[r] = bt;
        gamma[r] = valid ? -ic / Z : 0.0;
        rff[r] = sff;
        rfb[r] = sfb;
    }
    __syncthreads();
    if (tid == 0) {
        volatile double* vff = rff;
        volatile double* vfb = rfb;
        double pixel = 0.0, ff = 0.0, fb = 0.0;
        for (int r = 0; r < NC; ++r) {
            if (counts[r] >= 1)
                pixel += Es[2 * r] * invcnt[r];
            else if (r < B)
                pixel += 2.0;
        }
        pixel /= Z;
        for (int r = B; r < NC; ++r) {
            ff += vff[r];
            fb += vfb[r];
        }
        ff = F > 1.0 ? ff / (F * (F - 1.0)) : 0.0;
        double dis = 0.0;
        if (F >= 1.0 && has_bg)
            dis = 0.5 * ff + 0.5 * fb / (F * (double)B);
        else if (!has_bg)
            dis = 0.5 * ff + 1.0;
        loss[0] = (float)(dis + pixel);
        loss[1] = (float)dis;
        loss[2] = (float)pixel;
    }
}

// Gc[r][c] = G_r[c] / (count_r + eps): what a pixel of centre r receives through the centre; 0 for an empty centre
__global__ __launch_bounds__(256) void fd_grad_kernel(const double* __restrict__ cen, const double* __restrict__ Wsum,
                                                      const double* __restrict__ cvec, const double* __restrict__ alpha, int B, int K, int C,
                                                      int cblocks, double* __restrict__ Gc) {
    const int NC = B + K - 1;
    const int r = blockIdx.x / cblocks, c = (blockIdx.x % cblocks) * 256 + threadIdx.x;
    if (c >= C) return;
    const double ic = cvec[NC + r];
    double G = 0.0;
    if (ic != 0.0) {
        G = cvec[3 * (int64_t)NC + r] * Wsum[(int64_t)r * C + c] + cvec[2 * (int64_t)NC + r] * cen[(int64_t)r * C + c];
        if (r >= B) {
            const double* al = alpha + (int64_t)(r - B) * NC;
            for (int j = 0; j < NC; ++j) G += al[j] * cen[(int64_t)j * C + c];
        } else {
            for (int i = 0; i < K - 1; ++i) G += alpha[(int64_t)i * NC + r] * cen[(int64_t)(B + i) * C + c];
        }
    }
    Gc[(int64_t)r * C + c] = G * ic;
}

// ---- 4. backward ---------------------------------------------------------------------------------------------------------------------
// d_feat[b][c][n] = g (a_n c_k[c] + b_n f + Gc_k[c]); a workgroup owns 256 pixels of an image and a chunk of CC channels, the
// (c_k, Gc_k) pairs of the chunk in LDS
__global__ __launch_bounds__(256) void fd_bwd_kernel(const float* __restrict__ feat, const uint8_t* __restrict__ lab,
                                                     const double* __restrict__ pix, const double* __restrict__ cst,
                                                     const float* __restrict__ gscale, int B, int K, int C, int N, int CC, int tiles,
                                                     float* __restrict__ dfeat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fd_smem[];
    double2* tab = reinterpret_cast<double2*>(fd_smem);                  // [K][CC + 1]
    const int tid = threadIdx.x, NC = B + K - 1, ld = CC + 1;
    const int64_t b = blockIdx.x / tiles;
    const int p = (blockIdx.x % tiles) * 256 + tid;
    const int ch0 = blockIdx.y * CC, cc = min(CC, C - ch0);
    const double* Gc = cst + (int64_t)NC * C;
    for (int i = tid; i < K * cc; i += 256) {
        const int row = i / cc, c = i % cc;
        const int64_t r = row == 0 ? b : B + row - 1;
        tab[row * ld + c] = make_double2(cst[r * C + ch0 + c], Gc[r * C + ch0 + c]);
    }
    __syncthreads();
    if (p >= N) return;
    const double g = (double)gscale[0];
    const int64_t i = b * N + p;
    const double a = pix[2 * i], bb = pix[2 * i + 1];
    const double2* row = tab + (int)lab[i] * ld;
    const int64_t base = (b * C + ch0) * (int64_t)N + p;
#pragma unroll 8
    for (int c = 0; c < cc; ++c) {
        const double2 t = row[c];
        const double f = (double)feat[base + (int64_t)c * N];
        dfeat[base + (int64_t)c * N] = (float)(g * (a * t.x + bb * f + t.y));
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct fd_plan {
    int N, slab, S, NC;
    int64_t nslab, BN;
    size_t o_partial, o_W, o_M, o_alpha, o_slabsum, o_slabcnt, o_cvec, o_hdr, o_pixw, o_pixe, o_pixt, total;
};

static int fd_check(const char* who, int32_t B, int32_t K, int32_t C, int32_t h, int32_t w) {
    ACR_CHECK_ARG(B >= 1 && B <= FD_MAX_B, "%s: B=%d outside 1..%d", who, B, FD_MAX_B);
    ACR_CHECK_ARG(K >= 2 && K <= FD_MAX_K, "%s: K=%d outside 2..%d", who, K, FD_MAX_K);
    ACR_CHECK_ARG(C >= 1 && C <= FD_MAX_C, "%s: C=%d outside 1..%d", who, C, FD_MAX_C);
    ACR_CHECK_ARG(h >= 1 && w >= 1, "%s: h=%d, w=%d must be positive", who, h, w);
    ACR_CHECK_ARG((int64_t)B * h * w < (1ll << 31), "%s: B h w = %lld must stay below 2^31", who, (long long)B * h * w);
    return ACR_OK;
}

static fd_plan fd_make_plan(int32_t B, int32_t K, int32_t C, int32_t h, int32_t w) {
    fd_plan pl;
    pl.N = h * w;
    pl.slab = FD_SLAB * ((K + 31) / 32);
    pl.S = (pl.N + pl.slab - 1) / pl.slab;
    pl.NC = B + K - 1;
    pl.nslab = (int64_t)B * pl.S;
    pl.BN = (int64_t)B * pl.N;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += (bytes + 15) & ~(size_t)15;
        return at;
    };
    pl.o_partial = take((size_t)pl.nslab * K * C * 8);
    pl.o_W = take((size_t)pl.NC * C * 8);
    pl.o_M = take((size_t)(K - 1) * pl.NC * 8);
    pl.o_alpha = take((size_t)(K - 1) * pl.NC * 8);
    pl.o_slabsum = take((size_t)pl.nslab * K * 16);
    pl.o_slabcnt = take((size_t)pl.nslab * K * 4);
    pl.o_cvec = take((size_t)pl.NC * 8 * 8);
    pl.o_hdr = take(64);
    pl.o_pixw = take((size_t)pl.BN * 8);
    pl.o_pixe = take((size_t)pl.BN * 8);
    pl.o_pixt = take((size_t)pl.BN * 8);
    pl.total = o;
    return pl;
}

extern "C" int64_t acr_featdis_ws_bytes(int32_t B, int32_t K, int32_t C, int32_t h, int32_t w) {
    if (fd_check("acr_featdis_ws_bytes", B, K, C, h, w) != ACR_OK) return ACR_ERR_INVALID;
    return (int64_t)fd_make_plan(B, K, C, h, w).total;
}

template <bool WEIGHTED>
static void fd_launch_classsum(const fd_plan& pl, const float* feat, const uint8_t* lab, const double* pixw, int K, int C, double* partial,
                               hipStream_t st) {
    if (K <= FD_WIDE_MAX_K) {
        const size_t lds = (size_t)K * 64 * 8 + 64 * 8 + 64 * 4 + 64 * 65 * 4;
        hipLaunchKernelGGL((fd_classsum_kernel<WEIGHTED, 64>), dim3((unsigned)pl.nslab, (unsigned)((C + 63) / 64)), dim3(64), lds, st, feat, lab,
                           pixw, K, C, pl.N, pl.slab, pl.S, partial);
    } else {
        const size_t lds = (size_t)K * 32 * 8 + 64 * 8 + 64 * 4 + 32 * 65 * 4;
        hipLaunchKernelGGL((fd_classsum_kernel<WEIGHTED, 32>), dim3((unsigned)pl.nslab, (unsigned)((C + 31) / 32)), dim3(64), lds, st, feat, lab,
                           pixw, K, C, pl.N, pl.slab, pl.S, partial);
    }
}

extern "C" int acr_featdis_fwd(const float* seg, const float* feat, int32_t B, int32_t K, int32_t C, int32_t h, int32_t w, void* ws,
                               int64_t ws_bytes, float* loss, uint8_t* labels, int64_t* counts, double* pix, double* cst, void* stream) {
    const int rc = fd_check("acr_featdis_fwd", B, K, C, h, w);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(seg && feat && loss && labels && counts && pix && cst, "acr_featdis_fwd: null pointer");
    ACR_CHECK_ARG((((uintptr_t)pix | (uintptr_t)cst) & 15) == 0 && ((uintptr_t)counts & 7) == 0,
                  "acr_featdis_fwd: pix and cst must be aligned to 16 bytes, counts to 8");
    const fd_plan pl = fd_make_plan(B, K, C, h, w);
    ACR_CHECK_WS("acr_featdis_fwd", ws, 16, ws_bytes, pl.total);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    double* partial = reinterpret_cast<double*>(base + pl.o_partial);
    double* Wsum = reinterpret_cast<double*>(base + pl.o_W);
    double* M = reinterpret_cast<double*>(base + pl.o_M);
    double* alpha = reinterpret_cast<double*>(base + pl.o_alpha);
    double* slabsum = reinterpret_cast<double*>(base + pl.o_slabsum);
    int* slabcnt = reinterpret_cast<int*>(base + pl.o_slabcnt);
    double* cvec = reinterpret_cast<double*>(base + pl.o_cvec);
    double* hdr = reinterpret_cast<double*>(base + pl.o_hdr);
    double* pixw = reinterpret_cast<double*>(base + pl.o_pixw);
    double* pixe = reinterpret_cast<double*>(base + pl.o_pixe);
    double* pixt = reinterpret_cast<double*>(base + pl.o_pixt);
    double* cnorm = cvec;
    double* invcnt = cvec + pl.NC;
    double* cen = cst;
    double* Gc = cst + (int64_t)pl.NC * C;
    const int NC = pl.NC, cblocks = (C + 255) / 256, mblocks = (C + 31) / 32;

    hipLaunchKernelGGL(fd_label_kernel, dim3((unsigned)pl.nslab), dim3(256), 0, st, seg, K, pl.N, pl.slab, pl.S, labels, slabcnt);
    hipLaunchKernelGGL(fd_count_kernel, dim3((unsigned)NC), dim3(64), 0, st, (const int*)slabcnt, B, K, pl.S, counts, invcnt);
    hipLaunchKernelGGL(fd_hdr_kernel, dim3(1), dim3(256), 0, st, (const int64_t*)counts, B, K, hdr);
    fd_launch_classsum<false>(pl, feat, labels, nullptr, K, C, partial, st);
    hipLaunchKernelGGL(fd_merge_kernel, dim3((unsigned)(NC * mblocks)), dim3(256), 0, st, (const double*)partial, (const int64_t*)counts, B, K,
                       C, pl.S, mblocks, 1, cen);
    hipLaunchKernelGGL(fd_dots_kernel, dim3((unsigned)((int64_t)NC * K)), dim3(64), 0, st, (const double*)cen, B, C, NC, cnorm, M);
    {
        int CC = FD_TAB_DOUBLES / K - 1;
        if (CC > C) CC = C;
        const int64_t tiles256 = (pl.N + 255) / 256;
        const bool split = (int64_t)B * tiles256 < FD_WIDE_DOT_MIN_TILES;
        const int tiles = split ? (pl.N + 63) / 64 : (int)tiles256;
        size_t lds = (size_t)K * (CC + 1) * 8;
        if (lds < 2 * 256 * 8) lds = 2 * 256 * 8;
        if (split)
            hipLaunchKernelGGL(fd_pixdot_kernel<true>, dim3((unsigned)(B * tiles)), dim3(256), lds, st, feat, (const uint8_t*)labels,
                               (const double*)cen, (const double*)cnorm, (const double*)invcnt, (const double*)hdr, B, K, C, pl.N, CC, tiles,
                               pix, pixw, pixe, pixt);
        else
            hipLaunchKernelGGL(fd_pixdot_kernel<false>, dim3((unsigned)(B * tiles)), dim3(256), lds, st, feat, (const uint8_t*)labels,
                               (const double*)cen, (const double*)cnorm, (const double*)invcnt, (const double*)hdr, B, K, C, pl.N, CC, tiles,
                               pix, pixw, pixe, pixt);
    }
    hipLaunchKernelGGL(fd_pixsum_kernel, dim3((unsigned)pl.nslab), dim3(256), 0, st, (const uint8_t*)labels, (const double*)pixe,
                       (const double*)pixt, K, pl.N, pl.slab, pl.S, slabsum);
    fd_launch_classsum<true>(pl, feat, labels, pixw, K, C, partial, st);
    hipLaunchKernelGGL(fd_merge_kernel, dim3((unsigned)(NC * mblocks)), dim3(256), 0, st, (const double*)partial, (const int64_t*)counts, B, K,
                       C, pl.S, mblocks, 0, Wsum);
    hipLaunchKernelGGL(fd_merge_kernel, dim3((unsigned)NC), dim3(256), 0, st, (const double*)slabsum, (const int64_t*)counts, B, K, 2, pl.S, 1, 0,
                       cvec + 4 * (int64_t)NC);
    hipLaunchKernelGGL(fd_finish_kernel, dim3(1), dim3(256), 0, st, (const int64_t*)counts, (const double*)M, (const double*)hdr, B, K, cvec,
                       alpha, loss);
    hipLaunchKernelGGL(fd_grad_kernel, dim3((unsigned)(NC * cblocks)), dim3(256), 0, st, (const double*)cen, (const double*)Wsum,
                       (const double*)cvec, (const double*)alpha, B, K, C, cblocks, Gc);
    return acr_check_launch("acr_featdis_fwd");
}

extern "C" int acr_featdis_bwd(const float* feat, const uint8_t* labels, const double* pix, const double* cst, const float* gscale,
                               int32_t B, int32_t K, int32_t C, int32_t h, int32_t w, float* dfeat, void* stream) {
    const int rc = fd_check("acr_featdis_bwd", B, K, C, h, w);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(feat && labels && pix && cst && gscale && dfeat, "acr_featdis_bwd: null pointer");
    ACR_CHECK_ARG((((uintptr_t)pix | (uintptr_t)cst) & 15) == 0, "acr_featdis_bwd: pix and cst must be aligned to 16 bytes");
    const int N = h * w;
    int CC = FD_TAB_DOUBLES / (2 * K) - 1;
    if (CC > C) CC = C;
    const int tiles = (N + 255) / 256;
    const size_t lds = (size_t)K * (CC + 1) * 16;
    hipLaunchKernelGGL(fd_bwd_kernel, dim3((unsigned)(B * tiles), (unsigned)((C + CC - 1) / CC)), dim3(256), lds, (hipStream_t)stream, feat,
                       labels, pix, cst, gscale, B, K, C, N, CC, tiles, dfeat);
    return acr_check_launch("acr_featdis_bwd");
}
