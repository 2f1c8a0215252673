// The affinity stage of PSA (Ahn & Kwak, CVPR 2018) around the reference's pair labels (tool/torchutils.py:107-157
// ExtractAffinityLabelInRadius) and pair indices (tool/pyutils.py:125-159 get_indices_of_pairs): pair codes from a label map, the
// pair affinity exp(-mean_c |f_from - f_to|) with its three-term loss and gradient, and the random walk under those affinities.
// include/acr_hip.h states every rule in full.  fp32 tensors; every sum runs in double in an order that depends on the geometry
// only (offsets ascending, channels ascending, tiles ascending): no float atomics, bit-identical run to run, and a sample's
// result does not depend on the batch it rides in.  The only atomics are the 64-bit INTEGER pair counters.
//
// Offsets (dy, dx), the reference's order: dy = 0: dx = 1 .. R-1; then dy = 1 .. R-1, dx = -(R-1) .. R-1 where dx^2 + dy^2 < R^2.
// Every kernel is compiled per radius, so the offset loops unroll and the per-offset values of a pixel live in registers.
#include "acr_common.h"
#include "acr_reduce.h"

#define AFF_MIN_R 2
#define AFF_MAX_R 5
#define AFF_EPS 1e-5
#define AFF_TILE 16          // a workgroup of the loss kernels: 16 x 16 pixels, one thread each
#define AFF_CC 8             // channels staged in LDS per round
#define AFF_ST 48            // LDS row stride in floats: >= 16 + 2 (R-1) and = 16 mod 32, so the two rows a 32-lane group reads fall on disjoint banks
#define AFF_WALK_NT 1024
#define AFF_WALK_LDS 65536   // resident form: both padded planes within 64 KiB of LDS

static constexpr int aff_pairs_of(int R) {
    int n = 0;
    for (int dy = 0; dy < R; ++dy)
        for (int dx = -(R - 1); dx < R; ++dx)
            if ((dy > 0 || dx > 0) && dx * dx + dy * dy < R * R) ++n;
    return n;
}

// f(p, dy, dx) for every offset, p ascending; under full unrolling p, dy, dx are constants at every call
template <int R, typename F>
__device__ __forceinline__ void aff_for_each(F f) {
    int p = 0;
#pragma unroll
    for (int dy = 0; dy < R; ++dy) {
#pragma unroll
        for (int dx = -(R - 1); dx < R; ++dx) {
            if ((dy > 0 || dx > 0) && dx * dx + dy * dy < R * R) {
                f(p, dy, dx);
                ++p;
            }
        }
    }
}

// ---- pair codes ---------------------------------------------------------------------------------------------------------------
// One thread per from-pixel: its label once, the P partners' labels, P codes (stored along n: coalesced) and three counters that
// go wave -> workgroup -> one 64-bit integer atomic per workgroup and code.
template <int R>
__global__ __launch_bounds__(256) void aff_codes_kernel(const uint8_t* __restrict__ map, int S0, int S1, int stride, int h, int w,
                                                        uint8_t* __restrict__ codes, unsigned long long* __restrict__ counts) {
    constexpr int r = R - 1, P = aff_pairs_of(R);
    const int Nw = w - 2 * r, N = (h - r) * Nw;
    const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    unsigned cnt[3] = {0u, 0u, 0u};
    if (n < N) {
        const int yy = n / Nw, xx = n - yy * Nw;
        const uint8_t* m = map + (int64_t)b * S0 * S1;
        const int lf = m[(int64_t)(yy * stride) * S1 + (int64_t)(r + xx) * stride];
        uint8_t* out = codes + (int64_t)b * P * N + n;
        aff_for_each<R>([&](int p, int dy, int dx) {
            const int lt = m[(int64_t)((yy + dy) * stride) * S1 + (int64_t)(r + xx + dx) * stride];
            const bool valid = lf < 255 && lt < 255;
            int code = 0;
            if (lf == lt) {
                if (lf == 0) code = 1;
                else if (valid) code = 2;
            } else if (valid) {
                code = 3;
            }
            out[(int64_t)p * N] = (uint8_t)code;
            cnt[0] += code == 1;
            cnt[1] += code == 2;
            cnt[2] += code == 3;
        });
    }
    __shared__ unsigned sh[3][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        unsigned v = cnt[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) sh[k][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned t = sh[threadIdx.x][0] + sh[threadIdx.x][1] + sh[threadIdx.x][2] + sh[threadIdx.x][3];
        if (t) atomicAdd(counts + threadIdx.x, (unsigned long long)t);
    }
}

// ---- affinity and loss, forward -----------------------------------------------------------------------------------------------
// A workgroup owns 16 x 16 from-pixels of one sample.  Per round AFF_CC channels of the rows y .. y+r and columns x-r .. x+r the
// tile needs are staged in LDS; a thread keeps the P channel sums of its pixel in registers (double) and adds one channel at a
// time, channels ascending.  Pixels outside the image are staged as 0: only threads outside the from-region read them, and those
// write nothing.
template <int R>
__global__ __launch_bounds__(256) void aff_fwd_kernel(const float* __restrict__ feat, int C, int h, int w,
                                                      const uint8_t* __restrict__ codes, const int64_t* __restrict__ counts,
                                                      float* __restrict__ aff, float* __restrict__ g, double* __restrict__ partial) {
    constexpr int r = R - 1, P = aff_pairs_of(R), HR = AFF_TILE + r, HC = AFF_TILE + 2 * r;
    static_assert(HC <= AFF_ST, "LDS row stride too small");
    __shared__ float tile[AFF_CC][HR][AFF_ST];
    __shared__ double red[3][256];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int b = blockIdx.z, ty0 = blockIdx.y * AFF_TILE, tx0 = blockIdx.x * AFF_TILE;
    const int Nw = w - 2 * r, Nh = h - r;
    const int64_t hw = (int64_t)h * w;
    feat += (int64_t)b * C * hw;

    double acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0.0;

    for (int c0 = 0; c0 < C; c0 += AFF_CC) {
        const int nc = min(AFF_CC, C - c0);
        __syncthreads();                                     // the previous round's reads are done
        for (int i = tid; i < nc * HR * HC; i += 256) {
            const int c = i / (HR * HC), rem = i - c * (HR * HC), y = rem / HC, x = rem - y * HC;
            const int gy = ty0 + y, gx = tx0 + x;            // pixel coordinates: the halo starts r columns left of from-column tx0
            tile[c][y][x] = (gy < h && gx < w) ? feat[(int64_t)(c0 + c) * hw + (int64_t)gy * w + gx] : 0.f;
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const double me = (double)tile[c][ly][lx + r];
            aff_for_each<R>([&](int p, int dy, int dx) { acc[p] += fabs(me - (double)tile[c][ly + dy][lx + r + dx]); });
        }
    }

    const int yy = ty0 + ly, xx = tx0 + lx;
    const bool valid = yy < Nh && xx < Nw;
    double s[3] = {0.0, 0.0, 0.0};
    if (valid) {
        const int64_t N = (int64_t)Nh * Nw, n = (int64_t)yy * Nw + xx, base = (int64_t)b * P * N + n;
        double wk[3] = {0.0, 0.0, 0.0};
        if (codes) {
            wk[0] = 0.25 / ((double)counts[0] + AFF_EPS);
            wk[1] = 0.25 / ((double)counts[1] + AFF_EPS);
            wk[2] = 0.5 / ((double)counts[2] + AFF_EPS);
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const double a = exp(-(acc[p] / (double)C));
            if (aff) aff[base + (int64_t)p * N] = (float)a;
            if (codes) {
                const int code = codes[base + (int64_t)p * N];
                double gv = 0.0;
                if (code == 1 || code == 2) {
                    s[code - 1] += -log(a + AFF_EPS);
                    gv = wk[code - 1] * (a / (a + AFF_EPS));
                } else if (code == 3) {
                    const double q = 1.0 + AFF_EPS - a;
                    s[2] += -log(q);
                    gv = -wk[2] * (a / q);
                }
                g[base + (int64_t)p * N] = (float)gv;
            }
        }
    }
    if (!codes) return;                                      // uniform: the inference forward has no sums
    red[0][tid] = s[0];
    red[1][tid] = s[1];
    red[2][tid] = s[2];
    acr_tree_sum256(tid, [&](int i, int j) {
        red[0][i] += red[0][j];
        red[1][i] += red[1][j];
        red[2][i] += red[2][j];
    });
    if (tid == 0) {
        const int64_t blk = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[blk * 3 + 0] = red[0][0];
        partial[blk * 3 + 1] = red[1][0];
        partial[blk * 3 + 2] = red[2][0];
    }
}

// the workgroups' sums, workgroups ascending per thread, then the tree: loss4 = (loss, bg, fg, neg)
__global__ __launch_bounds__(256) void aff_loss_finish_kernel(const double* __restrict__ partial, int64_t nblk,
                                                              const int64_t* __restrict__ counts, float* __restrict__ loss4) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = tid; i < nblk; i += 256) {
        s[0] += partial[i * 3 + 0];
        s[1] += partial[i * 3 + 1];
        s[2] += partial[i * 3 + 2];
    }
    red[0][tid] = s[0];
    red[1][tid] = s[1];
    red[2][tid] = s[2];
    acr_tree_sum256(tid, [&](int i, int j) {
        red[0][i] += red[0][j];
        red[1][i] += red[1][j];
        red[2][i] += red[2][j];
    });
    if (tid == 0) {
        const double bg = red[0][0] / ((double)counts[0] + AFF_EPS);
        const double fg = red[1][0] / ((double)counts[1] + AFF_EPS);
        const double neg = red[2][0] / ((double)counts[2] + AFF_EPS);
        loss4[0] = (float)(bg / 4 + fg / 4 + neg / 2);
        loss4[1] = (float)bg;
        loss4[2] = (float)fg;
        loss4[3] = (float)neg;
    }
}

// ---- affinity loss, backward (gather) -----------------------------------------------------------------------------------------
// A workgroup owns 16 x 16 pixels of one sample; a thread keeps the 2 P pair gradients its pixel takes part in -- as the "from" of
// offset p, and as the "to" of the pair whose from-pixel lies at the mirrored offset -- in registers (0 where there is no such
// pair) and gathers sign(f_me - f_partner) per channel from the staged rows y-r .. y+r, columns x-r .. x+r.
template <int R>
__global__ __launch_bounds__(256) void aff_bwd_kernel(const float* __restrict__ feat, const float* __restrict__ g,
                                                      const float* __restrict__ gscale, int C, int h, int w, float* __restrict__ dfeat) {
    constexpr int r = R - 1, P = aff_pairs_of(R), HH = AFF_TILE + 2 * r;
    static_assert(HH <= AFF_ST, "LDS row stride too small");
    __shared__ float tile[AFF_CC][HH][AFF_ST];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int b = blockIdx.z, py0 = blockIdx.y * AFF_TILE, px0 = blockIdx.x * AFF_TILE;
    const int py = py0 + ly, px = px0 + lx;
    const int Nw = w - 2 * r, Nh = h - r;
    const int64_t hw = (int64_t)h * w, N = (int64_t)Nh * Nw;
    const bool inimg = py < h && px < w;
    feat += (int64_t)b * C * hw;
    dfeat += (int64_t)b * C * hw;
    g += (int64_t)b * P * N;

    float gf[P], gt[P];
    const bool isfrom = inimg && py < Nh && px >= r && px < w - r;
    aff_for_each<R>([&](int p, int dy, int dx) {
        gf[p] = isfrom ? g[(int64_t)p * N + (int64_t)py * Nw + (px - r)] : 0.f;
        const int fy = py - dy, fx = px - dx;
        const bool isto = inimg && fy >= 0 && fy < Nh && fx >= r && fx < w - r;
        gt[p] = isto ? g[(int64_t)p * N + (int64_t)fy * Nw + (fx - r)] : 0.f;
    });
    const double scale = (double)gscale[0] / (double)C;

    for (int c0 = 0; c0 < C; c0 += AFF_CC) {
        const int nc = min(AFF_CC, C - c0);
        __syncthreads();
        for (int i = tid; i < nc * HH * HH; i += 256) {
            const int c = i / (HH * HH), rem = i - c * (HH * HH), y = rem / HH, x = rem - y * HH;
            const int gy = py0 - r + y, gx = px0 - r + x;
            tile[c][y][x] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? feat[(int64_t)(c0 + c) * hw + (int64_t)gy * w + gx] : 0.f;
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const float me = tile[c][ly + r][lx + r];
            double s = 0.0;
            aff_for_each<R>([&](int p, int dy, int dx) {
                const float a = tile[c][ly + r + dy][lx + r + dx];
                s += (double)(me > a ? gf[p] : (me < a ? -gf[p] : 0.f));
                const float e = tile[c][ly + r - dy][lx + r - dx];
                s += (double)(me > e ? gt[p] : (me < e ? -gt[p] : 0.f));
            });
            if (inimg) dfeat[(int64_t)(c0 + c) * hw + (int64_t)py * w + px] = (float)(s * scale);
        }
    }
}

// ---- random walk --------------------------------------------------------------------------------------------------------------
// Weight table wt (B, 2 P + 1, h w): tap 0 the pixel itself, tap 1 + 2 p the partner at +offset p (the pair this pixel starts),
// tap 2 + 2 p the partner at -offset p (the pair that ends here); A = aff^beta, 1 for the pixel itself, 0 where there is no such
// pair; every tap divided by the column sum (1, then the taps ascending, in double).
template <int R>
__global__ __launch_bounds__(256) void aff_walk_weights_kernel(const float* __restrict__ aff, int h, int w, double beta,
                                                               float* __restrict__ wt) {
    constexpr int r = R - 1, P = aff_pairs_of(R), T = 2 * P + 1;
    const int hw = h * w, Nw = w - 2 * r, Nh = h - r;
    const int64_t N = (int64_t)Nh * Nw;
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= hw) return;
    const int py = j / w, px = j - py * w;
    aff += (int64_t)b * P * N;
    wt += (int64_t)b * T * hw + j;
    const bool isfrom = py < Nh && px >= r && px < w - r;
    auto fwd = [&](int p) { return isfrom ? pow((double)aff[(int64_t)p * N + (int64_t)py * Nw + (px - r)], beta) : 0.0; };
    auto bwd = [&](int p, int dy, int dx) {
        const int fy = py - dy, fx = px - dx;
        return (fy >= 0 && fy < Nh && fx >= r && fx < w - r) ? pow((double)aff[(int64_t)p * N + (int64_t)fy * Nw + (fx - r)], beta) : 0.0;
    };
    double colsum = 1.0;
    aff_for_each<R>([&](int p, int dy, int dx) {
        colsum += fwd(p);
        colsum += bwd(p, dy, dx);
    });
    wt[0] = (float)(1.0 / colsum);
    aff_for_each<R>([&](int p, int dy, int dx) {
        wt[(int64_t)(1 + 2 * p) * hw] = (float)(fwd(p) / colsum);
        wt[(int64_t)(2 + 2 * p) * hw] = (float)(bwd(p, dy, dx) / colsum);
    });
}

// One pixel of one step: new[j] = sum_t wt[t][j] * old[nbr_t(j)], taps ascending, in double, rounded once.  `old` is a PADDED plane:
// (R-1) w + (R-1) zeros lie in front of pixel 0 and behind pixel h w - 1, so j +- (dy w + dx) is always inside; a tap that leaves
// the image or wraps into a neighbouring row has weight 0 and meets a finite value.  oj = index of pixel j in `old`.
template <int R>
__device__ __forceinline__ float aff_walk_pixel(const float* __restrict__ wt_j, int hw, const float* old, int oj, int w) {
    double acc = (double)wt_j[0] * (double)old[oj];
    aff_for_each<R>([&](int p, int dy, int dx) {
        const int off = dy * w + dx;
        acc = fma((double)wt_j[(int64_t)(1 + 2 * p) * hw], (double)old[oj + off], acc);
        acc = fma((double)wt_j[(int64_t)(2 + 2 * p) * hw], (double)old[oj - off], acc);
    });
    return (float)acc;
}

// all steps of one (image, plane) in one workgroup, the padded plane ping-ponged in LDS
template <int R>
__global__ __launch_bounds__(AFF_WALK_NT) void aff_walk_resident_kernel(const float* __restrict__ wt, const float* __restrict__ scores,
                                                                        float* __restrict__ out, int K, int h, int w, int steps) {
    constexpr int r = R - 1, P = aff_pairs_of(R), T = 2 * P + 1;
    extern __shared__ float aff_walk_smem[];
    const int hw = h * w, pad = r * w + r, stride = hw + 2 * pad;
    const int plane = blockIdx.x, b = plane / K, tid = threadIdx.x;
    wt += (int64_t)b * T * hw;
    scores += (int64_t)plane * hw;
    out += (int64_t)plane * hw;
    for (int i = tid; i < 2 * stride; i += AFF_WALK_NT) aff_walk_smem[i] = 0.f;
    __syncthreads();
    for (int j = tid; j < hw; j += AFF_WALK_NT) aff_walk_smem[pad + j] = scores[j];
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int co = pad + (s & 1) * stride, no = pad + ((s & 1) ^ 1) * stride;
        for (int j = tid; j < hw; j += AFF_WALK_NT) aff_walk_smem[no + j] = aff_walk_pixel<R>(wt + j, hw, aff_walk_smem, co + j, w);
        __syncthreads();
    }
    const int fo = pad + (steps & 1) * stride;
    for (int j = tid; j < hw; j += AFF_WALK_NT) out[j] = aff_walk_smem[fo + j];
}

// one step on padded planes in global memory (planes, h w + 2 pad), through the same pixel function
template <int R>
__global__ __launch_bounds__(256) void aff_walk_step_kernel(const float* __restrict__ wt, const float* __restrict__ cur,
                                                            float* __restrict__ nxt, int K, int h, int w) {
    constexpr int r = R - 1, P = aff_pairs_of(R), T = 2 * P + 1;
    const int hw = h * w, pad = r * w + r, stride = hw + 2 * pad;
    const int j = blockIdx.x * 256 + threadIdx.x, plane = blockIdx.y, b = plane / K;
    if (j >= hw) return;
    nxt[(int64_t)plane * stride + pad + j] = aff_walk_pixel<R>(wt + (int64_t)b * T * hw + j, hw, cur + (int64_t)plane * stride, pad + j, w);
}

// dir 0: plain (planes, hw) -> padded; dir 1: padded -> plain.  The pads are never written.
__global__ __launch_bounds__(256) void aff_walk_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int hw, int pad, int dir) {
    const int j = blockIdx.x * 256 + threadIdx.x, plane = blockIdx.y;
    if (j >= hw) return;
    const int64_t plain = (int64_t)plane * hw + j, padded = (int64_t)plane * (hw + 2 * pad) + pad + j;
    if (dir == 0) dst[padded] = src[plain];
    else dst[plain] = src[padded];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
#define AFF_FOR_R(R, BODY)                       \
    switch (R) {                                 \
        case 2: { constexpr int RR = 2; BODY; } break; \
        case 3: { constexpr int RR = 3; BODY; } break; \
        case 4: { constexpr int RR = 4; BODY; } break; \
        case 5: { constexpr int RR = 5; BODY; } break; \
    }

static int aff_check_geo(const char* who, int32_t B, int32_t h, int32_t w, int32_t R) {
    ACR_CHECK_ARG(R >= AFF_MIN_R && R <= AFF_MAX_R, "%s: radius %d outside %d..%d", who, R, AFF_MIN_R, AFF_MAX_R);
    ACR_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d outside 1..65535", who, B);
    ACR_CHECK_ARG(h > R - 1 && w > 2 * (R - 1), "%s: a %d x %d grid has no pair at radius %d (needs h > %d, w > %d)", who, h, w, R, R - 1,
                  2 * (R - 1));
    ACR_CHECK_ARG(h <= 4096 && w <= 4096, "%s: grid %d x %d beyond 4096 x 4096", who, h, w);
    return ACR_OK;
}

extern "C" int32_t acr_aff_pairs(int32_t R) { return (R >= AFF_MIN_R && R <= AFF_MAX_R) ? aff_pairs_of(R) : -1; }

extern "C" int acr_aff_pair_codes(const uint8_t* label_map, int32_t B, int32_t S0, int32_t S1, int32_t stride, int32_t R, uint8_t* codes,
                                  int64_t* counts, void* stream) {
    ACR_CHECK_ARG(label_map && codes && counts, "acr_aff_pair_codes: null pointer");
    ACR_CHECK_ARG(stride >= 1 && S0 >= 1 && S1 >= 1 && S0 % stride == 0 && S1 % stride == 0,
                  "acr_aff_pair_codes: map %d x %d is no multiple of stride %d", S0, S1, stride);
    ACR_CHECK_ARG(S0 <= 32768 && S1 <= 32768, "acr_aff_pair_codes: map %d x %d beyond 32768 x 32768", S0, S1);
    const int h = S0 / stride, w = S1 / stride;
    int rc = aff_check_geo("acr_aff_pair_codes", B, h, w, R);
    if (rc != ACR_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st) != hipSuccess) {
        acr_set_error("acr_aff_pair_codes: clearing the counters failed");
        return ACR_ERR_INVALID;
    }
    const int N = (h - (R - 1)) * (w - 2 * (R - 1));
    const dim3 grid((N + 255) / 256, B);
    AFF_FOR_R(R, hipLaunchKernelGGL((aff_codes_kernel<RR>), grid, dim3(256), 0, st, label_map, S0, S1, stride, h, w, codes,
                                    (unsigned long long*)counts));
    return acr_check_launch("acr_aff_pair_codes");
}

static int64_t aff_loss_blocks(int32_t B, int32_t h, int32_t w, int32_t R) {
    const int Nh = h - (R - 1), Nw = w - 2 * (R - 1);
    return (int64_t)B * ((Nh + AFF_TILE - 1) / AFF_TILE) * ((Nw + AFF_TILE - 1) / AFF_TILE);
}

extern "C" int64_t acr_aff_loss_ws_bytes(int32_t B, int32_t h, int32_t w, int32_t R) {
    if (aff_check_geo("acr_aff_loss_ws_bytes", B, h, w, R) != ACR_OK) return -1;
    return aff_loss_blocks(B, h, w, R) * 3 * (int64_t)sizeof(double);
}

extern "C" int acr_aff_loss_fwd(const float* feat, int32_t B, int32_t C, int32_t h, int32_t w, int32_t R, const uint8_t* codes,
                                const int64_t* counts, float* aff, float* g, void* ws, int64_t ws_bytes, float* loss4, void* stream) {
    ACR_CHECK_ARG(feat, "acr_aff_loss_fwd: null pointer");
    ACR_CHECK_ARG(C >= 1 && C <= (1 << 20), "acr_aff_loss_fwd: C=%d outside 1..2^20", C);
    int rc = aff_check_geo("acr_aff_loss_fwd", B, h, w, R);
    if (rc != ACR_OK) return rc;
    if (codes) {
        ACR_CHECK_ARG(counts && g && ws && loss4, "acr_aff_loss_fwd: codes need counts, g, ws and loss4");
        ACR_CHECK_WS("acr_aff_loss_fwd", ws, 8, ws_bytes, acr_aff_loss_ws_bytes(B, h, w, R));
    } else {
        ACR_CHECK_ARG(aff, "acr_aff_loss_fwd: without codes there is nothing to write but aff");
    }
    const int Nh = h - (R - 1), Nw = w - 2 * (R - 1);
    const dim3 grid((Nw + AFF_TILE - 1) / AFF_TILE, (Nh + AFF_TILE - 1) / AFF_TILE, B);
    hipStream_t st = (hipStream_t)stream;
    AFF_FOR_R(R, hipLaunchKernelGGL((aff_fwd_kernel<RR>), grid, dim3(256), 0, st, feat, C, h, w, codes, counts, aff, g, (double*)ws));
    rc = acr_check_launch("acr_aff_loss_fwd");
    if (rc != ACR_OK || !codes) return rc;
    hipLaunchKernelGGL(aff_loss_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, aff_loss_blocks(B, h, w, R), counts, loss4);
    return acr_check_launch("acr_aff_loss_fwd (finish)");
}

extern "C" int acr_aff_loss_bwd(const float* feat, const float* g, const float* gscale, int32_t B, int32_t C, int32_t h, int32_t w,
                                int32_t R, float* dfeat, void* stream) {
    ACR_CHECK_ARG(feat && g && gscale && dfeat, "acr_aff_loss_bwd: null pointer");
    ACR_CHECK_ARG(feat != dfeat, "acr_aff_loss_bwd: dfeat must not be feat (a gather cannot run in place)");
    ACR_CHECK_ARG(C >= 1 && C <= (1 << 20), "acr_aff_loss_bwd: C=%d outside 1..2^20", C);
    int rc = aff_check_geo("acr_aff_loss_bwd", B, h, w, R);
    if (rc != ACR_OK) return rc;
    const dim3 grid((w + AFF_TILE - 1) / AFF_TILE, (h + AFF_TILE - 1) / AFF_TILE, B);
    AFF_FOR_R(R, hipLaunchKernelGGL((aff_bwd_kernel<RR>), grid, dim3(256), 0, (hipStream_t)stream, feat, g, gscale, C, h, w, dfeat));
    return acr_check_launch("acr_aff_loss_bwd");
}

extern "C" int acr_aff_walk_weights(const float* aff, int32_t B, int32_t h, int32_t w, int32_t R, double beta, float* wt, void* stream) {
    ACR_CHECK_ARG(aff && wt, "acr_aff_walk_weights: null pointer");
    ACR_CHECK_ARG(beta > 0, "acr_aff_walk_weights: beta=%g must be positive", beta);
    int rc = aff_check_geo("acr_aff_walk_weights", B, h, w, R);
    if (rc != ACR_OK) return rc;
    const dim3 grid((h * w + 255) / 256, B);
    AFF_FOR_R(R, hipLaunchKernelGGL((aff_walk_weights_kernel<RR>), grid, dim3(256), 0, (hipStream_t)stream, aff, h, w, beta, wt));
    return acr_check_launch("acr_aff_walk_weights");
}

static int64_t aff_walk_stride(int32_t h, int32_t w, int32_t R) { return (int64_t)h * w + 2 * ((int64_t)(R - 1) * w + (R - 1)); }

extern "C" int32_t acr_aff_walk_resident(int32_t h, int32_t w, int32_t R) {
    if (aff_check_geo("acr_aff_walk_resident", 1, h, w, R) != ACR_OK) return -1;
    return 2 * aff_walk_stride(h, w, R) * (int64_t)sizeof(float) <= AFF_WALK_LDS ? 1 : 0;
}

extern "C" int64_t acr_aff_walk_ws_bytes(int32_t B, int32_t K, int32_t h, int32_t w, int32_t R) {
    if (aff_check_geo("acr_aff_walk_ws_bytes", B, h, w, R) != ACR_OK || K < 1 || (int64_t)B * K > 65535) return -1;
    return 2 * (int64_t)B * K * aff_walk_stride(h, w, R) * (int64_t)sizeof(float);
}

extern "C" int acr_aff_walk(const float* wt, const float* scores, float* out, int32_t B, int32_t K, int32_t h, int32_t w, int32_t R,
                            int32_t steps, int32_t resident, void* ws, int64_t ws_bytes, void* stream) {
    ACR_CHECK_ARG(wt && scores && out, "acr_aff_walk: null pointer");
    ACR_CHECK_ARG(scores != out, "acr_aff_walk: out must not be scores");
    int rc = aff_check_geo("acr_aff_walk", B, h, w, R);
    if (rc != ACR_OK) return rc;
    ACR_CHECK_ARG(K >= 1 && (int64_t)B * K <= 65535, "acr_aff_walk: B * K = %lld outside 1..65535", (long long)B * K);
    ACR_CHECK_ARG(steps >= 0 && steps <= (1 << 20), "acr_aff_walk: steps=%d outside 0..2^20", steps);
    ACR_CHECK_ARG(resident >= -1 && resident <= 1, "acr_aff_walk: resident=%d is none of -1 (choose), 0, 1", resident);
    const int fits = acr_aff_walk_resident(h, w, R);
    ACR_CHECK_ARG(resident != 1 || fits == 1, "acr_aff_walk: two padded %d x %d planes do not fit in %d bytes of LDS", h, w, AFF_WALK_LDS);
    hipStream_t st = (hipStream_t)stream;
    const int hw = h * w, planes = B * K;
    if (steps == 0) {
        if (hipMemcpyAsync(out, scores, (size_t)planes * hw * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            acr_set_error("acr_aff_walk: copy failed");
            return ACR_ERR_INVALID;
        }
        return ACR_OK;
    }
    const int64_t stride = aff_walk_stride(h, w, R);
    if (resident == 1) {                                     // -1 chooses the stepwise form: the faster one at every plane count measured
        const size_t lds = (size_t)(2 * stride) * sizeof(float);
        AFF_FOR_R(R, hipLaunchKernelGGL((aff_walk_resident_kernel<RR>), dim3(planes), dim3(AFF_WALK_NT), lds, st, wt, scores, out, K, h, w,
                                        steps));
        return acr_check_launch("acr_aff_walk (resident)");
    }
    ACR_CHECK_WS("acr_aff_walk (stepwise)", ws, 4, ws_bytes, acr_aff_walk_ws_bytes(B, K, h, w, R));
    float* buf[2] = {(float*)ws, (float*)ws + (int64_t)planes * stride};
    if (hipMemsetAsync(ws, 0, (size_t)(2 * planes * stride) * sizeof(float), st) != hipSuccess) {
        acr_set_error("acr_aff_walk: clearing ws failed");
        return ACR_ERR_INVALID;
    }
    const dim3 grid((hw + 255) / 256, planes);
    const int pad = (R - 1) * w + (R - 1);
    hipLaunchKernelGGL(aff_walk_copy_kernel, grid, dim3(256), 0, st, scores, buf[0], hw, pad, 0);
    for (int s = 0; s < steps; ++s) {
        AFF_FOR_R(R, hipLaunchKernelGGL((aff_walk_step_kernel<RR>), grid, dim3(256), 0, st, wt, buf[s & 1], buf[(s & 1) ^ 1], K, h, w));
    }
    hipLaunchKernelGGL(aff_walk_copy_kernel, grid, dim3(256), 0, st, (const float*)buf[steps & 1], out, hw, pad, 1);
    return acr_check_launch("acr_aff_walk (stepwise)");
}
