// Pixel-adaptive mask refinement (pamr.py:10-144 of the reference: LocalAffinityAbs / LocalStDev / LocalAffinityCopy + PAMR.forward)
// as two fp32 kernels.  Both are streaming kernels over planar (.., H, W) tensors with one thread per pixel: consecutive lanes hold
// consecutive pixels of the flattened H * W plane, so every plane load and store is coalesced (a clamped gather at the image border
// repeats addresses inside a wave, which the vector cache merges).  No atomics and a fixed summation order: results are
// bit-reproducible and a sample's result does not depend on the batch it rides in.  Neighbour coordinates are clamped (replicate
// padding), so nothing outside the tensors is ever read.
//
//   neighbour p = 8 * i + j of dilation d_i: j walks (dy, dx) in {-1, 0, 1}^2 row-major without the centre.
#include "acr_common.h"

#define PAMR_MAX_DIL 8
#define PAMR_CH 8          // mask channels per propagate thread: the P weights are read once per chunk of PAMR_CH channels

struct pamr_dil {
    int d[PAMR_MAX_DIL];
};

// (dy, dx) of neighbour j in 0..7
#define PAMR_DY(j) ((((j) < 4 ? (j) : (j) + 1) / 3) - 1)
#define PAMR_DX(j) ((((j) < 4 ? (j) : (j) + 1) % 3) - 1)

// w[b][p][y][x] = softmax_p( mean_k -|x_k(y, x) - x_k(n_p)| / (1e-8 + 0.1 * std_k) ), std_k the unbiased deviation of the 9 * D
// samples of channel k (each dilation counts the centre once).  The samples are kept as differences to the centre -- exactly the
// |.| terms needed afterwards, and the deviation of the differences is the deviation of the samples -- so a flat neighbourhood
// gives differences, mean and deviation of exactly 0 and therefore exactly uniform weights.  Two-pass deviation; 8 * D
// differences and 8 * D running sums in registers.
template <int D>
__global__ __launch_bounds__(256) void pamr_affinity_kernel(const float* __restrict__ x, int K, int H, int W, pamr_dil dil,
                                                            float* __restrict__ w) {
    constexpr int P = 8 * D;
    const int64_t hw = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int py = (int)(pix / W), px = (int)(pix - (int64_t)py * W);
    const int b = blockIdx.y;
    x += (int64_t)b * K * hw;
    w += (int64_t)b * P * hw + pix;

    int offs_y[D][3], offs_x[D][3];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const int d = dil.d[i];
        offs_y[i][0] = max(py - d, 0) * W;
        offs_y[i][1] = py * W;
        offs_y[i][2] = min(py + d, H - 1) * W;
        offs_x[i][0] = max(px - d, 0);
        offs_x[i][1] = px;
        offs_x[i][2] = min(px + d, W - 1);
    }

    float acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0.f;
    const float n = (float)(9 * D);
    for (int k = 0; k < K; ++k) {
        const float* xk = x + (int64_t)k * hw;
        const float c = xk[pix];
        float df[P];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = xk[(int64_t)offs_y[i][PAMR_DY(j) + 1] + offs_x[i][PAMR_DX(j) + 1]];
                df[8 * i + j] = c - v;
                sum += df[8 * i + j];
            }
        const float mean = sum / n;
        float ssq = 0.f;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const float e = df[p] - mean;
            ssq += e * e;
        }
        ssq += (float)D * (mean * mean);                 // the D centre samples: difference 0
        const float sd = sqrtf(ssq / (n - 1.f));
        const float den = 1e-8f + 0.1f * sd;
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p] += -fabsf(df[p]) / den;
    }
    const float kf = (float)K;
    float mx = -INFINITY;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        acc[p] = acc[p] / kf;
        mx = fmaxf(mx, acc[p]);
    }
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        acc[p] = expf(acc[p] - mx);
        s += acc[p];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) w[(int64_t)p * hw] = acc[p] / s;
}

// One iteration: out[b][c][y][x] = sum_p w[b][p][y][x] * in[b][c][n_p(y, x)], p ascending.  blockIdx.y = chunk of PAMR_CH channels,
// blockIdx.z = sample: a thread reads each of its P weights once (streamed, never reused by another thread) and gathers PAMR_CH
// mask planes with it; the gathers overlap between neighbouring threads and iterations and are served by the caches.
__global__ __launch_bounds__(256) void pamr_propagate_kernel(const float* __restrict__ w, const float* __restrict__ in,
                                                             float* __restrict__ out, int C, int H, int W, pamr_dil dil, int n_dil) {
    const int64_t hw = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int py = (int)(pix / W), px = (int)(pix - (int64_t)py * W);
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * PAMR_CH;
    const int nc = min(PAMR_CH, C - c0);
    w += (int64_t)b * (8 * n_dil) * hw + pix;
    in += ((int64_t)b * C + c0) * hw;
    out += ((int64_t)b * C + c0) * hw + pix;
    float acc[PAMR_CH];
#pragma unroll
    for (int c = 0; c < PAMR_CH; ++c) acc[c] = 0.f;
    for (int i = 0; i < n_dil; ++i) {
        const int d = dil.d[i];
        const int oy[3] = {max(py - d, 0) * W, py * W, min(py + d, H - 1) * W};
        const int ox[3] = {max(px - d, 0), px, min(px + d, W - 1)};
        float wv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) wv[j] = w[(int64_t)(8 * i + j) * hw];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float* src = in + ((int64_t)oy[PAMR_DY(j) + 1] + ox[PAMR_DX(j) + 1]);
#pragma unroll
            for (int c = 0; c < PAMR_CH; ++c)
                if (c < nc) acc[c] += wv[j] * src[(int64_t)c * hw];
        }
    }
#pragma unroll
    for (int c = 0; c < PAMR_CH; ++c)
        if (c < nc) out[(int64_t)c * hw] = acc[c];
}

static int pamr_check_dil(const char* who, const int32_t* dilations, int32_t n_dil, pamr_dil* out) {
    ACR_CHECK_ARG(dilations, "%s: null pointer", who);
    ACR_CHECK_ARG(n_dil >= 1 && n_dil <= PAMR_MAX_DIL, "%s: n_dil=%d outside 1..%d", who, n_dil, PAMR_MAX_DIL);
    for (int i = 0; i < PAMR_MAX_DIL; ++i) out->d[i] = 1;
    for (int i = 0; i < n_dil; ++i) {
        ACR_CHECK_ARG(dilations[i] >= 1, "%s: dilation[%d]=%d < 1", who, i, dilations[i]);
        out->d[i] = dilations[i];
    }
    return ACR_OK;
}

static int pamr_check_dims(const char* who, int32_t B, int32_t C, int32_t H, int32_t W) {
    ACR_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "%s: bad geometry B=%d C=%d H=%d W=%d", who, B, C, H, W);
    ACR_CHECK_ARG((int64_t)H * W < (1ll << 31) - 256, "%s: image too large (%d x %d)", who, H, W);
    ACR_CHECK_ARG(B <= 65535 && (C + PAMR_CH - 1) / PAMR_CH <= 65535, "%s: B=%d C=%d beyond the launch grid", who, B, C);
    return ACR_OK;
}

extern "C" int acr_pamr_affinity(const float* x, int32_t B, int32_t K, int32_t H, int32_t W, const int32_t* dilations, int32_t n_dil,
                                 float* w_out, void* stream) {
    ACR_CHECK_ARG(x && w_out, "acr_pamr_affinity: null pointer");
    pamr_dil dil;
    int rc = pamr_check_dil("acr_pamr_affinity", dilations, n_dil, &dil);
    if (rc != ACR_OK) return rc;
    rc = pamr_check_dims("acr_pamr_affinity", B, K, H, W);
    if (rc != ACR_OK) return rc;
    const dim3 grid((unsigned)(((int64_t)H * W + 255) / 256), B);
    hipStream_t st = (hipStream_t)stream;
#define PAMR_AFF(DD) \
    case DD: hipLaunchKernelGGL((pamr_affinity_kernel<DD>), grid, dim3(256), 0, st, x, K, H, W, dil, w_out); break
    switch (n_dil) {
        PAMR_AFF(1);
        PAMR_AFF(2);
        PAMR_AFF(3);
        PAMR_AFF(4);
        PAMR_AFF(5);
        PAMR_AFF(6);
        PAMR_AFF(7);
        PAMR_AFF(8);
    }
#undef PAMR_AFF
    return acr_check_launch("acr_pamr_affinity");
}

extern "C" int acr_pamr_propagate(const float* w, const float* mask_in, float* mask_out, int32_t B, int32_t C, int32_t H, int32_t W,
                                  const int32_t* dilations, int32_t n_dil, void* stream) {
    ACR_CHECK_ARG(w && mask_in && mask_out, "acr_pamr_propagate: null pointer");
    ACR_CHECK_ARG(mask_in != mask_out, "acr_pamr_propagate: mask_in and mask_out must be different buffers (a gather cannot run in place)");
    pamr_dil dil;
    int rc = pamr_check_dil("acr_pamr_propagate", dilations, n_dil, &dil);
    if (rc != ACR_OK) return rc;
    rc = pamr_check_dims("acr_pamr_propagate", B, C, H, W);
    if (rc != ACR_OK) return rc;
    const dim3 grid((unsigned)(((int64_t)H * W + 255) / 256), (C + PAMR_CH - 1) / PAMR_CH, B);
    hipLaunchKernelGGL(pamr_propagate_kernel, grid, dim3(256), 0, (hipStream_t)stream, w, mask_in, mask_out, C, H, W, dil, n_dil);
    return acr_check_launch("acr_pamr_propagate");
}
