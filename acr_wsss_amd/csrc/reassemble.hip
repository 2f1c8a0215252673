// Read-out reassembly of the plain ViT backbones under seg=True (DPT/vit.py:263-341: Slice -> Transpose -> Unflatten -> 1x1 convolution
// -> ConvTranspose2d(f, f, s, stride=s); DPT/vit.py:117-146 runs them).  A transposed convolution whose kernel equals its stride has
// no overlapping outputs: it is a matrix product on the tokens (acr_gemm_f32, 'nn', the weight (ci, co, s, s) as stored) followed by
// what this file does -- token-major -> NCHW with a depth-to-space shuffle, the bias, and a skip of the first `start` tokens:
//
//   forward   out[b][co][i s + di][j s + dj] = y[b T + start + i gw + j][(co s + di) s + dj] (+ bias[co])
//   backward  dy[b T + start + i gw + j][(co s + di) s + dj] = dout[b][co][i s + di][j s + dj],   dy[b T + p][< C s^2] = 0 (p < start),
//             dbias[co] = sum_b sum_pixels dout[b][co]
//
// One workgroup owns one (sample, grid row, TJ grid columns, 64 token columns = 64 / s^2 channels) tile and turns it through LDS: the
// token side moves 256-byte runs (64 consecutive floats of a token row), the map side TJ * s consecutive floats of a (channel, row)
// line (256 bytes, 512 for s = 4).  s = 1 has no row structure on the map side (a channel's plane is gh * gw consecutive floats), so it
// runs as one grid row of gh * gw columns.  The LDS row pitch is 64 + s floats: the row-wise accesses of a 32-lane group fall on 32
// consecutive banks, the transposed ones on banks s * j + dj (j the token, dj < s), again all different.  Edge tiles are masked per
// element on both sides; no address outside the tensors is formed for a load or a store.
// dbias: every tile sums its channels' values in a fixed order (lane chains, then a butterfly over the 4 s^2 lanes of a channel) into
// a partial of its own in ws; a second kernel adds each channel's partials in double, again in a fixed order.  No atomics.
#include "acr_common.h"
#include "acr_reduce.h"

namespace {

template <int S>
struct Geo {
    static constexpr int TJ = S == 1 ? 64 : 32;             // grid columns (tokens) per tile
    static constexpr int CB = 64 / (S * S);                 // channels per tile: 64 token columns
    static constexpr int ST = 64 + S;                       // LDS row pitch in floats
    static constexpr int RW = TJ * S;                       // floats of one (channel, map row) line in a tile
    static constexpr int TPC = 256 / CB;                    // lanes that share a channel in the bias-gradient sum
};

struct Tile {
    int cb, jt, i, b;
};

__device__ __forceinline__ Tile tile_of(int bid, int ncb, int ntj, int gh) {
    Tile t;
    t.cb = bid % ncb;
    bid /= ncb;
    t.jt = bid % ntj;
    bid /= ntj;
    t.i = bid % gh;
    t.b = bid / gh;
    return t;
}

template <int S>
__global__ __launch_bounds__(256) void reassemble_fwd_kernel(const float* __restrict__ y, int64_t ldy, const float* __restrict__ bias, int T,
                                                             int start, int gh, int gw, int C, int ncb, int ntj, float* __restrict__ out) {
    using G = Geo<S>;
    __shared__ float tile[G::TJ * G::ST];
    const Tile t = tile_of(blockIdx.x, ncb, ntj, gh);
    const int tid = threadIdx.x, lc = tid & 63;
    const int col0 = t.cb * 64, j0 = t.jt * G::TJ, ncols = C * S * S;
    if (col0 + lc < ncols) {
        // Rows past the grid's edge are read at the tile's last valid row instead (j0 < gw, so there is one) and never used: with
        // nothing to decide per row, all TJ / 4 loads of a thread are in flight together.
        const float* src = y + ((int64_t)t.b * T + start + (int64_t)t.i * gw + j0) * ldy + col0 + lc;
        const int jlast = gw - 1 - j0;
        float v[G::TJ / 4];
#pragma unroll
        for (int m = 0; m < G::TJ / 4; ++m) v[m] = src[(int64_t)min((tid >> 6) + 4 * m, jlast) * ldy];
#pragma unroll
        for (int m = 0; m < G::TJ / 4; ++m) tile[((tid >> 6) + 4 * m) * G::ST + lc] = v[m];
    }
    __syncthreads();
    const int64_t ow = (int64_t)gw * S;
#pragma unroll 4
    for (int m = 0; m < G::TJ / 4; ++m) {
        const int e = tid + 256 * m;
        const int xx = e % G::RW, r = e / G::RW;            // r = cl * S + di: the line of the tile
        const int cl = r / S, di = r % S, j = xx / S, dj = xx % S;
        const int c = t.cb * G::CB + cl;
        if (c < C && j0 + j < gw) {
            float v = tile[j * G::ST + r * S + dj];
            if (bias) v += bias[c];
            out[((((int64_t)t.b * C + c) * gh + t.i) * S + di) * ow + (int64_t)j0 * S + xx] = v;
        }
    }
}

template <int S>
__global__ __launch_bounds__(256) void reassemble_bwd_kernel(const float* __restrict__ dout, int T, int start, int gh, int gw, int C, int ncb,
                                                             int ntj, float* __restrict__ dy, int64_t lddy, float* __restrict__ part) {
    using G = Geo<S>;
    __shared__ float tile[G::TJ * G::ST];
    const Tile t = tile_of(blockIdx.x, ncb, ntj, gh);
    const int tid = threadIdx.x, lc = tid & 63;
    const int col0 = t.cb * 64, j0 = t.jt * G::TJ, ncols = C * S * S;
    const int64_t ow = (int64_t)gw * S;
    const int xlast = (gw - j0) * S - 1;                    // the tile's last valid map column (j0 < gw)
#pragma unroll
    for (int m = 0; m < G::TJ / 4; ++m) {
        const int e = tid + 256 * m;
        const int xx = e % G::RW, r = e / G::RW;
        const int cl = r / S, di = r % S, j = xx / S, dj = xx % S;
        const int c = t.cb * G::CB + cl;
        // Past the edge the load goes to the last valid channel / map column of the tile instead (clamped: always inside dout), so
        // that no load waits for a decision; what it brings is dropped.  The masked part holds zeros: the sums below may take it.
        const int cc = min(c, C - 1), xc = min(xx, xlast);
        const float v = dout[((((int64_t)t.b * C + cc) * gh + t.i) * S + di) * ow + (int64_t)j0 * S + xc];
        tile[j * G::ST + r * S + dj] = (c < C && j0 + j < gw) ? v : 0.f;
    }
    __syncthreads();
    if (col0 + lc < ncols) {
        float* dst = dy + ((int64_t)t.b * T + start + (int64_t)t.i * gw + j0) * lddy + col0 + lc;
        for (int jr = tid >> 6; jr < G::TJ && j0 + jr < gw; jr += 4) dst[(int64_t)jr * lddy] = tile[jr * G::ST + lc];
        if (t.i == 0 && t.jt == 0)                          // the skipped tokens of this sample took no part in the forward
            for (int p = tid >> 6; p < start; p += 4) dy[((int64_t)t.b * T + p) * lddy + col0 + lc] = 0.f;
    }
    if (part) {
        const int cl = tid / G::TPC, k = tid % G::TPC;       // TPC = 4 s^2: lane k takes element k % s^2 of tokens k / s^2, + 4, + 8, ..
        float acc = 0.f;
#pragma unroll
        for (int m = 0; m < G::TJ / 4; ++m) acc += tile[(k / (S * S) + 4 * m) * G::ST + cl * S * S + k % (S * S)];
        acc = acr_lanes_sum<G::TPC>(acc);
        const int c = t.cb * G::CB + cl;
        if (k == 0 && c < C) part[(((int64_t)t.b * gh + t.i) * ntj + t.jt) * C + c] = acc;
    }
}

// dbias[c] = the channel's np partials in double: sixteen interleaved chains (chain g takes partials g, g + 16, .. in ascending order),
// then the sixteen in order.  A workgroup owns 16 channels; a chain loads eight partials at a time so that the loads overlap (one
// after the other, a channel's few hundred partials cost more than the shuffle itself).
__global__ __launch_bounds__(256) void reassemble_dbias_kernel(const float* __restrict__ part, int64_t np, int C, float* __restrict__ dbias) {
    __shared__ double sh[16][16];
    const int lc = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + lc;
    double acc = 0.0;
    if (c < C) {
        int64_t p = g;
        for (; p + 16 * 7 < np; p += 16 * 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = part[(p + 16 * k) * C + c];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc += (double)v[k];
        }
        for (; p < np; p += 16) acc += (double)part[p * C + c];
    }
    sh[g][lc] = acc;
    __syncthreads();
    if (g == 0 && c < C) {
        double t = sh[0][lc];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += sh[k][lc];
        dbias[c] = (float)t;
    }
}

struct Plan {
    int gh, gw, ncb, ntj;
    int64_t tiles;                                          // per sample
};

// s = 1: one grid row of gh * gw columns (see the head of the file)
Plan plan_of(int gh, int gw, int C, int s) {
    Plan p;
    if (s == 1) {
        p.gh = 1;
        p.gw = gh * gw;
    } else {
        p.gh = gh;
        p.gw = gw;
    }
    p.ncb = (int)(((int64_t)C * s * s + 63) / 64);
    p.ntj = (p.gw + (s == 1 ? 64 : 32) - 1) / (s == 1 ? 64 : 32);
    p.tiles = (int64_t)p.gh * p.ntj * p.ncb;
    return p;
}

bool shape_ok(int B, int gh, int gw, int C, int s) {
    if (!(s == 1 || s == 2 || s == 4) || B <= 0 || gh <= 0 || gw <= 0 || C <= 0) return false;
    if ((int64_t)gh * gw >= (1 << 26) || (int64_t)C * s * s >= (1 << 30)) return false;
    const Plan p = plan_of(gh, gw, C, s);
    return p.tiles * B < (int64_t)1 << 31 && (int64_t)B * p.gh * p.ntj * C < (int64_t)1 << 40;
}

}  // namespace

extern "C" size_t acr_reassemble_ws_bytes(int32_t B, int32_t gh, int32_t gw, int32_t C, int32_t s) {
    if (!shape_ok(B, gh, gw, C, s)) return 0;
    const Plan p = plan_of(gh, gw, C, s);
    return (size_t)((int64_t)B * p.gh * p.ntj * C) * sizeof(float);
}

#define REASSEMBLE_CHECK(name)                                                                                                          \
    ACR_CHECK_ARG(s == 1 || s == 2 || s == 4, name ": s must be 1, 2 or 4, got %d", s);                                                 \
    ACR_CHECK_ARG(B > 0 && gh > 0 && gw > 0 && C > 0 && T > 0, name ": bad shape (B=%d T=%d gh=%d gw=%d C=%d)", B, T, gh, gw, C);         \
    ACR_CHECK_ARG(start >= 0 && start <= 8, name ": start must be in 0 .. 8, got %d", start);                                           \
    ACR_CHECK_ARG(shape_ok(B, gh, gw, C, s), name ": shape out of range (B=%d gh=%d gw=%d C=%d s=%d)", B, gh, gw, C, s);                  \
    ACR_CHECK_ARG((int64_t)T == (int64_t)start + (int64_t)gh * gw, name ": T must be start + gh * gw (T=%d start=%d gh=%d gw=%d)", T,   \
                  start, gh, gw)

extern "C" int acr_reassemble_fwd(const float* y, int64_t ldy, const float* bias, int32_t B, int32_t T, int32_t start, int32_t gh, int32_t gw,
                                  int32_t C, int32_t s, float* out, void* stream) {
    REASSEMBLE_CHECK("acr_reassemble_fwd");
    ACR_CHECK_ARG(ldy >= (int64_t)C * s * s, "acr_reassemble_fwd: ldy %lld is below C * s * s = %lld", (long long)ldy, (long long)C * s * s);
    ACR_CHECK_ARG(y && out, "acr_reassemble_fwd: null pointer");
    const Plan p = plan_of(gh, gw, C, s);
    const dim3 grid((unsigned)(p.tiles * B)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (s == 1)
        hipLaunchKernelGGL(reassemble_fwd_kernel<1>, grid, block, 0, st, y, ldy, bias, T, start, p.gh, p.gw, C, p.ncb, p.ntj, out);
    else if (s == 2)
        hipLaunchKernelGGL(reassemble_fwd_kernel<2>, grid, block, 0, st, y, ldy, bias, T, start, p.gh, p.gw, C, p.ncb, p.ntj, out);
    else
        hipLaunchKernelGGL(reassemble_fwd_kernel<4>, grid, block, 0, st, y, ldy, bias, T, start, p.gh, p.gw, C, p.ncb, p.ntj, out);
    return acr_check_launch("acr_reassemble_fwd");
}

extern "C" int acr_reassemble_bwd(const float* dout, int32_t B, int32_t T, int32_t start, int32_t gh, int32_t gw, int32_t C, int32_t s, float* dy,
                                  int64_t lddy, float* dbias, void* ws, int64_t ws_bytes, void* stream) {
    REASSEMBLE_CHECK("acr_reassemble_bwd");
    ACR_CHECK_ARG(lddy >= (int64_t)C * s * s, "acr_reassemble_bwd: lddy %lld is below C * s * s = %lld", (long long)lddy, (long long)C * s * s);
    ACR_CHECK_ARG(dout && dy, "acr_reassemble_bwd: null pointer");
    const Plan p = plan_of(gh, gw, C, s);
    const int64_t np = (int64_t)B * p.gh * p.ntj;
    if (dbias) ACR_CHECK_WS("acr_reassemble_bwd (dbias)", ws, 4, ws_bytes, np * C * (int64_t)sizeof(float));
    float* part = dbias ? (float*)ws : nullptr;
    const dim3 grid((unsigned)(p.tiles * B)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (s == 1)
        hipLaunchKernelGGL(reassemble_bwd_kernel<1>, grid, block, 0, st, dout, T, start, p.gh, p.gw, C, p.ncb, p.ntj, dy, lddy, part);
    else if (s == 2)
        hipLaunchKernelGGL(reassemble_bwd_kernel<2>, grid, block, 0, st, dout, T, start, p.gh, p.gw, C, p.ncb, p.ntj, dy, lddy, part);
    else
        hipLaunchKernelGGL(reassemble_bwd_kernel<4>, grid, block, 0, st, dout, T, start, p.gh, p.gw, C, p.ncb, p.ntj, dy, lddy, part);
    if (dbias) hipLaunchKernelGGL(reassemble_dbias_kernel, dim3((C + 15) / 16), block, 0, st, part, np, C, dbias);
    return acr_check_launch("acr_reassemble_bwd");
}
