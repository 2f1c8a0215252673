// Training-time CAM targets: the patch CAMs of forward_cam, token-major (B, gh * gw, C), become the (B, C, oh, ow) stack that
// pseudo_sal.hip's labels are made from -- the reference's compute_cam_up (myTool.py:860-864: bilinear upsampling to the crop,
// times the image-level label) and, with `normalize`, the two-view sum and min-max normalisation it applies to patch CAMs
// (infer_cam.py:156-162, 201-202) -- in one pass over the output.  include/acr_hip.h states the rule in full; the interpolation
// is acr_resample.h's, so the planes equal acr_bilinear_resize's bit for bit.
//
// The kernel streams: the source is a few KB per image and stays in cache, the output is B * C * oh * ow * 4 bytes and every
// element of it is stored exactly once.  Typically 1-3 of 20 planes per image carry work, the others are +0, and which ones is
// known on the device only: so every plane is cut into slabs of whole rows (about TC_SLAB_ELEMS values, at most TC_MAX_SLABS per
// plane) and a workgroup takes one slab -- the present planes are spread over the chip, an absent plane's workgroups store zeros.
// Launches of one call, none of them data dependent:
//   extremes  (normalize only) min and max of s over each slab of a present plane -> ws[plane][slab] = {mn, mx}; stores nothing
//             else.  min / max are exact in any order: the result does not depend on the slab geometry.
//   write     recomputes s (the arithmetic is cheap next to the store), takes the plane's extremes from its slabs' pairs and
//             stores (s - mn) / ((mx - mn) + eps), or s.
// A workgroup of a present plane first copies the few source rows its slab reads into LDS (tc_stage; enlarging, 2-3 rows per
// view), so the four taps of a value are LDS reads; only a reduction so strong that those rows exceed TC_STAGE floats reads its
// taps from global memory.  Either way the values are the same expression on the same numbers.
// V values per thread and store (4: ow is a multiple of 4 and `out` is 16-byte aligned, so every row of every plane is; else 1).
#include "acr_resample.h"

#define TC_SLAB_ELEMS 4096               // values of a slab: 16 per thread of a workgroup
#define TC_MAX_SLABS 256                 // per plane: the write kernel's first wave folds them in four steps at most
#define TC_MAX_PLANES (1 << 22)          // B * C; planes * slabs is a launch's grid, below 2^31
#define TC_STAGE 4096                    // floats of LDS for a slab's source rows, both views (16 KB: 8 workgroups per CU keep theirs)

struct tc_geom {
    const float* cam1;
    const float* cam2;                   // nullable: the CAMs of the h-flipped view
    int64_t st, sb;                      // token and batch stride of both, in elements; the class stride is 1
    const float* label;                  // (B, C)
    int C, gh, gw, oh, ow;
    float sh, sw;                        // gh / oh, gw / ow
    int rows, ns;                        // rows of a slab, slabs of a plane
};

// rows per slab and slabs per plane; the same on the host side of both entry points
static void tc_slabs(int32_t oh, int32_t ow, int* rows, int* ns) {
    int r = TC_SLAB_ELEMS / ow;
    if (r < 1) r = 1;
    if ((oh + r - 1) / r > TC_MAX_SLABS) r = (oh + TC_MAX_SLABS - 1) / TC_MAX_SLABS;
    *rows = r;
    *ns = (oh + r - 1) / r;
}

// value of token o of a class column: p[(o - base) * st].  The column lies in global memory (base 0, st the token stride) or,
// staged, in LDS (the tokens from `base` on, st 1)
__device__ __forceinline__ float tc_up(const float* __restrict__ p, int64_t st, int base, const acr_taps& t) {
    return acr_bilerp(t.hy, t.ly, t.hx, t.lx, p[(t.o00 - base) * st], p[(t.o01 - base) * st], p[(t.o10 - base) * st], p[(t.o11 - base) * st]);
}

// s[Y, X] of the plane whose class column starts at p1 / p2: view 2 enters at the mirrored OUTPUT column (bilinear_kernel's hflip)
__device__ __forceinline__ float tc_value(const tc_geom& g, const float* __restrict__ p1, const float* __restrict__ p2, int64_t st, int base,
                                          float l, int Y, int X) {
    float s = tc_up(p1, st, base, acr_taps_of(Y, X, g.gh, g.gw, g.sh, g.sw)) * l;
    if (p2) s = s + tc_up(p2, st, base, acr_taps_of(Y, g.ow - 1 - X, g.gh, g.gw, g.sh, g.sw)) * l;
    return s;
}

// The source rows that the output rows [r0, r1) read -- the first tap of r0 to the second tap of r1 - 1: both are monotone in the
// row -- copied to `stage`, view 2 behind view 1, when they fit: the taps then come from LDS and a thread waits for global memory
// once, not once per value.  Returns the floats per view, 0 when they do not fit (a strong reduction: the taps stay in global
// memory).  The condition is the same for the whole workgroup.
__device__ __forceinline__ int tc_stage(const tc_geom& g, const float* __restrict__ p1, const float* __restrict__ p2, int r0, int r1,
                                        float* __restrict__ stage, int* base) {
    const int ylo = acr_taps_of(r0, 0, g.gh, g.gw, g.sh, g.sw).y0, yhi = acr_taps_of(r1 - 1, 0, g.gh, g.gw, g.sh, g.sw).y1;
    const int64_t n = (int64_t)(yhi - ylo + 1) * g.gw;
    if ((p2 ? 2 : 1) * n > TC_STAGE) return 0;
    *base = ylo * g.gw;
    for (int i = threadIdx.x; i < (int)n; i += 256) {
        stage[i] = p1[(int64_t)(*base + i) * g.st];
        if (p2) stage[n + i] = p2[(int64_t)(*base + i) * g.st];
    }
    __syncthreads();
    return (int)n;
}

// f(i, v) for every item i of the slab: V consecutive values of one row
template <int V, typename F>
__device__ __forceinline__ void tc_slab(const tc_geom& g, const float* __restrict__ p1, const float* __restrict__ p2, int64_t st, int base,
                                        float l, int r0, int items, F f) {
    const int nx = g.ow / V;
    for (int i = threadIdx.x; i < items; i += 256) {
        const int Y = r0 + i / nx, X = (i % nx) * V;
        float v[V];
#pragma unroll
        for (int u = 0; u < V; ++u) v[u] = tc_value(g, p1, p2, st, base, l, Y, X + u);
        f(i, v);
    }
}

template <int V>
__global__ __launch_bounds__(256) void tc_extremes_kernel(tc_geom g, float* __restrict__ ws) {
    __shared__ float stage[TC_STAGE];
    __shared__ float part[2][4];
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x / g.ns;
    const int slab = blockIdx.x % g.ns;
    const float l = g.label[plane];
    if (l == 0.f) return;                                // the whole workgroup: the write kernel does not read this plane's pairs
    const int64_t b = plane / g.C;
    const int c = (int)(plane % g.C);
    const float* p1 = g.cam1 + b * g.sb + c;
    const float* p2 = g.cam2 ? g.cam2 + b * g.sb + c : nullptr;
    const int r0 = slab * g.rows, r1 = min(g.oh, r0 + g.rows);
    const int items = (r1 - r0) * (g.ow / V);
    float mn = INFINITY, mx = -INFINITY;
    auto fold = [&](int, const float* v) {
#pragma unroll
        for (int u = 0; u < V; ++u) {
            mn = fminf(mn, v[u]);
            mx = fmaxf(mx, v[u]);
        }
    };
    int base = 0;
    const int n = tc_stage(g, p1, p2, r0, r1, stage, &base);
    if (n)
        tc_slab<V>(g, stage, p2 ? stage + n : nullptr, 1, base, l, r0, items, fold);
    else
        tc_slab<V>(g, p1, p2, g.st, 0, l, r0, items, fold);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    if ((tid & 63) == 0) part[0][tid >> 6] = mn, part[1][tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        float* o = ws + 2 * (plane * g.ns + slab);
        o[0] = fminf(fminf(part[0][0], part[0][1]), fminf(part[0][2], part[0][3]));
        o[1] = fmaxf(fmaxf(part[1][0], part[1][1]), fmaxf(part[1][2], part[1][3]));
    }
}

template <int V>
__global__ __launch_bounds__(256) void tc_write_kernel(tc_geom g, const float* __restrict__ ws, float eps, int normalize, float* __restrict__ out) {
    __shared__ float stage[TC_STAGE];
    __shared__ float ext[2];
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x / g.ns;
    const int slab = blockIdx.x % g.ns;
    const float l = g.label[plane];
    const int r0 = slab * g.rows, r1 = min(g.oh, r0 + g.rows);
    const int items = (r1 - r0) * (g.ow / V);
    float* dst = out + plane * ((int64_t)g.oh * g.ow) + (int64_t)r0 * g.ow;          // the slab is contiguous
    if (l == 0.f) {                                      // the whole workgroup: +0, the source is not read
        for (int i = tid; i < items; i += 256) {
            if (V == 4) {
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(dst + 4 * (int64_t)i) = z;
            } else {
                dst[i] = 0.f;
            }
        }
        return;
    }
    float mn = 0.f, den = 1.f;
    if (normalize) {                                     // the plane's extremes: the first wave folds the slabs' pairs
        if (tid < 64) {
            float a = INFINITY, z = -INFINITY;
            const float* pairs = ws + 2 * plane * g.ns;
            for (int i = tid; i < g.ns; i += 64) {
                a = fminf(a, pairs[2 * i]);
                z = fmaxf(z, pairs[2 * i + 1]);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                a = fminf(a, __shfl_xor(a, off));
                z = fmaxf(z, __shfl_xor(z, off));
            }
            if (tid == 0) ext[0] = a, ext[1] = z;
        }
        __syncthreads();
        mn = ext[0];
        den = (ext[1] - mn) + eps;
    }
    const int64_t b = plane / g.C;
    const int c = (int)(plane % g.C);
    const float* p1 = g.cam1 + b * g.sb + c;
    const float* p2 = g.cam2 ? g.cam2 + b * g.sb + c : nullptr;
    auto store = [&](int i, const float* s) {
        float v[V];
#pragma unroll
        for (int u = 0; u < V; ++u) v[u] = normalize ? (s[u] - mn) / den : s[u];
        if (V == 4) {
            const f32x4 q = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(dst + 4 * (int64_t)i) = q;
        } else {
            dst[i] = v[0];
        }
    };
    int base = 0;
    const int n = tc_stage(g, p1, p2, r0, r1, stage, &base);
    if (n)
        tc_slab<V>(g, stage, p2 ? stage + n : nullptr, 1, base, l, r0, items, store);
    else
        tc_slab<V>(g, p1, p2, g.st, 0, l, r0, items, store);
}

static bool tc_shape_ok(int32_t B, int32_t C, int32_t oh, int32_t ow) {
    return B >= 1 && C >= 1 && oh >= 1 && ow >= 1 && (int64_t)B * C <= TC_MAX_PLANES && (int64_t)oh * ow < (1ll << 31);
}

extern "C" int64_t acr_train_cam_ws_bytes(int32_t B, int32_t C, int32_t oh, int32_t ow) {
    if (!tc_shape_ok(B, C, oh, ow)) {
        acr_set_error("acr_train_cam_ws_bytes: B=%d C=%d oh=%d ow=%d outside the supported range", B, C, oh, ow);
        return ACR_ERR_INVALID;
    }
    int rows, ns;
    tc_slabs(oh, ow, &rows, &ns);
    return (int64_t)B * C * ns * 8;
}

extern "C" int acr_train_cam_f32(const float* cam1, const float* cam2, int64_t tok_stride, int64_t batch_stride, const float* label,
                                 int32_t B, int32_t C, int32_t gh, int32_t gw, int32_t oh, int32_t ow, float eps, int32_t normalize,
                                 void* ws, int64_t ws_bytes, float* out, void* stream) {
    ACR_CHECK_ARG(cam1 && label && out, "acr_train_cam_f32: null pointer");
    ACR_CHECK_ARG(tc_shape_ok(B, C, oh, ow), "acr_train_cam_f32: B=%d C=%d oh=%d ow=%d outside the supported range", B, C, oh, ow);
    ACR_CHECK_ARG(gh >= 1 && gw >= 1 && (int64_t)gh * gw < (1ll << 31), "acr_train_cam_f32: bad grid %d x %d", gh, gw);
    ACR_CHECK_ARG(tok_stride >= 0 && batch_stride >= 0, "acr_train_cam_f32: negative stride");
    ACR_CHECK_ARG(eps > 0.f, "acr_train_cam_f32: eps=%g is not positive", (double)eps);
    ACR_CHECK_ARG(normalize == 0 || normalize == 1, "acr_train_cam_f32: normalize=%d is neither 0 nor 1", normalize);
    tc_geom g;
    g.cam1 = cam1;
    g.cam2 = cam2;
    g.st = tok_stride;
    g.sb = batch_stride;
    g.label = label;
    g.C = C, g.gh = gh, g.gw = gw, g.oh = oh, g.ow = ow;
    g.sh = (float)gh / (float)oh;                        // torch's align_corners=False scale, as acr_bilinear_resize forms it
    g.sw = (float)gw / (float)ow;
    tc_slabs(oh, ow, &g.rows, &g.ns);
    const int64_t blocks = (int64_t)B * C * g.ns;        // <= 2^22 * 2^8
    if (normalize) ACR_CHECK_WS("acr_train_cam_f32", ws, 4, ws_bytes, blocks * 8);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = ow % 4 == 0 && ((uintptr_t)out & 15) == 0;
    float* pairs = reinterpret_cast<float*>(ws);
    if (vec) {
        if (normalize) hipLaunchKernelGGL(tc_extremes_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, g, pairs);
        hipLaunchKernelGGL(tc_write_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, g, (const float*)pairs, eps, normalize, out);
    } else {
        if (normalize) hipLaunchKernelGGL(tc_extremes_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, g, pairs);
        hipLaunchKernelGGL(tc_write_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, g, (const float*)pairs, eps, normalize, out);
    }
    return acr_check_launch("acr_train_cam_f32");
}
