// The 1x1 convolutions of the ResNetV2 stem: entries on the GEMM loops of gemm_f32.hip, and the split-product kernels that
// take the weight as an operand image (twins of conv3x3_wimg_kernel / conv3x3_wimg64_kernel in conv3x3.hip).
#include <type_traits>

#include "gemm_f32.h"

// ---------------------------------------------------------------------------------------------------------------------------------
// The stem's 1x1 convolutions (forward and input gradient) under split products: y[n] (M x pixels) = W (M x K) . x[n] (K x pixels).
// The weight is tiny and shared by every workgroup: it comes as an IMAGE (acr_x3_image / acr_x3_image_t of the standardised
// weight), so only the activation tile -- fp32 [k][pixels] as stored, no pass over the big tensors -- is split in registers:
// half the VALU work of gemm_f32_split_kernel per MFMA (that kernel is VALU-port bound, profiles/r04_pmc_split_gemm.txt).
// Slot = [A p0 p1 p2 (12 KiB, one contiguous piece of the image) | B fp32 16 k-rows x 128 pixels (8 KiB)], ring of 3, DMA two
// stages ahead, 5 pieces per wave and stage (3 of A, 2 of B); waits, barrier and interleaving as gemm_f32_planes_kernel.
// ---------------------------------------------------------------------------------------------------------------------------------
#define W_STAGE_B IMG_W_STAGE_B(S_TILE)             // 20 KiB
template <int ACT>
__global__ __launch_bounds__(256, 2) void gemm_f32_wimg_kernel(const GemmF32Args g) {
    __shared__ __attribute__((aligned(1024))) float smem[P_SLOTS * W_STAGE_B / 4];      // 60 KiB
    typedef __attribute__((address_space(3))) void* lds_vp;
    typedef const __attribute__((address_space(1))) void* glb_vp;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int ntile = g.tiles_launch;
    const int t0 = acr_xcd_remap(blockIdx.x, ntile * g.nsplit);
    const int split = t0 / ntile, tt = g.tile0 + (t0 - split * ntile);
    int tm, tn;
    if (ACT == 3) { tm = tt / g.tiles_n; tn = tt - tm * g.tiles_n; }
    else tile_coords(tt, g.tiles_m, g.tiles_n, tm, tn);
    const int m0 = tm * F_BM, n0 = tn * F_BN;
    const int zs = split / g.ksplit;
    const int kbeg = (split - zs * g.ksplit) * g.k_zs, kend = min(g.K, kbeg + g.kps);      // host: multiples of 16
    const int nkb = (g.K + P_BK - 1) / P_BK;
    const char* __restrict__ pa = reinterpret_cast<const char*>(g.a) + IMG_STAGE_OFF(tm, nkb, kbeg / P_BK, 3) + wave * 3072 + lane * 16;
    const float* __restrict__ pb = g.b + (int64_t)zs * g.b_zs + (int64_t)kbeg * g.ldb;
    int offb[2];                                            // B pieces 2 wave + i: k rows 2 (2 wave + i) + (lane >> 5), 4 pixels per lane
#pragma unroll
    for (int i = 0; i < 2; ++i) offb[i] = ((wave * 2 + i) * 2 + (lane >> 5)) * (int)g.ldb + min(n0 + 4 * (lane & 31), g.N - 4);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int nst = (kend - kbeg) / P_BK;
    char* sm = reinterpret_cast<char*>(smem);
    auto dma1 = [&](int st, int slot, int i) {              // i = 0..2: A pieces 3 wave + i; i = 3, 4: B pieces 2 wave + (i - 3)
        if (i < 3)
            __builtin_amdgcn_global_load_lds((glb_vp)(pa + (int64_t)st * (3 * IMG_PLANE_B) + i * 1024), (lds_vp)(sm + slot * W_STAGE_B + (wave * 3 + i) * 1024), 16, 0, 0);
        else
            __builtin_amdgcn_global_load_lds((glb_vp)(pb + (int64_t)st * P_BK * g.ldb + offb[i - 3]),
                                             (lds_vp)(sm + slot * W_STAGE_B + 3 * IMG_PLANE_B + (wave * 2 + i - 3) * 1024), 16, 0, 0);
    };
    const uint32_t lbase = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)sm;
    const uint32_t fa = IMG_FRAG_ADDR(lbase, wm * 64 + r, r, h);
    const uint32_t fb = lbase + 3 * IMG_PLANE_B + ((8 * h) * F_BN + wn * 64 + r) * 4;
#pragma unroll
    for (int i = 0; i < 5; ++i) dma1(0, 0, i);
#pragma unroll
    for (int i = 0; i < 5; ++i) dma1(min(1, nst - 1), 1, i);
    bf16x8 ap[2][2][3], bp[2][2][3];                        // [register set][block][plane]
    float rb[2][8];
    auto step = [&](int st, int slot, auto set_tag, auto first_tag) {
        constexpr int SET = decltype(set_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value;
        asm volatile("s_waitcnt vmcnt(5)" ::: "memory");    // younger: the 5 pieces of stage st + 1
        acr_barrier_nofence();
        const int rslot = slot == 0 ? 2 : slot - 1;         // (st + 2) % 3
        const int rst = min(st + 2, nst - 1);
#pragma unroll
        for (int i = 0; i < 5; ++i) dma1(rst, rslot, i);
        const uint32_t fas = fa + slot * W_STAGE_B, fbs = fb + slot * W_STAGE_B;
        // stage st: the B fragments raw (fp32, 8 k of one pixel per lane), the A fragments as planes
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            ACR_LDS_RD32(rb[j][0], fbs, 0 * F_BN * 4 + j * 128); ACR_LDS_RD32(rb[j][1], fbs, 1 * F_BN * 4 + j * 128); ACR_LDS_RD32(rb[j][2], fbs, 2 * F_BN * 4 + j * 128);
            ACR_LDS_RD32(rb[j][3], fbs, 3 * F_BN * 4 + j * 128); ACR_LDS_RD32(rb[j][4], fbs, 4 * F_BN * 4 + j * 128); ACR_LDS_RD32(rb[j][5], fbs, 5 * F_BN * 4 + j * 128);
            ACR_LDS_RD32(rb[j][6], fbs, 6 * F_BN * 4 + j * 128); ACR_LDS_RD32(rb[j][7], fbs, 7 * F_BN * 4 + j * 128);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ACR_LDS_RD128(ap[SET][i][0], fas, 0 * IMG_PLANE_B + i * 1024); ACR_LDS_RD128(ap[SET][i][1], fas, 1 * IMG_PLANE_B + i * 1024); ACR_LDS_RD128(ap[SET][i][2], fas, 2 * IMG_PLANE_B + i * 1024);
        }
        asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(rb[0][0]), "+v"(rb[0][1]), "+v"(rb[0][2]), "+v"(rb[0][3]), "+v"(rb[0][4]), "+v"(rb[0][5]), "+v"(rb[0][6]),
                     "+v"(rb[0][7]), "+v"(rb[1][0]), "+v"(rb[1][1]), "+v"(rb[1][2]), "+v"(rb[1][3]), "+v"(rb[1][4]), "+v"(rb[1][5]), "+v"(rb[1][6]), "+v"(rb[1][7]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x4 lo = {rb[j][0], rb[j][1], rb[j][2], rb[j][3]}, hi = {rb[j][4], rb[j][5], rb[j][6], rb[j][7]};
            split3_bf16(lo, hi, bp[SET][j][0], bp[SET][j][1], bp[SET][j][2]);
        }
        if (!FIRST) {
            ACR_MFMA6(acc[0][0], ap[SET ^ 1][0], bp[SET ^ 1][0]) ACR_MFMA6(acc[0][1], ap[SET ^ 1][0], bp[SET ^ 1][1]) ACR_MFMA6(acc[1][0], ap[SET ^ 1][1], bp[SET ^ 1][0]) ACR_MFMA6(acc[1][1], ap[SET ^ 1][1], bp[SET ^ 1][1])
#pragma unroll
            for (int it = 0; it < 24; ++it) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA of stage st - 1
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);      // four VALU instructions of stage st's split
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ap[SET][0][0]), "+v"(ap[SET][0][1]), "+v"(ap[SET][0][2]), "+v"(ap[SET][1][0]), "+v"(ap[SET][1][1]), "+v"(ap[SET][1][2]));
    };
    step(0, 0, std::integral_constant<int, 0>{}, std::true_type{});
    int slot = 1;
    for (int st = 1; st < nst; st += 2) {
        step(st, slot, std::integral_constant<int, 1>{}, std::false_type{});
        slot = slot == 2 ? 0 : slot + 1;
        if (st + 1 < nst) {
            step(st + 1, slot, std::integral_constant<int, 0>{}, std::false_type{});
            slot = slot == 2 ? 0 : slot + 1;
        }
    }
    if (nst & 1) { ACR_MFMA6(acc[0][0], ap[0][0], bp[0][0]) ACR_MFMA6(acc[0][1], ap[0][0], bp[0][1]) ACR_MFMA6(acc[1][0], ap[0][1], bp[0][0]) ACR_MFMA6(acc[1][1], ap[0][1], bp[0][1]) }
    else { ACR_MFMA6(acc[0][0], ap[1][0], bp[1][0]) ACR_MFMA6(acc[0][1], ap[1][0], bp[1][1]) ACR_MFMA6(acc[1][0], ap[1][1], bp[1][0]) ACR_MFMA6(acc[1][1], ap[1][1], bp[1][1]) }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the refills past the end
    __syncthreads();
    gemm_f32_finish<true, ACT>(g, acc, smem, split, tt, tn, m0, n0, zs, wm, wn, r, h, tid, 0.f, false);
}

// The same product for at most 64 output channels (the stem's 1x1 convolutions into / out of the 64-channel maps at 112 x 112, and
// CAM generation's large maps): with a 128-row tile the lower wave row has no outputs -- two of four waves only feed the DMA.
// Tile = 64 rows x 256 PIXELS, all four waves compute 64 x 64 on their own 64 pixels; the A stage is the upper half of the
// image's 128-row block (3 planes x 2 KiB).  Ring 3 slots x [A 6 KiB | B fp32 16 KiB]; per wave and stage 2 A pieces (wave 3
// re-fetches pieces 4, 5: identical bytes to the same place, the count stays uniform) + 4 B pieces (one k row of 256 pixels).
#define W64_BN 256
#define W64_A_B (3 * 2048)
#define W64_STAGE_B (W64_A_B + P_BK * W64_BN * 4)          // 22 KiB
template <int ACT>
__global__ __launch_bounds__(256, 2) void gemm_f32_wimg64_kernel(const GemmF32Args g) {
    __shared__ __attribute__((aligned(1024))) char sm[P_SLOTS * W64_STAGE_B];            // 66 KiB
    typedef __attribute__((address_space(3))) void* lds_vp;
    typedef const __attribute__((address_space(1))) void* glb_vp;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5, wn = wave;
    const int ntile = g.tiles_n;                            // one tile row (M <= 64)
    const int t0 = acr_xcd_remap(blockIdx.x, ntile * g.nsplit);
    const int split = t0 / ntile, tn = t0 - split * ntile;
    const int n0 = tn * W64_BN;
    const int zs = split / g.ksplit;
    const int kbeg = (split - zs * g.ksplit) * g.k_zs, kend = min(g.K, kbeg + g.kps);      // host: multiples of 16
    const int qa = wave < 3 ? 2 * wave : 4;
    const char* __restrict__ pa = reinterpret_cast<const char*>(g.a) + IMG_STAGE_OFF(0, 0, kbeg / P_BK, 3) + lane * 16;
    const float* __restrict__ pb = g.b + (int64_t)zs * g.b_zs + (int64_t)kbeg * g.ldb + min(n0 + 4 * lane, g.N - 4);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int nst = (kend - kbeg) / P_BK;
    auto issue = [&](int st, int slot) {
        char* d = sm + slot * W64_STAGE_B;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = qa + i;
            __builtin_amdgcn_global_load_lds((glb_vp)(pa + (int64_t)st * (3 * IMG_PLANE_B) + (q >> 1) * IMG_PLANE_B + (q & 1) * 1024), (lds_vp)(d + q * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((glb_vp)(pb + (int64_t)(st * P_BK + 4 * wave + i) * g.ldb), (lds_vp)(d + W64_A_B + (4 * wave + i) * 1024), 16, 0, 0);
    };
    const uint32_t lbase = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)sm;
    const uint32_t fa = IMG_FRAG_ADDR(lbase, r, r, h);
    const uint32_t fb = lbase + W64_A_B + ((8 * h) * W64_BN + wn * 64 + r) * 4;
    issue(0, 0);
    issue(min(1, nst - 1), 1);
    bf16x8 ap[2][2][3], bp[2][2][3];
    float rb[2][8];
    auto step = [&](int st, int slot, auto set_tag, auto first_tag) {
        constexpr int SET = decltype(set_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value;
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");    // younger: the 6 pieces of stage st + 1
        acr_barrier_nofence();
        const int rslot = slot == 0 ? 2 : slot - 1;
        issue(min(st + 2, nst - 1), rslot);
        const uint32_t fas = fa + slot * W64_STAGE_B, fbs = fb + slot * W64_STAGE_B;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            ACR_LDS_RD32(rb[j][0], fbs, 0 * W64_BN * 4 + j * 128); ACR_LDS_RD32(rb[j][1], fbs, 1 * W64_BN * 4 + j * 128);
            ACR_LDS_RD32(rb[j][2], fbs, 2 * W64_BN * 4 + j * 128); ACR_LDS_RD32(rb[j][3], fbs, 3 * W64_BN * 4 + j * 128);
            ACR_LDS_RD32(rb[j][4], fbs, 4 * W64_BN * 4 + j * 128); ACR_LDS_RD32(rb[j][5], fbs, 5 * W64_BN * 4 + j * 128);
            ACR_LDS_RD32(rb[j][6], fbs, 6 * W64_BN * 4 + j * 128); ACR_LDS_RD32(rb[j][7], fbs, 7 * W64_BN * 4 + j * 128);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ACR_LDS_RD128(ap[SET][i][0], fas, 0 * 2048 + i * 1024); ACR_LDS_RD128(ap[SET][i][1], fas, 1 * 2048 + i * 1024); ACR_LDS_RD128(ap[SET][i][2], fas, 2 * 2048 + i * 1024);
        }
        asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(rb[0][0]), "+v"(rb[0][1]), "+v"(rb[0][2]), "+v"(rb[0][3]), "+v"(rb[0][4]), "+v"(rb[0][5]), "+v"(rb[0][6]),
                     "+v"(rb[0][7]), "+v"(rb[1][0]), "+v"(rb[1][1]), "+v"(rb[1][2]), "+v"(rb[1][3]), "+v"(rb[1][4]), "+v"(rb[1][5]), "+v"(rb[1][6]), "+v"(rb[1][7]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x4 lo = {rb[j][0], rb[j][1], rb[j][2], rb[j][3]}, hi = {rb[j][4], rb[j][5], rb[j][6], rb[j][7]};
            split3_bf16(lo, hi, bp[SET][j][0], bp[SET][j][1], bp[SET][j][2]);
        }
        if (!FIRST) {
            ACR_MFMA6(acc[0][0], ap[SET ^ 1][0], bp[SET ^ 1][0]) ACR_MFMA6(acc[0][1], ap[SET ^ 1][0], bp[SET ^ 1][1]) ACR_MFMA6(acc[1][0], ap[SET ^ 1][1], bp[SET ^ 1][0]) ACR_MFMA6(acc[1][1], ap[SET ^ 1][1], bp[SET ^ 1][1])
#pragma unroll
            for (int it = 0; it < 24; ++it) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ap[SET][0][0]), "+v"(ap[SET][0][1]), "+v"(ap[SET][0][2]), "+v"(ap[SET][1][0]), "+v"(ap[SET][1][1]), "+v"(ap[SET][1][2]));
    };
    step(0, 0, std::integral_constant<int, 0>{}, std::true_type{});
    int slot = 1;
    for (int st = 1; st < nst; st += 2) {
        step(st, slot, std::integral_constant<int, 1>{}, std::false_type{});
        slot = slot == 2 ? 0 : slot + 1;
        if (st + 1 < nst) {
            step(st + 1, slot, std::integral_constant<int, 0>{}, std::false_type{});
            slot = slot == 2 ? 0 : slot + 1;
        }
    }
    if (nst & 1) { ACR_MFMA6(acc[0][0], ap[0][0], bp[0][0]) ACR_MFMA6(acc[0][1], ap[0][0], bp[0][1]) ACR_MFMA6(acc[1][0], ap[0][1], bp[0][0]) ACR_MFMA6(acc[1][1], ap[0][1], bp[0][1]) }
    else { ACR_MFMA6(acc[0][0], ap[1][0], bp[1][0]) ACR_MFMA6(acc[0][1], ap[1][0], bp[1][1]) ACR_MFMA6(acc[1][0], ap[1][1], bp[1][0]) ACR_MFMA6(acc[1][1], ap[1][1], bp[1][1]) }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the refills past the end
    if (ACT == 3) {                                         // K-split small launch: raw part sums into slab `split`
        float* slab = g.c + (int64_t)split * g.M * g.ldc;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = n0 + wn * 64 + j * 32 + r;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = i * 32 + acr_krow(e, h);
                    if (row < g.M && col < g.N) slab[(int64_t)row * g.ldc + col] = acc[i][j][e];
                }
            }
        return;
    }
    GemmF32Args gz = g;
    gz.c += (int64_t)zs * g.c_zs;
    if (gz.aux) gz.aux += (int64_t)zs * g.aux_zs;
    epilogue_f32<0, true>(gz, acc, 0, n0 + wn * 64, r, h);
}

// ---------------------------------------------------------------------------------------------------------------
// 1x1 convolutions of the ResNetV2 stem at the reference precision (models/resnetv2.py:186-190, fp32 NCHW, stride 1) on the
// same kernels, one z-slice per sample, no layout change:
//   forward  y[n] (co x hw) = W (co x ci) . x[n] (ci x hw)            A = W  [i][k] contiguous in k, B = x[n]  [k][i]
//   input    dx[n] (ci x hw) = W^T . dy[n] (co x hw) (+ addend[n])     A = W  read as [k = co][i = ci],  B = dy[n] [k][i]
//   weight   dW (co x ci) = sum_n dy[n] (co x hw) . x[n]^T            A = dy[n], B = x[n], both contiguous in the contraction
//            (hw): one fp32 slab per sample, summed in sample order (deterministic)
// ---------------------------------------------------------------------------------------------------------------
static void conv_args(GemmF32Args& g, int M, int N, int K) {
    g.bias = nullptr; g.aux = nullptr; g.ldaux = 0; g.c2 = nullptr; g.cs = nullptr; g.M = M; g.N = N; g.K = K;
    g.tiles_m = (M + F_BM - 1) / F_BM; g.tiles_n = (N + F_BN - 1) / F_BN; g.kps = (K + F_BK - 1) / F_BK * F_BK; g.k_zs = 0;
    g.a_zs = g.b_zs = g.c_zs = g.aux_zs = 0; g.ksplit = 1;
    g.tile0 = 0; g.tiles_launch = g.tiles_m * g.tiles_n;
}

// Small launches (CAM generation: two views of one image, 8-72 workgroups) under split products: the contraction is split into
// parts of at least 64 channels so that the launch fills the chip; raw part sums go to slabs [sample][part], summed in part
// order (+ addend) by conv1x1_ksum_kernel.
static int conv1x1_ksplit(int nsamp, int cout, int cin, int hw, int* kps_out, bool wide64 = false) {
    const int tiles = wide64 ? ((hw + 255) / 256) * nsamp : ((cout + F_BM - 1) / F_BM) * ((hw + F_BN - 1) / F_BN) * nsamp;
    *kps_out = (cin + S_BK - 1) / S_BK * S_BK;
    if (tiles >= 192 || (cin % F_BK) != 0) return 1;
    int ks = 512 / tiles;
    if (ks > cin / 64) ks = cin / 64;
    if (ks < 2) return 1;
    const int kps = ((cin + ks - 1) / ks + S_BK - 1) / S_BK * S_BK;
    *kps_out = kps;
    return (cin + kps - 1) / kps;
}
extern "C" size_t acr_conv1x1_ws_floats(int32_t math, int32_t nsamp, int32_t cout, int32_t cin, int32_t hw) {
    int kps;
    if (math != ACR_MATH_BF16X3) return 0;
    int ks = conv1x1_ksplit(nsamp, cout, cin, hw, &kps);
    if (cout <= 64) ks = max(ks, conv1x1_ksplit(nsamp, cout, cin, hw, &kps, true));      // acr_conv1x1_x3's 64 x 256 tiling
    return ks > 1 ? (size_t)ks * nsamp * cout * hw : 0;
}
__global__ __launch_bounds__(256) void conv1x1_ksum_kernel(const float* __restrict__ ws, int ks, int64_t per4, const float* __restrict__ addend,
                                                           float* __restrict__ y, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int64_t n = i / per4, e = i - n * per4;
    const f32x4* p = reinterpret_cast<const f32x4*>(ws) + n * ks * per4 + e;
    f32x4 s = p[0];
    for (int k = 1; k < ks; ++k) {
        const f32x4 v = p[(int64_t)k * per4];
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    if (addend) {
        const f32x4 v = reinterpret_cast<const f32x4*>(addend)[i];
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    reinterpret_cast<f32x4*>(y)[i] = s;
}

extern "C" int acr_conv1x1_f32(int32_t math, const float* w, int32_t w_transposed, const float* x, const float* addend, float* y, int32_t nsamp,
                               int32_t cout, int32_t cin, int32_t hw, float* ws, void* stream) {
    // cout / cin are the channel counts of THIS product.  w_transposed = 0: w is (cout, cin).  w_transposed = 1: w is stored
    // (cin, cout) -- the forward convolution's weight handed over as is for the input gradient, where the roles swap.
    ACR_CHECK_ARG(w && x && y, "acr_conv1x1_f32: null pointer");
    ACR_CHECK_ARG(nsamp > 0 && cout > 0 && cin > 0 && hw > 0 && (hw % 4) == 0 && (cin % 4) == 0 && (cout % 4) == 0,
                  "acr_conv1x1_f32: need hw, cin, cout %% 4 == 0 (n=%d co=%d ci=%d hw=%d)", nsamp, cout, cin, hw);
    ACR_CHECK_ARG(al16(w) && al16(x) && al16(y) && al16(addend), "acr_conv1x1_f32: 16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    GemmF32Args g;
    conv_args(g, cout, hw, cin);
    g.a = w; g.b = x; g.ldb = hw; g.b_zs = (int64_t)cin * hw;
    g.c = y; g.ldc = hw; g.c_zs = (int64_t)cout * hw;
    g.aux = addend; g.ldaux = hw; g.aux_zs = (int64_t)cout * hw;
    g.nsplit = nsamp;
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n * nsamp));
    const bool dma = (cin % F_BK) == 0;
    if (math == ACR_MATH_FP16X2) {
        acr_set_error("acr_conv1x1_f32: ACR_MATH_FP16X2 is built for the block Linears only (acr_gemm_f32)");
        return ACR_ERR_UNSUPPORTED;
    }
    ACR_CHECK_ARG(math == ACR_MATH_F32 || math == ACR_MATH_BF16X3, "acr_conv1x1_f32: bad math %d", math);
    const bool split = dma && math == ACR_MATH_BF16X3;
    int kps = 0;
    const int ks = (split && ws && al16(ws)) ? conv1x1_ksplit(nsamp, cout, cin, hw, &kps) : 1;
    if (ks > 1) {                           // K-split small launch: slabs [sample][part] of raw sums, then the part sum (+ addend)
        g.lda = w_transposed ? cout : cin;
        g.nsplit = nsamp * ks; g.ksplit = ks; g.kps = kps; g.k_zs = kps;
        g.c = ws; g.ldc = hw; g.aux = nullptr;
        const dim3 kgrid((unsigned)(g.tiles_m * g.tiles_n * nsamp * ks));
        if (!w_transposed) gemm_f32_conv_launch(GEMM_LOOP_SPLIT, true, false, 3, kgrid, g, st);
        else gemm_f32_conv_launch(GEMM_LOOP_SPLIT, false, false, 3, kgrid, g, st);
        const int64_t per4 = (int64_t)cout * hw / 4, n4 = per4 * nsamp;
        hipLaunchKernelGGL(conv1x1_ksum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float*)ws, ks, per4, addend, y, n4);
        return acr_check_launch("acr_conv1x1_f32(K-split)");
    }
    if (!w_transposed) {                    // w = (cout, cin): rows = output channels, k contiguous
        g.lda = cin;
        if (split) gemm_f32_conv_launch(GEMM_LOOP_SPLIT, true, false, 0, grid, g, st);
        else if (dma) gemm_f32_conv_launch(GEMM_LOOP_DMA, true, false, 0, grid, g, st);
        else gemm_f32_conv_launch(GEMM_LOOP_STAGED, true, false, 0, grid, g, st);
    } else {                                                // w = (cin, cout) as stored by the forward conv: A[i][k] = w[k][i]
        g.lda = cout;
        if (split) gemm_f32_conv_launch(GEMM_LOOP_SPLIT, false, false, 0, grid, g, st);
        else if (dma) gemm_f32_conv_launch(GEMM_LOOP_DMA, false, false, 0, grid, g, st);
        else gemm_f32_conv_launch(GEMM_LOOP_STAGED, false, false, 0, grid, g, st);
    }
    return acr_check_launch("acr_conv1x1_f32");
}

// The same convolution with the weight given as a split-product image (acr_x3_image of W (cout x cin) for the forward;
// acr_x3_image_t of the forward's W for the input gradient, where cout / cin are THIS product's): gemm_f32_wimg_kernel.
extern "C" int acr_conv1x1_x3(const float* w_img, const float* x, const float* addend, float* y, int32_t nsamp, int32_t cout, int32_t cin,
                              int32_t hw, float* ws, void* stream) {
    ACR_CHECK_ARG(w_img && x && y, "acr_conv1x1_x3: null pointer");
    ACR_CHECK_ARG(nsamp > 0 && cout > 0 && cin > 0 && hw >= 4 && (hw % 4) == 0 && (cin % P_BK) == 0 && (cout % 4) == 0,
                  "acr_conv1x1_x3: need hw, cout %% 4 == 0, cin %% 16 == 0 (n=%d co=%d ci=%d hw=%d)", nsamp, cout, cin, hw);
    ACR_CHECK_ARG(al16(w_img) && al16(x) && al16(y) && al16(addend), "acr_conv1x1_x3: 16-byte alignment");
    ACR_CHECK_ARG((int64_t)cin * hw < (1ll << 30), "acr_conv1x1_x3: sample too large for 32-bit offsets");
    hipStream_t st = (hipStream_t)stream;
    GemmF32Args g;
    conv_args(g, cout, hw, cin);
    g.a = w_img; g.lda = 0; g.b = x; g.ldb = hw; g.b_zs = (int64_t)cin * hw;
    g.c = y; g.ldc = hw; g.c_zs = (int64_t)cout * hw;
    g.aux = addend; g.ldaux = hw; g.aux_zs = (int64_t)cout * hw;
    g.nsplit = nsamp; g.kps = cin; g.k_zs = 0;
    const bool wide64 = cout <= 64 && hw >= 4;              // 64 x 256 tiles: all four waves compute (gemm_f32_wimg64_kernel)
    if (wide64) { g.tiles_m = 1; g.tiles_n = (hw + W64_BN - 1) / W64_BN; g.tiles_launch = g.tiles_n; }
    int kps = 0;
    const int ks = (ws && al16(ws)) ? conv1x1_ksplit(nsamp, cout, cin, hw, &kps, wide64) : 1;
    if (ks > 1) {                                           // K-split small launch (conv1x1_ksplit): slabs, then the part sum (+ addend)
        g.nsplit = nsamp * ks; g.ksplit = ks; g.kps = kps; g.k_zs = kps;
        g.c = ws; g.aux = nullptr;
        if (wide64) hipLaunchKernelGGL((gemm_f32_wimg64_kernel<3>), dim3((unsigned)(g.tiles_n * nsamp * ks)), dim3(256), 0, st, g);
        else
        hipLaunchKernelGGL((gemm_f32_wimg_kernel<3>), dim3((unsigned)(g.tiles_m * g.tiles_n * nsamp * ks)), dim3(256), 0, st, g);
        const int64_t per4 = (int64_t)cout * hw / 4, n4 = per4 * nsamp;
        hipLaunchKernelGGL(conv1x1_ksum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float*)ws, ks, per4, addend, y, n4);
        return acr_check_launch("acr_conv1x1_x3(K-split)");
    }
    if (wide64) hipLaunchKernelGGL((gemm_f32_wimg64_kernel<0>), dim3((unsigned)(g.tiles_n * nsamp)), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((gemm_f32_wimg_kernel<0>), dim3((unsigned)(g.tiles_m * g.tiles_n * nsamp)), dim3(256), 0, st, g);
    return acr_check_launch("acr_conv1x1_x3");
}

// pixels of a sample are additionally split so that tiles x samples x parts fills the chip's 512 workgroup slots (a 64x64
// weight at 112^2 is ONE tile per sample: 32 workgroups of 392 chunks each otherwise); at least 512 pixels per part
static int conv_wgrad_ksplit(int nsamp, int cout, int cin, int hw) {
    const int tiles = ((cout + F_BM - 1) / F_BM) * ((cin + F_BN - 1) / F_BN) * nsamp;
    int ks = 512 / tiles;
    const int maxs = hw / 512;
    if (ks > maxs) ks = maxs;
    if (ks < 1) ks = 1;
    const int kps = ((hw + ks - 1) / ks + F_BK - 1) / F_BK * F_BK;
    return (hw + kps - 1) / kps;                            // every part non-empty
}
extern "C" size_t acr_conv1x1_wgrad_f32_ws_floats(int32_t nsamp, int32_t cout, int32_t cin, int32_t hw) {
    return (size_t)nsamp * conv_wgrad_ksplit(nsamp, cout, cin, hw) * cout * cin;
}

extern "C" int acr_conv1x1_wgrad_f32(int32_t math, const float* dy, const float* x, int32_t nsamp, int32_t cout, int32_t cin, int32_t hw, float* ws,
                                     float* dw, void* stream) {
    ACR_CHECK_ARG(dy && x && ws && dw, "acr_conv1x1_wgrad_f32: null pointer");
    ACR_CHECK_ARG(nsamp > 0 && cout > 0 && cin > 0 && hw > 0 && (hw % 4) == 0 && (cin % 4) == 0 && (cout % 4) == 0,
                  "acr_conv1x1_wgrad_f32: need hw, cin, cout %% 4 == 0");
    ACR_CHECK_ARG(al16(dy) && al16(x) && al16(dw) && al16(ws), "acr_conv1x1_wgrad_f32: 16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    GemmF32Args g;
    conv_args(g, cout, cin, hw);
    g.a = dy; g.lda = hw; g.a_zs = (int64_t)cout * hw;
    g.b = x; g.ldb = hw; g.b_zs = (int64_t)cin * hw;
    g.c = ws; g.ldc = cin;
    const int ks = conv_wgrad_ksplit(nsamp, cout, cin, hw);
    g.ksplit = ks;
    g.kps = ((hw + ks - 1) / ks + F_BK - 1) / F_BK * F_BK;
    ACR_CHECK_ARG((int64_t)(ks - 1) * g.kps < hw, "acr_conv1x1_wgrad_f32: internal split plan");
    g.k_zs = g.kps;
    g.nsplit = nsamp * ks;
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n * g.nsplit));
    if (math == ACR_MATH_FP16X2) {
        acr_set_error("acr_conv1x1_wgrad_f32: ACR_MATH_FP16X2 is built for the block Linears only (acr_gemm_f32)");
        return ACR_ERR_UNSUPPORTED;
    }
    ACR_CHECK_ARG(math == ACR_MATH_F32 || math == ACR_MATH_BF16X3, "acr_conv1x1_wgrad_f32: bad math %d", math);
    // the split-product kernel advances in 16-deep stages: pixel counts that are multiples of 16 suffice (28 x 28 = 784 = 49 x 16
    // took the register-staged exact kernel before: 2.6 ms of the f32_split step)
    if ((hw % S_BK) == 0 && math == ACR_MATH_BF16X3)
        gemm_f32_conv_launch(GEMM_LOOP_SPLIT, true, true, 3, grid, g, st);
    else if ((hw % F_BK) == 0)
        gemm_f32_conv_launch(GEMM_LOOP_DMA, true, true, 3, grid, g, st);
    else
        gemm_f32_conv_launch(GEMM_LOOP_STAGED, true, true, 3, grid, g, st);
    const int64_t n4 = (int64_t)cout * cin / 4;
    if (!acr_slab_sum_wide(ws, g.nsplit, n4, dw, st)) gemm_f32_reduce(ws, g.nsplit, n4, dw, st);
    return acr_check_launch("acr_conv1x1_wgrad_f32");
}
