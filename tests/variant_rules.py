"""The choices the C entry points make on their own -- by a shape remainder, a leading dimension, a missing workspace or the low
bits of a pointer -- restated in Python, one function per choice.

tests/test_variants_gpu.py uses these functions to say which kernel variant a case reaches; tests/test_variants_cpu.py ties every
function to the source: each line of ``SOURCE`` must stand, whitespace normalised, in the named file of acr_wsss_amd/csrc, so that
a predicate edited there makes the tie fail instead of leaving a restatement that silently tests one side twice.

Alignments are given as the address modulo 16 (``None``: a null pointer, which the C predicates take as aligned)."""

# constants the predicates use (tied to their #define lines through SOURCE)
GW_BM, GB_BN = 320, 256                                      # gemm_bf16.hip: the wide kernel's tile
WIDE_MIN_TILES = 200
F_BM, F_BN, F_BK, S_BK = 128, 128, 32, 16                    # gemm_f32.h
C3_BM, C3_BN, C3_BK = 128, 128, 16                           # conv3x3.hip
SGD_CHUNK = 8192                                             # optim.hip (the tests read acr_sgd_chunk_elems(); this pins the tie)
MATH_SPLIT, MATH_FP16X2 = 1, 2                               # acr_math (include/acr_hip.h)
NT, NN, TN = 0, 1, 2
TN_NULL_WS_REFUSAL = "acr_gemm_f32: TN needs the acr_gemm_f32_ws_floats workspace"
FP16X2_REFUSAL = "acr_gemm_f32: fp16x2 needs the acr_gemm_f32_ws_floats workspace (16-byte aligned) and 16-byte aligned c / bias / aux / c2"


def al16(mod16):
    return mod16 is None or mod16 % 16 == 0


def _cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------
# acr_linear_bf16
# ------------------------------------------------------------------------------------------------
def linear_bf16_variant(M, N, ldy, ldr, y, bias, resid):
    """"scalar" (gemm_nt_bf16_kernel), "wide" (gemm_nt_bf16_wide_kernel) or "dma" (gemm_nt_bf16_dma_kernel)."""
    vec_ok = N % 8 == 0 and ldy % 8 == 0 and ldr % 8 == 0 and al16(y) and al16(bias) and al16(resid)
    if not vec_ok:
        return "scalar"
    tilesw = _cdiv(M, GW_BM) * _cdiv(N, GB_BN)
    return "wide" if tilesw >= WIDE_MIN_TILES else "dma"


# ------------------------------------------------------------------------------------------------
# acr_gemm_f32
# ------------------------------------------------------------------------------------------------
def gemm_tail_plan(M, N, K, x3=False):
    """(ntail, nsplit, kps) of gemm_tail_plan."""
    if K % F_BK != 0 or N % 4 != 0:
        return 0, 1, 0
    tiles = _cdiv(M, F_BM) * _cdiv(N, F_BN)
    small = tiles <= 256 if x3 else tiles * 3 <= 512
    R = tiles if small else tiles % 256
    if (not small and tiles < 512) or R == 0:
        return 0, 1, 0
    smin = 2 if (x3 and small) else 3
    s = min(512 // R, 16 if small else 8)
    s = min(s, K // (2 * F_BK))
    if s < smin:
        return 0, 1, 0
    kps = _cdiv(_cdiv(K, s), F_BK) * F_BK
    s = _cdiv(K, kps)
    if s < smin:
        return 0, 1, 0
    return R, s, kps


def gemm_f32_vec_ok(ldc, ldaux, c, bias, aux, c2):
    return al16(c) and ldc % 4 == 0 and al16(bias) and (aux is None or (al16(aux) and ldaux % 4 == 0)) and al16(c2)


def off32_ok(mode, M, N, K, lda, ldb):
    """The LDS-DMA loops address an operand with 32-bit element offsets."""
    lim = (1 << 31) - (1 << 20)
    ea = (K if mode == TN else M) * lda
    eb = (N if mode == NT else K) * ldb
    return ea < lim and eb < lim


def gemm_f32_variant(mode, math, M, N, K, lda=None, ldb=None, ldc=None, ldaux=0, ws=0, c=0, bias=None, aux=None, c2=None):
    """The product's loop and whether tail tiles are K-split: (loop, tail) with loop in "refused" (fp16x2 without its workspace or
    aligned operands; TN without a workspace), "planes" (both operands split once into images, gemm_f32_planes_kernel), "split"
    (gemm_f32_split_kernel), "dma" (gemm_f32_dma_kernel), "staged" (gemm_f32_kernel) and tail = gemm_tail_plan's ntail as it is
    used (0: no tail launch).  ``ws``: the workspace's address modulo 16, None for a null workspace.  ``lda`` / ``ldb``: the
    operands' pitches, dense by default."""
    lda = (M if mode == TN else K) if lda is None else lda
    ldb = (K if mode == NT else N) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    dma = K % F_BK == 0 and off32_ok(mode, M, N, K, lda, ldb)
    planes_on = math in (MATH_SPLIT, MATH_FP16X2)
    if mode == TN:
        if ws is None or (math == MATH_FP16X2 and not al16(ws)):
            return "refused", 0
        if planes_on:                                        # (the split loop behind this return is not reachable through the entry)
            return "planes", 0
        return ("dma" if dma else "staged"), 0
    ws_ok = ws is not None and al16(ws)
    vec_ok = gemm_f32_vec_ok(ldc, ldaux, c, bias, aux, c2)
    ntail = gemm_tail_plan(M, N, K)[0]
    if not dma or not ws_ok or not vec_ok:
        ntail = 0
    if math == MATH_FP16X2:
        return ("planes" if ws_ok and vec_ok else "refused"), 0
    if planes_on and ws_ok and vec_ok:
        return "planes", 0
    if dma and math == MATH_SPLIT:
        return "split", ntail
    return ("dma" if dma else "staged"), ntail


# ------------------------------------------------------------------------------------------------
# acr_sgd_step_bf16 / acr_sgd_step_f32
# ------------------------------------------------------------------------------------------------
def sgd_variant(grad, master, mom, param=None):
    """"vec" or "scalar", per tensor of the table (``param``: the bf16 working copy; the fp32 step has none)."""
    return "vec" if al16(grad) and al16(master) and al16(mom) and al16(param) else "scalar"


# ------------------------------------------------------------------------------------------------
# pool.hip
# ------------------------------------------------------------------------------------------------
def maxpool_fwd_variant(elsize, pt, pl, w, wo, x, y, amax):
    """"vec4" (maxpool_fwd_vec4_kernel) or "scalar" (maxpool_fwd_kernel); ``amax`` modulo 4 matters."""
    if elsize == 4 and pt == 0 and pl == 0 and w % 8 == 0 and wo * 2 == w and al16(x) and al16(y) and amax % 4 == 0:
        return "vec4"
    return "scalar"


def maxpool_bwd_variant(elsize, pt, pl, h, w, ho, wo, dy, amax, dx):
    """"2x8" (maxpool_bwd_vec2x8_kernel), "8wide" (maxpool_bwd_vec_kernel) or "scalar" (maxpool_bwd_kernel)."""
    if (elsize == 4 and pt == 0 and pl == 0 and w % 8 == 0 and h % 2 == 0 and wo * 2 == w and ho * 2 == h and al16(dx) and al16(dy)
            and amax % 4 == 0):
        return "2x8"
    if w % 8 == 0 and al16(dx):
        return "8wide"
    return "scalar"


def subsample2_variant(w, src, dst):
    """"vec" or "scalar" body of subsample2_fwd_kernel (src = x, dst = y) and subsample2_bwd_kernel (src = dy, dst = dx)."""
    return "vec" if w % 8 == 0 and al16(src) and al16(dst) else "scalar"


# ------------------------------------------------------------------------------------------------
# K-split of the small convolution launches
# ------------------------------------------------------------------------------------------------
def c3_fwd_ksplit(nsamp, cout, cin, HW, wide64=False, ntap=9):
    tiles = _cdiv(HW, 256) * nsamp if wide64 else _cdiv(cout, C3_BM) * _cdiv(HW, C3_BN) * nsamp
    nst = ntap * cin // C3_BK
    if tiles >= 192:
        return 1
    ks = min(512 // tiles, nst // 8)
    if ks < 2:
        return 1
    sps = _cdiv(nst, ks)
    return _cdiv(nst, sps)


def conv1x1_ksplit(nsamp, cout, cin, hw, wide64=False):
    tiles = _cdiv(hw, 256) * nsamp if wide64 else _cdiv(cout, F_BM) * _cdiv(hw, F_BN) * nsamp
    if tiles >= 192 or cin % F_BK != 0:
        return 1
    ks = min(512 // tiles, cin // 64)
    if ks < 2:
        return 1
    kps = _cdiv(_cdiv(cin, ks), S_BK) * S_BK
    return _cdiv(cin, kps)


def conv_ksplit(entry, ws, nsamp, cout, cin, HW, ntap=9, math=MATH_SPLIT):
    """Parts the contraction is split into by ``entry`` (1: unsplit) -- taken only with a 16-byte aligned workspace."""
    if ws is None or not al16(ws):
        return 1
    if entry == "acr_conv3x3_f32":
        return c3_fwd_ksplit(nsamp, cout, cin, HW)
    if entry == "acr_conv3x3_x3":
        return c3_fwd_ksplit(nsamp, cout, cin, HW, cout <= 64)
    if entry == "acr_conv_taps_x3":                          # (and yrows == cout: the forward; the tests run that)
        return c3_fwd_ksplit(nsamp, cout, cin, HW, cout <= 64, ntap)
    if entry == "acr_conv1x1_f32":
        return conv1x1_ksplit(nsamp, cout, cin, HW) if (math == MATH_SPLIT and cin % F_BK == 0) else 1
    if entry == "acr_conv1x1_x3":
        return conv1x1_ksplit(nsamp, cout, cin, HW, cout <= 64 and HW >= 4)
    raise KeyError(entry)


# ------------------------------------------------------------------------------------------------
# acr_train_cam_f32, acr_sal_pseudo_compose
# ------------------------------------------------------------------------------------------------
def train_cam_variant(ow, out):
    """16-byte ("vec") or 4-byte ("scalar") stores of tc_extremes_kernel / tc_write_kernel."""
    return "vec" if ow % 4 == 0 and al16(out) else "scalar"


def sal_pseudo_variant(hw, cams, saliency, saliency_out, label):
    """four pixels per thread ("vec") or one ("scalar") in psal_hist_kernel / psal_pixel_kernel; the byte maps count modulo 4."""
    return "vec" if hw % 4 == 0 and al16(cams) and (saliency | saliency_out | label) % 4 == 0 else "scalar"


# ------------------------------------------------------------------------------------------------
# acr_groupnorm_fwd_f32 / acr_groupnorm_bwd_f32: which kernel family a (sample, group) of cg channels x HW pixels takes
# ------------------------------------------------------------------------------------------------
GNF_GROUPS, GNF_MAXU, GNF_RV, GNF_RV_FWD_MAX, GNF_RV_BWD_MAX = 32, 64, 8, 25, 13
GNF_SHIFT_FAR = 0.96          # m1^2 / m2 above which the register-resident forward sums the group again about its mean


def gnf_units(cg, HW, nwaves):
    """(S, segv, units) of gnf_units"""
    vpc = HW >> 2
    S = 1 if cg >= nwaves else _cdiv(nwaves, cg)
    segv = _cdiv(_cdiv(vpc, S), 64) * 64
    S = _cdiv(vpc, segv)
    return S, segv, cg * S


def gnf_reg_plan_nt(cg, HW, nt):
    """(ok, nt, slots) of gnf_reg_plan_nt"""
    nw = nt // 64
    S, segv, units = gnf_units(cg, HW, nw)
    ch = _cdiv(segv, 64)
    upw = _cdiv(units, nw)
    return units <= GNF_MAXU, nt, upw * ch


def gnf_reg_plan(cg, HW, max_slots, backward):
    """(ok, nt, slots) of gnf_reg_plan"""
    if not backward:
        ok, nt, slots = gnf_reg_plan_nt(cg, HW, 1024 if cg * (HW >> 2) > 2048 else 256)
        return ok and slots <= max_slots and (slots <= GNF_RV or nt == 1024), nt, slots
    for nt in (256, 512, 1024):
        ok, nt, slots = gnf_reg_plan_nt(cg, HW, nt)
        if ok and slots <= max_slots:
            return True, nt, slots
    return False, 1024, slots


def gnf_fwd_parts(N, C, HW):
    """parts a (sample, group) is cut into by the small-launch forward (1: one workgroup per group)"""
    groups, nvec = N * GNF_GROUPS, (C // GNF_GROUPS) * HW // 4
    if groups > 128 or nvec < 4096:
        return 1
    P = min(512 // groups, 8)
    while P > 1 and nvec // P < 1024:
        P -= 1
    return P


def _gnf_reg_template(slots):
    return GNF_RV if slots <= GNF_RV else GNF_RV_BWD_MAX if slots <= GNF_RV_BWD_MAX else GNF_RV_FWD_MAX


def gnf_fwd_variant(N, C, HW, ws):
    """("parts", P), ("reg", threads, slot template) or ("streamed", threads); ``ws``: the small-launch workspace was passed"""
    cg = C // GNF_GROUPS
    P = gnf_fwd_parts(N, C, HW) if ws else 1
    if P > 1:
        return "parts", P
    ok, nt, slots = gnf_reg_plan(cg, HW, GNF_RV_FWD_MAX, False)
    if ok:
        return "reg", nt, GNF_RV if nt == 256 else _gnf_reg_template(slots)
    return "streamed", 1024 if cg * HW >= 32768 else 256


def gnf_bwd_variant(N, C, HW):
    """("reg", threads, slot template) or ("streamed", threads)"""
    cg = C // GNF_GROUPS
    ok, nt, slots = gnf_reg_plan(cg, HW, GNF_RV_BWD_MAX, True)
    if ok:
        return "reg", nt, GNF_RV if slots <= GNF_RV else GNF_RV_BWD_MAX
    return "streamed", 1024 if HW >= 4096 else 256


# ------------------------------------------------------------------------------------------------
# the source lines each restatement stands for: rule -> [(file under acr_wsss_amd/csrc, line)]
# ------------------------------------------------------------------------------------------------
SOURCE = {
    "linear_bf16_variant": [
        ("gemm_bf16.hip", "#define GB_BN 256"),
        ("gemm_bf16.hip", "#define GW_BM 320"),
        ("gemm_bf16.hip", "const int64_t tilesw = (int64_t)((M + GW_BM - 1) / GW_BM) * ((N + GB_BN - 1) / GB_BN);"),
        ("gemm_bf16.hip", "const bool wide_ok = tilesw >= 200;"),
        ("gemm_bf16.hip", "const bool vec_ok = (N % 8) == 0 && (ldy % 8) == 0 && (ldr % 8) == 0 && ((uintptr_t)y & 15) == 0 && "
                          "((uintptr_t)bias & 15) == 0 && ((uintptr_t)resid & 15) == 0;"),
        ("gemm_bf16.hip", "if (!vec_ok) \\"),
        ("gemm_bf16.hip", "else if (wide_ok) \\"),
    ],
    "gemm_tail_plan": [
        ("gemm_f32.h", "#define F_BM 128"), ("gemm_f32.h", "#define F_BN 128"), ("gemm_f32.h", "#define F_BK 32"),
        ("gemm_f32.hip", "if ((K % F_BK) != 0 || (N % 4) != 0) return p;"),
        ("gemm_f32.hip", "const int tiles = ((M + F_BM - 1) / F_BM) * ((N + F_BN - 1) / F_BN);"),
        ("gemm_f32.hip", "const bool small = x3 ? tiles <= 256 : tiles * 3 <= 512;"),
        ("gemm_f32.hip", "const int R = small ? tiles : tiles % 256;"),
        ("gemm_f32.hip", "if ((!small && tiles < 512) || R == 0) return p;"),
        ("gemm_f32.hip", "const int smin = x3 && small ? 2 : 3;"),
        ("gemm_f32.hip", "int s = 512 / R;"),
        ("gemm_f32.hip", "if (s > (small ? 16 : 8)) s = small ? 16 : 8;"),
        ("gemm_f32.hip", "const int maxs = K / (2 * F_BK);"),
        ("gemm_f32.hip", "if (s > maxs) s = maxs;"),
        ("gemm_f32.hip", "const int kps = ((K + s - 1) / s + F_BK - 1) / F_BK * F_BK;"),
        ("gemm_f32.hip", "s = (K + kps - 1) / kps;"),
        ("gemm_f32.hip", "p.ntail = R; p.nsplit = s; p.kps = kps;"),
    ],
    "gemm_f32_variant": [
        ("gemm_f32.h", "static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }"),
        ("gemm_f32.hip", "const bool split = math == ACR_MATH_BF16X3;"),
        ("gemm_f32.hip", "const bool dma = (K % F_BK) == 0 && off32_ok(M, N, K, lda, ldb, mode);"),
        ("gemm_f32.hip", "TailPlan tp = gemm_tail_plan(M, N, K);"),
        ("gemm_f32.hip", "const bool vec_ok = al16(c) && (ldc % 4) == 0 && (!bias || al16(bias)) && (!aux || (al16(aux) && (ldaux % 4) == 0)) && "
                         "(!c2 || al16(c2));"),
        ("gemm_f32.hip", "if (!dma || !ws || !al16(ws) || !vec_ok) tp.ntail = 0;"),
        ("gemm_f32.hip", 'ACR_CHECK_ARG(ws && al16(ws) && vec_ok, "%s");' % FP16X2_REFUSAL),
        ("gemm_f32.hip", "if (pl.on && ws && al16(ws) && vec_ok) {"),
        ("gemm_f32.hip", "if (dma && split) hipLaunchKernelGGL((gemm_f32_split_kernel<AK, BK_, ACTV>), grid, dim3(256), 0, st, g); \\"),
        ("gemm_f32.hip", "else if (dma) hipLaunchKernelGGL((gemm_f32_dma_kernel<AK, BK_, ACTV>), grid, dim3(256), 0, st, g); \\"),
        ("gemm_f32.hip", "if (tp.ntail) { // ... then the tail tiles, K-split into slabs, and their epilogue"),
        ("gemm_f32.hip", "const int64_t lim = (1ll << 31) - (1 << 20);"),
        ("gemm_f32.hip", "const int64_t ea = (mode == ACR_GEMM_TN ? K : M) * lda, eb = (mode == ACR_GEMM_NT ? N : K) * ldb;"),
        ("gemm_f32.hip", "return ea < lim && eb < lim;"),
        # TN
        ("gemm_f32.hip", 'ACR_CHECK_ARG(ws, "%s");' % TN_NULL_WS_REFUSAL),
        ("gemm_f32.hip", 'ACR_CHECK_ARG(al16(ws), "acr_gemm_f32: ws must be 16-byte aligned");'),
        ("gemm_f32.hip", "if (pl.on) { // both operands split once into images, then the product on the images"),
        ("gemm_f32.hip", "else if ((K % F_BK) == 0 && off32_ok(M, N, K, lda, ldb, mode))"),
        ("gemm_planes.hip", "if (math != ACR_MATH_BF16X3 && math != ACR_MATH_FP16X2) return p;"),
        ("gemm_planes.hip", "p.on = true; p.nkb = (K + P_BK - 1) / P_BK;"),
    ],
    "sgd_variant": [
        ("optim.hip", "#define SGD_CHUNK 8192"),
        ("optim.hip", "const bool vec = ((((uintptr_t)g | (uintptr_t)p) & 15) == 0) && ((((uintptr_t)t.master | (uintptr_t)t.mom) & 15) == 0);"),
        ("optim.hip", "const bool vec = ((((uintptr_t)g | (uintptr_t)t.master | (uintptr_t)t.mom) & 15) == 0);"),
    ],
    "maxpool_fwd_variant": [
        ("pool.hip", "if (sizeof(T) == 4 && pad_top == 0 && pad_left == 0 && (w % 8) == 0 && wo * 2 == w && ((uintptr_t)x & 15) == 0 && "
                     "((uintptr_t)y & 15) == 0 && ((uintptr_t)amax & 3) == 0) {"),
    ],
    "maxpool_bwd_variant": [
        ("pool.hip", "if (sizeof(T) == 4 && pad_top == 0 && pad_left == 0 && (w % 8) == 0 && (h % 2) == 0 && wo * 2 == w && ho * 2 == h && "
                     "((uintptr_t)dx & 15) == 0 && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)amax & 3) == 0) {"),
        ("pool.hip", "if ((w % 8) == 0 && ((uintptr_t)dx & 15) == 0) {"),
    ],
    "subsample2_variant": [
        ("pool.hip", "const bool vec = (w % 8) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;"),
        ("pool.hip", "const bool vec = (w % 8) == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)dy & 15) == 0;"),
    ],
    "c3_fwd_ksplit": [
        ("conv3x3.hip", "#define C3_BM 128"), ("conv3x3.hip", "#define C3_BN 128"), ("conv3x3.hip", "#define C3_BK 16"),
        ("conv3x3.hip", "const int tiles = wide64 ? ((HW + 255) / 256) * nsamp : ((cout + C3_BM - 1) / C3_BM) * ((HW + C3_BN - 1) / C3_BN) * nsamp;"),
        ("conv3x3.hip", "const int nst = ntap * cin / C3_BK;"),
        ("conv3x3.hip", "if (tiles >= 192) return 1;"),
        ("conv3x3.hip", "int ks = 512 / tiles;"),
        ("conv3x3.hip", "if (ks > nst / 8) ks = nst / 8;"),
        ("conv3x3.hip", "if (ks < 2) return 1;"),
        ("conv3x3.hip", "const int sps = (nst + ks - 1) / ks;"),
        ("conv3x3.hip", "return (nst + sps - 1) / sps;"),
    ],
    "conv1x1_ksplit": [
        ("gemm_f32.h", "#define S_BK 16"),
        ("conv1x1.hip", "const int tiles = wide64 ? ((hw + 255) / 256) * nsamp : ((cout + F_BM - 1) / F_BM) * ((hw + F_BN - 1) / F_BN) * nsamp;"),
        ("conv1x1.hip", "if (tiles >= 192 || (cin % F_BK) != 0) return 1;"),
        ("conv1x1.hip", "int ks = 512 / tiles;"),
        ("conv1x1.hip", "if (ks > cin / 64) ks = cin / 64;"),
        ("conv1x1.hip", "if (ks < 2) return 1;"),
        ("conv1x1.hip", "const int kps = ((cin + ks - 1) / ks + S_BK - 1) / S_BK * S_BK;"),
        ("conv1x1.hip", "return (cin + kps - 1) / kps;"),
    ],
    "conv_ksplit": [
        ("conv3x3.hip", "g.ksplit = (ws && ((uintptr_t)ws & 15) == 0) ? c3_fwd_ksplit(nsamp, cout, cin, g.HW) : 1;"),
        ("conv3x3.hip", "const bool wide64 = cout <= 64;"),
        ("conv3x3.hip", "g.ksplit = (ws && ((uintptr_t)ws & 15) == 0) ? c3_fwd_ksplit(nsamp, cout, cin, g.HW, wide64) : 1;"),
        ("conv3x3.hip", "g.ksplit = (ws && ((uintptr_t)ws & 15) == 0 && yrows == cout) ? c3_fwd_ksplit(nsamp, cout, cin, g.HW, wide64, ntap) : 1;"),
        ("conv1x1.hip", "const bool dma = (cin % F_BK) == 0;"),
        ("conv1x1.hip", "const bool split = dma && math == ACR_MATH_BF16X3;"),
        ("conv1x1.hip", "const int ks = (split && ws && al16(ws)) ? conv1x1_ksplit(nsamp, cout, cin, hw, &kps) : 1;"),
        ("conv1x1.hip", "const bool wide64 = cout <= 64 && hw >= 4;"),
        ("conv1x1.hip", "const int ks = (ws && al16(ws)) ? conv1x1_ksplit(nsamp, cout, cin, hw, &kps, wide64) : 1;"),
    ],
    "train_cam_variant": [
        ("traincam.hip", "const bool vec = ow % 4 == 0 && ((uintptr_t)out & 15) == 0;"),
    ],
    "sal_pseudo_variant": [
        ("pseudo_sal.hip", "const bool vec = hw % 4 == 0 && ((uintptr_t)cams & 15) == 0 && "
                           "(((uintptr_t)saliency | (uintptr_t)saliency_out | (uintptr_t)label) & 3) == 0;"),
    ],
    "gnf_units": [
        ("groupnorm_f32.hip", "u.S = cg >= nwaves ? 1 : (nwaves + cg - 1) / cg;"),
        ("groupnorm_f32.hip", "u.segv = ((vpc + u.S - 1) / u.S + 63) / 64 * 64;"),
        ("groupnorm_f32.hip", "u.S = (vpc + u.segv - 1) / u.segv;"),
        ("groupnorm_f32.hip", "u.units = cg * u.S;"),
    ],
    "gnf_reg_plan": [
        ("groupnorm_f32.hip", "#define GNF_RV 8"),
        ("groupnorm_f32.hip", "#define GNF_MAXU 64 // units per (sample, group): max(channels per group, waves) <= 64"),
        ("groupnorm_f32.hip", "p.ch = (p.un.segv + 63) / 64;"),
        ("groupnorm_f32.hip", "p.upw = (p.un.units + nw - 1) / nw;"),
        ("groupnorm_f32.hip", "p.slots = p.upw * p.ch;"),
        ("groupnorm_f32.hip", "p.ok = p.un.units <= GNF_MAXU;"),
        ("groupnorm_f32.hip", "p = gnf_reg_plan_nt(cg, HW, cg * (HW >> 2) > 2048 ? 1024 : 256);"),
        ("groupnorm_f32.hip", "p.ok = p.ok && p.slots <= max_slots && (p.slots <= GNF_RV || p.nt == 1024);"),
        ("groupnorm_f32.hip", "for (int nt = 256; nt <= 1024; nt *= 2) {"),
        ("groupnorm_f32.hip", "if (p.ok && p.slots <= max_slots) return p;"),
    ],
    "gnf_fwd_parts": [
        ("groupnorm_f32.hip", "#define GNF_GROUPS 32"),
        ("groupnorm_f32.hip", "const int groups = N * GNF_GROUPS, nvec = (C / GNF_GROUPS) * HW / 4;"),
        ("groupnorm_f32.hip", "if (groups > 128 || nvec < 4096) return 1;"),
        ("groupnorm_f32.hip", "int P = 512 / groups;"),
        ("groupnorm_f32.hip", "if (P > 8) P = 8;"),
        ("groupnorm_f32.hip", "while (P > 1 && nvec / P < 1024) --P; // at least 4 vectors per thread and part"),
        ("groupnorm_f32.hip", "return P > 1 ? (size_t)N * GNF_GROUPS * P * 2 : 0;"),
    ],
    "gnf_fwd_variant": [
        ("groupnorm_f32.hip", "#define GNF_SHIFT_FAR 0.96f"),
        ("groupnorm_f32.hip", "if (__builtin_amdgcn_readfirstlane((int)(m1 * m1 > GNF_SHIFT_FAR * m2))) {"),
        ("groupnorm_f32.hip", "#define GNF_RV_FWD_MAX 25"), ("groupnorm_f32.hip", "#define GNF_RV_BWD_MAX 13"),
        ("groupnorm_f32.hip", "const int P = ws ? gnf_fwd_parts(N, C, HW) : 1;"),
        ("groupnorm_f32.hip", "if (P > 1) { // small launch: every (sample, group) cut into P parts, two launches"),
        ("groupnorm_f32.hip", "const int nvec = cg * HW / 4, vper = (nvec + P - 1) / P;"),
        ("groupnorm_f32.hip", "const GnfRegPlan rp = gnf_reg_plan(cg, HW, GNF_RV_FWD_MAX, false);"),
        ("groupnorm_f32.hip", "const bool big = (int64_t)cg * HW >= 32768; // >= 8 vectors per thread at 1024 threads"),
        ("groupnorm_f32.hip", "if ((P).nt == 256) GNF_LAUNCH_REG(KERNEL, 256, GNF_RV, P, __VA_ARGS__) \\"),
        ("groupnorm_f32.hip", "else if ((P).slots <= GNF_RV) GNF_LAUNCH_REG(KERNEL, 1024, GNF_RV, P, __VA_ARGS__) \\"),
        ("groupnorm_f32.hip", "else if ((P).slots <= GNF_RV_BWD_MAX) GNF_LAUNCH_REG(KERNEL, 1024, GNF_RV_BWD_MAX, P, __VA_ARGS__) \\"),
    ],
    "gnf_bwd_variant": [
        ("groupnorm_f32.hip", "const GnfRegPlan rp = gnf_reg_plan(cg, HW, GNF_RV_BWD_MAX, true);"),
        ("groupnorm_f32.hip", "const bool big = (int64_t)HW >= 4096; // per-channel loops: 1024 threads only when a channel feeds them"),
        ("groupnorm_f32.hip", "if ((P).slots <= GNF_RV) { GNF_LAUNCH_REG_NT(KERNEL, GNF_RV, P, __VA_ARGS__) } \\"),
        ("groupnorm_f32.hip", "else { GNF_LAUNCH_REG_NT(KERNEL, GNF_RV_BWD_MAX, P, __VA_ARGS__) }"),
    ],
}
