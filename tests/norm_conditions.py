"""Ill-conditioned inputs for the norm kernels (GroupNorm, LayerNorm, weight standardisation), stated once for the CPU test that
proves the cases decisive (tests/test_norm_conditions_cpu.py) and the GPU test that runs the kernels on them
(tests/test_norm_conditions_gpu.py).

Every case is a seeded set of fp32 CPU tensors (holding bf16 values where the kernel stores bf16), the float64 result of the
operation on them (``ref``) and torch's own CPU result in the kernel's storage type (``tor``; bf16 storage: torch's fp32 result on
the bf16 values, rounded to bf16 -- what a kernel with fp32 arithmetic can be held to, and the smaller error of the two).  Cases are cached: treat them as
read-only.

Tolerance rule (``rule``), per compared quantity: the device error against float64 may be at most

    max(2 x the error of torch's CPU result in the same storage type on the same inputs, the existing kernel_checks.TOL entry)

Both terms come from the reference side.  ``rule`` also asserts the cap that keeps the first term small: torch's fp32 error is
at most ``CAP`` of max|reference| (bf16 storage: at most the TOL entry itself), so the rule never grants more than twice that.

A fused ReLU: the float64 gradients and torch's are both routed through the float64 result's mask, so that torch's error is the
error of its arithmetic, not of elements that fall on the other side of zero (kernel_checks routes the device's gradients through
the device's own mask in the same way)."""
import functools
import math

import torch
import torch.nn.functional as F

import kernel_checks as KC

F32, BF16 = torch.float32, torch.bfloat16
CAP = 5e-5
GN_EPS, LN_EPS, WS_EPS = 1e-5, 1e-6, 1e-5
GN_SIGMAS, LN_SIGMAS, WS_SIGMAS = 100.0, 1000.0, 100.0
GN_CONDITIONS = ("offset", "first", "first_offset", "last", "channel_first", "part_first", "constant", "first_4", "first_6")
# first_4 / first_6: the first element 4 resp. 6 sigma out -- either side of GNF_SHIFT_FAR (m1^2 / m2 = k^2 / (1 + k^2): 0.941 and
# 0.973 against 0.96), where the register-resident forward leaves its shifted sums for the two-pass
GN_FIRST_SIGMAS = {"first_4": 4.0, "first_6": 6.0}


def gn_sigmas(cond):
    return GN_FIRST_SIGMAS.get(cond, GN_SIGMAS)
LN_CONDITIONS = ("offset", "first", "last", "constant", "tiny", "huge")
DYADIC = (3.25, -0.5, 1024.0, -7.75, 0.125, 96.0, -640.0, 1.5)


def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _store(t, dtype):
    """fp32 tensor holding values of the storage type"""
    return t.to(dtype).float()


def place_outliers(rows, cols, sigmas, dtype):
    """rows: (R, n) fp32 of storage-type values.  Sets rows[:, cols] to the mean + ``sigmas`` standard deviations of the row's
    OTHER elements (float64 statistics), rounded to the storage type and, where the rounding fell short, moved up until it is at
    least that far out."""
    keep = torch.ones(rows.shape[1], dtype=torch.bool)
    keep[cols] = False
    rest = rows[:, keep].double()
    m, s = rest.mean(1, keepdim=True), rest.std(1, unbiased=False, keepdim=True)
    v = _store((m + sigmas * s).float(), dtype)
    for _ in range(4):
        short = (v.double() - m) < sigmas * s
        v = torch.where(short, _store(v + v.abs() * 2.0 ** -6 if dtype == BF16 else torch.nextafter(v, torch.full_like(v, math.inf)), dtype), v)
    rows[:, cols] = v.expand(-1, len(cols))
    return rows


def outlier_sigmas(rows, cols):
    """how many standard deviations of the row's other elements the elements at ``cols`` lie from their mean (float64), the least"""
    keep = torch.ones(rows.shape[1], dtype=torch.bool)
    keep[cols] = False
    rest = rows[:, keep].double()
    m, s = rest.mean(1, keepdim=True), rest.std(1, unbiased=False, keepdim=True)
    return float(((rows[:, cols].double() - m).abs() / s).min())


# ------------------------------------------------------------------------------------------------
# GroupNorm(32)
# ------------------------------------------------------------------------------------------------
def gn_outlier_cols(shape, cond, parts=None):
    """element indices inside a (sample, group) that ``cond`` makes outliers ([] for offset / constant); ``parts`` = (P, vper) of
    the small-launch path for part_first"""
    N, C, H, W = shape
    cg, HW = C // 32, H * W
    if cond in ("first", "first_offset") or cond in GN_FIRST_SIGMAS:
        return [0]
    if cond == "last":
        return [cg * HW - 1]
    if cond == "channel_first":
        return [c * HW for c in range(cg)]
    if cond == "part_first":
        P, vper = parts
        return [4 * p * vper for p in range(P)]
    return []


def gn_input(shape, cond, dtype=F32, parts=None):
    N, C, H, W = shape
    cg, HW = C // 32, H * W
    g = _gen(N, C, H, W, GN_CONDITIONS.index(cond), dtype == BF16)
    if cond == "constant":
        v = torch.tensor([DYADIC[i % len(DYADIC)] for i in range(N * 32)])
        return v.view(N * 32, 1).expand(-1, cg * HW).reshape(shape).contiguous()
    x = torch.randn(N * 32, cg * HW, generator=g) * 1.7
    if cond == "offset":
        x = x + (1000.0 if dtype == F32 else 16.0)
    if cond == "first_offset":
        x = x + 100.0
    x = _store(x, dtype)
    cols = gn_outlier_cols(shape, cond, parts)
    if cols:
        place_outliers(x, cols, gn_sigmas(cond), dtype)
    return x.reshape(shape).contiguous()


def _gn_run(x, w, b, r, dy, act, dt, mask):
    ls = [t.to(dt).clone().requires_grad_(True) for t in (x, w, b)] + ([r.to(dt).clone().requires_grad_(True)] if r is not None else [])
    pre = F.group_norm(ls[0], 32, ls[1], ls[2], GN_EPS)
    if r is not None:
        pre = pre + ls[3]
    y = pre if act == "none" else F.relu(pre)
    if mask is None:
        mask = torch.ones_like(pre, dtype=torch.bool) if act == "none" else pre.detach() > 0
    gs = torch.autograd.grad(pre, ls, grad_outputs=(dy.double() * mask).to(dt))
    out = dict(y=y.detach(), dx=gs[0], dgamma=gs[1], dbeta=gs[2])
    if r is not None:
        out["dresid"] = gs[3]
    return out, mask


@functools.lru_cache(maxsize=None)
def gn_case(shape, cond, act, dtype=F32, parts=None):
    N, C, H, W = shape
    x = gn_input(shape, cond, dtype, parts)
    g = _gen(C, H, 17)
    w = _store(1 + 0.2 * torch.randn(C, generator=g), dtype)
    b = _store(0.3 * torch.randn(C, generator=g), dtype)
    r = _store(torch.randn(shape, generator=g), dtype) if act == "add_relu" else None
    dy = _store(torch.randn(shape, generator=g), dtype)
    ref, mask = _gn_run(x, w, b, r, dy, act, torch.float64, None)
    tor, _ = _gn_run(x, w, b, r, dy, act, F32, mask)
    tor = {k: _store(v, dtype) for k, v in tor.items()}
    return dict(x=x, w=w, b=b, r=r, dy=dy, ref=ref, tor=tor, cols=gn_outlier_cols(shape, cond, parts), cond=cond, dtype=dtype)


def gn_constant_bound(case, floor):
    """|y - ref| allowed on a constant group: one rounding of the mean (2^-23 |v|, taken twice) amplified by rstd = eps^-1/2 and
    the largest |gamma|, plus the existing tolerance ``floor`` (absolute)."""
    v = float(case["x"].abs().max())
    return 2 * 2.0 ** -23 * v * GN_EPS ** -0.5 * float(case["w"].abs().max()) + floor


# ------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------
def ln_input(M, C, cond, dtype=F32):
    g = _gen(M, C, LN_CONDITIONS.index(cond), dtype == BF16, 3)
    if cond == "constant":
        return torch.tensor([DYADIC[i % len(DYADIC)] for i in range(M)]).view(M, 1).expand(-1, C).contiguous()
    x = torch.randn(M, C, generator=g) * 2
    if cond == "offset":
        x = x + (1000.0 if dtype == F32 else 16.0)
    if cond == "tiny":
        x = x * 2.0 ** -60
    if cond == "huge":
        x = x * 2.0 ** 50
    x = _store(x, dtype)
    if cond in ("first", "last"):
        place_outliers(x, [0 if cond == "first" else C - 1], LN_SIGMAS, dtype)
    return x


def _ln_run(x, w, b, dy, ds, dt, lin, dz):
    ls = [t.to(dt).clone().requires_grad_(True) for t in (x, w, b) + tuple(lin)]
    h = F.layer_norm(ls[0], (x.shape[-1],), ls[1], ls[2], LN_EPS)
    if lin:
        y = F.linear(h, ls[3], ls[4])
        gs = list(torch.autograd.grad([y, ls[0]], ls, grad_outputs=[dz.to(dt), ds.to(dt)]))
    else:
        y = h
        gs = list(torch.autograd.grad([y, ls[0]], ls, grad_outputs=[dy.to(dt), ds.to(dt)]))
    out = dict(y=y.detach(), dx=gs[0], dgamma=gs[1], dbeta=gs[2])
    if lin:
        out.update(dW=gs[3], db=gs[4])
    return out


@functools.lru_cache(maxsize=None)
def ln_case(M, C, cond, dtype=F32, nout=0):
    """LayerNorm rows with the skip gradient ``ds`` added into dx; ``nout`` > 0: followed by a Linear(C, nout) seeded with dz"""
    x = ln_input(M, C, cond, dtype)
    g = _gen(M, C, 29)
    w = _store(1 + 0.2 * torch.randn(C, generator=g), dtype)
    b = _store(0.3 * torch.randn(C, generator=g), dtype)
    dy = _store(torch.randn(M, C, generator=g), dtype)
    ds = _store(torch.randn(M, C, generator=g), dtype)
    lin, dz = (), None
    if nout:
        lin = (torch.randn(nout, C, generator=g) * C ** -0.5, 0.1 * torch.randn(nout, generator=g))
        dz = torch.randn(M, nout, generator=g)
    ref = _ln_run(x, w, b, dy, ds, torch.float64, lin, dz)
    tor = {k: _store(v, dtype) for k, v in _ln_run(x, w, b, dy, ds, F32, lin, dz).items()}
    cols = [0] if cond == "first" else [C - 1] if cond == "last" else []
    return dict(x=x, w=w, b=b, dy=dy, ds=ds, lin=lin, dz=dz, ref=ref, tor=tor, cols=cols, cond=cond, dtype=dtype)


def ln_constant_bound(case, floor):
    return 2 * 2.0 ** -23 * float(case["x"].abs().max()) * LN_EPS ** -0.5 * float(case["w"].abs().max()) + floor


# ------------------------------------------------------------------------------------------------
# weight standardisation: one condition per output channel, by channel index modulo 3; the last channel is a constant filter
# ------------------------------------------------------------------------------------------------
WS_SHAPES = ((64, 3, 7, 7), (64, 64, 1, 1), (33, 5, 1, 1))
WS_CONDITIONS = ("far_mean", "outlier", "plain")
WS_SEED = 0


def ws_input(shape, dtype=F32):
    """channels 0, 3, 6, ...: 0.5 + 1e-3 randn, a mean far above the std (bf16, whose spacing at 0.5 is 2e-3: 0.5 + 2^-6 randn;
    filters of fewer than 16 weights: 0.5 + 8e-3 randn -- the std of five samples falls to a third of the nominal one by chance,
    and at 1e-3 torch's own fp32 error, the spacing at 0.5 over that std, then breaks the cap: 6e-5 to 2e-4 by seed);
    1, 4, 7, ...: 0.3 randn with weight 0 at 100 sigma; 2, 5, 8, ...: 0.3 randn + 0.05; the last channel: one dyadic constant"""
    cout, n = shape[0], shape[1] * shape[2] * shape[3]
    g = _gen(cout, n, dtype == BF16, 41 + WS_SEED)
    w = torch.randn(cout, n, generator=g)
    w[0::3] = 0.5 + (2.0 ** -6 if dtype == BF16 else 1e-3 if n >= 16 else 8e-3) * w[0::3]
    w[1::3] = 0.3 * w[1::3]
    w[2::3] = 0.3 * w[2::3] + 0.05
    w = _store(w, dtype)
    w[1::3] = place_outliers(w[1::3].clone(), [0], WS_SIGMAS, dtype)
    w[cout - 1] = 0.375
    return w.reshape(shape).contiguous()


def ws_expr(w, eps=WS_EPS):
    """the expression kernel_checks.verify_weight_std holds the kernel to (std_conv.py:56-59)"""
    std, mean = torch.std_mean(w, dim=[1, 2, 3], keepdim=True, unbiased=False)
    return (w - mean) / (std + eps)


@functools.lru_cache(maxsize=None)
def ws_case(cond, dtype=F32):
    """all of WS_SHAPES (one launch), judged on the channels of ``cond`` (``keep``: their indices per weight, never the constant
    filter, whose float64 gradient is NaN: d std / d w at std = 0) so that a tolerance of the maximum is set by those channels
    alone.  torch's result in bf16 storage is the fp32 expression on the bf16 values, rounded to bf16 -- the composite run in
    bf16 rounds (w - mean) itself and says nothing about a kernel."""
    ws = [ws_input(s, dtype) for s in WS_SHAPES]
    g = _gen(53, dtype == BF16)
    gs = [_store(torch.randn(s, generator=g), dtype) for s in WS_SHAPES]
    j = WS_CONDITIONS.index(cond)
    out = dict(ws=ws, gs=gs, keep=[torch.arange(j, s[0] - 1, 3) for s in WS_SHAPES], dtype=dtype, cond=cond)
    for name, dt in (("ref", torch.float64), ("tor", torch.float32)):
        res = {}
        for i, (w, gr, k) in enumerate(zip(ws, gs, out["keep"])):
            wl = w.to(dt).clone().requires_grad_(True)
            o = ws_expr(wl)
            (dw,) = torch.autograd.grad(o[k], wl, grad_outputs=gr.to(dt)[k])
            res["w_hat[%d]" % i], res["dw[%d]" % i] = o.detach()[k], dw[k]
        out[name] = res if dt == torch.float64 else {k: _store(v, dtype) for k, v in res.items()}
    return out


# ------------------------------------------------------------------------------------------------
# the tolerance rule
# ------------------------------------------------------------------------------------------------
def gn_base(case, forward_only=False):
    """the existing TOL entries of kernel_checks.verify_groupnorm per quantity"""
    t = dict(KC.TOL["groupnorm"][case["dtype"]])
    if forward_only:                                         # the split small launches: of max(1, max|y|)
        t["y"] = dict(atol=KC.TOL["groupnorm_forward_only"] * max(1.0, float(case["ref"]["y"].abs().max())))
    return t


def ln_base(case):
    """... of verify_layernorm (bf16 d(gamma), d(beta): the absolute part cut so that the bound stays below dparam_of_max)"""
    t = KC.TOL["layernorm"][case["dtype"]]
    out = dict(y=t["y"], dx=t["dx"])
    for q in ("dgamma", "dbeta"):
        out[q] = dict(t["dparam"])
        if "dparam_of_max" in t:
            out[q]["atol"] = min(out[q]["atol"], (t["dparam_of_max"] - out[q]["tol"]) * float(case["ref"][q].abs().max()))
    return out


def ln_image_base(case):
    return {k: KC.TOL["ln_image"]["linear"] for k in case["ref"]}


def ws_base(case):
    t = KC.TOL["weight_std"][case["dtype"]]
    return {"%s[%d]" % (k, i): t[k] for k in ("w_hat", "dw") for i in range(len(WS_SHAPES))}


def floor_of(entry, ref):
    """the absolute bound a TOL entry gives on ``ref``"""
    return entry.get("atol", 0.0) + entry.get("tol", 0.0) * float(ref.abs().max())


def rule(case, base, only=None, tol_only=()):
    """name -> dict(atol=bound) by the module's rule for every quantity of ``case``; ``base``: name -> the existing TOL entry
    (keywords of Cmp.check).  Asserts the cap on torch's own error.  Also returns torch's errors: (tols, torch_errors).
    ``tol_only``: quantities for which torch's result is no comparator (its error is above the cap at some of the shapes): they are held to the TOL
    entry alone, the smaller bound."""
    tols, terrs = {}, {}
    for name, ref in case["ref"].items():
        if only is not None and name not in only:
            continue
        ref = ref.double()
        assert torch.isfinite(ref).all(), name
        scale = float(ref.abs().max())
        terr = float((case["tor"][name].double() - ref).abs().max())
        t = base[name]
        assert not t.get("rtol"), "the rule is stated for tolerances of the maximum"
        floor = t.get("atol", 0.0) + t.get("tol", 0.0) * scale
        cap = CAP * scale if case["dtype"] == F32 else floor
        if name in tol_only:
            tols[name], terrs[name] = dict(atol=floor), terr
            continue
        assert terr <= cap, "%s: torch's own error %.3e is above the cap %.3e (max|ref| %.3e): change the case" % (name, terr, cap, scale)
        tols[name], terrs[name] = dict(atol=max(2.0 * terr, floor)), terr
    return tols, terrs


# ------------------------------------------------------------------------------------------------
# the one-pass statistics the fp32 GroupNorm forward used before its variance was made robust, restated in fp32 numpy: the shift
# is the group's first element, 1024 lanes sum (x - x0) and (x - x0)^2 sequentially over elements lane, lane + 1024, ..., a
# pairwise tree adds the lanes, and rstd = rsqrt(max(m2 - m1^2, 0) + eps).  Kept as a property of the cases: they must tell this
# from an accurate kernel.
# ------------------------------------------------------------------------------------------------
def shifted_one_pass_gn(x, w, b, eps=GN_EPS, lanes=1024):
    import numpy as np
    N, C, H, W = x.shape
    cg, n = C // 32, (C // 32) * H * W
    xs = x.numpy().reshape(N * 32, n)
    x0 = xs[:, :1]
    pad = (-n) % lanes
    d = np.concatenate([xs - x0, np.zeros((N * 32, pad), np.float32)], 1).reshape(N * 32, -1, lanes)
    s1, s2 = np.zeros((N * 32, lanes), np.float32), np.zeros((N * 32, lanes), np.float32)
    for i in range(d.shape[1]):
        s1 = s1 + d[:, i]
        s2 = s2 + d[:, i] * d[:, i]
    while s1.shape[1] > 1:
        h = s1.shape[1] // 2
        s1, s2 = s1[:, :h] + s1[:, h:], s2[:, :h] + s2[:, h:]
    inv = np.float32(1.0 / n)
    m1, m2 = s1 * inv, s2 * inv
    mean = x0 + m1
    rstd = np.float32(1) / np.sqrt(np.maximum(m2 - m1 * m1, np.float32(0)) + np.float32(eps))
    ga = w.numpy().reshape(1, 32, cg, 1) * rstd.reshape(N, 32, 1, 1)
    be = b.numpy().reshape(1, 32, cg, 1) - mean.reshape(N, 32, 1, 1) * ga
    y = xs.reshape(N, 32, cg, H * W) * ga + be
    return torch.from_numpy(y.astype(np.float32).reshape(N, C, H, W))


# ------------------------------------------------------------------------------------------------
# the cases both test files run
# ------------------------------------------------------------------------------------------------
ALL_GN = tuple(c for c in GN_CONDITIONS if c != "part_first" and c not in GN_FIRST_SIGMAS)
NEAR = tuple(GN_FIRST_SIGMAS)
# shape -> (kernel family forward, backward by variant_rules.gnf_*_variant, conditions); the parts shape runs without gradients
GN_F32_SHAPES = {
    (1, 256, 28, 28): (("reg", 256, 8), ("reg", 256, 8), ALL_GN + NEAR),
    (1, 128, 112, 112): (("reg", 1024, 13), ("reg", 1024, 13), ("first", "offset")),
    (1, 256, 112, 112): (("reg", 1024, 25), ("streamed", 1024), ("first", "offset") + NEAR),
    (1, 256, 128, 128): (("streamed", 1024), ("streamed", 1024), ALL_GN),
    (2, 256, 48, 48): (("parts", 4), None, ("first", "offset", "part_first")),
    (2, 64, 8, 8): (("reg", 256, 8), ("reg", 256, 8), ("first", "offset")),
}
GN_BF16_SHAPES = {(2, 64, 8, 8): ("offset", "first", "constant"), (1, 256, 28, 28): ("offset", "first", "constant")}
ACTS = ("none", "relu", "add_relu")
LN_WIDTHS = (256, 768, 1024)
LN_ROWS = 8
LN_IMAGE = (64, 512, 96)                                     # rows, C, the Linear's outputs
LN_IMAGE_CONDITIONS = ("offset", "first", "last")


def gn_parts(shape):
    """(P, vper) of the small-launch forward at ``shape``"""
    import variant_rules as VR
    N, C, H, W = shape
    P = VR.gnf_fwd_parts(N, C, H * W)
    return P, -(-((C // 32) * H * W // 4) // P)


def gn_tol_only(cond, dtype=F32):
    """fp32 GroupNorm on offset data: torch's CPU backward forms d(gamma) as (sum dy x - mean sum dy) rstd, a difference of two
    sums 600 times its size at offset 1000 -- its error there is 1e-4 to 7e-4 of the maximum (first_offset, offset 100: up to
    8e-5), above the cap.  d(gamma) of these conditions is held to the TOL entry alone."""
    return ("dgamma",) if dtype == F32 and cond in ("offset", "first_offset") else ()


def gn_f32_cases():
    """(shape, condition) of every fp32 GroupNorm case"""
    return [(s, c) for s, (_, _, conds) in GN_F32_SHAPES.items() for c in conds]
