"""The ten bf16-storage decoder entry points (acr_bn2d_*_bf16, acr_relu_*_bf16, acr_upsample2x_*_bf16) through the C ABI.

Yardstick: the fp32 entry point of the same name on the exact fp32 upcasts of the same bf16 inputs (include/acr_hip.h defines a
bf16 output as that result rounded to nearest even).  tests/decoder_bf16_checks.py states the acceptance rule; this file does not
know whether the kernels kept the fp32 kernels' summation order: bf16 outputs may use the midpoint window (capped), doubles are held
to the reordering bound of their sums computed from the inputs, floats to 1 ulp, and the number of bit-equal values is printed.
Seeds: for every case the first seed is taken at which the float64 restatement (tests/decoder_ref.py) puts at most CAP of the
elements of each bf16 output into the window; the share is printed.
Every case runs twice (bit-identical) and every output lies between two guard bands of a sentinel pattern that must survive."""
import functools

import numpy as np
import pytest
import torch

import decoder_bf16_checks as K
import decoder_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
MOMENTUM, EPS = 0.1, 1e-5
GUARD = 64                      # elements on either side: a multiple of 16 bytes for every dtype, so the view stays 16-byte aligned
SENTINEL = 0xA5
U = 2.0 ** -53
# (N, C, H*W): the legal minimum n = 2; odd, no vector body, every plane misaligned; exactly one 4-value vector per plane, and two;
# head + body + tail with planes at odd offsets; two slabs per channel whose boundary falls inside a row (n = 1401 > 1024)
BN_SHAPES = [(2, 1, 1), (1, 3, 7), (2, 5, 4), (2, 5, 8), (2, 3, 35), (3, 2, 467)]


def bf16_values(rng, shape, mean=0.0, scale=1.0):
    """random values that are exactly representable in bf16, as float32 numpy"""
    a = (mean + scale * rng.standard_normal(shape)).astype(np.float32)
    return K.bf16_to_f32(K.bf16_rne(a)).reshape(shape)


def guarded(shape, dtype):
    full = torch.empty(int(np.prod(shape)) + 2 * GUARD, dtype=dtype, device=DEV)
    full.view(torch.uint8).fill_(SENTINEL)
    return full, full[GUARD:GUARD + int(np.prod(shape))].view(shape)


def guards_intact(full):
    b = full.view(torch.uint8)
    g = GUARD * full.element_size()
    return bool((b[:g] == SENTINEL).all()) and bool((b[-g:] == SENTINEL).all())


def host(t):
    """numpy of a device tensor; bf16 as its uint16 bit patterns"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16).copy() if t.dtype == torch.bfloat16 else t.numpy().copy()


class Call:
    """one storage type's view of the library: ``fn(name)`` the entry point, ``dev(a)`` an input on the device, ``out(shape)`` a
    guarded output"""
    def __init__(self, store):
        from acr_wsss_amd import _lib as L
        self.L, self.lib, self.store = L, L.load(), store
        self.dtype = torch.bfloat16 if store == "bf16" else torch.float32
        self.fulls = []

    def fn(self, name):
        if self.store == "bf16":
            name = (name[:-4] if name.endswith("_f32") else name) + "_bf16"
        return getattr(self.lib, name)

    def dev(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(self.dtype)

    def out(self, shape, dtype=None, init=None):
        full, view = guarded(shape, dtype or self.dtype)
        self.fulls.append(full)
        if init is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(DEV))
        return view

    def ws(self, n, c, hw):
        nbytes = self.lib.acr_bn2d_ws_bytes(n, c, hw)
        assert nbytes > 0
        return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes

    def intact(self):
        torch.cuda.synchronize()
        return all(guards_intact(f) for f in self.fulls)


def check_outputs(where, got, ref, bounds):
    """got / ref: name -> numpy (uint16 = bf16 bits in ``got``, then ``ref`` holds the fp32 yardstick); bounds: name -> bound of a
    double output.  Applies the rule of the module docstring and prints the count of bit-equal values."""
    bad, line = [], []
    for name, g in got.items():
        r = ref[name]
        if g.dtype == np.uint16:
            res = K.accept_bf16(g, r, name)
            line.append("%s %d/%d exact, %d in the window" % (name, res["exact"], res["size"], res["exempt"]))
        elif g.dtype == np.float64:
            res = K.close_f64(g, r, bounds[name])
            line.append("%s %d/%d bit-equal" % (name, res["equal"], res["size"]))
        else:
            res = K.close_f32(g, r)
            line.append("%s %d/%d bit-equal" % (name, res["equal"], res["size"]))
        if not res["ok"]:
            bad.append((name, res))
    print("%s: %s" % (where, "; ".join(line)))
    assert not bad, (where, bad)


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s differs between two runs" % k


# ------------------------------------------------------------------------------------------------
# BatchNorm2d, fused
# ------------------------------------------------------------------------------------------------
def bn_inputs(shape, nres, seed, first=0.0):
    """``first`` > 0: every channel's first value, the shift of the kernel's sums, lies at least that many standard deviations
    above the mean of the channel's other values"""
    n, c, hw = shape
    rng = np.random.default_rng(1000 * seed + 31 * n + 7 * c + hw + nres)
    full = (n, c, hw, 1)
    x = bf16_values(rng, full, 0.5)
    if first:
        rest = x.astype(np.float64).transpose(1, 0, 2, 3).reshape(c, -1)[:, 1:]
        v = (rest.mean(1) + first * rest.std(1)).astype(np.float32)
        x[0, :, 0, 0] = K.bf16_to_f32(K.bf16_rne(v * np.float32(1 + 2.0 ** -7)))       # rounding to bf16 moves a value by at most 2^-8 of it
        assert ((x[0, :, 0, 0] - rest.mean(1)) / rest.std(1)).min() >= first
    return dict(x=x, dy=bf16_values(rng, full), res=[bf16_values(rng, full) for _ in range(nres)],
                gamma=bf16_values(rng, c, 1.0, 0.1), beta=bf16_values(rng, c, 0.0, 0.1),
                rm=(0.2 * rng.standard_normal(c)).astype(np.float32), rv=(0.5 + rng.random(c)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def bn_case(shape, relu, nres, training, first=0.0):
    """the inputs at the first seed whose restatement keeps the window share of y and dx under the cap, and the bounds of the
    double outputs from those inputs; treat as read-only"""
    for seed in range(64):
        c = bn_inputs(shape, nres, seed, first)
        f = R.bn_fwd(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], training, MOMENTUM, EPS, relu, *(c["res"] + [None, None])[:2])
        dx, dgamma, dbeta, g = R.bn_bwd(c["x"], c["gamma"], f["mean"], f["invstd"], c["dy"], training, mask=(f["pre"] > 0) if relu else None)
        shares = (K.window_share(f["y"]), K.window_share(dx))
        if max(shares) <= K.CAP:
            break
    else:
        raise AssertionError("no seed keeps the window share under the cap for %s" % (shape,))
    n = shape[0] * shape[2]
    x = c["x"].astype(np.float64)
    d = np.abs(x - x[0:1, :, 0:1]).sum(axis=(0, 2, 3))                       # sum |x - shift| per channel
    d2 = ((x - x[0:1, :, 0:1]) ** 2).sum(axis=(0, 2, 3))
    b_a, b_b = U * n * d, U * n * d2                                            # reordering bounds of the two slab sums
    b_mean = b_a / n + 2 * U * np.abs(f["mean"])
    b_var = (b_b + 2 * d / n * b_a) / n + 4 * U * (d2 / n)                      # var = (b - a^2 / n) / n
    b_inv = 0.5 * f["invstd"] ** 3 * b_var + 4 * U * f["invstd"]
    # eval mode: stats are the running statistics and 1 / sqrt(running_var + eps), no sum in them; dgamma / dbeta are floats (1 ulp)
    bounds = dict(stats=np.stack([b_mean, b_inv], 1).reshape(-1) if training else 0.0)
    c.update(seed=seed, shares=shares, bounds=bounds)
    return c


def run_bn(store, case, shape, relu, training):
    n, c, hw = shape
    k = Call(store)
    L = k.L
    x, dy, gamma, beta = k.dev(case["x"]), k.dev(case["dy"]), k.dev(case["gamma"]), k.dev(case["beta"])
    res = [k.dev(r) for r in case["res"]] + [None, None]
    rm, rv = k.out((c,), torch.float32, case["rm"]), k.out((c,), torch.float32, case["rv"])
    stats, y = k.out((c, 2), torch.float64), k.out(case["x"].shape)
    ws, nbytes = k.ws(n, c, hw)
    rc = k.fn("acr_bn2d_fwd")(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(res[0]), L.ptr(res[1]), n, c, hw,
                              1 if training else 0, EPS, MOMENTUM, 1 if relu else 0, L.ptr(ws), nbytes, L.ptr(stats), L.ptr(y), L.stream_ptr())
    assert rc == 0, L.load().acr_last_error()
    dx, dgamma, dbeta = k.out(case["x"].shape), k.out((c,), torch.float32), k.out((c,), torch.float32)
    dres = k.out(case["x"].shape) if relu else None
    rc = k.fn("acr_bn2d_bwd")(L.ptr(x), L.ptr(y), L.ptr(dy), L.ptr(gamma), L.ptr(stats), n, c, hw, 1 if training else 0, 1 if relu else 0,
                              L.ptr(ws), nbytes, L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dres), L.stream_ptr())
    assert rc == 0, L.load().acr_last_error()
    assert k.intact(), "a guard band was written (%s)" % store
    out = dict(y=host(y), stats=host(stats), running_mean=host(rm), running_var=host(rv), dx=host(dx), dgamma=host(dgamma), dbeta=host(dbeta))
    if relu:
        out["dres"] = host(dres)
    return out


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("nres", [0, 1, 2])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn2d_bf16_is_the_rounded_fp32_entry_point(shape, relu, nres, training):
    case = bn_case(shape, relu, nres, training)
    print("\nbn %s relu%d res%d train%d: seed %d, window share of y %.1e, dx %.1e (restatement)"
          % (shape, relu, nres, training, case["seed"], case["shares"][0], case["shares"][1]))
    ref = run_bn("f32", case, shape, relu, training)
    got = run_bn("bf16", case, shape, relu, training)
    same_bits(got, run_bn("bf16", case, shape, relu, training))
    b = case["bounds"]
    check_outputs("bn %s" % (shape,), got, ref, dict(stats=b["stats"]))
    if not training:                                         # nothing is updated in eval mode
        assert np.array_equal(got["running_mean"], case["rm"]) and np.array_equal(got["running_var"], case["rv"])


@pytest.mark.parametrize("relu,nres", [(False, 0), (True, 2)])
@pytest.mark.parametrize("shape", [(2, 5, 8), (3, 2, 467)], ids=lambda s: "x".join(map(str, s)))
def test_bn2d_bf16_first_value_outlier(shape, relu, nres):
    """Every channel's first value -- the shift of the kernel's (double) sums -- at 100 standard deviations, by the rule above."""
    case = bn_case(shape, relu, nres, True, 100.0)
    print("\nbn %s relu%d res%d, first value at 100 sigma: seed %d, window share of y %.1e, dx %.1e (restatement)"
          % (shape, relu, nres, case["seed"], case["shares"][0], case["shares"][1]))
    ref = run_bn("f32", case, shape, relu, True)
    got = run_bn("bf16", case, shape, relu, True)
    same_bits(got, run_bn("bf16", case, shape, relu, True))
    check_outputs("bn %s first value at 100 sigma" % (shape,), got, ref, dict(stats=case["bounds"]["stats"]))


def test_bn2d_bf16_refuses_one_value_per_channel():
    from acr_wsss_amd import _abi
    k = Call("bf16")
    L = k.L
    x = torch.zeros(1, 3, 1, 1, device=DEV, dtype=torch.bfloat16)
    g = torch.ones(3, device=DEV, dtype=torch.bfloat16)
    rm, rv = torch.zeros(3, device=DEV), torch.ones(3, device=DEV)
    stats, y = torch.empty(3, 2, dtype=torch.float64, device=DEV), torch.empty_like(x)
    ws, nbytes = k.ws(1, 3, 1)
    rc = k.fn("acr_bn2d_fwd")(L.ptr(x), L.ptr(g), L.ptr(g), L.ptr(rm), L.ptr(rv), None, None, 1, 3, 1, 1, EPS, MOMENTUM, 0, L.ptr(ws), nbytes,
                              L.ptr(stats), L.ptr(y), L.stream_ptr())
    assert rc == _abi.constants["ACR_ERR_INVALID"]
    gathered = torch.tensor([[1.0, 0.0, 0.0]] * 3, dtype=torch.float64, device=DEV)
    stats3 = torch.empty(9, dtype=torch.float64, device=DEV)
    rc = k.fn("acr_bn2d_fwd_merged")(L.ptr(x), L.ptr(g), L.ptr(g), L.ptr(rm), L.ptr(rv), None, None, 1, 3, 1, L.ptr(gathered), 1, EPS,
                                     MOMENTUM, 0, L.ptr(ws), nbytes, L.ptr(stats3), L.ptr(y), L.stream_ptr())
    assert rc == _abi.constants["ACR_ERR_INVALID"]           # a merged count below 2


# ------------------------------------------------------------------------------------------------
# BatchNorm2d, cross-rank: two ranks emulated in one process, the gather is a torch.stack
# ------------------------------------------------------------------------------------------------
def run_sync(store, ranks, c, hw, relu):
    """ranks: per rank dict(x, dy, res, ...).  moments -> merge -> fwd_merged, bwd_sums -> merge -> bwd_merged; everything returned"""
    k = Call(store)
    L = k.L
    W = len(ranks)
    st = []
    for r in ranks:
        n = r["x"].shape[0]
        ws, nbytes = k.ws(n, c, hw)
        s = dict(n=n, ws=ws, nbytes=nbytes, x=k.dev(r["x"]), dy=k.dev(r["dy"]), res=[k.dev(a) for a in r["res"]] + [None, None],
                 moments=k.out((c, 3), torch.float64))
        rc = k.fn("acr_bn2d_moments")(L.ptr(s["x"]), n, c, hw, L.ptr(ws), nbytes, L.ptr(s["moments"]), L.stream_ptr())
        assert rc == 0, L.load().acr_last_error()
        st.append(s)
    gathered = torch.stack([s["moments"] for s in st]).contiguous()
    gamma, beta = k.dev(ranks[0]["gamma"]), k.dev(ranks[0]["beta"])
    for s in st:
        s["rm"], s["rv"] = k.out((c,), torch.float32, ranks[0]["rm"]), k.out((c,), torch.float32, ranks[0]["rv"])
        s["stats"], s["y"] = k.out((3 * c,), torch.float64), k.out((s["n"], c, hw, 1))
        rc = k.fn("acr_bn2d_fwd_merged")(L.ptr(s["x"]), L.ptr(gamma), L.ptr(beta), L.ptr(s["rm"]), L.ptr(s["rv"]), L.ptr(s["res"][0]),
                                         L.ptr(s["res"][1]), s["n"], c, hw, L.ptr(gathered), W, EPS, MOMENTUM, 1 if relu else 0, L.ptr(s["ws"]),
                                         s["nbytes"], L.ptr(s["stats"]), L.ptr(s["y"]), L.stream_ptr())
        assert rc == 0, L.load().acr_last_error()
    for s in st:
        s["sums"], s["dgamma"], s["dbeta"] = k.out((c, 2), torch.float64), k.out((c,), torch.float32), k.out((c,), torch.float32)
        rc = k.fn("acr_bn2d_bwd_sums")(L.ptr(s["x"]), L.ptr(s["y"]), L.ptr(s["dy"]), L.ptr(s["stats"]), s["n"], c, hw, 1 if relu else 0,
                                       L.ptr(s["ws"]), s["nbytes"], L.ptr(s["sums"]), L.ptr(s["dgamma"]), L.ptr(s["dbeta"]), L.stream_ptr())
        assert rc == 0, L.load().acr_last_error()
    gsums = torch.stack([s["sums"] for s in st]).contiguous()
    out = {}
    for i, s in enumerate(st):
        s["dx"] = k.out((s["n"], c, hw, 1))
        s["dres"] = k.out((s["n"], c, hw, 1)) if relu else None
        rc = k.fn("acr_bn2d_bwd_merged")(L.ptr(s["x"]), L.ptr(s["y"]), L.ptr(s["dy"]), L.ptr(gamma), L.ptr(s["stats"]), L.ptr(gsums), W, s["n"],
                                         c, hw, 1 if relu else 0, L.ptr(s["ws"]), s["nbytes"], L.ptr(s["dx"]), L.ptr(s["dres"]), L.stream_ptr())
        assert rc == 0, L.load().acr_last_error()
        for name in ("moments", "stats", "y", "rm", "rv", "sums", "dgamma", "dbeta", "dx") + (("dres",) if relu else ()):
            out["%s%d" % (name, i)] = host(s[name])
    assert k.intact(), "a guard band was written (%s)" % store
    return out


@pytest.mark.parametrize("relu,nres", [(False, 0), (True, 2)])
@pytest.mark.parametrize("hw", [6, 35])
def test_cross_rank_chain_bf16_follows_the_fp32_chain(hw, relu, nres):
    c, sizes = 3, (1, 2)
    for seed in range(64):
        whole = bn_inputs((sum(sizes), c, hw), nres, 50 + seed)
        f = R.bn_fwd(whole["x"], whole["gamma"], whole["beta"], whole["rm"], whole["rv"], True, MOMENTUM, EPS, relu, *(whole["res"] + [None, None])[:2])
        dx, _, _, g = R.bn_bwd(whole["x"], whole["gamma"], f["mean"], f["invstd"], whole["dy"], True, mask=(f["pre"] > 0) if relu else None)
        shares = (K.window_share(f["y"]), K.window_share(dx))
        if max(shares) <= K.CAP:
            break
    print("\nsync hw=%d relu%d: seed %d, window share of y %.1e, dx %.1e (restatement)" % (hw, relu, 50 + seed, shares[0], shares[1]))
    ranks, at = [], 0
    for n in sizes:
        ranks.append(dict(whole, x=whole["x"][at:at + n], dy=whole["dy"][at:at + n], res=[r[at:at + n] for r in whole["res"]]))
        at += n
    ref = run_sync("f32", ranks, c, hw, relu)
    got = run_sync("bf16", ranks, c, hw, relu)
    same_bits(got, run_sync("bf16", ranks, c, hw, relu))
    # bounds of the doubles from the inputs: every one is a sum over at most n values of the whole batch (or derived from two)
    n = sum(sizes) * hw
    x = whole["x"].astype(np.float64)
    spread = np.abs(x - x.mean(axis=(0, 2, 3), keepdims=True)).sum(axis=(0, 2, 3)) + n * np.abs(x).max()
    sq = (x ** 2).sum(axis=(0, 2, 3)) * 4
    b_mean = U * n * spread + 2 * U * np.abs(f["mean"])
    b_m2 = U * n * sq * 4
    b_inv = 0.5 * f["invstd"] ** 3 * b_m2 / n + 4 * U * f["invstd"]
    xhat = (x - f["mean"][None, :, None, None]) * f["invstd"][None, :, None, None]
    b_sums = np.stack([U * n * np.abs(g).sum(axis=(0, 2, 3)), U * n * np.abs(g * xhat).sum(axis=(0, 2, 3)) * 2], 1).reshape(-1)
    bounds = {}
    for i in range(len(sizes)):
        bounds["moments%d" % i] = np.stack([np.zeros(c), b_mean, b_m2], 1).reshape(-1)
        bounds["stats%d" % i] = np.concatenate([np.stack([b_mean, b_inv], 1).reshape(-1), np.zeros(c)])
        bounds["sums%d" % i] = b_sums
    check_outputs("sync hw=%d" % hw, got, ref, bounds)


# ------------------------------------------------------------------------------------------------
# ReLU
# ------------------------------------------------------------------------------------------------
def run_relu(store, x, dy):
    k = Call(store)
    L = k.L
    n = x.size
    xd, gd = k.dev(x), k.dev(dy)
    y, dx = k.out((n,)), k.out((n,))
    assert k.fn("acr_relu_fwd_f32")(L.ptr(xd), n, L.ptr(y), L.stream_ptr()) == 0
    assert k.fn("acr_relu_bwd_f32")(L.ptr(y), L.ptr(gd), n, L.ptr(dx), L.stream_ptr()) == 0
    assert k.intact(), "a guard band was written (%s)" % store
    return dict(y=host(y), dx=host(dx))


@pytest.mark.parametrize("n", [1, 7, 8, 8 * 256 + 5])
def test_relu_bf16(n):
    rng = np.random.default_rng(n)
    x, dy = bf16_values(rng, n), bf16_values(rng, n)
    x[::5] = 0.0
    ref, got = run_relu("f32", x, dy), run_relu("bf16", x, dy)
    same_bits(got, run_relu("bf16", x, dy))
    check_outputs("relu n=%d" % n, got, ref, {})
    assert np.array_equal(K.bf16_to_f32(got["y"]), np.maximum(x, 0)) and np.array_equal(K.bf16_to_f32(got["dx"]), np.where(x > 0, dy, 0))


# ------------------------------------------------------------------------------------------------
# x2 upsampling
# ------------------------------------------------------------------------------------------------
def run_up(store, x, dy):
    k = Call(store)
    L = k.L
    p, h, w = x.shape
    xd, gd = k.dev(x), k.dev(dy)
    y, dx = k.out((p, 2 * h, 2 * w)), k.out((p, h, w))
    assert k.fn("acr_upsample2x_fwd")(L.ptr(xd), p, h, w, 2 * h, 2 * w, L.ptr(y), L.stream_ptr()) == 0
    assert k.fn("acr_upsample2x_bwd")(L.ptr(gd), p, h, w, 2 * h, 2 * w, L.ptr(dx), L.stream_ptr()) == 0
    assert k.intact(), "a guard band was written (%s)" % store
    return dict(y=host(y), dx=host(dx))


@pytest.mark.parametrize("shape", [(3, 1, 1), (2, 1, 5), (2, 4, 3), (1, 5, 8), (2, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_upsample2x_bf16(shape):
    p, h, w = shape
    for seed in range(64):
        rng = np.random.default_rng(100 * seed + p + 3 * h + 5 * w)
        x, dy = bf16_values(rng, shape), bf16_values(rng, (p, 2 * h, 2 * w))
        shares = (K.window_share(R.upsample2x(x[None])), K.window_share(R.upsample2x_bwd(dy[None])))
        if max(shares) <= K.CAP:
            break
    print("\nupsample %s: seed %d, window share of y %.1e, dx %.1e (restatement)" % (shape, seed, shares[0], shares[1]))
    ref, got = run_up("f32", x, dy), run_up("bf16", x, dy)
    same_bits(got, run_up("bf16", x, dy))
    check_outputs("upsample %s" % (shape,), got, ref, {})


def test_upsample2x_bf16_refuses_other_ratios():
    from acr_wsss_amd import _abi
    k = Call("bf16")
    L = k.L
    x, y = torch.zeros(1, 4, 4, device=DEV, dtype=torch.bfloat16), torch.zeros(1, 12, 8, device=DEV, dtype=torch.bfloat16)
    assert k.fn("acr_upsample2x_fwd")(L.ptr(x), 1, 4, 4, 12, 8, L.ptr(y), L.stream_ptr()) == _abi.constants["ACR_ERR_UNSUPPORTED"]
    assert k.fn("acr_upsample2x_bwd")(L.ptr(y), 1, 4, 4, 12, 8, L.ptr(x), L.stream_ptr()) == _abi.constants["ACR_ERR_UNSUPPORTED"]
