"""Launch census: which public ``ops`` entries a real model run calls, at which shapes, and an fp64 checker for each.

``Census.install(monkeypatch)`` wraps every entry in ``ENTRIES`` (the backbone, the heads, CAM generation and the loss look them up
on the module at call time).  A wrapper records metadata only -- the entry, each tensor's shape / dtype / requires_grad, the
scalar arguments, whether an operand image came along, the path flags of ``ops`` in force and the grad mode -- and calls the
entry.  No clone, no sync.  Identical records merge, so ``census.records`` is the set of distinct launches.

``CHECKERS[name](record, cmp)`` rebuilds seeded inputs at exactly the recorded shapes (batch included, so the K-split / slab
choices are those of the real launch), runs the entry down the same path (same ``math``, same operand images, same grad mode)
and compares the output and every input / weight gradient with float64 torch math through ``cmp``.  Each tolerance is the one
of the hand-written kernel test for that kernel (tests/test_kernels_gpu.py, tests/test_fp16x2_gpu.py), never looser.  ``cmp``
also proves every comparison can fail: one element of the kernel's output moved by 4x the tolerance must be rejected.
"""
import inspect
import sys
import zlib
from collections import Counter, namedtuple

import torch
import torch.nn.functional as F

from acr_wsss_amd import ops

ENTRIES = (
    "conv1x1", "conv1x1_skip", "conv3x3", "conv_s2", "subsample2", "maxpool3x3s2_same", "groupnorm_act", "weight_std_all", "tokens",
    "layer_norm_skip", "layer_norm_image", "linear_or_hip", "mlp", "mlp_f32",
    "attention_core", "attention_core_oimg", "attn_probs", "attn_dprobs",
    "getam_row_accum", "getam_rows_accum", "patch_cam", "bilinear_resize", "aff_refine_batch",
    "consistency", "mlsm_loss",
)
PATH_FLAGS = ("CONV3X3_WIMG", "GN_RELU_MASK", "X3_IMAGES", "ATTN_F32_SCORES")

# ops.<name>( calls of the model that are not kernel launches of their own: dispatch predicates, plans, buffers / caches and the
# image builders whose images the recorded entries consume (and that the checkers rebuild)
NOT_LAUNCHES = {
    "_f32_ok": "predicate",
    "conv_s2_plan": "tap-table plan (host side)",
    "MeanStack": "owner of the head-mean buffer the attention launches write",
    "WeightTransposes": "cache of W^T copies, refreshed after the optimizer step",
    "x3_image_many": "image builder: the weight images that conv1x1 / conv3x3 / conv_s2 consume",
    "prebuild_weight_images": "image builder: the block Linears' weight images, refreshed after the optimizer step",
    "invalidate_weight_images": "drops cached weight images (host side)",
}


def is_not_a_launch(name):
    return name in NOT_LAUNCHES or name.endswith("_fusable") or name.endswith("_usable")


T = namedtuple("T", "shape dtype requires_grad expanded")          # a tensor argument
Lin = namedtuple("Lin", "out_features in_features bias requires_grad")
LN = namedtuple("LN", "C eps requires_grad")
Stack = namedtuple("Stack", "shape")
Mod = namedtuple("Mod", "cls training")
Record = namedtuple("Record", "name args flags grad")


def _desc(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if torch.is_tensor(v):
        expanded = v.numel() > 1 and 0 in v.stride()
        return T(tuple(v.shape), str(v.dtype).replace("torch.", ""), bool(v.requires_grad), expanded)
    if isinstance(v, torch.nn.Linear):
        return Lin(v.out_features, v.in_features, v.bias is not None, bool(v.weight.requires_grad))
    if isinstance(v, torch.nn.LayerNorm):
        return LN(v.normalized_shape[0], v.eps, bool(v.weight.requires_grad))
    if isinstance(v, ops.MeanStack):
        return Stack(tuple(v.buf.shape))
    if isinstance(v, torch.nn.Module):
        return Mod(type(v).__name__, bool(v.training))
    if isinstance(v, (list, tuple)):
        return tuple(_desc(u) for u in v)
    raise TypeError("launch census: no descriptor for %r" % type(v))


class Census:
    """Records the distinct launches of the entries in ENTRIES while installed."""

    def __init__(self):
        self.counts = Counter()
        self.originals = {n: getattr(ops, n) for n in ENTRIES}
        self._sigs = {n: inspect.signature(f) for n, f in self.originals.items()}
        self._depth = 0

    @property
    def records(self):
        return list(self.counts)

    @property
    def launches(self):
        return sum(self.counts.values())

    def install(self, monkeypatch):
        for name in ENTRIES:
            monkeypatch.setattr(ops, name, self._wrap(name))

    def _wrap(self, name):
        fn, sig = self.originals[name], self._sigs[name]

        def wrapper(*args, **kwargs):
            if self._depth:                                 # an entry called by an entry: recorded once, as the outer one
                return fn(*args, **kwargs)
            b = sig.bind(*args, **kwargs)
            b.apply_defaults()
            rec = Record(name, tuple((k, _desc(v)) for k, v in b.arguments.items()),
                         tuple((f, getattr(ops, f)) for f in PATH_FLAGS), torch.is_grad_enabled())
            self.counts[rec] += 1
            self._depth += 1
            try:
                return fn(*args, **kwargs)
            finally:
                self._depth -= 1

        return wrapper

    def summary(self):
        by = Counter(r.name for r in self.counts)
        return "%d launches, %d distinct: %s" % (self.launches, len(self.counts), ", ".join("%s %d" % kv for kv in sorted(by.items())))


def fmt(rec):
    """One line per record: the entry and its arguments (tensors as shape/dtype, '+g' = requires grad)."""
    def one(v):
        if isinstance(v, T):
            return "%s%s%s%s" % ("x".join(map(str, v.shape)) or "()", "" if v.dtype == "float32" else ":" + v.dtype,
                                 "+g" if v.requires_grad else "", "~expanded" if v.expanded else "")
        if isinstance(v, Lin):
            return "Linear(%d->%d)" % (v.in_features, v.out_features)
        if isinstance(v, LN):
            return "LayerNorm(%d)" % v.C
        if isinstance(v, Stack):
            return "MeanStack%s" % (v.shape,)
        if isinstance(v, Mod):
            return "%s(%s)" % (v.cls, "train" if v.training else "eval")
        if isinstance(v, tuple):
            return "[%s]" % ", ".join(one(u) for u in v)
        return repr(v)
    args = ", ".join("%s=%s" % (k, one(v)) for k, v in rec.args if v is not None)
    flags = ",".join(f for f, on in rec.flags if not on)
    return "%s(%s)%s%s" % (rec.name, args, "" if rec.grad else " no_grad", " flags-off:" + flags if flags else "")


# ------------------------------------------------------------------------------------------------
# comparison with a proof that it can fail
# ------------------------------------------------------------------------------------------------
class Cmp:
    """Collects failures.  ``check(label, got, want, tol=, rtol=, atol=)`` passes iff |got - want| <= atol + tol * max|want| +
    rtol * |want| everywhere (tol = rtol = atol = 0: bit-equal values), and then asserts that the same comparison rejects ``got``
    with its element at argmax|want| moved by 4x the tolerance there."""

    def __init__(self):
        self.failures = []
        self.compared = 0
        self.where = ""
        self.grad_mode = True

    def fail(self, msg):
        self.failures.append("%s: %s" % (self.where, msg))

    @staticmethod
    def _ratio(got, want, bound):
        d = (got - want).abs()
        if not torch.isfinite(d).all():
            return float("inf")
        if bound is None:
            return float("inf") if bool((d > 0).any()) else 0.0
        return float((d / bound).max())

    def check(self, label, got, want, tol=0.0, rtol=0.0, atol=0.0):
        self.compared += 1
        if got is None or want is None:
            self.fail("%s: missing (%s vs %s)" % (label, got is None, want is None))
            return
        got, want = got.detach().double(), want.detach().double()
        if got.shape != want.shape or want.numel() == 0:
            self.fail("%s: shape %s vs reference %s" % (label, tuple(got.shape), tuple(want.shape)))
            return
        scale = float(want.abs().max())
        if not (scale > 0 or (tol == 0 and rtol == 0 and atol == 0)):
            self.fail("%s: the reference is all zero or not finite (max %r): nothing to compare against" % (label, scale))
            return
        exact = tol == 0 and rtol == 0 and atol == 0
        bound = None if exact else atol + tol * scale + rtol * want.abs()
        r = self._ratio(got, want, bound)
        if not r <= 1.0:
            err = float((got - want).abs().max()) if torch.isfinite(got).all() else float("nan")
            self.fail("%s: max |err| %.3e, %.2fx the tolerance (tol %g, rtol %g, atol %.3e, max|ref| %.3e)"
                      % (label, err, r, tol, rtol, atol, scale))
            return
        # the comparison must be able to fail: move one element by 4x its tolerance
        i = int(want.abs().reshape(-1).argmax())
        bad = got.clone().reshape(-1)
        step = 4 * float(bound.reshape(-1)[i]) if not exact else max(abs(float(want.reshape(-1)[i])), 1.0) * 2.0 ** -20
        bad[i] += step
        if not self._ratio(bad.reshape(want.shape), want, bound) > 1.0:
            self.fail("%s: self-check -- an element moved by 4x the tolerance was NOT rejected" % label)


# ------------------------------------------------------------------------------------------------
# input builders
# ------------------------------------------------------------------------------------------------
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float64": torch.float64}


class Inputs:
    def __init__(self, rec):
        self.rec = rec
        self.a = dict(rec.args)
        self.dev = torch.device("cuda:0")
        self.g = torch.Generator(device=self.dev)
        self.g.manual_seed(zlib.crc32(repr(rec).encode()) & 0x7FFFFFFF)

    def randn(self, shape, scale=1.0, offset=0.0, dtype=torch.float32):
        return (torch.randn(tuple(shape), generator=self.g, device=self.dev) * scale + offset).to(dtype)

    def rand(self, shape):
        return torch.rand(tuple(shape), generator=self.g, device=self.dev)

    def tensor(self, d, scale=1.0, offset=0.0):
        """A fresh tensor like descriptor ``d`` (requires_grad as recorded)."""
        return self.randn(d.shape, scale, offset, DTYPES[d.dtype]).requires_grad_(d.requires_grad)

    def linear(self, d, weight_gain=1.0, bias_scale=1.0):
        lin = torch.nn.Linear(d.in_features, d.out_features, bias=d.bias).to(self.dev)
        with torch.no_grad():
            lin.weight.copy_(self.randn(lin.weight.shape, weight_gain * d.in_features ** -0.5))
            if d.bias:
                lin.bias.copy_(self.randn(lin.bias.shape, bias_scale))
        lin.requires_grad_(d.requires_grad)
        return lin

    def layernorm(self, d):
        ln = torch.nn.LayerNorm(d.C, eps=d.eps).to(self.dev)
        with torch.no_grad():
            ln.weight.copy_(self.randn((d.C,), 0.2, 1.0))
            ln.bias.copy_(self.randn((d.C,), 0.3))
        ln.requires_grad_(d.requires_grad)
        return ln


def _leaves(*ts):
    return [t for t in ts if t is not None and t.requires_grad]


def _grads(outs, seeds, leaves):
    """d(sum_i <out_i, seed_i>)/d leaves (None where a leaf got no gradient)."""
    pairs = [(o, s) for o, s in zip(outs, seeds) if o is not None and s is not None and o.requires_grad]
    if not leaves or not pairs:
        return [None] * len(leaves)
    loss = sum((o.double() * s.double()).sum() for o, s in pairs)
    return list(torch.autograd.grad(loss, leaves, allow_unused=True))


def _double_leaf(t):
    return t.detach().double().requires_grad_(t.requires_grad)


def _check_grads(cmp, names, got, want, tols):
    if not cmp.grad_mode:                                    # the recorded launch ran without autograd: forward only
        return
    for n, a, b, tol in zip(names, got, want, tols):
        if b is None and a is None:
            continue
        cmp.check(n, a, b, **tol)


# ------------------------------------------------------------------------------------------------
# checkers
# ------------------------------------------------------------------------------------------------
CHECKERS = {}


def checker(*names):
    def reg(fn):
        for n in names:
            CHECKERS[n] = fn
        return fn
    return reg


def _f32(d):
    return d.dtype == "float32"


@checker("conv1x1", "conv1x1_skip")
def check_conv1x1(rec, cmp):
    """fp32: test_conv1x1_f32 (1e-5 of the max for y, dx, dw); bf16: test_conv1x1_bf16."""
    I = Inputs(rec)
    xd, wdsc = I.a["x"], I.a["weight"]
    co, ci = wdsc.shape[:2]
    x = I.tensor(xd)
    w = I.tensor(wdsc, ci ** -0.5)
    wt = w.detach().reshape(co, ci).t().contiguous() if I.a["wt"] is not None else None
    imgs = None
    if I.a["imgs"] is not None:                              # ResNetV2's group images of W and W^T (StdConv2dSame.image_specs)
        wv = w.detach()
        imgs = tuple(ops.x3_image_many([(wv, 0, co, ci, ci, ci, 0, 1), (wv, 0, ci, co, 1, co, 0, ci)], I.dev))
    skip = rec.name == "conv1x1_skip"
    with torch.set_grad_enabled(rec.grad):
        out = CENSUS_ORIGINALS[rec.name](x, w, wt, I.a["math"], imgs)
        y, sk = (out[0], out[1]) if skip else (out, None)
        dy = I.randn(y.shape, dtype=y.dtype)
        ds = I.randn(x.shape, dtype=x.dtype) if sk is not None else None
        leaves = _leaves(x, w)
        got = _grads([y, sk], [dy, ds], leaves)
    xr, wr = _double_leaf(x), _double_leaf(w)
    ref = F.conv2d(xr, wr)
    want = _grads([ref, xr if sk is not None else None], [dy, ds], _leaves(xr, wr))
    f32 = _f32(xd)
    cmp.check("y", y, ref, tol=1e-5 if f32 else 1e-2)
    _check_grads(cmp, [n for n, t in (("dx", x), ("dw", w)) if t.requires_grad], got, want,
                 [dict(tol=1e-5 if f32 else 1.5e-2) if t is x else dict(tol=1e-5 if f32 else 1e-2) for t in leaves])


def _conv_same_ref(xd, wd, stride):
    import math
    k = wd.shape[2]
    pads = []
    for n in (xd.shape[3], xd.shape[2]):
        t = max((math.ceil(n / stride) - 1) * stride + k - n, 0)
        pads += [t // 2, t - t // 2]
    return F.conv2d(F.pad(xd, pads), wd, stride=stride)


def _conv_check(rec, cmp, run, ref_fn):
    """Common body of the split-product convolutions: 1e-5 of the max for y, dx, dw (test_conv3x3_split, test_conv_s2_split)."""
    I = Inputs(rec)
    xd, wdsc = I.a["x"], I.a["weight"]
    co, ci, k, _ = wdsc.shape
    x = I.tensor(xd)
    w = I.tensor(wdsc, (k * k * ci) ** -0.5)
    with torch.set_grad_enabled(rec.grad):
        y = run(I, x, w)
        dy = I.randn(y.shape)
        leaves = _leaves(x, w)
        got = _grads([y], [dy], leaves)
    xr, wr = _double_leaf(x), _double_leaf(w)
    ref = ref_fn(xr, wr)
    want = _grads([ref], [dy], _leaves(xr, wr))
    cmp.check("y", y, ref, tol=1e-5)
    _check_grads(cmp, ["dx" if t is x else "dw" for t in leaves], got, want, [dict(tol=1e-5)] * len(leaves))


def _images_of(I, w, stride):
    """The weight images ResNetV2 makes for a convolution (StdConv2dSame.image_specs: the product's own layout)."""
    from acr_wsss_amd.backbone import StdConv2dSame
    co, ci, k, _ = w.shape
    conv = StdConv2dSame(ci, co, k, stride=stride)
    conv.acr_math = 1
    specs = conv.image_specs(w.detach())
    assert specs is not None, "the recorded launch had weight images, but the product's image_specs gives none"
    return tuple(ops.x3_image_many(list(specs), I.dev))


@checker("conv3x3")
def check_conv3x3(rec, cmp):
    def run(I, x, w):
        imgs = _images_of(I, w, 1) if I.a["imgs"] is not None else None
        return CENSUS_ORIGINALS["conv3x3"](x, w, imgs)
    _conv_check(rec, cmp, run, lambda x, w: F.conv2d(x, w, padding=1))


@checker("conv_s2")
def check_conv_s2(rec, cmp):
    def run(I, x, w):
        imgs = _images_of(I, w, 2) if I.a["imgs"] is not None else None
        return CENSUS_ORIGINALS["conv_s2"](x, w, imgs)
    _conv_check(rec, cmp, run, lambda x, w: _conv_same_ref(x, w, 2))


@checker("subsample2")
def check_subsample2(rec, cmp):
    """Bit-equal to x[:, :, ::2, ::2] and its autograd backward (test_subsample2)."""
    I = Inputs(rec)
    x = I.tensor(I.a["x"])
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS["subsample2"](x)
        dy = I.randn(y.shape)
        got = _grads([y], [dy], _leaves(x))
    xr = _double_leaf(x)
    ref = xr[:, :, ::2, ::2]
    want = _grads([ref], [dy], _leaves(xr))
    cmp.check("y", y, ref)
    _check_grads(cmp, ["dx"], got, want, [{}])


@checker("maxpool3x3s2_same")
def check_maxpool(rec, cmp):
    """-inf SAME padding + 3x3/2 max: values bit-equal, dx to 1e-6 (test_maxpool_same_bf16, fp32)."""
    I = Inputs(rec)
    x = I.tensor(I.a["x"])
    pt, pl, ph, pw = (I.a[k] for k in ("pt", "pl", "ph", "pw"))
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS["maxpool3x3s2_same"](x, pt, pl, ph, pw)
        dy = I.randn(y.shape, dtype=y.dtype)
        got = _grads([y], [dy], _leaves(x))
    xr = _double_leaf(x)
    ref = F.max_pool2d(F.pad(xr, [pl, pw - pl, pt, ph - pt], value=-float("inf")), 3, 2)
    want = _grads([ref], [dy], _leaves(xr))
    f32 = _f32(I.a["x"])
    cmp.check("y", y, ref, **({} if f32 else dict(tol=1e-2)))
    _check_grads(cmp, ["dx"], got, want, [dict(rtol=1e-6, atol=1e-6) if f32 else dict(rtol=2e-2, atol=2e-2)])


@checker("groupnorm_act")
def check_groupnorm(rec, cmp):
    """fp32 with a backward: test_groupnorm_f32 (y 1e-5, dx 2e-5, dgamma / dbeta 2e-5 + 1e-6, dresid 1e-6 of the max); forward-only
    (the split small launches of CAM generation): test_groupnorm_f32_small_launch_parts (2e-5 of max(1, max|y|))."""
    I = Inputs(rec)
    xd = I.a["x"]
    assert _f32(xd), "bf16 GroupNorm: not part of the fp32 census"
    act, eps = I.a["act"], I.a["eps"]
    x = I.tensor(xd, 1.7, 0.3)
    w = I.randn(I.a["weight"].shape, 0.2, 1.0).requires_grad_(I.a["weight"].requires_grad)
    b = I.randn(I.a["bias"].shape, 0.3).requires_grad_(I.a["bias"].requires_grad)
    r = I.tensor(I.a["resid"]) if I.a["resid"] is not None else None
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS["groupnorm_act"](x, w, b, act, r, eps)
        dy = I.randn(y.shape)
        leaves = _leaves(x, w, b, r)
        got = _grads([y], [dy], leaves)
    xr, wr, br = _double_leaf(x), _double_leaf(w), _double_leaf(b)
    rr = _double_leaf(r) if r is not None else None
    ref = F.group_norm(xr, 32, wr, br, eps)
    if rr is not None:
        ref = ref + rr
    if act != "none":
        ref = ref * (y.detach() > 0).double()               # the kernel's own mask: elements within 1e-7 of 0 may differ
    want = _grads([ref], [dy], _leaves(xr, wr, br, rr))
    if leaves:
        cmp.check("y", y, ref, tol=1e-5)
    else:
        cmp.check("y", y, ref, atol=2e-5 * max(1.0, float(ref.abs().max())))
    names = {id(x): ("dx", dict(tol=2e-5)), id(w): ("dgamma", dict(tol=2e-5, atol=1e-6)), id(b): ("dbeta", dict(tol=2e-5, atol=1e-6))}
    if r is not None:
        names[id(r)] = ("dresid", dict(tol=1e-6))
    _check_grads(cmp, [names[id(t)][0] for t in leaves], got, want, [names[id(t)][1] for t in leaves])


@checker("weight_std_all")
def check_weight_std(rec, cmp):
    """test_weight_std_all_f32: 1e-5 of the max forward, 5e-5 backward, per weight."""
    I = Inputs(rec)
    eps = I.a["eps"]
    ws = [I.tensor(d, 0.3, 0.05) for d in I.a["weights"]]
    with torch.set_grad_enabled(rec.grad):
        outs = CENSUS_ORIGINALS["weight_std_all"](ws, eps)
        gs = [I.randn(o.shape) for o in outs]
        got = _grads(outs, gs, _leaves(*ws))
    wr = [_double_leaf(w) for w in ws]
    refs = []
    for w in wr:
        std, mean = torch.std_mean(w, dim=[1, 2, 3], keepdim=True, unbiased=False)
        refs.append((w - mean) / (std + eps))
    want = _grads(refs, gs, _leaves(*wr))
    for i, (o, r) in enumerate(zip(outs, refs)):
        cmp.check("w_hat[%d]" % i, o, r, tol=1e-5)
    _check_grads(cmp, ["dw[%d]" % i for i, w in enumerate(ws) if w.requires_grad], got, want, [dict(tol=5e-5)] * len(got))


@checker("tokens")
def check_tokens(rec, cmp):
    """test_tokens_assembly: forward and dy bit-equal to the fp32 torch chain; dbias / dprefix / dpos to 2e-6 * sqrt(B) of the max
    (here against float64)."""
    I = Inputs(rec)
    y, bias, prefix, pos = (I.tensor(I.a[k]) for k in ("y", "bias", "prefix", "pos"))
    B = y.shape[0]
    with torch.set_grad_enabled(rec.grad):
        tok = CENSUS_ORIGINALS["tokens"](y, bias, prefix, pos)
        dt = I.randn(tok.shape)
        leaves = _leaves(y, bias, prefix, pos)
        got = _grads([tok], [dt], leaves)

    def chain(y, bias, prefix, pos):
        return torch.cat([prefix.unsqueeze(0).expand(B, -1, -1), (y + bias.view(1, -1, 1, 1)).flatten(2).transpose(1, 2)], dim=1) + pos
    with torch.no_grad():
        cmp.check("tokens (vs the fp32 chain)", tok, chain(y, bias, prefix, pos))
    rs = [_double_leaf(t) for t in (y, bias, prefix, pos)]
    ref = chain(*rs)
    want = _grads([ref], [dt], _leaves(*rs))
    names = {id(y): ("dy", {}), id(bias): ("dbias", dict(tol=2e-6 * B ** 0.5)), id(prefix): ("dprefix", dict(tol=2e-6 * B ** 0.5)),
             id(pos): ("dpos", dict(tol=2e-6 * B ** 0.5))}
    if y.requires_grad:                                      # a transposed copy: bit-equal to the fp32 chain's gradient too
        want[0] = want[0].float()
    _check_grads(cmp, [names[id(t)][0] for t in leaves], got, want, [names[id(t)][1] for t in leaves])


@checker("layer_norm_skip")
def check_layer_norm_skip(rec, cmp):
    """test_layernorm_f32: y, dx (with the fused skip gradient), dgamma, dbeta to 2e-5 of the max."""
    I = Inputs(rec)
    x = I.tensor(I.a["x"], 2.0, 0.5)
    ln = I.layernorm(I.a["ln"])
    with torch.set_grad_enabled(rec.grad):
        y, skip = CENSUS_ORIGINALS["layer_norm_skip"](x, ln)
        dy, ds = I.randn(y.shape), I.randn(x.shape)
        leaves = _leaves(x, ln.weight, ln.bias)
        got = _grads([y, skip], [dy, ds], leaves)
    xr, wr, br = _double_leaf(x), _double_leaf(ln.weight), _double_leaf(ln.bias)
    ref = F.layer_norm(xr, (x.shape[-1],), wr, br, ln.eps)
    want = _grads([ref, xr], [dy, ds], _leaves(xr, wr, br))
    tol = 2e-5 if _f32(I.a["x"]) else 2e-2
    cmp.check("y", y, ref, tol=tol if _f32(I.a["x"]) else 1.2e-2)
    names = {id(x): "dx", id(ln.weight): "dgamma", id(ln.bias): "dbeta"}
    _check_grads(cmp, [names[id(t)] for t in leaves], got, want, [dict(tol=tol)] * len(leaves))


def _ln_image_composite(I, cmp, rec, ln_d, xd, consumer, tol):
    """LayerNorm leaving as its consumer's operand image (test_layernorm_image_f32): ``consumer(h, skip, image) -> output`` with the
    consumer's own parameters in ``consumer.params``; everything against float64 at ``tol`` of the max."""
    x = I.tensor(xd, 2.0, 0.5)
    ln = I.layernorm(ln_d)
    with torch.set_grad_enabled(rec.grad):
        h, skip, img = CENSUS_ORIGINALS["layer_norm_image"](x, ln)
        out = consumer.run(h, skip, img)
        dz = I.randn(out.shape)
        leaves = _leaves(x, ln.weight, ln.bias, *consumer.params)
        got = _grads([out], [dz], leaves)
    xr, wr, br = _double_leaf(x), _double_leaf(ln.weight), _double_leaf(ln.bias)
    pr = [_double_leaf(p) for p in consumer.params]
    ref = consumer.ref(F.layer_norm(xr, (x.shape[-1],), wr, br, ln.eps), xr, pr)
    want = _grads([ref], [dz], _leaves(xr, wr, br, *pr))
    cmp.check("y", out, ref, tol=tol)
    names = ["dx", "dgamma", "dbeta"] + ["d" + n for n in consumer.names]
    allp = [x, ln.weight, ln.bias] + list(consumer.params)
    ids = [id(p) for p in allp]
    _check_grads(cmp, [names[ids.index(id(t))] for t in leaves], got, want, [dict(tol=tol)] * len(leaves))


class _LinConsumer:
    def __init__(self, lin, math, resid=None):
        self.lin, self.math = lin, math
        self.params = [p for p in (lin.weight, lin.bias) if p is not None]
        self.names = ["W", "b"][:len(self.params)]

    def run(self, h, skip, img):
        return CENSUS_ORIGINALS["linear_or_hip"](h, self.lin, None, True, math=self.math, x_image=img)

    def ref(self, hr, xr, pr):
        return F.linear(hr, *pr)


class _MlpConsumer:
    def __init__(self, fc1, fc2, math):
        self.fc1, self.fc2, self.math = fc1, fc2, math
        self.params = [fc1.weight, fc1.bias, fc2.weight, fc2.bias]
        self.names = ["W1", "b1", "W2", "b2"]

    def run(self, h, skip, img):
        return CENSUS_ORIGINALS["mlp_f32"](h, self.fc1, self.fc2, skip, self.math, img)

    def ref(self, hr, xr, pr):
        return xr + F.linear(F.gelu(F.linear(hr, pr[0], pr[1])), pr[2], pr[3])


@checker("layer_norm_image")
def check_layer_norm_image(rec, cmp):
    """norm -> Linear (the qkv shape, C -> 3C) with LN(x) as the Linear's image: test_layernorm_image_f32's 2e-5.  The consumers the
    model actually ran are checked as composites by their own records (linear_or_hip / mlp_f32 with x_image)."""
    I = Inputs(rec)
    ln_d, xd = I.a["ln"], I.a["x"]
    C = ln_d.C
    lin = I.linear(Lin(3 * C, C, True, True))
    _ln_image_composite(I, cmp, rec, ln_d, xd, _LinConsumer(lin, 1), 2e-5)


def _placeholder_input(xd):
    """The input descriptor of a Linear / MLP that read a LayerNorm image: the LayerNorm's x (same shape, a real tensor)."""
    return T(xd.shape, xd.dtype, xd.requires_grad, False)


def _attn_ref(qkv, H):
    B, Tn, _ = qkv.shape
    q, k, v = qkv.reshape(B, Tn, 3, H, 64).permute(2, 0, 3, 1, 4)
    P = ((q @ k.transpose(-2, -1)) * 64 ** -0.5).softmax(-1)
    return (P @ v).transpose(1, 2).reshape(B, Tn, H * 64), P


@checker("linear_or_hip")
def check_linear(rec, cmp):
    """Plain: y, dx, dW, db to 1e-5 of the max (test_gemm_f32_linear for math 0 / 1, test_linear_f32_fp16x2_against_fp64 for math 2),
    d(resid) == dy.  With an operand image from a LayerNorm (x is its expanded placeholder): the LN -> Linear composite at
    test_layernorm_image_f32's 2e-5.  With the attention output's image: that image bit-equal to the image pass over o
    (test_attention_output_image_is_the_pass_image), and the Linear on it against float64 at 1e-5."""
    I = Inputs(rec)
    xd, lin_d, math = I.a["x"], I.a["lin"], I.a["math"]
    assert _f32(xd) and I.a["use_hip"], "bf16 / stock Linears: not part of the fp32 census"
    if I.a["x_image"] is not None and xd.expanded:
        lin = I.linear(lin_d)
        _ln_image_composite(I, cmp, rec, LN(lin_d.in_features, 1e-6, lin_d.requires_grad), _placeholder_input(xd), _LinConsumer(lin, math), 2e-5)
        return
    lin = I.linear(lin_d)
    r = I.tensor(I.a["resid"]) if I.a["resid"] is not None else None
    img = None
    if I.a["x_image"] is not None:                           # proj behind attention_core_oimg
        B, Tn, D = xd.shape
        qkv = I.randn((B, Tn, 3 * D), 1.5)
        with torch.no_grad():                                # the image needs resident scores: here they serve the head mean
            o, _, img = CENSUS_ORIGINALS["attention_core_oimg"](qkv, D // 64, ops.MeanStack(B, 1, Tn, I.dev), 0, None, 1)
        if img is None:
            cmp.fail("the attention forward wrote no output image at %s, but the recorded launch had one" % (tuple(qkv.shape),))
            return
        cmp.check("o image (vs the image pass)", img.view(torch.int32), ops.x3_image(o.reshape(B * Tn, D)).view(torch.int32))
        x = o.detach().requires_grad_(xd.requires_grad)
    else:
        x = I.tensor(xd)
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS["linear_or_hip"](x, lin, r, True, math=math, x_image=img)
        dy = I.randn(y.shape)
        leaves = _leaves(x, lin.weight, lin.bias, r)
        got = _grads([y], [dy], leaves)
    xr, wr = _double_leaf(x), _double_leaf(lin.weight)
    br = _double_leaf(lin.bias) if lin.bias is not None else None
    rr = _double_leaf(r) if r is not None else None
    ref = F.linear(xr, wr, br) + (rr if rr is not None else 0)
    want = _grads([ref], [dy], _leaves(xr, wr, br, rr))
    cmp.check("y", y, ref, tol=1e-5)
    names = {id(x): ("dx", dict(tol=1e-5)), id(lin.weight): ("dW", dict(tol=1e-5))}
    if lin.bias is not None:
        names[id(lin.bias)] = ("db", dict(tol=1e-5))
    if r is not None:
        names[id(r)] = ("dresid", {})
    _check_grads(cmp, [names[id(t)][0] for t in leaves], got, want, [names[id(t)][1] for t in leaves])


@checker("mlp_f32")
def check_mlp_f32(rec, cmp):
    """fc2(GELU(fc1(x))) + resid: output and all gradients to 2e-5 of the max for math 0 / 1 (test_fused_mlp_f32) and 1e-5 for
    math 2 (test_mlp_f32_fp16x2_against_fp64); with a LayerNorm image: the LN -> MLP composite at test_layernorm_image_f32's 3e-5."""
    I = Inputs(rec)
    xd, math = I.a["x"], I.a["math"]
    fc1, fc2 = I.linear(I.a["fc1"], 3.0, 0.3), I.linear(I.a["fc2"], 1.0, 0.3)
    tol = 1e-5 if math == 2 else 2e-5
    if I.a["x_image"] is not None:
        _ln_image_composite(I, cmp, rec, LN(fc1.in_features, 1e-6, I.a["fc1"].requires_grad), _placeholder_input(xd),
                            _MlpConsumer(fc1, fc2, math), 3e-5 if math != 2 else tol)
        return
    x = I.tensor(xd)
    r = I.tensor(I.a["resid"]) if I.a["resid"] is not None else None
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS["mlp_f32"](x, fc1, fc2, r, math)
        dy = I.randn(y.shape)
        ps = [fc1.weight, fc1.bias, fc2.weight, fc2.bias]
        leaves = _leaves(x, r, *ps)
        got = _grads([y], [dy], leaves)
    xr = _double_leaf(x)
    rr = _double_leaf(r) if r is not None else None
    pr = [_double_leaf(p) for p in ps]
    ref = F.linear(F.gelu(F.linear(xr, pr[0], pr[1])), pr[2], pr[3]) + (rr if rr is not None else 0)
    want = _grads([ref], [dy], _leaves(xr, rr, *pr))
    cmp.check("y", y, ref, tol=tol)
    allp, names = [x, r] + ps, ["dx", "dresid", "dW1", "db1", "dW2", "db2"]
    ids = [id(p) if p is not None else None for p in allp]
    _check_grads(cmp, [names[ids.index(id(t))] for t in leaves], got, want, [dict(tol=tol)] * len(leaves))


@checker("mlp")
def check_mlp_bf16(rec, cmp):
    """bf16 fused MLP: test_fused_mlp_bf16's 2.5e-2 of the max for the output and every gradient."""
    I = Inputs(rec)
    xd = I.a["x"]
    fc1, fc2 = I.linear(I.a["fc1"], 3.0, 0.3).to(torch.bfloat16), I.linear(I.a["fc2"], 1.0, 0.3).to(torch.bfloat16)
    x = I.tensor(xd)
    r = I.tensor(I.a["resid"]) if I.a["resid"] is not None else None
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS["mlp"](x, fc1, fc2, r)
        dy = I.randn(y.shape, dtype=y.dtype)
        ps = [fc1.weight, fc1.bias, fc2.weight, fc2.bias]
        leaves = _leaves(x, r, *ps)
        got = _grads([y], [dy], leaves)
    xr = _double_leaf(x)
    rr = _double_leaf(r) if r is not None else None
    pr = [_double_leaf(p) for p in ps]
    ref = F.linear(F.gelu(F.linear(xr, pr[0], pr[1])), pr[2], pr[3]) + (rr if rr is not None else 0)
    want = _grads([ref], [dy], _leaves(xr, rr, *pr))
    cmp.check("y", y, ref, tol=2.5e-2)
    _check_grads(cmp, ["g%d" % i for i in range(len(leaves))], got, want, [dict(tol=2.5e-2)] * len(leaves))


@checker("attention_core", "attention_core_oimg")
def check_attention(rec, cmp):
    """test_attention_f32's bounds: o rtol 1e-4 / atol 2e-5, head mean rtol 1e-4 / atol 1e-7, dqkv 3e-5 of the max -- with the
    head-mean gradient when the model trained (the loss reads the maps) and without it in CAM generation.  The _oimg form: its
    output image bit-equal to the image pass over o (test_attention_output_image_is_the_pass_image)."""
    I = Inputs(rec)
    qd, heads, math = I.a["qkv"], I.a["heads"], I.a["math"]
    assert _f32(qd), "bf16 attention: not part of the fp32 census"
    B, Tn, _ = qd.shape
    qkv = I.tensor(qd, 1.5)
    sd = I.a["stack"]
    stack = None
    if sd is not None:
        stack = ops.MeanStack(B, sd.shape[1], Tn, I.dev)
        stack.buf.fill_(float("nan"))
    layer = I.a["layer"]
    owner = I.a["owner"]
    with_g = owner is not None and owner.training and stack is not None
    oimg = rec.name == "attention_core_oimg"
    with torch.set_grad_enabled(rec.grad):
        out = CENSUS_ORIGINALS[rec.name](qkv, heads, stack, layer, None, math)
        o, pm = out[0], out[1]
        d_o = I.randn(o.shape)
        gpm = I.randn(pm.shape) if (with_g and pm is not None) else None
        got = _grads([o, pm], [d_o, gpm], _leaves(qkv))
    if oimg:
        if out[2] is None:
            # documented: the forward writes no image where it runs split-tail workgroups; proj then images o itself (its own record)
            if ops.L.load().acr_attn_fwd_oimg_offered(ops._desc(B, heads, Tn, torch.float32, math=1)):
                cmp.fail("no output image at %s although the forward offers one" % (tuple(qd.shape),))
        else:
            cmp.check("o image (vs the image pass)", out[2].view(torch.int32), ops.x3_image(o.detach().reshape(B * Tn, -1)).view(torch.int32))
    qr = _double_leaf(qkv)
    o_ref, P = _attn_ref(qr, heads)
    pm_ref = P.mean(1)
    want = _grads([o_ref, pm_ref], [d_o, gpm], _leaves(qr))
    cmp.check("o", o, o_ref, rtol=1e-4, atol=2e-5)
    if stack is not None:
        cmp.check("head mean", pm, pm_ref, rtol=1e-4, atol=1e-7)
        others = torch.cat([stack.buf[:, :layer], stack.buf[:, layer + 1:]], 1)
        if not bool(torch.isnan(others).all()):
            cmp.fail("the launch wrote outside its layer's slice of the head-mean stack")
    _check_grads(cmp, ["dqkv"] if qkv.requires_grad else [], got, want, [dict(tol=3e-5)])


def _qkv_lse(I, qd, heads):
    qkv = I.randn(qd.shape, 1.0).requires_grad_(True)
    o, _ = CENSUS_ORIGINALS["attention_core"](qkv, heads, None, 0, None)
    return qkv.detach(), o.grad_fn.saved_tensors[2]


def _dprobs_ref(qkv, d_o, heads):
    B, Tn, _ = qkv.shape
    v = qkv.double().reshape(B, Tn, 3, heads, 64)[:, :, 2].permute(0, 2, 1, 3)
    return d_o.double().reshape(B, Tn, heads, 64).permute(0, 2, 1, 3) @ v.transpose(-2, -1)


@checker("attn_probs")
def check_attn_probs(rec, cmp):
    """test_probs_dprobs_getam_row: P to rtol 1e-4 / atol 1e-7."""
    I = Inputs(rec)
    qkv, lse2 = _qkv_lse(I, I.a["qkv"], I.a["heads"])
    P = CENSUS_ORIGINALS["attn_probs"](qkv, lse2, I.a["heads"])
    cmp.check("P", P, _attn_ref(qkv.double(), I.a["heads"])[1], rtol=1e-4, atol=1e-7)


@checker("attn_dprobs")
def check_attn_dprobs(rec, cmp):
    """test_probs_dprobs_getam_row: dO V^T to rtol 1e-4 / atol 1e-4."""
    I = Inputs(rec)
    qkv = I.randn(I.a["qkv"].shape)
    d_o = I.randn(I.a["d_o"].shape)
    dP = CENSUS_ORIGINALS["attn_dprobs"](qkv, d_o, I.a["heads"])
    cmp.check("dP", dP, _dprobs_ref(qkv, d_o, I.a["heads"]), rtol=1e-4, atol=1e-4)


def _getam_ref(qkv, d_o, heads, func):
    gr = _dprobs_ref(qkv, d_o, heads)                       # (B, H, T, T)
    cm = _attn_ref(qkv.double(), heads)[1]
    mg = gr.clamp(min=0).mean(1)
    mcg = (gr * cm).clamp(min=0).mean(1)
    return {"grad": mg, "cam_grad": mcg, "grad_s": mg * mg, "cam_grad_s": mcg * mg}[func][:, 0]     # row 0 of every sample: (B, T)


@checker("getam_row_accum", "getam_rows_accum")
def check_getam(rec, cmp):
    """test_probs_dprobs_getam_row: the accumulated GETAM row(s) to rtol 1e-4 / atol 1e-6 of the max."""
    I = Inputs(rec)
    heads, func = I.a["heads"], I.a["func"]
    qkv, lse2 = _qkv_lse(I, I.a["qkv"], heads)
    d_o = I.randn(I.a["d_o"].shape)
    ref = _getam_ref(qkv, d_o, heads, func)
    if rec.name == "getam_row_accum":
        b = I.a["batch"]
        row0 = I.randn(I.a["cam_row"].shape)
        row = row0.clone()
        CENSUS_ORIGINALS["getam_row_accum"](qkv, d_o, lse2, heads, b, func, row)
        want = ref[b] + row0.double()
        cmp.check("row", row, want, rtol=1e-4, atol=1e-6 * float(ref[b].abs().max()))
    else:
        rows0 = I.randn(I.a["cam_rows"].shape)
        rows = rows0.clone()
        CENSUS_ORIGINALS["getam_rows_accum"](qkv, d_o, lse2, heads, func, rows)
        cmp.check("rows", rows, ref + rows0.double(), rtol=1e-4, atol=1e-6 * float(ref.abs().max()))


@checker("patch_cam")
def check_patch_cam(rec, cmp):
    """test_cam_readouts: relu(x W^T + b) to rtol 1e-4 / atol 1e-5."""
    I = Inputs(rec)
    x = I.randn(I.a["x"].shape)
    w = I.randn(I.a["weight"].shape, I.a["weight"].shape[1] ** -0.5)
    b = I.randn(I.a["bias"].shape)
    out = CENSUS_ORIGINALS["patch_cam"](x, w, b)
    cmp.check("cam", out, F.relu(F.linear(x.double(), w.double(), b.double())), rtol=1e-4, atol=1e-5)


@checker("bilinear_resize")
def check_bilinear(rec, cmp):
    """test_cam_readouts: resize (+ channel multiply, h-flip, accumulate) to rtol 1e-5 / atol 1e-6.  The sampling grid is the one of
    the reference's fp32 F.interpolate (source coordinates and weights in fp32, infer_cam.py:157-160), which the kernel reproduces;
    everything after the interpolation is float64.  (A float64 grid differs by up to ~1e-5 on random 8x-32x upsampled data.)"""
    I = Inputs(rec)
    src = I.randn(I.a["src"].shape)
    oh, ow = I.a["out_hw"]
    al, cl, hf = I.a["align_corners"], I.a["channels_last"], I.a["hflip"]
    mul = I.randn(I.a["chan_mul"].shape) if I.a["chan_mul"] is not None else None
    out0 = I.randn(I.a["out"].shape) if I.a["out"] is not None else None
    out = out0.clone() if out0 is not None else None
    got = CENSUS_ORIGINALS["bilinear_resize"](src, (oh, ow), al, chan_mul=mul, hflip=hf, out=out, channels_last=cl)
    s = src.permute(2, 0, 1) if cl else src
    ref = F.interpolate(s[None], (oh, ow), mode="bilinear", align_corners=bool(al))[0].double()
    if mul is not None:
        ref = ref * mul.double().reshape(-1, 1, 1)
    if hf:
        ref = ref.flip(-1)
    if out0 is not None:
        ref = ref + out0.double()
    cmp.check("resized", got, ref, rtol=1e-5, atol=1e-6)


@checker("aff_refine_batch")
def check_aff_refine(rec, cmp):
    """test_cam_readouts (aff_refine): patch_aff @ cam to rtol 1e-5 / atol 1e-6 * T, per sample of the batch."""
    I = Inputs(rec)
    stack = I.rand(I.a["stack"].shape)
    cams = I.rand(I.a["cams"].shape)
    Tn = stack.shape[-1]
    out = CENSUS_ORIGINALS["aff_refine_batch"](stack, cams)
    ref = torch.stack([(stack[s, :, 1:, 1:].double().sum(0) @ cams[s].double().t()).t() for s in range(stack.shape[0])])
    cmp.check("refined", out, ref, rtol=1e-5, atol=1e-6 * Tn)


def _flip_perm(p, dev):
    return torch.arange(p * p, device=dev).reshape(p, p).flip(1).reshape(-1)


@checker("consistency")
def check_consistency(rec, cmp):
    """test_consistency: both terms to 2e-6 relative (+ 1e-9), the stack gradient to rtol 1e-5 / atol 1e-12."""
    I = Inputs(rec)
    ad = I.a["a"]
    assert I.a["a2"] is None, "the model passes the fused two-view stack"
    a = I.rand(ad.shape).requires_grad_(ad.requires_grad)
    p = I.a["p"]
    B = a.shape[0] // 2
    w = (1.7, -0.6)
    with torch.set_grad_enabled(rec.grad):
        cls, aff = CENSUS_ORIGINALS["consistency"](a, p)
        got = _grads([cls, aff], [torch.tensor(w[0]), torch.tensor(w[1])], _leaves(a))
    ar = _double_leaf(a)
    pi = _flip_perm(p, I.dev)
    a1, a2 = ar[:B], ar[B:]
    rc = (a1[:, :, 0, 1:] - a2[:, :, 0, 1:][:, :, pi]).abs().mean()
    ra = (a1[:, :, 1:, 1:] - a2[:, :, 1:, 1:][:, :, pi][:, :, :, pi]).abs().mean()
    want = _grads([rc, ra], [torch.tensor(w[0]), torch.tensor(w[1])], _leaves(ar))
    cmp.check("cls_align", cls, rc, rtol=2e-6, atol=1e-9)
    cmp.check("aff_align", aff, ra, rtol=2e-6, atol=1e-9)
    _check_grads(cmp, ["da"] if a.requires_grad else [], got, want, [dict(rtol=1e-5, atol=1e-12)])


@checker("mlsm_loss")
def check_mlsm(rec, cmp):
    """test_mlsm_loss: the loss and its logit gradient to 2e-6 relative."""
    I = Inputs(rec)
    x = I.tensor(I.a["x"], 6.0)
    y = (I.rand(I.a["y"].shape) > 0.7).float()
    with torch.set_grad_enabled(rec.grad):
        loss = CENSUS_ORIGINALS["mlsm_loss"](x, y)
        got = _grads([loss], [torch.tensor(2.5)], _leaves(x))
    xr = _double_leaf(x)
    ref = F.multilabel_soft_margin_loss(xr, y.double())
    want = _grads([ref], [torch.tensor(2.5)], _leaves(xr))
    cmp.check("loss", loss, ref, rtol=2e-6)
    _check_grads(cmp, ["dx"] if x.requires_grad else [], got, want, [dict(tol=2e-6)])


CENSUS_ORIGINALS = {n: getattr(ops, n) for n in ENTRIES}      # the entries as defined (checkers call these, never a wrapper)


def check_all(records, cmp, only=None):
    """Run every record through its checker; a record whose entry has no checker is a failure."""
    for rec in records:
        cmp.where = fmt(rec)
        cmp.grad_mode = rec.grad
        fn = CHECKERS.get(rec.name)
        if fn is None:
            cmp.fail("no checker registered for entry %r" % rec.name)
            continue
        try:
            fn(rec, cmp)
        except Exception as e:                               # a checker that cannot run is a failure of that record
            cmp.fail("checker raised %s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else ""))
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# library fallbacks: stock functional calls made on behalf of the model
# ------------------------------------------------------------------------------------------------
FALLBACK_FUNCS = ("conv2d", "linear", "layer_norm", "group_norm")


class FallbackAudit:
    """Counts calls of F.conv2d / F.linear / F.layer_norm / F.group_norm whose nearest caller outside torch is a function of
    acr_wsss_amd (a module's forward reached through nn.Module counts for the acr_wsss_amd code that called the module).
    Keys: (function, caller module, caller qualname, first input's shape)."""

    def __init__(self):
        self.calls = Counter()

    def install(self, monkeypatch):
        for name in FALLBACK_FUNCS:
            monkeypatch.setattr(F, name, self._wrap(name, getattr(F, name)))

    def _wrap(self, name, fn):
        def wrapper(*args, **kwargs):
            f = sys._getframe(1)
            while f is not None and f.f_globals.get("__name__", "").startswith("torch"):
                f = f.f_back
            mod = f.f_globals.get("__name__", "") if f is not None else ""
            if mod.startswith("acr_wsss_amd"):
                slf = f.f_locals.get("self")
                qual = (type(slf).__name__ + "." if slf is not None else "") + f.f_code.co_name
                shape = tuple(args[0].shape) if args and torch.is_tensor(args[0]) else ()
                self.calls[(name, mod.split(".")[-1], qual, shape)] += 1
            return fn(*args, **kwargs)
        return wrapper

    def sites(self):
        """{(function, module, caller)} -- shapes merged."""
        return sorted(set(k[:3] for k in self.calls))
