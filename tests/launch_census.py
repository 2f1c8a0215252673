"""Launch census: which public ``ops`` entries a real model run calls, at which shapes, and a checker for each.

``Census.install(monkeypatch)`` wraps every entry in ``ENTRIES`` (the backbone, the heads, CAM generation and the loss look them up
on the module at call time).  A wrapper records metadata only -- the entry, each tensor's shape / dtype / requires_grad, the
scalar arguments, whether an operand image came along, the path flags of ``ops`` in force and the grad mode -- and calls the
entry.  No clone, no sync.  Identical records merge, so ``census.records`` is the set of distinct launches.

``CHECKERS[name](record, cmp)`` is the record half of a check: it rebuilds seeded inputs at exactly the recorded shapes (batch
included, so the K-split / slab choices are those of the real launch) and runs the entry down the same path (same ``math``, same
operand images, same grad mode).  The verify half -- the float64 reference, the tolerances, the comparison of the output and of
every input / weight gradient through ``cmp`` -- is the ``verify_*`` function of that entry in tests/kernel_checks.py, the very
one the hand-written kernel tests (tests/test_kernels_gpu.py, tests/test_fp16x2_gpu.py) call on their own shapes: one reference
and one set of tolerances per entry, used by both.
"""
import inspect
import sys
import zlib
from collections import Counter, namedtuple

import torch
import torch.nn.functional as F

import kernel_checks as KC
from acr_wsss_amd import ops
from kernel_checks import Cmp, _grads, _leaves               # noqa: F401  (Cmp: the callers' handle on it)

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
    with torch.set_grad_enabled(rec.grad):
        out = CENSUS_ORIGINALS[rec.name](x, w, wt, I.a["math"], imgs)
        y, sk = (out[0], out[1]) if rec.name == "conv1x1_skip" else (out, None)
        dy = I.randn(y.shape, dtype=y.dtype)
        ds = I.randn(x.shape, dtype=x.dtype) if sk is not None else None
        got = _grads([y, sk], [dy, ds], _leaves(x, w))
    KC.verify_conv1x1(cmp, x, w, y, sk, dy, ds, got)


def _images_of(I, w, stride):
    """The weight images ResNetV2 makes for a convolution (StdConv2dSame.image_specs: the product's own layout)."""
    from acr_wsss_amd.backbone import StdConv2dSame
    co, ci, k, _ = w.shape
    conv = StdConv2dSame(ci, co, k, stride=stride)
    conv.acr_math = 1
    specs = conv.image_specs(w.detach())
    assert specs is not None, "the recorded launch had weight images, but the product's image_specs gives none"
    return tuple(ops.x3_image_many(list(specs), I.dev))


@checker("conv3x3", "conv_s2")
def check_conv_same(rec, cmp):
    I = Inputs(rec)
    xd, wdsc = I.a["x"], I.a["weight"]
    co, ci, k, _ = wdsc.shape
    stride = 1 if rec.name == "conv3x3" else 2
    x = I.tensor(xd)
    w = I.tensor(wdsc, (k * k * ci) ** -0.5)
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS[rec.name](x, w, _images_of(I, w, stride) if I.a["imgs"] is not None else None)
        dy = I.randn(y.shape)
        got = _grads([y], [dy], _leaves(x, w))
    KC.verify_conv_same(cmp, x, w, stride, y, dy, got)


@checker("subsample2")
def check_subsample2(rec, cmp):
    I = Inputs(rec)
    x = I.tensor(I.a["x"])
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS["subsample2"](x)
        dy = I.randn(y.shape)
        got = _grads([y], [dy], _leaves(x))
    KC.verify_subsample2(cmp, x, y, dy, got)


@checker("maxpool3x3s2_same")
def check_maxpool(rec, cmp):
    I = Inputs(rec)
    x = I.tensor(I.a["x"])
    pads = [I.a[k] for k in ("pt", "pl", "ph", "pw")]
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS["maxpool3x3s2_same"](x, *pads)
        dy = I.randn(y.shape, dtype=y.dtype)
        got = _grads([y], [dy], _leaves(x))
    KC.verify_maxpool(cmp, x, *pads, y, dy, got)


@checker("groupnorm_act")
def check_groupnorm(rec, cmp):
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
        got = _grads([y], [dy], _leaves(x, w, b, r))
    KC.verify_groupnorm(cmp, x, w, b, r, act, y, dy, got, eps)


@checker("weight_std_all")
def check_weight_std(rec, cmp):
    I = Inputs(rec)
    eps = I.a["eps"]
    ws = [I.tensor(d, 0.3, 0.05) for d in I.a["weights"]]
    with torch.set_grad_enabled(rec.grad):
        outs = CENSUS_ORIGINALS["weight_std_all"](ws, eps)
        gs = [I.randn(o.shape) for o in outs]
        got = _grads(outs, gs, _leaves(*ws))
    KC.verify_weight_std(cmp, ws, outs, gs, got, eps)


@checker("tokens")
def check_tokens(rec, cmp):
    I = Inputs(rec)
    y, bias, prefix, pos = (I.tensor(I.a[k]) for k in ("y", "bias", "prefix", "pos"))
    with torch.set_grad_enabled(rec.grad):
        tok = CENSUS_ORIGINALS["tokens"](y, bias, prefix, pos)
        dt = I.randn(tok.shape)
        got = _grads([tok], [dt], _leaves(y, bias, prefix, pos))
    KC.verify_tokens(cmp, y, bias, prefix, pos, tok, dt, got)


@checker("layer_norm_skip")
def check_layer_norm_skip(rec, cmp):
    I = Inputs(rec)
    x = I.tensor(I.a["x"], 2.0, 0.5)
    ln = I.layernorm(I.a["ln"])
    with torch.set_grad_enabled(rec.grad):
        y, skip = CENSUS_ORIGINALS["layer_norm_skip"](x, ln)
        dy, ds = I.randn(y.shape), I.randn(x.shape)
        got = _grads([y, skip], [dy, ds], _leaves(x, ln.weight, ln.bias))
    KC.verify_layernorm(cmp, x, ln.weight, ln.bias, ln.eps, y, skip, dy, ds, got)


def _ln_image_composite(I, cmp, rec, ln_d, xd, kind, mods, math):
    """LayerNorm leaving as its consumer's operand image, run as the composite the model runs: ``kind`` "linear" (mods = the
    Linear) or "mlp" (mods = fc1, fc2, which also reads the skip)."""
    x = I.tensor(xd, 2.0, 0.5)
    ln = I.layernorm(ln_d)
    params = [p for m in mods for p in (m.weight, m.bias) if p is not None]
    with torch.set_grad_enabled(rec.grad):
        h, skip, img = CENSUS_ORIGINALS["layer_norm_image"](x, ln)
        if kind == "linear":
            out = CENSUS_ORIGINALS["linear_or_hip"](h, mods[0], None, True, math=math, x_image=img)
        else:
            out = CENSUS_ORIGINALS["mlp_f32"](h, mods[0], mods[1], skip, math, img)
        dz = I.randn(out.shape)
        got = _grads([out], [dz], _leaves(x, ln.weight, ln.bias, *params))
    KC.verify_ln_consumer(cmp, x, ln, kind, params, out, dz, skip, None, got, math)


@checker("layer_norm_image")
def check_layer_norm_image(rec, cmp):
    """norm -> Linear (the qkv shape, C -> 3C) with LN(x) as the Linear's image.  The consumers the model actually ran are checked
    as composites by their own records (linear_or_hip / mlp_f32 with x_image)."""
    I = Inputs(rec)
    ln_d, xd = I.a["ln"], I.a["x"]
    lin = I.linear(Lin(3 * ln_d.C, ln_d.C, True, True))
    _ln_image_composite(I, cmp, rec, ln_d, xd, "linear", [lin], 1)


def _placeholder_input(xd):
    """The input descriptor of a Linear / MLP that read a LayerNorm image: the LayerNorm's x (same shape, a real tensor)."""
    return T(xd.shape, xd.dtype, xd.requires_grad, False)


@checker("linear_or_hip")
def check_linear(rec, cmp):
    """Plain: the Linear.  With an operand image from a LayerNorm (x is its expanded placeholder): the LN -> Linear composite.  With
    the attention output's image: that image bit-equal to the image pass over o, and the Linear on it."""
    I = Inputs(rec)
    xd, lin_d, math = I.a["x"], I.a["lin"], I.a["math"]
    assert _f32(xd) and I.a["use_hip"], "bf16 / stock Linears: not part of the fp32 census"
    lin = I.linear(lin_d)
    if I.a["x_image"] is not None and xd.expanded:
        _ln_image_composite(I, cmp, rec, LN(lin_d.in_features, 1e-6, lin_d.requires_grad), _placeholder_input(xd), "linear", [lin], math)
        return
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
        got = _grads([y], [dy], _leaves(x, lin.weight, lin.bias, r))
    KC.verify_linear(cmp, x, lin.weight, lin.bias, r, y, dy, got)


@checker("mlp", "mlp_f32")
def check_mlp(rec, cmp):
    """fc2(GELU(fc1(x))) + resid, fp32 (mlp_f32, by math) or bf16 (mlp); with a LayerNorm image: the LN -> MLP composite."""
    I = Inputs(rec)
    xd, f32 = I.a["x"], rec.name == "mlp_f32"
    math = I.a["math"] if f32 else 0
    fc1, fc2 = I.linear(I.a["fc1"], 3.0, 0.3), I.linear(I.a["fc2"], 1.0, 0.3)
    if not f32:
        fc1, fc2 = fc1.to(torch.bfloat16), fc2.to(torch.bfloat16)
    elif I.a["x_image"] is not None:
        _ln_image_composite(I, cmp, rec, LN(fc1.in_features, 1e-6, I.a["fc1"].requires_grad), _placeholder_input(xd), "mlp", [fc1, fc2], math)
        return
    x = I.tensor(xd)
    r = I.tensor(I.a["resid"]) if I.a["resid"] is not None else None
    ps = [fc1.weight, fc1.bias, fc2.weight, fc2.bias]
    with torch.set_grad_enabled(rec.grad):
        y = CENSUS_ORIGINALS[rec.name](x, fc1, fc2, r, math) if f32 else CENSUS_ORIGINALS[rec.name](x, fc1, fc2, r)
        dy = I.randn(y.shape, dtype=y.dtype)
        got = _grads([y], [dy], _leaves(x, r, *ps))
    KC.verify_mlp(cmp, x, r, ps, y, dy, got, math)


@checker("attention_core", "attention_core_oimg")
def check_attention(rec, cmp):
    """With the head-mean gradient when the model trained (the loss reads the maps) and without it in CAM generation.  The _oimg
    form: its output image bit-equal to the image pass over o."""
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
    with torch.set_grad_enabled(rec.grad):
        out = CENSUS_ORIGINALS[rec.name](qkv, heads, stack, layer, None, math)
        o, pm = out[0], out[1]
        d_o = I.randn(o.shape)
        gpm = I.randn(pm.shape) if (with_g and pm is not None) else None
        got = _grads([o, pm], [d_o, gpm], _leaves(qkv))
    if rec.name == "attention_core_oimg":
        if out[2] is None:
            # documented: the forward writes no image where it runs split-tail workgroups; proj then images o itself (its own record)
            if ops.L.load().acr_attn_fwd_oimg_offered(ops._desc(B, heads, Tn, torch.float32, math=1)):
                cmp.fail("no output image at %s although the forward offers one" % (tuple(qd.shape),))
        else:
            cmp.check("o image (vs the image pass)", out[2].view(torch.int32), ops.x3_image(o.detach().reshape(B * Tn, -1)).view(torch.int32))
    KC.verify_attention(cmp, qkv, heads, o, pm if stack is not None else None, d_o, gpm, got)
    if stack is not None:
        others = torch.cat([stack.buf[:, :layer], stack.buf[:, layer + 1:]], 1)
        if not bool(torch.isnan(others).all()):
            cmp.fail("the launch wrote outside its layer's slice of the head-mean stack")


def _qkv_lse(I, qd, heads):
    qkv = I.randn(qd.shape, 1.0).requires_grad_(True)
    o, _ = CENSUS_ORIGINALS["attention_core"](qkv, heads, None, 0, None)
    return qkv.detach(), o.grad_fn.saved_tensors[2]


@checker("attn_probs")
def check_attn_probs(rec, cmp):
    I = Inputs(rec)
    qkv, lse2 = _qkv_lse(I, I.a["qkv"], I.a["heads"])
    KC.verify_attn_probs(cmp, qkv, I.a["heads"], CENSUS_ORIGINALS["attn_probs"](qkv, lse2, I.a["heads"]))


@checker("attn_dprobs")
def check_attn_dprobs(rec, cmp):
    I = Inputs(rec)
    qkv = I.randn(I.a["qkv"].shape)
    d_o = I.randn(I.a["d_o"].shape)
    KC.verify_attn_dprobs(cmp, qkv, d_o, I.a["heads"], CENSUS_ORIGINALS["attn_dprobs"](qkv, d_o, I.a["heads"]))


@checker("getam_row_accum", "getam_rows_accum")
def check_getam(rec, cmp):
    I = Inputs(rec)
    heads, func = I.a["heads"], I.a["func"]
    qkv, lse2 = _qkv_lse(I, I.a["qkv"], heads)
    d_o = I.randn(I.a["d_o"].shape)
    P_ref, dP_ref = KC.attn_ref(qkv.double(), heads)[1], KC.dprobs_ref(qkv, d_o, heads)
    if rec.name == "getam_row_accum":
        b = I.a["batch"]
        row0 = I.randn(I.a["cam_row"].shape)
        row = row0.clone()
        CENSUS_ORIGINALS["getam_row_accum"](qkv, d_o, lse2, heads, b, func, row)
        KC.verify_getam(cmp, P_ref, dP_ref, func, row, row0, batch=b)
    else:
        rows0 = I.randn(I.a["cam_rows"].shape)
        rows = rows0.clone()
        CENSUS_ORIGINALS["getam_rows_accum"](qkv, d_o, lse2, heads, func, rows)
        KC.verify_getam(cmp, P_ref, dP_ref, func, rows, rows0)


@checker("patch_cam")
def check_patch_cam(rec, cmp):
    I = Inputs(rec)
    x = I.randn(I.a["x"].shape)
    w = I.randn(I.a["weight"].shape, I.a["weight"].shape[1] ** -0.5)
    b = I.randn(I.a["bias"].shape)
    KC.verify_patch_cam(cmp, x, w, b, CENSUS_ORIGINALS["patch_cam"](x, w, b))


@checker("bilinear_resize")
def check_bilinear(rec, cmp):
    I = Inputs(rec)
    src = I.randn(I.a["src"].shape)
    hw = I.a["out_hw"]
    al, cl, hf = I.a["align_corners"], I.a["channels_last"], I.a["hflip"]
    mul = I.randn(I.a["chan_mul"].shape) if I.a["chan_mul"] is not None else None
    out0 = I.randn(I.a["out"].shape) if I.a["out"] is not None else None
    out = out0.clone() if out0 is not None else None
    got = CENSUS_ORIGINALS["bilinear_resize"](src, tuple(hw), al, chan_mul=mul, hflip=hf, out=out, channels_last=cl)
    KC.verify_bilinear(cmp, src, hw, al, cl, hf, mul, out0, got)


@checker("aff_refine_batch")
def check_aff_refine(rec, cmp):
    I = Inputs(rec)
    stack = I.rand(I.a["stack"].shape)
    cams = I.rand(I.a["cams"].shape)
    KC.verify_aff_refine(cmp, stack, cams, CENSUS_ORIGINALS["aff_refine_batch"](stack, cams))


@checker("consistency")
def check_consistency(rec, cmp):
    I = Inputs(rec)
    ad = I.a["a"]
    assert I.a["a2"] is None, "the model passes the fused two-view stack"
    a = I.rand(ad.shape).requires_grad_(ad.requires_grad)
    p = I.a["p"]
    w = (1.7, -0.6)
    with torch.set_grad_enabled(rec.grad):
        cls, aff = CENSUS_ORIGINALS["consistency"](a, p)
        got = _grads([cls, aff], [torch.tensor(w[0]), torch.tensor(w[1])], _leaves(a))
    KC.verify_consistency(cmp, a, p, w, cls, aff, got)


@checker("mlsm_loss")
def check_mlsm(rec, cmp):
    I = Inputs(rec)
    x = I.tensor(I.a["x"], 6.0)
    y = (I.rand(I.a["y"].shape) > 0.7).float()
    with torch.set_grad_enabled(rec.grad):
        loss = CENSUS_ORIGINALS["mlsm_loss"](x, y)
        got = _grads([loss], [torch.tensor(2.5)], _leaves(x))
    KC.verify_mlsm(cmp, x, y, 2.5, loss, got)


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
