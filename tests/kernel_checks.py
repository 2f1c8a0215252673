"""One float64 check per public ``ops`` entry: the reference, the tolerances and the comparison.

Both the hand-written kernel tests (tests/test_kernels_gpu.py, tests/test_fp16x2_gpu.py: their own shapes, seeds and input
distributions) and the launch census (tests/launch_census.py: the shapes the model really launches) run an entry themselves and
hand what went in and what came out to the ``verify_*`` function of that entry.  It rebuilds the computation in float64 torch
math, takes the same seeds through the reference's backward and compares output and gradients through ``Cmp`` -- which also
proves every comparison can fail.  A tolerance is written once, in ``TOL`` below; a caller that needs another value says so at its
call site (``tols`` of the norm checks: name of a compared quantity -> keywords of ``Cmp.check`` that replace its ``TOL`` entry).

Conventions: ``got`` is the list of the kernel's gradients, one per input that requires grad, in the order the function names its
inputs (``grads_of(x, w, ...)`` for a test that called ``backward()``).  A seed of ``None`` means that output took no part in the
backward.  Tolerances are keyword sets of ``Cmp.check``: ``tol`` of max|reference|, ``rtol`` of |reference| elementwise, ``atol``.
"""
import math

import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
EXACT = {}


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
        self.log = []                                        # (label, max |err|, max |reference|) of every value comparison

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
        self.log.append((label, float((got - want).abs().max()), scale))
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


def grads_of(*ts):
    """``got`` of a test that ran ``backward()``: the .grad of every input that requires one."""
    return [t.grad for t in _leaves(*ts)]


def _named(cmp, inputs, names, tols, got, want):
    """_check_grads over the inputs that require grad: ``inputs`` / ``names`` / ``tols`` run parallel (None: input absent)."""
    keep = [i for i, t in enumerate(inputs) if t is not None and t.requires_grad]
    _check_grads(cmp, [names[i] for i in keep], got, want, [tols[i] for i in keep])


def _dl(t):
    return _double_leaf(t) if t is not None else None


# ------------------------------------------------------------------------------------------------
# tolerances: every literal once
# ------------------------------------------------------------------------------------------------
TOL = {
    # fp32 on the fp32 GEMM kernels (exact MFMA, split products, fp16x2): 1e-5 of the max; bf16: 8 significant bits
    "conv1x1": {F32: dict(y=dict(tol=1e-5), dx=dict(tol=1e-5), dw=dict(tol=1e-5)),
                BF16: dict(y=dict(tol=1e-2), dx=dict(tol=1.5e-2), dw=dict(tol=1e-2))},
    "conv": dict(tol=1e-5),                                  # conv3x3 / conv_s2: y, dx, dw
    "maxpool_dx": {F32: dict(rtol=1e-6, atol=1e-6),         # a pixel collects up to 4 window gradients: summation order only
                   BF16: dict(rtol=2e-2, atol=2e-2)},
    "groupnorm": {F32: dict(y=dict(tol=1e-5), dx=dict(tol=2e-5), dgamma=dict(tol=2e-5, atol=1e-6), dbeta=dict(tol=2e-5, atol=1e-6),
                            dresid=dict(tol=1e-6)),
                  BF16: dict(y=dict(tol=1.2e-2), dx=dict(tol=2e-2), dgamma=dict(tol=2e-2, atol=1e-2), dbeta=dict(tol=2e-2, atol=1e-2),
                             dresid=dict(tol=1e-2))},
    "groupnorm_forward_only": 2e-5,                          # of max(1, max|y|): the split small launches sum in another order
    "weight_std": {F32: dict(w_hat=dict(tol=1e-5), dw=dict(tol=5e-5)),
                   BF16: dict(w_hat=dict(tol=1e-2), dw=dict(tol=2e-2, atol=1e-3))},
    "tokens_sum": 2e-6,                                      # dbias / dprefix / dpos: times sqrt(B), of the max
    "layernorm": {F32: dict(y=dict(tol=2e-5), dx=dict(tol=2e-5), dparam=dict(tol=2e-5)),
                  # bf16 dgamma / dbeta: 1e-2 of the max + 1e-2 (sums over all rows), and at most 2e-2 of the max
                  BF16: dict(y=dict(tol=1.2e-2), dx=dict(tol=2e-2), dparam=dict(tol=1e-2, atol=1e-2), dparam_of_max=2e-2)},
    "ln_image": {"linear": dict(tol=2e-5), "mlp": dict(tol=3e-5)},
    "linear": {F32: dict(y=dict(tol=1e-5), dx=dict(tol=1e-5), dW=dict(tol=1e-5), db=dict(tol=1e-5)),
               BF16: dict(y=dict(tol=1e-2), dx=dict(tol=1.5e-2), dW=dict(tol=1.5e-2), db=dict(tol=1e-2, atol=1e-2))},
    "mlp": {0: dict(tol=2e-5), 1: dict(tol=2e-5), 2: dict(tol=1e-5), BF16: dict(tol=2.5e-2)},      # by math resp. bf16 tensors
    "attention": {F32: dict(o=dict(rtol=1e-4, atol=2e-5), pm=dict(rtol=1e-4, atol=1e-7), dqkv=dict(tol=3e-5)),
                  BF16: dict(o=dict(tol=1.5e-2), pm=dict(rtol=2e-3, atol=1e-6),
                             # MFMA path (P / dS rounded to bf16 before the second products) resp. exact-fp32 math with bf16 I/O
                             dqkv={False: dict(tol=2.5e-2), True: dict(tol=1e-2)}, dqkv_mean={False: 3e-3, True: 1.5e-3})},
    "probs": {F32: dict(rtol=1e-4, atol=1e-7), BF16: dict(rtol=2e-3, atol=1e-6)},
    "dprobs": {F32: dict(rtol=1e-4, atol=1e-4), BF16: dict(rtol=1e-3, atol=1e-3)},
    "getam": dict(rtol=1e-4, atol_of_max=1e-6),
    "patch_cam": dict(rtol=1e-4, atol=1e-5),
    "bilinear": dict(rtol=1e-5, atol=1e-6),
    "aff_refine": dict(rtol=1e-5, atol_per_token=1e-6),
    "consistency": dict(term=dict(rtol=2e-6, atol=1e-9), da=dict(rtol=1e-5, atol=1e-12)),
    "mlsm": dict(loss=dict(rtol=2e-6), dx=dict(tol=2e-6)),
}


# ------------------------------------------------------------------------------------------------
# convolutions, pooling
# ------------------------------------------------------------------------------------------------
def verify_conv1x1(cmp, x, w, y, skip, dy, ds, got):
    """conv1x1 / conv1x1_skip (``skip``: the shortcut's view of x, its gradient seed ``ds`` added into dx; None for plain conv1x1)
    vs float64 conv2d."""
    xr, wr = _double_leaf(x), _double_leaf(w)
    ref = F.conv2d(xr, wr)
    want = _grads([ref, xr if skip is not None else None], [dy, ds], _leaves(xr, wr))
    t = TOL["conv1x1"][x.dtype]
    cmp.check("y", y, ref, **t["y"])
    _named(cmp, [x, w], ["dx", "dw"], [t["dx"], t["dw"]], got, want)
    return ref.detach()


def conv_same_ref(xd, wd, stride):
    """TF-SAME convolution as the reference computes it: F.pad (odd pixel right / bottom) + F.conv2d (std_conv.py:56-65)."""
    k = wd.shape[2]
    pads = []
    for n in (xd.shape[3], xd.shape[2]):
        t = max((math.ceil(n / stride) - 1) * stride + k - n, 0)
        pads += [t // 2, t - t // 2]
    return F.conv2d(F.pad(xd, pads), wd, stride=stride)


def verify_conv_same(cmp, x, w, stride, y, dy, got):
    """conv3x3 (stride 1) / conv_s2 (stride 2, 3x3 and 7x7): the split-product SAME convolutions vs float64 pad + conv2d."""
    xr, wr = _double_leaf(x), _double_leaf(w)
    ref = conv_same_ref(xr, wr, stride)
    want = _grads([ref], [dy], _leaves(xr, wr))
    cmp.check("y", y, ref, **TOL["conv"])
    _named(cmp, [x, w], ["dx", "dw"], [TOL["conv"]] * 2, got, want)
    return ref.detach()


def verify_subsample2(cmp, x, y, dy, got):
    """Bit-equal to x[:, :, ::2, ::2] and its autograd backward."""
    xr = _double_leaf(x)
    ref = xr[:, :, ::2, ::2]
    want = _grads([ref], [dy], _leaves(xr))
    cmp.check("y", y, ref, **EXACT)
    _named(cmp, [x], ["dx"], [EXACT], got, want)


def verify_maxpool(cmp, x, pt, pl, ph, pw, y, dy, got):
    """-inf SAME padding + 3x3/2 max: a maximum of the inputs is one of them, so the values are bit-equal in either dtype; dx sums
    up to four routed gradients."""
    xr = _double_leaf(x)
    ref = F.max_pool2d(F.pad(xr, [pl, pw - pl, pt, ph - pt], value=-float("inf")), 3, 2)
    want = _grads([ref], [dy], _leaves(xr))
    cmp.check("y", y, ref, **EXACT)
    _named(cmp, [x], ["dx"], [TOL["maxpool_dx"][x.dtype]], got, want)


# ------------------------------------------------------------------------------------------------
# norms, weight standardisation, token assembly
# ------------------------------------------------------------------------------------------------
def verify_groupnorm(cmp, x, w, b, r, act, y, dy, got, eps=1e-5, tols=None):
    """GroupNorm(32) [+ residual] [+ ReLU].  The value is compared with the float64 ReLU; the backward goes through the kernel's own
    mask (elements within rounding of 0 may fall on either side, and the gradient follows the side the kernel took).  Without any
    gradient (CAM generation's split small launches) the forward-only bound applies.  Returns the reference output."""
    xr, wr, br, rr = _double_leaf(x), _double_leaf(w), _double_leaf(b), _dl(r)
    pre = F.group_norm(xr, 32, wr, br, eps)
    if rr is not None:
        pre = pre + rr
    ref = pre if act == "none" else F.relu(pre)
    routed = pre if act == "none" else pre * (y.detach() > 0).double()
    want = _grads([routed], [dy], _leaves(xr, wr, br, rr))
    t = dict(TOL["groupnorm"][x.dtype], **(tols or {}))
    if _leaves(x, w, b, r) or (tols and "y" in tols):
        cmp.check("y", y, ref, **t["y"])
    else:
        cmp.check("y", y, ref, atol=TOL["groupnorm_forward_only"] * max(1.0, float(ref.abs().max())))
    _named(cmp, [x, w, b, r], ["dx", "dgamma", "dbeta", "dresid"], [t["dx"], t["dgamma"], t["dbeta"], t["dresid"]], got, want)
    return ref.detach()


def verify_weight_std(cmp, ws, outs, gs, got, eps=1e-5, tols=None, keep=None):
    """(w - mean) / (std + eps) per output channel (std_conv.py:56-59), per weight of the launch.  ``keep``: per weight, the
    output channels that are compared (all by default; their gradients are those of the kept channels' outputs alone)."""
    wr = [_double_leaf(w) for w in ws]
    keep = keep if keep is not None else [slice(None)] * len(ws)
    refs = []
    for w in wr:
        std, mean = torch.std_mean(w, dim=[1, 2, 3], keepdim=True, unbiased=False)
        refs.append((w - mean) / (std + eps))
    want = _grads([r[k] for r, k in zip(refs, keep)], [g[k] if g is not None else None for g, k in zip(gs, keep)], _leaves(*wr))
    t, tols = TOL["weight_std"][ws[0].dtype], tols or {}
    for i, (o, r) in enumerate(zip(outs, refs)):
        cmp.check("w_hat[%d]" % i, o[keep[i]], r[keep[i]], **tols.get("w_hat[%d]" % i, t["w_hat"]))
    names = ["dw[%d]" % i for i in range(len(ws))]
    kept = iter(keep[i] for i, w in enumerate(ws) if w.requires_grad)
    sel = [(a[k] if a is not None else None, b[k] if b is not None else None) for (a, b), k in zip(zip(got, want), kept)] if got else []
    _named(cmp, ws, names, [tols.get(n, t["dw"]) for n in names], [a for a, _ in sel], [b for _, b in sel])


def verify_tokens(cmp, y, bias, prefix, pos, tok, dt, got):
    """Forward and dy bit-equal to the fp32 torch chain (vision_transformer.py:449-467: same order of the two additions; dy is a
    transposed copy); dbias / dprefix / dpos sum over B samples (and the tokens): summation-order tolerance against float64."""
    B = y.shape[0]

    def chain(y, bias, prefix, pos):
        return torch.cat([prefix.unsqueeze(0).expand(B, -1, -1), (y + bias.view(1, -1, 1, 1)).flatten(2).transpose(1, 2)], dim=1) + pos
    with torch.no_grad():
        cmp.check("tokens (vs the fp32 chain)", tok, chain(y, bias, prefix, pos), **EXACT)
    rs = [_double_leaf(t) for t in (y, bias, prefix, pos)]
    want = _grads([chain(*rs)], [dt], _leaves(*rs))
    if y.requires_grad:
        want[0] = want[0].float()
    s = dict(tol=TOL["tokens_sum"] * B ** 0.5)
    _named(cmp, [y, bias, prefix, pos], ["dy", "dbias", "dprefix", "dpos"], [EXACT, s, s, s], got, want)


def verify_layernorm(cmp, x, weight, bias, eps, y, skip, dy, ds, got, tols=None):
    """LayerNorm over the last dimension (``skip``: the residual stream's view of x, its seed ``ds`` is the fused skip gradient;
    None for the plain form)."""
    xr, wr, br = _double_leaf(x), _double_leaf(weight), _double_leaf(bias)
    ref = F.layer_norm(xr, (x.shape[-1],), wr, br, eps)
    want = _grads([ref, xr if skip is not None else None], [dy, ds], _leaves(xr, wr, br))
    t = TOL["layernorm"][x.dtype]
    tp = [t["dparam"], t["dparam"]]
    if "dparam_of_max" in t:                                 # ... and never above that share of the max: cut the absolute part
        by = dict(zip(map(id, _leaves(xr, wr, br)), want))
        for i, p in enumerate((wr, br)):
            if by.get(id(p)) is not None:
                room = (t["dparam_of_max"] - tp[i]["tol"]) * float(by[id(p)].abs().max())
                tp[i] = dict(tp[i], atol=min(tp[i]["atol"], room))
    tols = tols or {}
    cmp.check("y", y, ref, **tols.get("y", t["y"]))
    _named(cmp, [x, weight, bias], ["dx", "dgamma", "dbeta"], [tols.get("dx", t["dx"]), tols.get("dgamma", tp[0]), tols.get("dbeta", tp[1])], got, want)


def verify_ln_consumer(cmp, x, ln, kind, params, out, dz, skip, ds, got, math=1, tols=None):
    """LayerNorm leaving as its consumer's operand image, checked as the composite it is: ``kind`` "linear": Linear(LN(x)) with
    ``params`` (W, b); "mlp": x + fc2(GELU(fc1(LN(x)))) with (W1, b1, W2, b2).  ``ds`` seeds the skip output where the caller used
    it on its own.  ``got``: gradients of x, gamma, beta, then the consumer's parameters."""
    xr, wr, br = _double_leaf(x), _double_leaf(ln.weight), _double_leaf(ln.bias)
    pr = [_double_leaf(p) for p in params]
    hr = F.layer_norm(xr, (x.shape[-1],), wr, br, ln.eps)
    if kind == "linear":
        ref, names = F.linear(hr, *pr), ["dW", "db"][:len(pr)]
    else:
        ref, names = xr + F.linear(F.gelu(F.linear(hr, pr[0], pr[1])), pr[2], pr[3]), ["dW1", "db1", "dW2", "db2"]
    want = _grads([ref, xr if ds is not None else None], [dz, ds], _leaves(xr, wr, br, *pr))
    tol = TOL["mlp"][2] if (kind == "mlp" and math == 2) else TOL["ln_image"][kind]
    tols = tols or {}
    cmp.check("y", out, ref, **tols.get("y", tol))
    inputs = [x, ln.weight, ln.bias] + list(params)
    names = ["dx", "dgamma", "dbeta"] + names
    _named(cmp, inputs, names, [tols.get(n, tol) for n in names], got, want)


# ------------------------------------------------------------------------------------------------
# Linears
# ------------------------------------------------------------------------------------------------
def verify_linear(cmp, x, weight, bias, resid, y, dy, got):
    """y = x W^T + b (+ resid); d(resid) is dy itself."""
    xr, wr, br, rr = _double_leaf(x), _double_leaf(weight), _dl(bias), _dl(resid)
    ref = F.linear(xr, wr, br) + (rr if rr is not None else 0)
    want = _grads([ref], [dy], _leaves(xr, wr, br, rr))
    t = TOL["linear"][x.dtype]
    cmp.check("y", y, ref, **t["y"])
    _named(cmp, [x, weight, bias, resid], ["dx", "dW", "db", "dresid"], [t["dx"], t["dW"], t["db"], EXACT], got, want)


def verify_mlp(cmp, x, resid, params, y, dy, got, math=0):
    """fc2(GELU(fc1(x))) (+ resid), exact-erf GELU, ``params`` = (W1, b1, W2, b2): output and every gradient at one tolerance, by
    ``math`` for fp32 tensors (0 exact fp32, 1 split products, 2 fp16x2)."""
    xr, rr = _double_leaf(x), _dl(resid)
    pr = [_double_leaf(p) for p in params]
    ref = F.linear(F.gelu(F.linear(xr, pr[0], pr[1])), pr[2], pr[3]) + (rr if rr is not None else 0)
    want = _grads([ref], [dy], _leaves(xr, rr, *pr))
    tol = TOL["mlp"][BF16 if x.dtype == BF16 else math]
    cmp.check("y", y, ref, **tol)
    _named(cmp, [x, resid] + list(params), ["dx", "dresid", "dW1", "db1", "dW2", "db2"], [tol] * 6, got, want)


# ------------------------------------------------------------------------------------------------
# attention and its read-outs
# ------------------------------------------------------------------------------------------------
def attn_ref(qkv, H):
    """(o, P) of models/vision_transformer.py:203-211 in the dtype of ``qkv`` (pass float64)."""
    B, Tn, _ = qkv.shape
    q, k, v = qkv.reshape(B, Tn, 3, H, 64).permute(2, 0, 3, 1, 4)
    P = ((q @ k.transpose(-2, -1)) * 64 ** -0.5).softmax(-1)
    return (P @ v).transpose(1, 2).reshape(B, Tn, H * 64), P


def dprobs_ref(qkv, d_o, heads):
    B, Tn, _ = qkv.shape
    v = qkv.double().reshape(B, Tn, 3, heads, 64)[:, :, 2].permute(0, 2, 1, 3)
    return d_o.double().reshape(B, Tn, heads, 64).permute(0, 2, 1, 3) @ v.transpose(-2, -1)


def verify_attention(cmp, qkv, heads, o, pm, d_o, gpm, got, f32math=False):
    """o and the head mean of the probabilities (DPT/ACR.py:107-112; ``pm`` None: not requested) and dqkv, with the head-mean
    gradient ``gpm`` or without.  bf16 tensors (inputs rounded once, fp64 math on the rounded values): dqkv also in the mean;
    ``f32math``: the exact-fp32-math kernels with bf16 I/O."""
    qr = _double_leaf(qkv)
    o_ref, P = attn_ref(qr, heads)
    pm_ref = P.mean(1)
    want = _grads([o_ref, pm_ref if pm is not None else None], [d_o, gpm], _leaves(qr))
    t = TOL["attention"][qkv.dtype]
    cmp.check("o", o, o_ref, **t["o"])
    if pm is not None:
        cmp.check("head mean", pm, pm_ref, **t["pm"])
    if qkv.dtype == BF16:
        _named(cmp, [qkv], ["dqkv"], [t["dqkv"][f32math]], got, want)
        if got and got[0] is not None and want[0] is not None:
            mean, bound = float((got[0].double() - want[0]).abs().mean()), t["dqkv_mean"][f32math] * float(want[0].abs().max())
            if not mean <= bound:
                cmp.fail("dqkv: mean |err| %.3e above %.3e" % (mean, bound))
    else:
        _named(cmp, [qkv], ["dqkv"], [t["dqkv"]], got, want)


def verify_attn_probs(cmp, qkv, heads, P):
    """The probabilities recomputed from the saved row statistics.  Returns the float64 P."""
    P_ref = attn_ref(qkv.detach().double(), heads)[1]
    cmp.check("P", P, P_ref, **TOL["probs"][qkv.dtype])
    return P_ref


def verify_attn_dprobs(cmp, qkv, d_o, heads, dP):
    """dO V^T per head.  Returns the float64 dP."""
    dP_ref = dprobs_ref(qkv.detach(), d_o, heads)
    cmp.check("dP", dP, dP_ref, **TOL["dprobs"][qkv.dtype])
    return dP_ref


def verify_getam(cmp, P_ref, dP_ref, func, got, start=None, batch=None, times=1):
    """Row 0 of the GETAM map ``func`` of every sample (``batch``: of that sample only), accumulated ``times`` times onto ``start``
    (None: zeros)."""
    mg = dP_ref.clamp(min=0).mean(1)
    mcg = (dP_ref * P_ref).clamp(min=0).mean(1)
    ref = {"grad": mg, "cam_grad": mcg, "grad_s": mg * mg, "cam_grad_s": mcg * mg}[func][:, 0] * times      # (B, T)
    if batch is not None:
        ref = ref[batch]
    want = ref + (start.double() if start is not None else 0)
    t = TOL["getam"]
    cmp.check("row" if batch is not None else "rows", got, want, rtol=t["rtol"], atol=t["atol_of_max"] * float(ref.abs().max()))


def verify_patch_cam(cmp, x, w, b, out):
    cmp.check("cam", out, F.relu(F.linear(x.double(), w.double(), b.double())), **TOL["patch_cam"])


def verify_bilinear(cmp, src, out_hw, align_corners, channels_last, hflip, chan_mul, out0, got):
    """Resize (+ channel multiply, h-flip, accumulate onto ``out0``).  The sampling grid is the one of the reference's fp32
    F.interpolate (source coordinates and weights in fp32, infer_cam.py:157-160), which the kernel reproduces; everything after the
    interpolation is float64.  (A float64 grid differs by up to ~1e-5 on random 8x-32x upsampled data.)"""
    s = src.permute(2, 0, 1) if channels_last else src
    ref = F.interpolate(s[None], tuple(out_hw), mode="bilinear", align_corners=bool(align_corners))[0].double()
    if chan_mul is not None:
        ref = ref * chan_mul.double().reshape(-1, 1, 1)
    if hflip:
        ref = ref.flip(-1)
    if out0 is not None:
        ref = ref + out0.double()
    cmp.check("resized", got, ref, **TOL["bilinear"])


def verify_aff_refine(cmp, stack, cams, out):
    """patch_aff @ cam per sample: ``stack`` (S, L, T, T), ``cams`` (S, n, T - 1)."""
    Tn = stack.shape[-1]
    ref = torch.stack([(stack[s, :, 1:, 1:].double().sum(0) @ cams[s].double().t()).t() for s in range(stack.shape[0])])
    t = TOL["aff_refine"]
    cmp.check("refined", out, ref, rtol=t["rtol"], atol=t["atol_per_token"] * Tn)


# ------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------
def flip_perm(p, dev):
    return torch.arange(p * p, device=dev).reshape(p, p).flip(1).reshape(-1)


def verify_consistency(cmp, a, p, w, cls, aff, got):
    """Both terms of the fused two-view stack ``a`` (2B, L, T, T) and the stack gradient under the seeds ``w`` = (w_cls, w_aff).
    A term that is exactly zero in float64 (identical views) must come out exactly zero."""
    B = a.shape[0] // 2
    ar = _double_leaf(a)
    pi = flip_perm(p, a.device)
    a1, a2 = ar[:B], ar[B:]
    rc = (a1[:, :, 0, 1:] - a2[:, :, 0, 1:][:, :, pi]).abs().mean()
    ra = (a1[:, :, 1:, 1:] - a2[:, :, 1:, 1:][:, :, pi][:, :, :, pi]).abs().mean()
    seeds = [torch.as_tensor(float(w[0])), torch.as_tensor(float(w[1]))]
    want = _grads([rc, ra], seeds, _leaves(ar))
    t = TOL["consistency"]
    cmp.check("cls_align", cls, rc, **(t["term"] if float(rc.detach()) != 0 else EXACT))
    cmp.check("aff_align", aff, ra, **(t["term"] if float(ra.detach()) != 0 else EXACT))
    _named(cmp, [a], ["da"], [t["da"]], got, want)


def verify_mlsm(cmp, x, y, seed, loss, got):
    """F.multilabel_soft_margin_loss in float64 and its logit gradient under the upstream gradient ``seed``."""
    xr = _double_leaf(x)
    ref = F.multilabel_soft_margin_loss(xr, y.double())
    want = _grads([ref], [torch.as_tensor(float(seed))], _leaves(xr))
    t = TOL["mlsm"]
    cmp.check("loss", loss, ref, **t["loss"])
    _named(cmp, [x], ["dx"], [t["dx"]], got, want)
