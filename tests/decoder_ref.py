"""Float64 numpy restatement of the DPT decoder's pieces (DPT/blocks.py:277-413): BatchNorm2d forward and backward with the
running update, the x2 ``align_corners=True`` bilinear upsampling and its adjoint, the residual unit and the fusion block, each
with a hand-written backward.  tests/test_decoder_cpu.py pins it to torch's float64 autograd and to the reference's own results
(tests/golden/decoder_block_{a,b}.npz); tests/test_decoder_gpu.py holds the kernels against it.

The upsampling's source indices and weights are computed in fp32, as torch computes them (and the kernels reproduce); everything
after them is float64."""
import numpy as np

F64 = np.float64


def sample(a, stride):
    """how the fixtures store a tensor: flat, every ``stride``-th value where it has more than 4096"""
    a = np.asarray(a).reshape(-1)
    return a[::stride].copy() if a.size > 4096 else a.copy()


def block_layout(features):
    """key -> shape of a fusion block's parameters (the reference's FeatureFusionBlock_custom state dict without the buffers)"""
    f = features
    out = {"out_conv.weight": (f, f, 1, 1), "out_conv.bias": (f,)}
    for u in ("resConfUnit1.", "resConfUnit2."):
        out.update({u + "conv1.weight": (f, f, 3, 3), u + "conv2.weight": (f, f, 3, 3), u + "bn1.weight": (f,), u + "bn1.bias": (f,),
                    u + "bn2.weight": (f,), u + "bn2.bias": (f,)})
    return out


def block_params(fx):
    """the parameters of a block fixture: weights from tests/golden/recipe.py, the running statistics as the fixture stores them
    (``before:``).  name -> fp32 numpy array"""
    from recipe import recipe_tensor
    p = {k: recipe_tensor(k, s, 0).numpy() for k, s in block_layout(int(fx["features"])).items()}
    p.update({k[len("before:"):]: v for k, v in fx.items() if k.startswith("before:")})
    return p


# ------------------------------------------------------------------------------------------------
# BatchNorm2d
# ------------------------------------------------------------------------------------------------
def bn_fwd(x, gamma, beta, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5, relu=False, resid=None,
           resid2=None):
    """dict: y, pre (before the ReLU), mean, invstd, running_mean / running_var AFTER the call (copies; None where none given)"""
    x, gamma, beta = np.asarray(x, F64), np.asarray(gamma, F64), np.asarray(beta, F64)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    rm = None if running_mean is None else np.asarray(running_mean, F64).copy()
    rv = None if running_var is None else np.asarray(running_var, F64).copy()
    if training:
        if n < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        mean = x.mean(axis=(0, 2, 3))
        var = ((x - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
        if rm is not None:
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * var * n / (n - 1)
    else:
        mean, var = rm, rv
    invstd = 1.0 / np.sqrt(var + eps)
    pre = (x - mean[None, :, None, None]) * (invstd * gamma)[None, :, None, None] + beta[None, :, None, None]
    for r in (resid, resid2):
        if r is not None:
            pre = pre + np.asarray(r, F64)
    return dict(y=np.maximum(pre, 0) if relu else pre, pre=pre, mean=mean, invstd=invstd, running_mean=rm, running_var=rv)


def bn_bwd(x, gamma, mean, invstd, dy, training=True, mask=None):
    """(dx, dgamma, dbeta, dres): ``mask`` the ReLU's pass mask (None: no ReLU); dres the gradient of either addend"""
    x, gamma, g = np.asarray(x, F64), np.asarray(gamma, F64), np.asarray(dy, F64)
    if mask is not None:
        g = g * mask
    xhat = (x - mean[None, :, None, None]) * invstd[None, :, None, None]
    dbeta, dgamma = g.sum(axis=(0, 2, 3)), (g * xhat).sum(axis=(0, 2, 3))
    k = (gamma * invstd)[None, :, None, None]
    if training:
        n = x.shape[0] * x.shape[2] * x.shape[3]
        dx = k * (g - (dbeta / n)[None, :, None, None] - xhat * (dgamma / n)[None, :, None, None])
    else:
        dx = k * g
    return dx, dgamma, dbeta, g


# ------------------------------------------------------------------------------------------------
# x2 bilinear upsampling, align_corners=True
# ------------------------------------------------------------------------------------------------
def up_taps(n_in):
    """(i0, i1, lambda) per destination index of an axis n_in -> 2 n_in, torch's rule in fp32"""
    n_out = 2 * n_in
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    lam = np.clip((src - i0.astype(np.float32)).astype(np.float32), 0, 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, lam.astype(F64)


def _up_matrix(n_in):
    i0, i1, lam = up_taps(n_in)
    m = np.zeros((2 * n_in, n_in), F64)
    np.add.at(m, (np.arange(2 * n_in), i0), 1.0 - lam)
    np.add.at(m, (np.arange(2 * n_in), i1), lam)
    return m


def upsample2x(x):
    x = np.asarray(x, F64)
    return np.einsum("Yy,ncyx,Xx->ncYX", _up_matrix(x.shape[2]), x, _up_matrix(x.shape[3]))


def upsample2x_bwd(dy):
    dy = np.asarray(dy, F64)
    return np.einsum("Yy,ncYX,Xx->ncyx", _up_matrix(dy.shape[2] // 2), dy, _up_matrix(dy.shape[3] // 2))


# ------------------------------------------------------------------------------------------------
# stride-1 SAME convolution (3x3 and 1x1)
# ------------------------------------------------------------------------------------------------
def conv_fwd(x, w, b=None):
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    k = w.shape[2]
    p = k // 2
    n, c, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    y = np.zeros((n, w.shape[0], h, wd), F64)
    for i in range(k):
        for j in range(k):
            y += np.einsum("nchw,oc->nohw", xp[:, :, i:i + h, j:j + wd], w[:, :, i, j])
    return y if b is None else y + np.asarray(b, F64)[None, :, None, None]


def conv_bwd(x, w, dy):
    """(dx, dw, db)"""
    x, w, dy = np.asarray(x, F64), np.asarray(w, F64), np.asarray(dy, F64)
    k = w.shape[2]
    p = k // 2
    n, c, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    dxp, dw = np.zeros_like(xp), np.zeros_like(w)
    for i in range(k):
        for j in range(k):
            dxp[:, :, i:i + h, j:j + wd] += np.einsum("nohw,oc->nchw", dy, w[:, :, i, j])
            dw[:, :, i, j] = np.einsum("nohw,nchw->oc", dy, xp[:, :, i:i + h, j:j + wd])
    return dxp[:, :, p:p + h, p:p + wd], dw, dy.sum(axis=(0, 2, 3))


# ------------------------------------------------------------------------------------------------
# residual unit and fusion block.  ``p``: name -> array with the module's own state-dict keys (conv1.weight, bn1.weight,
# bn1.bias, bn1.running_mean, bn1.running_var, ...); ``prefix`` selects a sub-module
# ------------------------------------------------------------------------------------------------
def rcu_fwd(p, prefix, x, addend=None, training=True, momentum=0.1, eps=1e-5):
    """blocks.py:320-343 (+ the fusion block's ``output + res`` when ``addend`` is given).  Returns (out, cache); the cache holds
    the two ReLU inputs (``relu_in``) and the running statistics after the call (``running``)."""
    g = lambda k: np.asarray(p[prefix + k], F64)
    x = np.asarray(x, F64)
    a0 = np.maximum(x, 0)
    c1 = conv_fwd(a0, g("conv1.weight"))
    b1 = bn_fwd(c1, g("bn1.weight"), g("bn1.bias"), g("bn1.running_mean"), g("bn1.running_var"), training, momentum, eps, relu=True)
    c2 = conv_fwd(b1["y"], g("conv2.weight"))
    b2 = bn_fwd(c2, g("bn2.weight"), g("bn2.bias"), g("bn2.running_mean"), g("bn2.running_var"), training, momentum, eps, resid=x,
                resid2=addend)
    running = {prefix + "bn1.running_mean": b1["running_mean"], prefix + "bn1.running_var": b1["running_var"],
               prefix + "bn2.running_mean": b2["running_mean"], prefix + "bn2.running_var": b2["running_var"]}
    cache = dict(x=x, a0=a0, c1=c1, b1=b1, c2=c2, b2=b2, training=training, relu_in=[x, b1["pre"]], running=running)
    return b2["y"], cache


def rcu_bwd(p, prefix, cache, dout):
    """(dx, d_addend, grads) with grads keyed like the parameters"""
    g = lambda k: np.asarray(p[prefix + k], F64)
    t = cache["training"]
    dc2, dg2, db2, dres = bn_bwd(cache["c2"], g("bn2.weight"), cache["b2"]["mean"], cache["b2"]["invstd"], dout, t)
    da1, dw2, _ = conv_bwd(cache["b1"]["y"], g("conv2.weight"), dc2)
    dc1, dg1, db1, _ = bn_bwd(cache["c1"], g("bn1.weight"), cache["b1"]["mean"], cache["b1"]["invstd"], da1, t, mask=cache["b1"]["pre"] > 0)
    da0, dw1, _ = conv_bwd(cache["a0"], g("conv1.weight"), dc1)
    dx = da0 * (cache["x"] > 0) + dres
    grads = {prefix + "conv1.weight": dw1, prefix + "conv2.weight": dw2, prefix + "bn1.weight": dg1, prefix + "bn1.bias": db1,
             prefix + "bn2.weight": dg2, prefix + "bn2.bias": db2}
    return dx, dres, grads


def fusion_fwd(p, xs, training=True, momentum=0.1, eps=1e-5):
    """blocks.py:392-413 on one or two inputs.  Returns (out, cache); cache["relu_in"] lists every ReLU input in call order."""
    cache = dict(n=len(xs), relu_in=[], running={})
    output = np.asarray(xs[0], F64)
    if len(xs) == 2:
        output, cache["u1"] = rcu_fwd(p, "resConfUnit1.", xs[1], addend=output, training=training, momentum=momentum, eps=eps)
        cache["relu_in"] += cache["u1"]["relu_in"]
        cache["running"].update(cache["u1"]["running"])
    output, cache["u2"] = rcu_fwd(p, "resConfUnit2.", output, training=training, momentum=momentum, eps=eps)
    cache["relu_in"] += cache["u2"]["relu_in"]
    cache["running"].update(cache["u2"]["running"])
    cache["up"] = upsample2x(output)
    return conv_fwd(cache["up"], p["out_conv.weight"], p["out_conv.bias"]), cache


def fusion_bwd(p, cache, dout):
    """(list of input gradients, grads)"""
    dup, dwo, dbo = conv_bwd(cache["up"], p["out_conv.weight"], dout)
    grads = {"out_conv.weight": dwo, "out_conv.bias": dbo}
    d, _, g2 = rcu_bwd(p, "resConfUnit2.", cache["u2"], upsample2x_bwd(dup))
    grads.update(g2)
    if cache["n"] == 1:
        return [d], grads
    dx1, dx0, g1 = rcu_bwd(p, "resConfUnit1.", cache["u1"], d)
    grads.update(g1)
    return [dx0, dx1], grads
