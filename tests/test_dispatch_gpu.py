"""Every HIP dispatch predicate of acr_wsss_amd/ops.py at its edge: one table per predicate.

An INSIDE case is the smallest or most awkward shape the predicate accepts along one clause: the test asserts the predicate, runs the
public op (forward and, where it has one, backward) and hands what went in and what came out to the ``verify_*`` function of that entry
in tests/kernel_checks.py -- float64 reference, tolerances of ``KC.TOL``.  An OUTSIDE case differs from an inside one in that clause
(a few differ in two; their ids say so): it goes through the MODULE or
dispatcher that owns the predicate, under the launch census and the fallback audit (tests/launch_census.py), and must

  * not raise,
  * launch nothing of the guarded entry and reach the stock library call instead,
  * pass the same ``verify_*`` against float64.

The contract behind the outside cases: a module forward never raises over a shape, stride or alignment the stock op accepts, and a
predicate that says yes is accepted by its entry point (16-byte alignment of the operands included -- the ``align`` cases hand a
contiguous view that starts 4 bytes into its buffer).

Where a dispatcher is itself the census entry (``ops.layer_norm_skip``, ``ops.linear_or_hip``) "nothing of the guarded entry" reads:
the result's autograd node is not the HIP Function.  A stock library result that misses a ``KC.TOL`` bound is held to the rule of
tests/test_decoder_gpu.py::compare instead -- at most 2x the error torch's CPU result shows against float64 on the same case, with
a floor of 4 fp32 ulps of the largest reference value; the figures are printed when that happens.

Shapes of the tables that an older parametrisation already holds, and that are therefore not repeated here:
  layer_norm (1, 256), fp32 and bf16     tests/test_kernels_gpu.py::test_layernorm_f32 / test_layernorm_bf16 [1-256]
  linear (M=1, K=32, N=32), math 0 / 1   tests/test_kernels_gpu.py::test_gemm_f32_linear [*-1-32-32]
Two predicates said yes to what their code refuses and were narrowed; their cases moved to the outside tables:
  tokens P = 0         the empty prefix has no address: the entry point's null-pointer check refused it
  conv_s2 k = 7        with an input that wants a gradient: the 7x7 tap plan has no input-gradient pass
"""
import zlib
from collections import namedtuple

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import kernel_checks as KC
import launch_census as LC
from kernel_checks import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULPS = 4 * 2.0 ** -23                                        # the floor of tests/test_decoder_gpu.py::compare
DT = {"f32": F32, "bf16": BF16}


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _t(g, shape, dtype=F32, scale=1.0, offset=0.0, grad=True, dev=DEV):
    """Seeded on the CPU (the same values on either device), rounded to ``dtype`` once."""
    return (torch.randn(tuple(shape), generator=g) * scale + offset).to(dtype).to(dev).requires_grad_(grad)


def _off4(t):
    """``t`` as a contiguous view that starts 4 bytes into its buffer (tests/test_decoder_gpu.py:
    test_batchnorm_repeats_bit_for_bit_and_takes_unaligned_views)."""
    k = 4 // t.element_size()
    buf = torch.zeros(t.numel() + k, dtype=t.dtype, device=t.device)
    buf[k:].copy_(t.detach().reshape(-1))
    v = buf[k:].view(t.shape)
    assert v.is_contiguous() and (not v.is_cuda or v.data_ptr() % 16 == 4)
    return v.requires_grad_(t.requires_grad)


def _layout(t, layout):
    if layout == "off4":
        return _off4(t)
    if layout == "nhwc":
        v = t.detach().contiguous(memory_format=torch.channels_last).requires_grad_(t.requires_grad)
        assert not v.is_contiguous()
        return v
    return t


def _watch(run):
    """``run()`` under the launch census and the fallback audit -> (its result, names of the entries launched, fallback sites)."""
    census, audit = LC.Census(), LC.FallbackAudit()
    with pytest.MonkeyPatch.context() as mp:
        census.install(mp)
        audit.install(mp)
        out = run()
        torch.cuda.synchronize()
    return out, census, audit.sites()


class StockCmp(KC.Cmp):
    """``KC.Cmp`` for results of stock library ops: a quantity that misses its ``KC.TOL`` bound is compared again under the rule of
    tests/test_decoder_gpu.py::compare -- ``cpu()`` gives torch's CPU results of the same case by label, computed only then."""

    def __init__(self, cpu):
        super().__init__()
        self._cpu, self._vals = cpu, None

    def check(self, label, got, want, **tol):
        n = len(self.failures)
        super().check(label, got, want, **tol)
        if len(self.failures) == n or got is None or want is None:
            return
        if self._vals is None:
            self._vals = self._cpu()
        tor = self._vals.get(label)
        if tor is None:
            return
        miss = self.failures.pop()
        ref = want.detach().double().cpu()
        terr = float((tor.detach().double().cpu().reshape(ref.shape) - ref).abs().max())
        derr = float((got.detach().double().cpu() - ref).abs().max())
        floor = ULPS * float(ref.abs().max())
        print("[stock] %s\n[stock]   device err %.3e, torch CPU err %.3e, floor %.3e" % (miss, derr, terr, floor))
        super().check(label, got, want, atol=max(2.0 * terr, floor))


def _labelled(names, inputs, got, y):
    keep = [n for n, t in zip(names, inputs) if t is not None and t.requires_grad]
    return dict(zip(keep, got), y=y)


def _passes(cmp):
    assert cmp.compared > 0
    assert not cmp.failures, "\n".join(cmp.failures)


def _launched(census):
    return set(r.name for r in census.records)


def _outside(run, verify, guarded, stock):
    """The three assertions of an outside case (module docstring).  ``guarded``: census entries that must not have launched;
    ``stock``: the (function, module, caller) site the audit must have seen."""
    res, census, sites = _watch(lambda: run(DEV))
    assert not (_launched(census) & set(guarded)), "%s launched: %s" % (guarded, sorted(LC.fmt(r) for r in census.records))
    assert stock in sites, (stock, sites)
    cmp = StockCmp(lambda: run("cpu")["labelled"])
    verify(cmp, res)
    _passes(cmp)
    return res, census


# ------------------------------------------------------------------------------------------------
# convolutions: conv1x1_fusable, conv3x3_fusable, conv_s2_fusable behind StdConv2dSame
# ------------------------------------------------------------------------------------------------
Conv = namedtuple("Conv", "N cin cout k stride H W dtype math how layout grad", defaults=(1, 1, 8, 8, "f32", 1, "op", "nchw", True))
CONV_ENTRIES = ("conv1x1", "conv1x1_skip", "conv3x3", "conv_s2")
CONV_STOCK = ("conv2d", "backbone", "StdConv2dSame.forward")


def _conv_run(c, dev):
    """how = "op": the public op (conv1x1_skip / conv3x3 / conv_s2); "forward" / "forward_skip": StdConv2dSame with the given weight
    as its standardised one (what ResNetV2 hands it for one forward)."""
    from acr_wsss_amd import backbone, ops
    g = _gen(c)
    dtype = DT[c.dtype]
    x_grad = c.grad and not (c.k == 7 and c.how == "op")         # the 7x7 reads the image: it has no input-gradient pass
    x = _layout(_t(g, (c.N, c.cin, c.H, c.W), dtype, grad=x_grad, dev=dev), c.layout)
    w = _t(g, (c.cout, c.cin, c.k, c.k), dtype, (c.k * c.k * c.cin) ** -0.5, grad=c.grad, dev=dev)
    skip = None
    with torch.set_grad_enabled(c.grad):
        if c.how == "op":
            if c.k == 1:
                y, skip = ops.conv1x1_skip(x, w, None, c.math)
            else:
                y = ops.conv3x3(x, w) if c.stride == 1 else ops.conv_s2(x, w)
        else:
            conv = backbone.StdConv2dSame(c.cin, c.cout, c.k, stride=c.stride).to(dev).to(dtype)
            conv.acr_math, conv._w_hat = c.math, w
            if c.how == "forward_skip":
                y, skip = conv.forward_skip(x)
                skip = skip if c.stride == 1 else None       # a strided shortcut: the float64 check seeds the convolution only
            else:
                y = conv(x)
        dy = _t(g, y.shape, dtype, grad=False, dev=dev)
        ds = _t(g, x.shape, dtype, grad=False, dev=dev) if skip is not None else None
        got = KC._grads([y, skip], [dy, ds], KC._leaves(x, w))
    return dict(c=c, x=x, w=w, y=y, skip=skip, dy=dy, ds=ds, got=got, labelled=_labelled(["dx", "dw"], [x, w], got, y))


def _conv_verify(cmp, r):
    c = r["c"]
    cmp.grad_mode = c.grad
    if c.k == 1 and c.stride == 1:
        KC.verify_conv1x1(cmp, r["x"], r["w"], r["y"], r["skip"], r["dy"], r["ds"], r["got"])
    elif c.k == 1:                                           # a strided 1x1 is a 1x1 of every other pixel: that entry's bounds, by dtype
        xr, wr = KC._double_leaf(r["x"]), KC._double_leaf(r["w"])
        ref = F.conv2d(xr, wr, stride=c.stride)
        want = KC._grads([ref], [r["dy"]], KC._leaves(xr, wr))
        t = KC.TOL["conv1x1"][r["x"].dtype]
        cmp.check("y", r["y"], ref, **t["y"])
        KC._named(cmp, [r["x"], r["w"]], ["dx", "dw"], [t["dx"], t["dw"]], r["got"], want)
    else:
        KC.verify_conv_same(cmp, r["x"], r["w"], c.stride, r["y"], r["dy"], r["got"])


def _conv_fusable(c, x, w):
    from acr_wsss_amd import ops
    if c.k == 1:
        return ops.conv1x1_fusable(x, w, c.stride)
    with torch.set_grad_enabled(c.grad):
        return ops.conv3x3_fusable(x, w, c.stride, c.math) if c.stride == 1 else ops.conv_s2_fusable(x, w, c.stride, c.math)


def _ids(table):
    return list(table)


CONV1X1_IN = {"smallest-2x4": (1, 64, 64, 2, 4), "hw72-channels-64-not-128": (2, 192, 320, 6, 12), "hw40-odd-batch": (3, 64, 192, 5, 8)}


@pytest.mark.parametrize("mode", ["f32-math0", "f32-math1", "bf16"])
@pytest.mark.parametrize("name", _ids(CONV1X1_IN))
def test_conv1x1_inside(name, mode):
    N, cin, cout, H, W = CONV1X1_IN[name]
    c = Conv(N, cin, cout, 1, 1, H, W, mode.split("-")[0], int(mode[-1]) if "math" in mode else 0)
    r = _conv_run(c, DEV)
    assert _conv_fusable(c, r["x"], r["w"]) and r["skip"] is not None
    cmp = KC.Cmp()
    _conv_verify(cmp, r)
    _passes(cmp)


# (N, cin, cout, k, stride, H, W, layout): one clause of conv1x1_fusable each
CONV1X1_OUT = {"hw36": (2, 64, 64, 1, 1, 6, 6, "nchw"), "hw25": (2, 64, 64, 1, 1, 5, 5, "nchw"), "cin96": (2, 96, 64, 1, 1, 2, 4, "nchw"),
               "cout96": (2, 64, 96, 1, 1, 2, 4, "nchw"), "channels-last": (2, 64, 64, 1, 1, 2, 4, "nhwc"),
               "stride2-5x5-subsamples-to-3x3": (2, 64, 64, 1, 2, 5, 5, "nchw"), "align-off4": (2, 192, 320, 1, 1, 6, 12, "off4")}


@pytest.mark.parametrize("how", ["forward", "forward_skip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", _ids(CONV1X1_OUT))
def test_conv1x1_outside(name, dtype, how):
    N, cin, cout, k, stride, H, W, layout = CONV1X1_OUT[name]
    c = Conv(N, cin, cout, k, stride, H, W, dtype, 1, how, layout)
    r, census = _outside(lambda dev: _conv_run(c, dev), _conv_verify, CONV_ENTRIES, CONV_STOCK)
    assert not _conv_fusable(c, r["x"], r["w"])
    if stride == 2:                                          # the subsampled 3x3 map is what the predicate refused (H*W = 9)
        assert "subsample2" in _launched(census) or dtype == "bf16"


CONV3X3_IN = {"one-row-1x16": (1, 16, 16, 1, 16), "hw48-3x16": (1, 32, 16, 3, 16), "w20-4x20": (2, 16, 32, 4, 20)}


@pytest.mark.parametrize("name", _ids(CONV3X3_IN))
def test_conv3x3_inside(name):
    N, cin, cout, H, W = CONV3X3_IN[name]
    c = Conv(N, cin, cout, 3, 1, H, W)
    r = _conv_run(c, DEV)
    assert _conv_fusable(c, r["x"], r["w"])
    cmp = KC.Cmp()
    _conv_verify(cmp, r)
    _passes(cmp)


# (N, cin, cout, H, W, math, layout)
CONV3X3_OUT = {"w18-not-a-multiple-of-4": (1, 16, 16, 8, 18, 1, "nchw"), "hw40-2x20": (1, 16, 16, 2, 20, 1, "nchw"),
               "cin24": (1, 24, 16, 4, 16, 1, "nchw"), "math0": (1, 16, 16, 4, 16, 0, "nchw"), "align-off4": (2, 16, 32, 4, 20, 1, "off4")}


@pytest.mark.parametrize("name", _ids(CONV3X3_OUT))
def test_conv3x3_outside(name):
    N, cin, cout, H, W, math, layout = CONV3X3_OUT[name]
    c = Conv(N, cin, cout, 3, 1, H, W, "f32", math, "forward", layout)
    r, _ = _outside(lambda dev: _conv_run(c, dev), _conv_verify, CONV_ENTRIES, CONV_STOCK)
    assert not _conv_fusable(c, r["x"], r["w"])


@pytest.mark.parametrize("H,W", [(4, 12), (3, 8)], ids=["w12-h4", "w8-h3"])
def test_conv3x3_narrow_map_is_widened(H, W):
    """A map narrower than the kernels' 16-pixel rows reaches ``ops.conv3x3`` on a copy widened with zero columns (the SAME padding
    of the last real column) and equals the float64 convolution of the UNWIDENED input, gradients through the pad and the cut
    included; the library is not reached."""
    c = Conv(2, 16, 32, 3, 1, H, W, "f32", 1, "forward")
    r, census, sites = _watch(lambda: _conv_run(c, DEV))
    assert not _conv_fusable(c, r["x"], r["w"])
    recs = [dict(rec.args)["x"].shape for rec in census.records if rec.name == "conv3x3"]
    assert recs == [(2, 16, H, 16)], recs
    assert CONV_STOCK not in sites, sites
    assert r["y"].shape == (2, 32, H, W) and r["y"].is_contiguous()
    cmp = KC.Cmp()
    _conv_verify(cmp, r)
    _passes(cmp)


# (cin, cout, k, H, W, grad)
CONV_S2_IN = {"k3-one-output-row-2x32": (16, 16, 3, 2, 32, True), "k7-3ch-2x32": (3, 16, 7, 2, 32, True), "k7-4ch-2x32": (4, 16, 7, 2, 32, True),
              "k3-odd-7x15-no-grad": (16, 16, 3, 7, 15, False), "k7-odd-9x7-no-grad": (3, 32, 7, 9, 7, False)}


@pytest.mark.parametrize("name", _ids(CONV_S2_IN))
def test_conv_s2_inside(name):
    """With gradients where the case says so (the 7x7 reads the image: weight gradient only, as in the model)."""
    cin, cout, k, H, W, grad = CONV_S2_IN[name]
    c = Conv(1, cin, cout, k, 2, H, W, grad=grad)
    r = _conv_run(c, DEV)
    assert _conv_fusable(c, r["x"], r["w"])
    cmp = KC.Cmp()
    _conv_verify(cmp, r)
    _passes(cmp)


def test_conv_s2_takes_an_unaligned_input():
    """conv_s2_fusable has no alignment clause: the space-to-depth pass reads an input that starts 4 bytes into its buffer scalar by
    scalar, and everything behind it works on the kernels' own buffers.  Through the module: the kernel launches, the library is not
    reached."""
    c = Conv(1, 16, 16, 3, 2, 2, 32, "f32", 1, "forward", "off4")
    r, census, sites = _watch(lambda: _conv_run(c, DEV))
    assert _conv_fusable(c, r["x"], r["w"]) and r["x"].data_ptr() % 16 == 4
    assert "conv_s2" in _launched(census) and CONV_STOCK not in sites
    cmp = KC.Cmp()
    _conv_verify(cmp, r)
    _passes(cmp)


# 4x24: output width 12 AND H2*W2 = 24; 8x24 differs from an inside shape in the output width only
CONV_S2_OUT = {"out-width-12-4x24": (16, 16, 3, 4, 24, True, "nchw"), "out-width-12-8x24": (16, 16, 3, 8, 24, True, "nchw"),
               "odd-height-3x32": (16, 16, 3, 3, 32, True, "nchw"), "h2w2-9-5x5-no-grad": (16, 16, 3, 5, 5, False, "nchw"),
               "k7-5ch-no-grad": (5, 16, 7, 2, 32, False, "nchw"), "k7-input-wants-a-gradient": (3, 16, 7, 2, 32, True, "nchw"),
               }


@pytest.mark.parametrize("name", _ids(CONV_S2_OUT))
def test_conv_s2_outside(name):
    cin, cout, k, H, W, grad, layout = CONV_S2_OUT[name]
    c = Conv(1, cin, cout, k, 2, H, W, "f32", 1, "forward", layout, grad)
    r, _ = _outside(lambda dev: _conv_run(c, dev), _conv_verify, CONV_ENTRIES, CONV_STOCK)
    assert not _conv_fusable(c, r["x"], r["w"])
    assert (r["x"].requires_grad and r["w"].requires_grad) == grad


# ------------------------------------------------------------------------------------------------
# groupnorm_fusable behind GroupNormAct
# ------------------------------------------------------------------------------------------------
GN = namedtuple("GN", "N C H W dtype act how layout", defaults=("op", "nchw"))
ACTS = ["none", "relu", "add_relu"]


def _gn_run(c, dev):
    from acr_wsss_amd import backbone, ops
    g = _gen(c)
    dtype = DT[c.dtype]
    shape = (c.N, c.C, c.H, c.W)
    x = _layout(_t(g, shape, dtype, 1.7, 0.3, dev=dev), c.layout)
    r = _t(g, shape, dtype, dev=dev) if c.act == "add_relu" else None
    gn = backbone.GroupNormAct(c.C, apply_act=c.act != "none").to(dev).to(dtype)
    with torch.no_grad():
        gn.weight.copy_(_t(g, (c.C,), dtype, 0.2, 1.0, False, dev))
        gn.bias.copy_(_t(g, (c.C,), dtype, 0.3, 0.0, False, dev))
    y = ops.groupnorm_act(x, gn.weight, gn.bias, c.act, r) if c.how == "op" else gn(x, r)
    dy = _t(g, shape, dtype, grad=False, dev=dev)
    ins = [x, gn.weight, gn.bias, r]
    got = KC._grads([y], [dy], KC._leaves(*ins))
    return dict(c=c, x=x, w=gn.weight, b=gn.bias, r=r, y=y, dy=dy, got=got,
                labelled=_labelled(["dx", "dgamma", "dbeta", "dresid"], ins, got, y))


def _gn_verify(cmp, r):
    KC.verify_groupnorm(cmp, r["x"], r["w"], r["b"], r["r"], r["c"].act, r["y"], r["dy"], r["got"])


GN_IN = {"f32-one-vector-per-channel-1x4": (1, 32, 1, 4, "f32"), "f32-32-channels-per-group-2x2": (2, 1024, 2, 2, "f32"),
         "f32-3-channels-per-group-3x4": (1, 96, 3, 4, "f32"), "bf16-smallest-2x4": (1, 32, 2, 4, "bf16"),
         "bf16-largest-register-group-13x8192": (1, 416, 64, 128, "bf16")}


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("name", _ids(GN_IN))
def test_groupnorm_inside(name, act):
    from acr_wsss_amd import ops
    c = GN(*GN_IN[name], act)
    if name.startswith("bf16-largest"):
        assert (c.C // 32) * c.H * c.W // 8 == 1024 * 13
    r = _gn_run(c, DEV)
    assert ops.groupnorm_fusable(r["x"], r["r"])
    cmp = KC.Cmp()
    _gn_verify(cmp, r)
    _passes(cmp)


GN_OUT = {"f32-hw6-2x3": (1, 32, 2, 3, "f32", "nchw"), "f32-hw25-5x5": (1, 32, 5, 5, "f32", "nchw"),
          "f32-64-channels-per-group-2048": (1, 2048, 4, 4, "f32", "nchw"), "f32-align-off4": (1, 96, 3, 4, "f32", "off4"),
          "bf16-one-vector-over-40x205": (1, 416, 40, 205, "bf16", "nchw"), "bf16-hw12": (1, 32, 3, 4, "bf16", "nchw"),
          "bf16-128-channels-per-group-4096": (1, 4096, 2, 4, "bf16", "nchw"), "bf16-align-off4": (1, 32, 2, 4, "bf16", "off4")}


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("name", _ids(GN_OUT))
def test_groupnorm_outside(name, act):
    from acr_wsss_amd import ops
    N, C, H, W, dtype, layout = GN_OUT[name]
    c = GN(N, C, H, W, dtype, act, "module", layout)
    if "one-vector-over" in name:
        assert (H * W) % 8 == 0 and (C // 32) * H * W // 8 == 1024 * 13 + 13
    r, _ = _outside(lambda dev: _gn_run(c, dev), _gn_verify, ("groupnorm_act",), ("group_norm", "backbone", "GroupNormAct.forward"))
    assert not ops.groupnorm_fusable(r["x"], r["r"])


def test_groupnorm_outside_unaligned_residual():
    """The residual alone starts 4 bytes into its buffer: its entry points check that pointer too."""
    from acr_wsss_amd import backbone, ops

    def run(dev):
        g = _gen("gn-resid-off4")
        x, r = _t(g, (1, 96, 3, 4), scale=1.7, offset=0.3, dev=dev), _off4(_t(g, (1, 96, 3, 4), dev=dev))
        gn = backbone.GroupNormAct(96, apply_act=False).to(dev)
        y = gn(x, r)
        dy = _t(g, y.shape, grad=False, dev=dev)
        ins = [x, gn.weight, gn.bias, r]
        got = KC._grads([y], [dy], KC._leaves(*ins))
        return dict(c=GN(1, 96, 3, 4, "f32", "add_relu"), x=x, w=gn.weight, b=gn.bias, r=r, y=y, dy=dy, got=got,
                    labelled=_labelled(["dx", "dgamma", "dbeta", "dresid"], ins, got, y))
    r, _ = _outside(run, _gn_verify, ("groupnorm_act",), ("group_norm", "backbone", "GroupNormAct.forward"))
    assert ops.groupnorm_fusable(r["x"], None) and not ops.groupnorm_fusable(r["x"], r["r"])


# ------------------------------------------------------------------------------------------------
# layer_norm_fusable behind ops.layer_norm / ops.layer_norm_skip
# ------------------------------------------------------------------------------------------------
LNC = namedtuple("LNC", "M C dtype how layout", defaults=("layer_norm_skip", "rows"))


def _ln_run(c, dev):
    from acr_wsss_amd import ops
    g = _gen(c)
    dtype = DT[c.dtype]
    if c.layout == "every-other-column":
        x = _t(g, (c.M, 2 * c.C), dtype, 2.0, 0.5, False, dev)[:, ::2].requires_grad_(True)
        assert not x.is_contiguous()
    else:
        x = _layout(_t(g, (c.M, c.C), dtype, 2.0, 0.5, dev=dev), c.layout)
    ln = nn.LayerNorm(c.C, eps=1e-6).to(dev).to(dtype)
    with torch.no_grad():
        ln.weight.copy_(_t(g, (c.C,), dtype, 0.2, 1.0, False, dev))
        ln.bias.copy_(_t(g, (c.C,), dtype, 0.3, 0.0, False, dev))
    if c.how == "layer_norm_skip":
        y, skip = ops.layer_norm_skip(x, ln)
    else:
        y, skip = ops.layer_norm(x, ln), None
    dy = _t(g, y.shape, dtype, grad=False, dev=dev)
    ds = _t(g, x.shape, dtype, grad=False, dev=dev) if skip is not None else None
    ins = [x, ln.weight, ln.bias]
    got = KC._grads([y, skip], [dy, ds], KC._leaves(*ins))
    return dict(c=c, x=x, ln=ln, y=y, skip=skip, dy=dy, ds=ds, got=got, labelled=_labelled(["dx", "dgamma", "dbeta"], ins, got, y))


def _ln_verify(cmp, r):
    ln = r["ln"]
    KC.verify_layernorm(cmp, r["x"], ln.weight, ln.bias, ln.eps, r["y"], r["skip"], r["dy"], r["ds"], r["got"])


def _hip_node(y, *names):
    return y.grad_fn is not None and any(n in type(y.grad_fn).__name__ for n in names)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M,C", [(3, 512), (5, 1024)], ids=["two-vectors-512", "widest-1024"])
def test_layer_norm_inside(M, C, dtype):
    from acr_wsss_amd import ops
    r = _ln_run(LNC(M, C, dtype), DEV)
    assert ops.layer_norm_fusable(r["x"], r["ln"]) and _hip_node(r["y"], "LayerNormFn")
    cmp = KC.Cmp()
    _ln_verify(cmp, r)
    _passes(cmp)


LN_OUT = {"c1280-over-1024": (3, 1280, "rows"), "c384-not-a-multiple-of-256": (3, 384, "rows"), "c192": (3, 192, "rows"),
          "every-other-column": (3, 256, "every-other-column"), "align-off4": (3, 512, "off4")}


@pytest.mark.parametrize("how", ["layer_norm", "layer_norm_skip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", _ids(LN_OUT))
def test_layer_norm_outside(name, dtype, how):
    from acr_wsss_amd import ops
    M, C, layout = LN_OUT[name]
    c = LNC(M, C, dtype, how, layout)
    r, _ = _outside(lambda dev: _ln_run(c, dev), _ln_verify, (), ("layer_norm", "ops", how))
    assert not ops.layer_norm_fusable(r["x"], r["ln"]) and not _hip_node(r["y"], "LayerNormFn")


# ------------------------------------------------------------------------------------------------
# linear_f32_usable behind ops.linear_or_hip
# ------------------------------------------------------------------------------------------------
LinC = namedtuple("LinC", "M K N math layout", defaults=(0, "rows"))


def _lin_run(c, dev):
    from acr_wsss_amd import ops
    g = _gen(c)
    x = _layout(_t(g, (c.M, c.K), dev=dev), c.layout)
    lin = nn.Linear(c.K, c.N).to(dev)
    with torch.no_grad():
        lin.weight.copy_(_t(g, (c.N, c.K), scale=c.K ** -0.5, grad=False, dev=dev))
        lin.bias.copy_(_t(g, (c.N,), grad=False, dev=dev))
    r = _t(g, (c.M, c.N), dev=dev)
    y = ops.linear_or_hip(x, lin, r, True, math=c.math)
    dy = _t(g, y.shape, grad=False, dev=dev)
    ins = [x, lin.weight, lin.bias, r]
    got = KC._grads([y], [dy], KC._leaves(*ins))
    return dict(c=c, x=x, lin=lin, r=r, y=y, dy=dy, got=got, labelled=_labelled(["dx", "dW", "db", "dresid"], ins, got, y))


def _lin_verify(cmp, r):
    KC.verify_linear(cmp, r["x"], r["lin"].weight, r["lin"].bias, r["r"], r["y"], r["dy"], r["got"])


@pytest.mark.parametrize("math", [0, 1])
def test_linear_inside_k36_n36(math):
    """K = N = 36: multiples of 4 that are no multiple of 8 or 32, three rows.  ((1, 32, 32): test_gemm_f32_linear.)"""
    from acr_wsss_amd import ops
    r = _lin_run(LinC(3, 36, 36, math), DEV)
    assert ops.linear_f32_usable(r["x"], r["lin"].weight) and _hip_node(r["y"], "LinearF32Fn")
    cmp = KC.Cmp()
    _lin_verify(cmp, r)
    _passes(cmp)


LIN_OUT = {"k28-under-32": (3, 28, 36, "rows"), "k34-not-a-multiple-of-4": (3, 34, 36, "rows"), "n30": (3, 36, 30, "rows"),
           "align-off4": (3, 36, 36, "off4")}


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("name", _ids(LIN_OUT))
def test_linear_outside(name, math):
    from acr_wsss_amd import ops
    M, K, N, layout = LIN_OUT[name]
    c = LinC(M, K, N, math, layout)
    r, _ = _outside(lambda dev: _lin_run(c, dev), _lin_verify, (), ("linear", "ops", "linear_or_hip"))
    assert not ops.linear_f32_usable(r["x"], r["lin"].weight) and not _hip_node(r["y"], "LinearF32Fn", "LinearBf16Fn")


# ------------------------------------------------------------------------------------------------
# mlp_fusable / mlp_f32_usable behind Mlp
# ------------------------------------------------------------------------------------------------
MlpC = namedtuple("MlpC", "M D Hd dtype math how")


def _mlp_run(c, dev):
    from acr_wsss_amd import backbone, ops
    g = _gen(c)
    dtype = DT[c.dtype]
    m = backbone.Mlp(c.D, c.Hd).to(dev)
    with torch.no_grad():
        m.fc1.weight.mul_(3.0)                               # pre-activations of O(1): both GELU branches
        m.fc1.bias.copy_(_t(g, (c.Hd,), scale=0.3, grad=False, dev=dev))
        m.fc2.bias.copy_(_t(g, (c.D,), scale=0.3, grad=False, dev=dev))
    m = m.to(dtype)
    m.acr_math = c.math
    x, r = _t(g, (1, c.M, c.D), dtype, dev=dev), _t(g, (1, c.M, c.D), dtype, dev=dev)
    if c.how == "op":
        y = ops.mlp(x, m.fc1, m.fc2, r) if dtype == BF16 else ops.mlp_f32(x, m.fc1, m.fc2, r, c.math)
    else:
        y = m(x, resid=r)
    dy = _t(g, y.shape, dtype, grad=False, dev=dev)
    ps = [m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias]
    got = KC._grads([y], [dy], KC._leaves(x, r, *ps))
    return dict(c=c, m=m, x=x, r=r, ps=ps, y=y, dy=dy, got=got,
                labelled=_labelled(["dx", "dresid", "dW1", "db1", "dW2", "db2"], [x, r] + ps, got, y))


def _mlp_verify(cmp, r):
    KC.verify_mlp(cmp, r["x"], r["r"], r["ps"], r["y"], r["dy"], r["got"], r["c"].math)


@pytest.mark.parametrize("mode", ["bf16-64-64", "f32-32-32-math0", "f32-32-32-math1"])
def test_mlp_inside(mode):
    from acr_wsss_amd import ops
    c = MlpC(5, 64, 64, "bf16", 0, "op") if mode.startswith("bf16") else MlpC(5, 32, 32, "f32", int(mode[-1]), "op")
    r = _mlp_run(c, DEV)
    m = r["m"]
    assert ops.mlp_fusable(r["x"], m.fc1, m.fc2) if c.dtype == "bf16" else ops.mlp_f32_usable(r["x"], m.fc1, m.fc2, r["r"])
    cmp = KC.Cmp()
    _mlp_verify(cmp, r)
    _passes(cmp)


@pytest.mark.parametrize("mode", ["bf16-hidden-96", "f32-hidden-30-math0", "f32-hidden-30-math1"])
def test_mlp_outside(mode):
    """The Linears go one by one through ``linear_or_hip``: those it still covers stay on the GEMM kernels (bf16 fc1, K = 64), the
    others reach F.linear."""
    from acr_wsss_amd import ops
    c = MlpC(5, 64, 96, "bf16", 0, "module") if mode.startswith("bf16") else MlpC(5, 32, 30, "f32", int(mode[-1]), "module")
    r, census = _outside(lambda dev: _mlp_run(c, dev), _mlp_verify, ("mlp", "mlp_f32"), ("linear", "ops", "linear_or_hip"))
    m = r["m"]
    assert not ops.mlp_fusable(r["x"], m.fc1, m.fc2) and not ops.mlp_f32_usable(r["x"], m.fc1, m.fc2, r["r"])
    assert "linear_or_hip" in _launched(census)


# ------------------------------------------------------------------------------------------------
# ln_image_usable behind Block
# ------------------------------------------------------------------------------------------------
def _block_ref(x, blk):
    """x + attn(LN(x)), then + mlp(LN(.)) in the dtype of ``x`` (float64), the attention from KC.attn_ref."""
    p = {k: KC._double_leaf(v) for k, v in blk.named_parameters()}
    D = x.shape[-1]
    h = F.layer_norm(x, (D,), p["norm1.weight"], p["norm1.bias"], blk.norm1.eps)
    o, _ = KC.attn_ref(F.linear(h, p["attn.qkv.weight"], p["attn.qkv.bias"]), blk.attn.num_heads)
    x = x + F.linear(o, p["attn.proj.weight"], p["attn.proj.bias"])
    h = F.layer_norm(x, (D,), p["norm2.weight"], p["norm2.bias"], blk.norm2.eps)
    return x + F.linear(F.gelu(F.linear(h, p["mlp.fc1.weight"], p["mlp.fc1.bias"])), p["mlp.fc2.weight"], p["mlp.fc2.bias"]), p


@pytest.mark.parametrize("hidden", [32, 28], ids=["inside-hidden-32", "outside-hidden-28"])
def test_block_ln_image(hidden):
    """A Block of dim 256 with 4 heads under split products.  Hidden size 32: both norms leave as operand images (layer_norm_image,
    mlp_f32 with an image).  Hidden size 28 (under the 32 columns a split-product Linear needs): the non-image branch of
    Block.forward -- HIP LayerNorm and attention Linears, the MLP's two Linears on F.linear.  Output and every gradient against
    float64 at the sum of the bounds of the chain's links in KC.TOL (LN -> qkv image, attention gradient, proj Linear, LN -> MLP
    image): each link may add its own bound to what the next one receives."""
    from acr_wsss_amd import backbone, ops
    g = _gen("block", hidden)
    blk = backbone.set_math(backbone.Block(256, 4, mlp_ratio=hidden / 256).to(DEV), 1)
    assert blk.mlp.fc1.out_features == hidden
    with torch.no_grad():
        for ln in (blk.norm1, blk.norm2):
            ln.weight.copy_(_t(g, (256,), scale=0.2, offset=1.0, grad=False))
            ln.bias.copy_(_t(g, (256,), scale=0.3, grad=False))
    x = _t(g, (2, 5, 256), scale=2.0, offset=0.5)
    inside = hidden == 32
    assert ops.ln_image_usable(x, blk.norm1, blk.attn.qkv, 1)
    assert ops.ln_image_usable(x, blk.norm2, blk.mlp.fc1, 1) == inside and ops.mlp_f32_usable(x, blk.mlp.fc1, blk.mlp.fc2) == inside
    params = list(blk.parameters())

    def run():
        y = blk(x)
        dy = _t(g, y.shape, grad=False)
        return y, dy, KC._grads([y], [dy], [x] + params)
    (y, dy, got), census, sites = _watch(run)
    names = _launched(census)
    if inside:
        assert {"layer_norm_image", "mlp_f32", "attention_core_oimg"} <= names and "layer_norm_skip" not in names, names
        assert not sites, sites
    else:
        assert not ({"layer_norm_image", "mlp_f32", "mlp"} & names) and {"layer_norm_skip", "attention_core_oimg"} <= names, names
        assert sites == [("linear", "ops", "linear_or_hip")], sites
    xr = KC._double_leaf(x)
    ref, p = _block_ref(xr, blk)
    want = KC._grads([ref], [dy], [xr] + [p[k] for k, _ in blk.named_parameters()])
    t = KC.TOL
    tol = dict(tol=t["ln_image"]["linear"]["tol"] + t["attention"][F32]["dqkv"]["tol"] + t["linear"][F32]["y"]["tol"] + t["ln_image"]["mlp"]["tol"])
    cmp = KC.Cmp()
    cmp.check("y", y, ref, **tol)
    for n, a, b in zip(["dx"] + ["d " + k for k, _ in blk.named_parameters()], got, want):
        cmp.check(n, a, b, **tol)
    _passes(cmp)


# ------------------------------------------------------------------------------------------------
# tokens_fusable behind VisionTransformer.embed_tokens
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,h,w,P", [(2, 40, 3, 5, 8), (1, 33, 1, 1, 1)], ids=["prefix-8", "one-patch-d33"])
def test_tokens_inside(B, D, h, w, P):
    from acr_wsss_amd import ops
    g = _gen("tokens", B, D, h, w, P)
    y, bias, prefix, pos = _t(g, (B, D, h, w)), _t(g, (D,)), _t(g, (P, D)), _t(g, (1, P + h * w, D))
    assert ops.tokens_fusable(y, bias, prefix, pos)
    tok = ops.tokens(y, bias, prefix, pos)
    dt = _t(g, tok.shape, grad=False)
    cmp = KC.Cmp()
    KC.verify_tokens(cmp, y, bias, prefix, pos, tok, dt, KC._grads([tok], [dt], [y, bias, prefix, pos]))
    _passes(cmp)


class _PatchGrid(nn.Module):
    """Stands in for the ResNetV2 stem in front of the token assembly: every 16th pixel of a 64-channel image."""
    num_features = 64

    def forward(self, x, taps=None):
        return x[:, :, ::16, ::16].contiguous()


def _vit(g, P, table_side, D=64):
    """A one-block hybrid VisionTransformer whose prefix has P rows and whose position table is that of a table_side^2 grid."""
    from acr_wsss_amd import backbone
    vit = backbone.VisionTransformer(embed_dim=D, depth=1, num_heads=1, hybrid=False, img_size=16 * table_side, num_classes=2, in_chans=64)
    vit.patch_embed = backbone.HybridEmbed(_PatchGrid(), D)
    vit.num_tokens = vit.start_index = P
    vit.cls_token = nn.Parameter(_t(g, (1, P, D), grad=False, dev="cpu"))
    vit.pos_embed = nn.Parameter(_t(g, (1, P + table_side ** 2, D), grad=False, dev="cpu"))
    with torch.no_grad():
        vit.patch_embed.proj.bias.copy_(_t(g, (D,), grad=False, dev="cpu"))
    return vit.to(DEV)


@pytest.mark.parametrize("P,table_side", [(9, 4), (0, 4), (1, 3)], ids=["prefix-9", "prefix-0", "table-of-a-3x3-grid"])
def test_tokens_outside(P, table_side):
    """The token assembly of VisionTransformer.embed_tokens on a 4 x 4 patch grid, checked on the very tensors the dispatch saw (y is
    the projection's output): against the fp32 chain bit for bit and against float64.  9 prefix rows (the kernel holds 8) and none
    (an empty prefix has no address) take the torch chain.  A position table of another grid is refused as it stands; the module
    resizes it first (the bilinear branch of ``_resize_pos_embed``) and the RESIZED table is one the kernel takes -- the census shows
    that launch, and the gradient reaches the stored table through the resize."""
    from acr_wsss_amd import ops
    g = _gen("vit-tokens", P, table_side)
    vit = _vit(g, P, table_side)
    img = _t(g, (2, 64, 64, 64), grad=False)
    seen = {}
    fusable = ops.tokens_fusable

    def spy(y, bias, prefix, pos):
        for t in (y, bias, prefix, pos):
            if t.requires_grad and not t.is_leaf:
                t.retain_grad()
        seen["args"], seen["ok"] = (y, bias, prefix, pos), fusable(y, bias, prefix, pos)
        return seen["ok"]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "tokens_fusable", spy)
        (tok, _), census, _ = _watch(lambda: vit.embed_tokens(img))
    y, bias, prefix, pos = seen["args"]
    assert tok.shape == (2, P + 16, 64) and prefix.shape[0] == P
    recs = [dict(r.args)["pos"].shape for r in census.records if r.name == "tokens"]
    if table_side == 4:
        assert not seen["ok"] and not recs, recs
    else:
        assert not fusable(y, bias, prefix, vit.pos_embed) and seen["ok"] and recs == [(1, 17, 64)], recs
    dt = _t(g, tok.shape, grad=False)
    (tok.double() * dt.double()).sum().backward()
    # the prefix is the class-token parameter's rows (the torch chain reads the parameter itself); none at P = 0
    got = [y.grad, bias.grad] + ([vit.cls_token.grad[0]] if P else []) + [pos.grad]
    cmp = KC.Cmp()
    KC.verify_tokens(cmp, y, bias, prefix if P else prefix.detach(), pos, tok, dt, got)
    _passes(cmp)
    assert vit.pos_embed.grad is not None and vit.pos_embed.grad.shape == vit.pos_embed.shape and bool(vit.pos_embed.grad.abs().sum() > 0)
