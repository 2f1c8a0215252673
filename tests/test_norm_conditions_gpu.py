"""The norm kernels on ill-conditioned statistics: fp32 and bf16 GroupNorm, LayerNorm (plain, with the skip gradient, and leaving as
its Linear's operand image) and weight standardisation on the cases of tests/norm_conditions.py -- offsets far above the spread,
single outliers at the places a shifted or partial sum could hang on (the first and the last element of a group, the first pixel
of every channel, the first element of every part of the small launches), constant groups, rows scaled to 2^-60 and 2^50.

Tolerance (``norm_conditions.rule``): per compared quantity the device error against float64 may be at most
max(2 x the error of torch's CPU result in the same storage type on the same inputs, the existing kernel_checks.TOL entry); every
case prints the device error, torch's error and their ratio.  Two quantities have no torch comparator: the forward of a constant
group or row is held to one rounding of the mean amplified by rstd (``_constant_elementwise``); its backward is asserted finite
and repeatable only -- the float64 xhat is exactly 0 there, so d(gamma) has an all-zero reference, and a mean that is off by that
one rounding (sum * (1 / n) is not v for every n) moves the device's xhat by rstd times as much.  And the constant filter of the weight standardisation, whose w_hat is exactly 0 and whose backward is only asserted finite, because
the float64 reference's own gradient is NaN at std = 0."""
import pytest
import torch

import kernel_checks as KC
import norm_conditions as NC
import variant_rules as VR

pytestmark = pytest.mark.gpu

F32, BF16 = NC.F32, NC.BF16
DEV = "cuda:0"


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")


def _dev(t, dtype, grad=True):
    return t.to(DEV).to(dtype).requires_grad_(grad) if t is not None else None


def _finish(cmp, where, terrs=None):
    for label, err, scale in cmp.log:
        te = (terrs or {}).get(label)
        print("%s %s: device err %.3e, torch err %s, ratio %s, max|ref| %.3e"
              % (where, label, err, "%.3e" % te if te is not None else "-", "%.2f" % (err / max(te, 1e-300)) if te is not None else "-", scale))
    assert not cmp.failures, "\n".join(cmp.failures)


def _gn_tols(case, forward_only=False):
    """(tols, torch's errors) of a GroupNorm case by the module's rule"""
    base = NC.gn_base(case, forward_only)
    if case["cond"] == "constant":
        return dict(base, y=dict(atol=NC.gn_constant_bound(case, NC.floor_of(base["y"], case["ref"]["y"])))), {}
    return NC.rule(case, base, only=("y",) if forward_only else None, tol_only=NC.gn_tol_only(case["cond"], case["dtype"]))


def _gn_device(case, act, dtype, ops):
    x, w, b, r = (_dev(case[k], dtype) for k in ("x", "w", "b", "r"))
    dy = _dev(case["dy"], dtype, False)
    assert ops.groupnorm_fusable(x, r)
    y = ops.groupnorm_act(x, w, b, act, r)
    y.saved_mask_dtype = y.grad_fn.saved_tensors[4].dtype if r is not None else None      # (freed by the backward)
    (y.float() * dy.float()).sum().backward()
    return x, w, b, r, dy, y


def _grads_or_none(case, *leaves):
    """the gradients a check compares: none on a constant group or row (module docstring), where they must be finite"""
    if case["cond"] != "constant":
        return KC.grads_of(*leaves)
    assert all(bool(torch.isfinite(t.grad).all()) for t in leaves if t is not None)
    return []


def _constant_elementwise(case, y, eps, base_y):
    """A constant group or row, forward: |y - ref| <= 2 * 2^-23 |v| rstd max|gamma| + the TOL entry, element by element (v: the
    element's own group value; rstd = eps^-1/2)."""
    ref = case["ref"]["y"].double()
    bound = 2 * 2.0 ** -23 * case["x"].double().abs() * eps ** -0.5 * float(case["w"].abs().max()) + NC.floor_of(base_y, ref)
    assert bool(((y.detach().cpu().double() - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------
# fp32 GroupNorm
# ------------------------------------------------------------------------------------------------
GN_GRAD_CASES = [(s, c) for s, c in NC.gn_f32_cases() if NC.GN_F32_SHAPES[s][0][0] != "parts"]
GN_PARTS_CASES = [(s, c) for s, c in NC.gn_f32_cases() if NC.GN_F32_SHAPES[s][0][0] == "parts"]


@pytest.mark.parametrize("act", NC.ACTS)
@pytest.mark.parametrize("shape,cond", GN_GRAD_CASES, ids=_ids)
def test_groupnorm_f32(shape, cond, act, monkeypatch):
    from acr_wsss_amd import ops
    N, C, H, W = shape
    fwd, bwd, _ = NC.GN_F32_SHAPES[shape]
    assert VR.gnf_fwd_variant(N, C, H * W, False) == fwd and VR.gnf_bwd_variant(N, C, H * W) == bwd
    case = NC.gn_case(shape, cond, act, F32)
    tols, terrs = _gn_tols(case)
    x, w, b, r, dy, y = _gn_device(case, act, F32, ops)
    cmp = KC.Cmp()
    KC.verify_groupnorm(cmp, x, w, b, r, act, y, dy, _grads_or_none(case, x, w, b, r), NC.GN_EPS, tols=tols)
    _finish(cmp, "gn f32 %s %s %s" % (_ids(shape), cond, act), terrs)
    if cond == "constant":
        _constant_elementwise(case, y, NC.GN_EPS, NC.gn_base(case)["y"])
    # deterministic: a second run gives the same bits
    x2, w2, b2, r2, _, y2 = _gn_device(case, act, F32, ops)
    assert torch.equal(y2, y) and torch.equal(x2.grad, x.grad) and torch.equal(w2.grad, w.grad) and torch.equal(b2.grad, b.grad)
    if cond == "first" and act == "add_relu":               # the mask path and the residual path take the same decisions
        monkeypatch.setattr(ops, "GN_RELU_MASK", False)
        x3, w3, b3, r3, _, y3 = _gn_device(case, act, F32, ops)
        assert y3.saved_mask_dtype == torch.float32 and y.saved_mask_dtype == torch.uint8
        for a, c in ((y3, y), (x3.grad, x.grad), (r3.grad, r.grad), (w3.grad, w.grad), (b3.grad, b.grad)):
            assert torch.equal(a, c)


@pytest.mark.parametrize("act", NC.ACTS)
@pytest.mark.parametrize("shape,cond", GN_PARTS_CASES, ids=_ids)
def test_groupnorm_f32_small_launch_parts(shape, cond, act):
    """The gradient-free forward that cuts every (sample, group) into parts; part_first puts an outlier at each part's start."""
    from acr_wsss_amd import _lib, ops
    N, C, H, W = shape
    P, vper = NC.gn_parts(shape)
    nws = _lib.load().acr_groupnorm_fwd_ws_floats(N, C, H * W)
    assert nws > 0 and nws == N * 32 * 2 * P and VR.gnf_fwd_variant(N, C, H * W, True) == NC.GN_F32_SHAPES[shape][0] == ("parts", P)
    case = NC.gn_case(shape, cond, act, F32, (P, vper) if cond == "part_first" else None)
    tols, terrs = _gn_tols(case, forward_only=True)
    x, w, b, r = (_dev(case[k], F32, False) for k in ("x", "w", "b", "r"))
    with torch.no_grad():
        y = ops.groupnorm_act(x, w, b, act, r)
        assert torch.equal(y, ops.groupnorm_act(x, w, b, act, r))
    cmp = KC.Cmp()
    ref = KC.verify_groupnorm(cmp, x, w, b, r, act, y, None, [], NC.GN_EPS, tols=tols)
    _finish(cmp, "gn f32 parts %s %s %s" % (_ids(shape), cond, act), terrs)
    y1 = ops.groupnorm_act(x.clone().requires_grad_(True), w, b, act, r)       # one workgroup per (sample, group)
    assert (y - y1).abs().max() <= KC.TOL["groupnorm_forward_only"] * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------
# bf16 GroupNorm
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", NC.ACTS)
@pytest.mark.parametrize("shape,cond", [(s, c) for s, cs in NC.GN_BF16_SHAPES.items() for c in cs], ids=_ids)
def test_groupnorm_bf16(shape, cond, act):
    from acr_wsss_amd import ops
    case = NC.gn_case(shape, cond, act, BF16)
    tols, terrs = _gn_tols(case)
    x, w, b, r, dy, y = _gn_device(case, act, BF16, ops)
    cmp = KC.Cmp()
    KC.verify_groupnorm(cmp, x, w, b, r, act, y, dy, _grads_or_none(case, x, w, b, r), NC.GN_EPS, tols=tols)
    _finish(cmp, "gn bf16 %s %s %s" % (_ids(shape), cond, act), terrs)
    if cond == "constant":
        _constant_elementwise(case, y, NC.GN_EPS, NC.gn_base(case)["y"])


# ------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------
def _ln_module(case, C, dtype):
    ln = torch.nn.LayerNorm(C, eps=NC.LN_EPS).to(DEV).to(dtype)
    with torch.no_grad():
        ln.weight.copy_(case["w"])
        ln.bias.copy_(case["b"])
    return ln


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
@pytest.mark.parametrize("cond", NC.LN_CONDITIONS)
@pytest.mark.parametrize("C", NC.LN_WIDTHS)
def test_layernorm_with_skip(C, cond, dtype):
    from acr_wsss_amd import ops
    case = NC.ln_case(NC.LN_ROWS, C, cond, dtype)
    base = NC.ln_base(case)
    if cond == "constant":
        tols, terrs = dict(base, y=dict(atol=NC.ln_constant_bound(case, NC.floor_of(base["y"], case["ref"]["y"])))), {}
    else:
        tols, terrs = NC.rule(case, base)
    x, dy, ds = _dev(case["x"], dtype), _dev(case["dy"], dtype, False), _dev(case["ds"], dtype, False)
    ln = _ln_module(case, C, dtype)
    assert ops.layer_norm_fusable(x, ln)
    y, skip = ops.layer_norm_skip(x, ln)
    assert "LayerNormFn" in type(y.grad_fn).__name__
    ((y.float() * dy.float()).sum() + (skip.float() * ds.float()).sum()).backward()
    cmp = KC.Cmp()
    KC.verify_layernorm(cmp, x, ln.weight, ln.bias, ln.eps, y, skip, dy, ds, _grads_or_none(case, x, ln.weight, ln.bias), tols=tols)
    _finish(cmp, "ln %s %d %s" % (_ids(dtype), C, cond), terrs)
    if cond == "constant":
        _constant_elementwise(case, y, NC.LN_EPS, base["y"])


@pytest.mark.parametrize("cond", NC.LN_IMAGE_CONDITIONS)
def test_layernorm_image_with_linear_consumer(cond):
    """LayerNorm leaving as the split-product operand image of the Linear behind it (math 1), judged as that composite."""
    from acr_wsss_amd import ops
    M, C, nout = NC.LN_IMAGE
    case = NC.ln_case(M, C, cond, F32, nout)
    tols, terrs = NC.rule(case, NC.ln_image_base(case))
    x, dz, ds = _dev(case["x"], F32), _dev(case["dz"], F32, False), _dev(case["ds"], F32, False)
    ln = _ln_module(case, C, F32)
    lin = torch.nn.Linear(C, nout).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(case["lin"][0])
        lin.bias.copy_(case["lin"][1])
    assert ops.ln_image_usable(x, ln, lin, 1)
    h, skip, hi = ops.layer_norm_image(x, ln)
    y = ops.linear_or_hip(h, lin, None, True, math=1, x_image=hi)
    ((y * dz).sum() + (skip * ds).sum()).backward()
    got = [x.grad, ln.weight.grad, ln.bias.grad, lin.weight.grad, lin.bias.grad]
    cmp = KC.Cmp()
    KC.verify_ln_consumer(cmp, x, ln, "linear", [lin.weight, lin.bias], y, dz, skip, ds, got, tols=tols)
    _finish(cmp, "ln image %s" % cond, terrs)


# ------------------------------------------------------------------------------------------------
# weight standardisation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
def test_weight_std(dtype):
    """All three filter shapes in one launch; every condition judged on its own channels.  The constant filter: w_hat is exactly
    0; its gradient is only asserted finite -- the float64 reference's own gradient is NaN there (d std / d w at std = 0)."""
    from acr_wsss_amd import ops
    case = NC.ws_case(NC.WS_CONDITIONS[0], dtype)
    ws = [_dev(w, dtype) for w in case["ws"]]
    gs = [_dev(g, dtype, False) for g in case["gs"]]
    outs = ops.weight_std_all(ws)
    tr = ops.WeightStdAllFn.last_transposed                  # bf16 1x1 filters also leave as (cin, cout) from the same launch
    assert [t is not None for t in tr] == [False, dtype == BF16, dtype == BF16]
    if dtype == BF16:
        assert torch.equal(tr[1], outs[1].reshape(64, 64).t()) and torch.equal(tr[2], outs[2].reshape(33, 5).t())
    sum((o.float() * g.float()).sum() for o, g in zip(outs, gs)).backward()
    for cond in NC.WS_CONDITIONS:
        case = NC.ws_case(cond, dtype)
        tols, terrs = NC.rule(case, NC.ws_base(case))
        cmp = KC.Cmp()
        KC.verify_weight_std(cmp, ws, outs, gs, KC.grads_of(*ws), NC.WS_EPS, tols=tols, keep=[k.to(DEV) for k in case["keep"]])
        _finish(cmp, "weight_std %s %s" % (_ids(dtype), cond), terrs)
    for w, o in zip(ws, outs):
        assert float(o[-1].abs().max()) == 0.0 and bool(torch.isfinite(w.grad[-1]).all())
