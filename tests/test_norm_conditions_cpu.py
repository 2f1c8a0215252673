"""tests/norm_conditions.py without a GPU: the cases are what they say and decide what tests/test_norm_conditions_gpu.py asks.

For every (kernel, shape, condition) of the GPU file: the references are finite, an outlier lies at least the stated number of
standard deviations from the mean of the rest of its group (float64), and torch's own fp32 error against float64 is at most 5e-5
of max|reference| -- ``norm_conditions.rule`` asserts that cap wherever it forms a tolerance, so the rule max(2 x torch's error,
the existing TOL entry) never grants more than 1e-4 of the maximum.  And the cases tell an accurate GroupNorm from the shifted
one-pass statistics the fp32 forward once used: a restatement of those fails ``first`` and passes ``offset``."""
import pytest
import torch

import norm_conditions as NC
import variant_rules as VR

F32, BF16 = NC.F32, NC.BF16


def _check_outliers(case, rows, sigmas):
    if case["cols"]:
        assert NC.outlier_sigmas(rows, case["cols"]) >= sigmas
        others = torch.ones(rows.shape[1], dtype=torch.bool)
        others[case["cols"]] = False
        assert float(rows[:, others].double().std(1).max()) < 1e3      # the rest is ordinary data


@pytest.mark.parametrize("shape,cond", NC.gn_f32_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_groupnorm_f32_cases(shape, cond):
    N, C, H, W = shape
    fwd, bwd, _ = NC.GN_F32_SHAPES[shape]
    assert VR.gnf_fwd_variant(N, C, H * W, fwd[0] == "parts") == fwd
    assert bwd is None or VR.gnf_bwd_variant(N, C, H * W) == bwd
    parts = NC.gn_parts(shape) if cond == "part_first" else None
    # every act on the small shapes, the plain norm on the large ones (the GPU file forms the other tolerances, cap included)
    for act in (NC.ACTS if C * H * W <= 256 * 28 * 28 else ("none",)):
        case = NC.gn_case(shape, cond, act, F32, parts)
        if cond == "constant":
            assert torch.isfinite(case["ref"]["y"]).all() and len(set(case["x"].reshape(N * 32, -1)[:, 0].tolist())) == min(N * 32, len(NC.DYADIC))
            assert bool((case["x"].reshape(N * 32, -1) == case["x"].reshape(N * 32, -1)[:, :1]).all())
            continue
        NC.rule(case, NC.gn_base(case, fwd[0] == "parts"), only=("y",) if fwd[0] == "parts" else None, tol_only=NC.gn_tol_only(cond))
        _check_outliers(case, case["x"].reshape(N * 32, -1), NC.gn_sigmas(cond))
        if cond in NC.GN_FIRST_SIGMAS:                       # on its side of the kernel's switch, in every group
            xs = case["x"].reshape(N * 32, -1).double()
            rho = (xs.mean(1) - xs[:, 0]) ** 2 / ((xs - xs[:, :1]) ** 2).mean(1)
            assert bool((rho < VR.GNF_SHIFT_FAR - 0.01).all()) if cond == "first_4" else bool((rho > VR.GNF_SHIFT_FAR + 0.01).all())
    if cond == "part_first":
        P, vper = parts
        assert P == fwd[1] and case["cols"] == [4 * p * vper for p in range(P)] and case["cols"][-1] < (C // 32) * H * W


@pytest.mark.parametrize("shape", sorted(NC.GN_BF16_SHAPES))
def test_groupnorm_bf16_cases(shape):
    for cond in NC.GN_BF16_SHAPES[shape]:
        for act in NC.ACTS:
            case = NC.gn_case(shape, cond, act, BF16)
            assert all(torch.isfinite(v).all() for v in case["ref"].values())
            assert torch.equal(case["x"], case["x"].bfloat16().float())
            if cond != "constant":
                NC.rule(case, NC.gn_base(case))
                _check_outliers(case, case["x"].reshape(shape[0] * 32, -1), NC.GN_SIGMAS)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cond", NC.LN_CONDITIONS)
@pytest.mark.parametrize("C", NC.LN_WIDTHS)
def test_layernorm_cases(C, cond, dtype):
    case = NC.ln_case(NC.LN_ROWS, C, cond, dtype)
    assert all(torch.isfinite(v).all() for v in case["ref"].values())
    if cond != "constant":
        NC.rule(case, NC.ln_base(case))
    _check_outliers(case, case["x"], NC.LN_SIGMAS)
    if cond == "tiny":
        assert 0 < float(case["x"].abs().max()) < 2.0 ** -55
    if cond == "huge":
        assert float(case["x"].abs().max()) > 2.0 ** 50


@pytest.mark.parametrize("cond", NC.LN_IMAGE_CONDITIONS)
def test_layernorm_image_cases(cond):
    M, C, nout = NC.LN_IMAGE
    case = NC.ln_case(M, C, cond, F32, nout)
    NC.rule(case, NC.ln_image_base(case))
    _check_outliers(case, case["x"], NC.LN_SIGMAS)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cond", NC.WS_CONDITIONS)
def test_weight_std_cases(cond, dtype):
    case = NC.ws_case(cond, dtype)
    NC.rule(case, NC.ws_base(case))
    for w, k in zip(case["ws"], case["keep"]):
        rows = w.reshape(w.shape[0], -1)
        assert len(k) >= 10 and int(k.max()) < w.shape[0] - 1
        if cond == "far_mean":
            far = rows[k].double()
            assert float((far.mean(1) / far.std(1)).min()) > (10 if dtype == BF16 else 40)      # a mean far above the std
        if cond == "outlier":
            assert NC.outlier_sigmas(rows[k], [0]) >= NC.WS_SIGMAS
        assert bool((rows[-1] == rows[-1, 0]).all())                  # the constant filter: its float64 w_hat is exactly 0
        assert float(NC.ws_expr(w.double())[-1].abs().max()) == 0.0


def _one_pass_error(cond):
    shape = (1, 256, 28, 28)                                  # groups of 8 x 784
    case = NC.gn_case(shape, cond, "none", F32)
    tols, terrs = NC.rule(case, NC.gn_base(case), only=("y",))
    y = NC.shifted_one_pass_gn(case["x"], case["w"], case["b"])
    return float((y.double() - case["ref"]["y"]).abs().max()), tols["y"]["atol"], terrs["y"]


def test_the_cases_catch_shifted_one_pass_statistics():
    """sum(x - x0), sum((x - x0)^2) about the group's first element and m2 - m1^2 in fp32: fine against a common offset, wrong
    by far more than the rule allows once that first element is an outlier."""
    err, bound, terr = _one_pass_error("offset")
    print("offset: one-pass error %.3e, torch %.3e, bound %.3e" % (err, terr, bound))
    assert err <= bound
    err, bound, terr = _one_pass_error("first")
    print("first: one-pass error %.3e, torch %.3e, bound %.3e" % (err, terr, bound))
    assert err > 4 * bound
    for cond in ("first_offset", "channel_first"):
        err, bound, _ = _one_pass_error(cond)
        assert err > bound, cond
    err, bound, _ = _one_pass_error("last")                   # the shift is ordinary data: the outlier is one large square
    assert err <= bound
