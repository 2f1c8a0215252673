"""The DPT decoder off the GPU: the float64 restatement tests/decoder_ref.py against torch's float64 autograd and against the
reference's own fusion-block results (tests/golden/decoder_block_{a,b}.npz, written by tests/golden/make_decoder_golden.py), the
state-dict layouts of ``ACR(..., seg=True)`` against the reference's (state_dict_layout_seg_*.json), ``seg=False`` unchanged, and
the argument handling of acr_wsss_amd/decoder.py (no CPU path, unsupported configurations)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import decoder_ref as R
from conftest import GOLDEN, load_golden

RTOL = 1e-11                                                 # float64 against float64: summation order only


def _close(got, want, what, rtol=RTOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= rtol * max(np.abs(want).max(), 1e-300), (what, err, np.abs(want).max())


# ------------------------------------------------------------------------------------------------
# the restatement against torch's float64 autograd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("nres", [0, 1, 2])
def test_batchnorm_restatement_against_torch_float64(training, relu, nres):
    rng = np.random.default_rng(5 + nres)
    shape = (3, 5, 9, 4)
    x, dy = rng.standard_normal(shape), rng.standard_normal(shape)
    res = [rng.standard_normal(shape) for _ in range(nres)]
    gamma, beta = 1 + 0.1 * rng.standard_normal(5), 0.1 * rng.standard_normal(5)
    rm, rv = 0.2 * rng.standard_normal(5), 0.5 + rng.random(5)
    bn = nn.BatchNorm2d(5, momentum=0.3).double().train(training)
    with torch.no_grad():
        for t, v in ((bn.weight, gamma), (bn.bias, beta), (bn.running_mean, rm), (bn.running_var, rv)):
            t.copy_(torch.from_numpy(v))
    xt = torch.from_numpy(x).requires_grad_(True)
    rt = [torch.from_numpy(r).requires_grad_(True) for r in res]
    pre = bn(xt) + sum(rt) if rt else bn(xt)
    yt = F.relu(pre) if relu else pre
    yt.backward(torch.from_numpy(dy))
    f = R.bn_fwd(x, gamma, beta, rm, rv, training, 0.3, bn.eps, relu, *(res + [None, None])[:2])
    _close(f["y"], yt.detach().numpy(), "y")
    _close(f["running_mean"], bn.running_mean.numpy(), "running_mean")
    _close(f["running_var"], bn.running_var.numpy(), "running_var")
    dx, dgamma, dbeta, dres = R.bn_bwd(x, gamma, f["mean"], f["invstd"], dy, training, mask=(f["pre"] > 0) if relu else None)
    _close(dx, xt.grad.numpy(), "dx", 1e-10)
    _close(dgamma, bn.weight.grad.numpy(), "dgamma", 1e-10)
    _close(dbeta, bn.bias.grad.numpy(), "dbeta", 1e-10)
    for r in rt:
        _close(dres, r.grad.numpy(), "dres")
    if training:
        assert not np.array_equal(f["running_mean"], rm)
    else:
        assert np.array_equal(f["running_mean"], rm) and np.array_equal(f["running_var"], rv)


def test_batchnorm_restatement_refuses_one_value_per_channel():
    with pytest.raises(ValueError):
        R.bn_fwd(np.zeros((1, 3, 1, 1)), np.ones(3), np.zeros(3))
    R.bn_fwd(np.zeros((1, 3, 1, 1)), np.ones(3), np.zeros(3), np.zeros(3), np.ones(3), training=False)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (2, 5, 1, 9), (2, 5, 9, 1), (1, 2, 33, 70)])
def test_upsampling_restatement_against_torch(shape):
    """The taps are computed in fp32; torch's float64 result computes them in float64.  The source index differs by its fp32
    rounding (up to 8e-6 of a pixel at index 69), times a difference of neighbours of a few max|x|: 5e-5 max|x|.  The backward is
    the exact adjoint of the forward."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal(shape)
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=True)
    dy = rng.standard_normal(yt.shape)
    yt.backward(torch.from_numpy(dy))
    y = R.upsample2x(x)
    assert np.abs(y - yt.detach().numpy()).max() <= 5e-5 * np.abs(x).max()
    assert np.abs(R.upsample2x_bwd(dy) - xt.grad.numpy()).max() <= 5e-5 * 4 * np.abs(dy).max()
    # adjoint: <up(x), dy> == <x, up^T(dy)>
    a, b = float((y * dy).sum()), float((x * R.upsample2x_bwd(dy)).sum())
    assert abs(a - b) <= 1e-12 * max(abs(a), 1.0)
    # and the fp32 taps are torch's fp32 taps: on an index ramp the fp32 result is reproduced to an fp32 ulp
    ramp = np.arange(shape[3], dtype=np.float64)[None, None, None, :].repeat(shape[2], 2)
    t32 = F.interpolate(torch.from_numpy(ramp).float(), scale_factor=2, mode="bilinear", align_corners=True).numpy()
    assert np.abs(R.upsample2x(ramp) - t32).max() <= 2.0 ** -22 * max(shape[3], 1)


class _TorchRCU(nn.Module):
    """a plain torch composition of blocks.py:277-345 (bn=True), float64"""

    def __init__(self, f):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(f, f, 3, 1, 1, bias=False), nn.Conv2d(f, f, 3, 1, 1, bias=False)
        self.bn1, self.bn2 = nn.BatchNorm2d(f), nn.BatchNorm2d(f)

    def forward(self, x):
        return self.bn2(self.conv2(F.relu(self.bn1(self.conv1(F.relu(x)))))) + x


class _TorchFusion(nn.Module):
    def __init__(self, f):
        super().__init__()
        self.out_conv = nn.Conv2d(f, f, 1)
        self.resConfUnit1, self.resConfUnit2 = _TorchRCU(f), _TorchRCU(f)

    def forward(self, *xs):
        out = xs[0]
        if len(xs) == 2:
            out = out + self.resConfUnit1(xs[1])
        out = self.resConfUnit2(out)
        return self.out_conv(F.interpolate(out, scale_factor=2, mode="bilinear", align_corners=True))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("ninputs", [1, 2])
def test_fusion_block_restatement_against_torch_float64(ninputs, training):
    torch.manual_seed(3)
    f, shape = 4, (2, 4, 5, 7)
    blk = _TorchFusion(f).double()
    with torch.no_grad():
        for k, v in blk.state_dict().items():
            if "running_mean" in k:
                v.copy_(0.2 * torch.randn_like(v))
            elif "running_var" in k:
                v.copy_(0.5 + torch.rand_like(v))
            elif v.dim() == 1 and "bn" in k and v.is_floating_point():
                v.copy_((1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn_like(v))
    p = {k: v.detach().clone().numpy() for k, v in blk.state_dict().items() if v.is_floating_point()}
    blk.train(training)
    xs = [torch.randn(shape, dtype=torch.float64, requires_grad=True) for _ in range(ninputs)]
    out = blk(*xs)
    dy = torch.randn_like(out)
    out.backward(dy)
    got, cache = R.fusion_fwd(p, [x.detach().numpy() for x in xs], training=training)
    # the upsampling's fp32 taps against torch's float64 taps: 4e-6 of the scale
    tol = 2e-5
    _close(got, out.detach().numpy(), "out", tol)
    dxs, grads = R.fusion_bwd(p, cache, dy.numpy())
    for i, x in enumerate(xs):
        _close(dxs[i], x.grad.numpy(), "dx%d" % i, tol)
    for k, prm in blk.named_parameters():
        if prm.grad is not None:
            _close(grads[k], prm.grad.numpy(), k, tol)
    assert len(cache["relu_in"]) == 2 * ninputs
    for k, v in cache["running"].items():
        _close(v, blk.state_dict()[k].numpy(), k, 1e-10)


# ------------------------------------------------------------------------------------------------
# the restatement against the reference's own results
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,mode", [("a", "train"), ("b", "train"), ("b", "eval")])
def test_fusion_block_restatement_against_the_reference_fixture(tag, mode):
    fx = load_golden("decoder_block_" + tag)
    pre = "" if mode == "train" else "eval_"
    stride = int(fx["stride"])
    p = R.block_params(fx)
    xs = [fx["x%d" % i] for i in range(2) if "x%d" % i in fx]
    out, cache = R.fusion_fwd(p, xs, training=(mode == "train"))
    dxs, grads = R.fusion_bwd(p, cache, fx["dy"])
    # the reference's float64 run decides its upsampling taps in float64, the restatement in fp32 (as torch's fp32 kernels and
    # the HIP ones do): they differ by a few 1e-7 of a pixel, so 2e-5 of the maximum here and fp32-level agreement below
    tol = 2e-5
    _close(R.sample(out, stride), fx[pre + "out64"], "out64", tol)
    for i, d in enumerate(dxs):
        _close(R.sample(d, stride), fx[pre + "dx%d_64" % i], "dx%d" % i, tol)
    seen = 0
    for k, v in fx.items():
        if k.startswith(pre + "grad64:"):
            _close(R.sample(grads[k.split(":", 1)[1]], stride), v, k, tol)
            seen += 1
    assert seen == (14 if len(xs) == 2 else 8)
    for k, v in cache["running"].items():
        if mode == "train":
            _close(v, fx["after64:" + k], k, 1e-10)
            assert np.abs(fx["after32:" + k] - v).max() <= 1e-5 * np.abs(v).max()
        else:
            assert np.array_equal(fx["eval_after32:" + k], fx["before:" + k])
    # the fixture's seed was chosen so that no ReLU decision hangs on rounding: restated here from the float64 tensors
    assert len(cache["relu_in"]) == len(fx[pre + "relu_dev32"])
    for r, dev, mn in zip(cache["relu_in"], fx[pre + "relu_dev32"], fx[pre + "relu_min64"]):
        assert abs(np.abs(r).min() - mn) <= 1e-6 * max(mn, 1e-30) + 1e-12
        assert np.abs(r).min() > 8.0 * dev
    # and the reference's fp32 run agrees with its float64 run at fp32 level
    assert np.abs(fx[pre + "out32"] - fx[pre + "out64"]).max() <= 2e-5 * np.abs(fx[pre + "out64"]).max()


# ------------------------------------------------------------------------------------------------
# the model surface
# ------------------------------------------------------------------------------------------------
def _layout(model):
    return {k: list(v.shape) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("tag,name", [("hybrid", "vitb_hybrid"), ("vitb", "vitb"), ("deit", "deit"), ("distil", "deit_distilled")])
def test_seg_true_layout_matches_the_reference(tag, name):
    from acr_wsss_amd.DPT.ACR import ACR
    with open(os.path.join(GOLDEN, "state_dict_layout_seg_%s.json" % tag)) as f:
        want = json.load(f)
    got = _layout(ACR(20, name, seg=True, use_pretrain=False))
    assert list(got) == list(want)                               # the reference's key order too
    assert got == want
    assert any(k.startswith("scratch.refinenet4.resConfUnit2.bn2.running_var") for k in got)


@pytest.mark.parametrize("fn,name", [("state_dict_layout.json", "vitb_hybrid"), ("state_dict_layout_vitb.json", "vitb")])
def test_seg_false_layout_is_unchanged(fn, name):
    from acr_wsss_amd.DPT.ACR import ACR
    with open(os.path.join(GOLDEN, fn)) as f:
        want = json.load(f)
    for kw in ({}, {"seg": False}):
        got = _layout(ACR(20, name, use_pretrain=False, **kw))
        assert got == want and not any("refinenet" in k for k in got)


def test_features_argument_sizes_the_decoder():
    from acr_wsss_amd.DPT.ACR import ACR
    from acr_wsss_amd import decoder as D
    m = ACR(20, "vitb_hybrid", seg=True, features=16, use_pretrain=False)
    assert tuple(m.scratch.refinenet1.resConfUnit1.conv1.weight.shape) == (16, 16, 3, 3)
    assert isinstance(m.scratch.refinenet3, D.FeatureFusionBlock_custom)
    head = D.SegmentationHead(16, 20)
    assert list(head.state_dict()) == ["0.weight", "1.weight", "1.bias", "1.running_mean", "1.running_var", "1.num_batches_tracked",
                                       "4.weight", "4.bias"]
    assert tuple(head[4].weight.shape) == (21, 16, 1, 1) and head[0].bias is None
    m.set_math("f32_split")
    assert m.scratch.refinenet2.resConfUnit2.acr_math == 1 and m.scratch.refinenet2.acr_math == 1


def test_cpu_tensors_raise():
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd._lib import AcrHipError
    from acr_wsss_amd.DPT.ACR import ACR
    x = torch.zeros(2, 4, 3, 3)
    with pytest.raises(AcrHipError):
        D.batch_norm_act(x, nn.BatchNorm2d(4))
    with pytest.raises(AcrHipError):
        D.upsample2x(x)
    with pytest.raises(AcrHipError):
        D.relu(x)
    with pytest.raises(AcrHipError):
        D.FeatureFusionBlock_custom(4, nn.ReLU(False), bn=True)(x)
    with pytest.raises(AcrHipError):
        D.SegmentationHead(4, 3)(x)
    m = ACR(20, "vitb_hybrid", seg=True, features=16, use_pretrain=False)
    with pytest.raises(AcrHipError):
        D.decode(m, torch.zeros(1, 3, 64, 64))


def test_unsupported_configurations_raise():
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd.DPT.ACR import ACR
    act = nn.ReLU(False)
    for kw in (dict(bn=False), dict(bn=True, deconv=True), dict(bn=True, expand=True), dict(bn=True, align_corners=False)):
        with pytest.raises(NotImplementedError):
            D.FeatureFusionBlock_custom(8, act, **kw)
    with pytest.raises(NotImplementedError):
        D.FeatureFusionBlock_custom(8, nn.GELU(), bn=True)
    with pytest.raises(NotImplementedError):
        D.ResidualConvUnit_custom(8, act, False)
    x = torch.zeros(2, 4, 3, 3)
    with pytest.raises(NotImplementedError):
        D.batch_norm_act(x, nn.BatchNorm2d(4, momentum=None))
    with pytest.raises(NotImplementedError):
        D.batch_norm_act(x, nn.BatchNorm2d(4, affine=False))
    with pytest.raises(ValueError):
        D.batch_norm_act(x, nn.BatchNorm2d(4), act="gelu")
    with pytest.raises(ValueError):
        D.batch_norm_act(x, nn.BatchNorm2d(4), resid2=x)
    with pytest.raises(ValueError):
        D.decode(ACR(20, "vit_tiny", use_pretrain=False), torch.zeros(1, 3, 64, 64))          # built without seg=True
    with pytest.raises(NotImplementedError):
        D.decode(ACR(20, "vit_tiny", seg=True, features=16, use_pretrain=False), torch.zeros(1, 3, 64, 64))   # not the hybrid
