"""The pseudo-label segmentation loss on the device (csrc/segloss.hip behind acr_segloss_fwd / acr_segloss_bwd /
acr_dense_energy_dot, acr_wsss_amd/segloss.py) against the float64 restatement tests/segloss_ref.py -- pinned to torch's and the
reference's own CPU results by test_segloss_cpu.py -- and against those results themselves (tests/golden/segloss_{a..c}.npz).

Cross-entropy tolerance: device and torch's CPU fp32 result are both compared with the float64 restatement; the device's error
may be at most 2x the error torch's own fp32 result shows on the same case, with a floor of 4 fp32 ulps (4 * 2^-23) of the largest
reference value.  No absolute number is fixed in advance.  Counts are exact; forward and backward repeat bit for bit.
Energy: AS bit for bit against the reference's C++ lattice; E within the fp32 summation bound K n 2^-24 sum|terms| of the float64
sum; the gradient exactly -2 weight / B * AS."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pseudo_ref as PR
import segloss_ref as R
from kernel_checks import EXACT, Cmp
from acr_wsss_amd import pseudo as P
from acr_wsss_amd import segloss as S
from oracle import crf_oracle as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULPS = 4 * 2.0 ** -23
# (B, K, h, w, W, H): a non-integer ratio with edge clamping; a degenerate source; the identity resize with K above a wave's
# lanes; 70 x 33 = 2310 pixels = 10 partial-sum workgroups of 256 per image
SHAPES = {"a": (2, 21, 5, 7, 37, 41), "b": (1, 2, 1, 1, 3, 2), "k81": (2, 81, 6, 6, 6, 6), "c": (3, 21, 9, 4, 70, 33)}


@functools.lru_cache(maxsize=None)
def case(tag, scale=1, kind="random"):
    """(logits, label) of a shape: the fixture's where one exists, seeded otherwise; treat as read-only"""
    B, K, h, w, W, H = SHAPES[tag]
    if tag in ("a", "b", "c") and kind == "random":
        g = np.load(os.path.join(GOLDEN, "segloss_%s.npz" % tag))
        logits, label = g["logits"], g["label"]
    else:
        rng = np.random.default_rng(31 + len(tag) + 7 * len(kind))
        logits = (2.0 * rng.standard_normal((B, K, h, w))).astype(np.float32)
        label = R.labels_case(rng, B, K, W, H, kind)
    return (logits * np.float32(scale)).astype(np.float32), label


@functools.lru_cache(maxsize=None)
def reference(tag, scale, kind, ba, g=(1.0, 0.0, 0.0)):
    logits, label = case(tag, scale, kind)
    return R.split_ce(logits, label, ba, g=g)


def torch_cpu(logits, label, ba, g=(1.0, 0.0, 0.0), d_probs=None):
    """F.interpolate + the label edit of myTool.py:845-848 + two nn.CrossEntropyLoss(ignore_index=255), fp32 on the CPU"""
    x = torch.from_numpy(logits).clone().requires_grad_(True)
    lab = torch.from_numpy(label.astype(np.int64))
    lab[lab >= logits.shape[1]] = 255
    pred = F.interpolate(x, tuple(label.shape[1:]), mode="bilinear", align_corners=False)
    bg_label, fg_label = lab.clone(), lab.clone()
    bg_label[lab != 0] = 255
    fg_label[lab == 0] = 255
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    bg, fg = crit(pred, bg_label), crit(pred, fg_label)
    if ba:
        bg, fg = bg / logits.shape[0], fg / logits.shape[0]
    ce = bg + fg
    total = sum(gi * t for gi, t in zip(g, (ce, bg, fg)) if gi != 0)
    if d_probs is not None:
        total = total + (pred.softmax(1) * torch.from_numpy(d_probs)).sum()
    total.backward()
    return dict(celoss=ce.detach(), bg=bg.detach(), fg=fg.detach(), d_logits=x.grad)


def device(logits, label, ba, g=(1.0, 0.0, 0.0)):
    x = torch.from_numpy(logits).to(DEV).requires_grad_(True)
    ce, bg, fg, sums, counts = S.split_cross_entropy(x, label, ba, return_stats=True)
    sum(gi * t for gi, t in zip(g, (ce, bg, fg)) if gi != 0).backward()
    return dict(celoss=ce.detach().cpu(), bg=bg.detach().cpu(), fg=fg.detach().cpu(), d_logits=x.grad.cpu(), sums=sums.cpu(),
                counts=counts.cpu().numpy())


def compare(cmp, what, dev, tor, ref):
    """the tolerance rule of the module docstring for one quantity; NaN must meet NaN"""
    ref = torch.as_tensor(np.asarray(ref, np.float64))
    dev, tor = dev.double().reshape(ref.shape), tor.double().reshape(ref.shape)
    if torch.isnan(ref).any():
        assert torch.isnan(ref).all() and torch.isnan(dev).all() and torch.isnan(tor).all(), what
        return
    if not ref.abs().max() > 0:                          # an all-zero reference (no pixel counts): zero, bit for bit
        cmp.check(what, dev, ref, **EXACT)
        return
    terr, derr = float((tor - ref).abs().max()), float((dev - ref).abs().max())
    floor = ULPS * float(ref.abs().max())
    print("%s %s: device err %.3e, torch fp32 err %.3e, ratio %.2f, floor %.3e" % (cmp.where, what, derr, terr, derr / max(terr, 1e-300), floor))
    cmp.check(what, dev, ref, atol=max(2.0 * terr, floor))


def check_case(tag, scale, kind, ba, g=(1.0, 0.0, 0.0)):
    logits, label = case(tag, scale, kind)
    B = logits.shape[0]
    ref = reference(tag, scale, kind, ba, g)
    tor = torch_cpu(logits, label, ba, g)
    dev = device(logits, label, ba, g)
    cmp = Cmp()
    cmp.where = "%s x%d %s ba%d" % (tag, scale, kind, ba)
    for name in ("celoss", "bg", "fg", "d_logits"):
        compare(cmp, name, dev[name], tor[name], ref[name])
    compare(cmp, "sums", dev["sums"], torch.from_numpy(ref["sums"]).float(), ref["sums"])
    np.testing.assert_array_equal(dev["counts"], ref["counts"])
    # no Inf or NaN in the gradient beyond what torch gives
    assert not (~torch.isfinite(dev["d_logits"]) & torch.isfinite(tor["d_logits"])).any()
    assert not cmp.failures, "\n".join(cmp.failures)
    return dev, tor, ref


@pytest.mark.parametrize("ba", [False, True])
@pytest.mark.parametrize("scale", [1, 30])
@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_cross_entropy_forward_and_backward(tag, scale, ba):
    dev, tor, ref = check_case(tag, scale, "random", ba)
    assert np.isfinite(ref["celoss"]) and ref["counts"][-1].min() > 0
    if scale == 30:                                      # a naive exp would overflow: logits reach beyond 88
        assert np.abs(case(tag, scale)[0]).max() > 88 or tag == "b"
    if tag in ("a", "b", "c") and scale == 1:            # the reference's own numbers, under the same rule
        g = np.load(os.path.join(GOLDEN, "segloss_%s.npz" % tag))
        cmp = Cmp()
        cmp.where = "%s fixture ba%d" % (tag, ba)
        for name in ("celoss", "bg", "fg", "d_logits"):
            fx = torch.from_numpy(np.asarray(g["%s_ba%d" % (name, int(ba))]))
            compare(cmp, name, dev[name], fx, ref[name])
        np.testing.assert_array_equal(dev["counts"][-1], g["counts"])
        assert not cmp.failures, "\n".join(cmp.failures)


def test_output_gradients_of_all_three_terms():
    check_case("a", 1, "random", False, g=(0.5, 2.0, -1.0))
    check_case("c", 1, "random", True, g=(0.0, 1.0, 3.0))


def test_only_background_all_ignored_and_labels_above_k():
    dev, tor, ref = check_case("a", 1, "bg", False)
    assert torch.isnan(dev["fg"]) and torch.isnan(dev["celoss"]) and torch.isfinite(dev["bg"]) and torch.isfinite(dev["d_logits"]).all()
    assert dev["counts"][-1, 1] == 0 and dev["counts"][-1, 0] > 0
    dev, tor, ref = check_case("a", 1, "ignore", True)
    assert torch.isnan(dev["bg"]) and torch.isnan(dev["fg"]) and not dev["counts"].any()
    assert torch.isfinite(dev["d_logits"]).all() or not torch.isfinite(tor["d_logits"]).all()
    # a label in K..254 is ignored like 255: identical bits
    logits, label = case("a")
    assert ((label >= 21) & (label < 255)).any()
    plain = label.copy()
    plain[label >= 21] = 255
    one, two = device(logits, label, False), device(logits, plain, False)
    for name in ("celoss", "bg", "fg", "d_logits", "sums"):
        assert torch.equal(one[name], two[name]), name
    np.testing.assert_array_equal(one["counts"], two["counts"])


def test_forward_and_backward_repeat_bit_for_bit_and_take_device_labels():
    logits, label = case("c")
    one = device(logits, label, False)
    two = device(logits, torch.from_numpy(label).to(DEV), False)
    for name in ("celoss", "bg", "fg", "d_logits", "sums"):
        assert one[name].numpy().tobytes() == two[name].numpy().tobytes(), name
    np.testing.assert_array_equal(one["counts"], two["counts"])
    x = torch.from_numpy(logits).to(DEV)
    with pytest.raises(ValueError):
        S.split_cross_entropy(x[:, :1], label)
    with pytest.raises(ValueError):
        S.split_cross_entropy(x, label[:, :8])
    with pytest.raises(ValueError):
        S.split_cross_entropy(x, label.astype(np.int32))


# ------------------------------------------------------------------------------------------------
# dense energy
# ------------------------------------------------------------------------------------------------
def bilateral(img, planes, srgb, sxy):
    """bilateralfilter.cpp:22-41 on img (h, w, 3) uint8 and planes (K, h, w) fp32: the reference's C++ compiled under oracle/_ref
    where that was built, else the oracle's numpy lattice, which test_crf_cpu.py pins to that C++ bit for bit"""
    lib = C.load_ref()
    if lib is not None:
        return C.ref_bilateralfilter(lib, img, planes, srgb, sxy)
    k, h, w = planes.shape
    lat = C.lattice_init(C.bilateral_features(img, sxy, srgb))
    return np.ascontiguousarray(C.lattice_compute(lat, np.ascontiguousarray(planes.reshape(k, h * w).T)).T.reshape(k, h, w))


def energy_case(seed, B, K, W, H, roi_kind="random"):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (B, 3, 1, 1)) + 40 * (np.arange(W)[None, None, :, None] > W // 2)
    img = np.clip(base + rng.integers(-25, 26, (B, 3, W, H)), 0, 255).astype(np.uint8)       # noisy, two regions
    z = rng.standard_normal((B, K, W, H))
    probs = (np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)).astype(np.float32)
    roi = np.zeros((B, W, H), np.float32) if roi_kind == "zero" else (rng.random((B, W, H)) > 0.2).astype(np.float32) * rng.choice(
        np.array([1.0, 0.5], np.float32), (B, W, H))
    return img, probs, roi


def check_energy(img, probs, roi, weight, srgb, sxy, sf):
    """the layer on (img, probs, roi) against the reference lattice applied to the layer's own (resized) inputs"""
    layer = S.DenseEnergyLoss(weight, srgb, sxy, sf)
    p = torch.from_numpy(probs).to(DEV).requires_grad_(True)
    E = layer(img, p, roi, None)
    E.backward()
    images, ps, rs, sxy2 = layer.inputs(img, p.detach(), roi)
    images, ps, rs = images.cpu().numpy(), ps.cpu().numpy(), rs.cpu().numpy()
    B, K = ps.shape[:2]
    assert sxy2 == sxy * sf
    AS = np.stack([bilateral(images[b], rs[b][None] * ps[b], srgb, sxy2) * rs[b][None] for b in range(B)])
    got_AS = S.filtered_probs(*(torch.from_numpy(a).to(DEV) for a in (images, ps, rs)), srgb, sxy2).cpu().numpy()
    np.testing.assert_array_equal(got_AS, AS)                                   # bit for bit
    terms = ps.astype(np.float64) * AS.astype(np.float64)
    want_E, want_grad = R.energy(ps, AS, weight)
    bound = (weight / B) * K * ps.shape[2] * ps.shape[3] * 2.0 ** -24 * np.abs(terms).sum() + abs(want_E) * 2.0 ** -23
    print("energy %s K=%d sf=%g: E %.9g vs %.9g, err %.3e, bound %.3e" % (ps.shape[2:], K, sf, float(E), want_E, abs(float(E) - want_E), bound))
    assert abs(float(E) - want_E) <= bound
    return p.grad.cpu().numpy(), AS, (images, ps, rs)


@pytest.mark.parametrize("K", [3, 21])
@pytest.mark.parametrize("wh", [(16, 20), (33, 29)])
def test_energy_filter_sum_and_defined_gradient(wh, K):
    B, weight = 2, 0.75
    img, probs, roi = energy_case(41 + K, B, K, *wh)
    grad, AS, _ = check_energy(img, probs, roi, weight, 15.0, 40.0, 1.0)
    assert np.abs(AS).max() > 0 and (AS[roi[:, None].repeat(K, 1) == 0] == 0).all()
    np.testing.assert_array_equal(grad, np.float32(-2.0 * weight / B) * AS)    # exactly -2 weight / B * AS
    img, probs, roi = energy_case(41 + K, B, K, *wh, roi_kind="zero")
    layer = S.DenseEnergyLoss(weight, 15.0, 40.0, 1.0)
    p = torch.from_numpy(probs).to(DEV).requires_grad_(True)
    E = layer(img, p, roi, None)
    E.backward()
    assert float(E) == 0.0 and not p.grad.cpu().numpy().any()


def test_energy_scale_factor_half_against_the_restatement():
    B, K, W, H, weight = 2, 3, 33, 29, 0.75
    img, probs, roi = energy_case(51, B, K, W, H)
    grad, AS, (images, ps, rs) = check_energy(img, probs, roi, weight, 15.0, 40.0, 0.5)
    want_img, want_ps, want_roi = R.energy_inputs(img, probs, roi, 0.5)
    assert images.shape == (B, 16, 14, 3) and ps.shape == (B, K, 16, 14)
    np.testing.assert_array_equal(images, want_img)
    np.testing.assert_array_equal(rs, want_roi)
    cmp = Cmp()
    cmp.where = "scale_factor 0.5"
    cmp.check("probs", torch.from_numpy(ps), torch.from_numpy(want_ps), atol=ULPS)           # probabilities are <= 1
    # the gradient returns through the resize: the adjoint of the bilinear rule applied to -2 weight / B * AS
    want = R.upsample_transposed(R.energy(ps, AS, weight)[1], W, H)
    cmp.check("d_probs", torch.from_numpy(grad), torch.from_numpy(want), atol=ULPS * float(np.abs(want).max()))
    assert not cmp.failures, "\n".join(cmp.failures)


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_joint_loss_on_the_device_mask_and_backward_through_both_terms():
    # seed 22: the restated rule gives 807 ignored, 71 background and 277 foreground pixels, so both terms have a count
    cams, classes, la, ha, _ = PR.decisive_case(seed=22, k=3, w=33, h=35, classes=[1, 8, 14])
    mask = P.seg_label(cams, classes, la, ha, ignore_uncertain=True, device=DEV)
    assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (33, 35)
    host = mask.cpu().numpy()
    assert (host == 255).any() and (host == 0).any() and ((host > 0) & (host < 21)).any()
    rng = np.random.default_rng(22)
    B, K, h, w, W, H = 1, 21, 9, 10, 33, 35
    logits = (2.0 * rng.standard_normal((B, K, h, w))).astype(np.float32)
    img = rng.integers(0, 256, (B, 3, W, H)).astype(np.uint8)
    crop = np.ones((W, H, B), np.float32)
    crop[:4] = 0
    weight = 0.5
    layer = S.DenseEnergyLoss(weight, 15.0, 40.0, 1.0)
    outs = []
    for label in (mask, host):                            # the device tensor (no host trip) and its numpy copy: the same bits
        x = torch.from_numpy(logits).to(DEV).requires_grad_(True)
        ce, dl = S.joint_loss(img, x, label, crop, False, layer)
        (ce + dl).backward()
        outs.append((ce.detach().cpu(), dl.detach().cpu(), x.grad.cpu()))
    for a, b in zip(*outs):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    ce, dl, grad = outs[0]
    # loss.backward() through split_cross_entropy + DenseEnergyLoss: the energy's gradient enters as d_probs
    label = host[None]
    probs = R.split_ce(logits, label)["probs"]
    x = torch.from_numpy(logits).to(DEV)
    _, p_dev, _, _ = S._split_ce(x, label, False, True)
    roi = np.ascontiguousarray(crop.transpose(2, 0, 1))
    images = torch.from_numpy(np.ascontiguousarray(img.transpose(0, 2, 3, 1))).to(DEV)
    AS = S.filtered_probs(images, p_dev, torch.from_numpy(roi).to(DEV), 15.0, 40.0).cpu().numpy()
    d_probs = np.float32(-2.0 * weight / B) * AS
    ref = R.split_ce(logits, label, False, d_probs=d_probs)
    tor = torch_cpu(logits, label, False, d_probs=d_probs)
    cmp = Cmp()
    cmp.where = "joint"
    compare(cmp, "celoss", ce, tor["celoss"], ref["celoss"])
    compare(cmp, "probs", p_dev.cpu(), F.interpolate(torch.from_numpy(logits), (W, H), mode="bilinear", align_corners=False).softmax(1), probs)
    compare(cmp, "d_logits", grad, tor["d_logits"], ref["d_logits"])
    want_E = R.energy(p_dev.cpu().numpy(), AS, weight)[0]
    assert abs(float(dl) - want_E) <= K * W * H * 2.0 ** -24 * weight * np.abs(p_dev.cpu().numpy().astype(np.float64) * AS).sum() + abs(want_E) * 2.0 ** -23
    assert not cmp.failures, "\n".join(cmp.failures)
