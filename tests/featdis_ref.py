"""The class-centre feature-distance loss restated on torch CPU tensors, as include/acr_hip.h defines it (the reference's
``compute_dis_no_batch``, myTool.py:1624-1710, with the classes 1..K-1 for its 1..20), and the seeded cases of its tests.  Run on
float64 tensors it is the expectation of test_featdis_cpu.py / test_featdis_gpu.py; run on float32 tensors it is what torch's fp32
shows on a case (the yardstick of the device's tolerance) and the composition scripts/bench_featdis.py times.  The gradient is
autograd's: ``norm`` has torch's rule d|x|/dx := 0 at x = 0."""
import numpy as np
import torch

EPS = 1e-7
# tag: (B, K, C, h, w)
CASES = {
    "a": (2, 21, 16, 5, 7),                # mixed labels
    "b": (2, 21, 1024, 3, 3),              # the reference's channel count
    "c": (2, 21, 8, 3, 3),                 # no background anywhere
    "d": (2, 21, 8, 3, 3),                 # no foreground
    "e": (2, 21, 8, 4, 4),                 # image 0 without background
    "f": (1, 21, 8, 3, 3),                 # one foreground class, two pixels
}


def cos(x, y):
    """compute_cos: x (n, C), y (m, C) -> (n, m)"""
    return x @ y.t() / (x.norm(dim=1)[:, None] * y.norm(dim=1)[None, :] + EPS)


def feature_distance(seg, feat):
    """seg (B, K, h, w), feat (B, C, h, w) of one float dtype -> (loss, dis, pixel_dis, labels (B, h, w) uint8, counts (B + K - 1)
    int64: n_b per image, then m_i per class).  Differentiable in feat."""
    B, K, h, w = seg.shape
    C, N = feat.shape[1], h * w
    dt = feat.dtype
    lab = seg.detach().argmax(1).reshape(B * N)
    f = feat.reshape(B, C, N).permute(0, 2, 1).reshape(B * N, C)
    img = torch.arange(B).repeat_interleave(N)
    cid = torch.where(lab == 0, img, B + lab - 1)                 # the centre of a pixel: its image's background, or its class
    NC = B + K - 1
    counts = torch.bincount(cid, minlength=NC)
    div = (counts.double() + EPS).to(dt)                          # the divisors n + eps, formed in double
    cen = torch.zeros(NC, C, dtype=dt).index_add(0, cid, f) / div[:, None]
    valid = counts >= 1
    mine = cen[cid]
    per_pixel = 1 - (f * mine).sum(1) / (f.norm(dim=1) * mine.norm(dim=1) + EPS)
    per_centre = torch.zeros(NC, dtype=dt).index_add(0, cid, per_pixel) / div
    Fn = int(valid[B:].sum())
    pixel_dis = (per_centre[valid].sum() + 2.0 * int((~valid[:B]).sum())) / (Fn + B)
    g, cb = cen[B:][valid[B:]], cen[:B]
    has_bg = bool(valid[:B].any())
    zero = torch.zeros((), dtype=dt)
    if Fn > 1:
        m = 1 + cos(g, g)
        ff = (m.sum() - m.diagonal().sum()) / (Fn * (Fn - 1))
    else:
        ff = zero
    if Fn >= 1 and has_bg:
        dis = 0.5 * ff + 0.5 * (1 + cos(g, cb)).mean()
    elif not has_bg:
        dis = 0.5 * ff + 1
    else:
        dis = zero
    return dis + pixel_dis, dis, pixel_dis, lab.reshape(B, h, w).to(torch.uint8), counts


def loss_and_grad(seg, feat, dtype, upstream=1.0):
    """numpy or tensors in -> (loss, dis, pixel_dis, d_feat * upstream, labels, counts) as numpy, evaluated in ``dtype``"""
    s = torch.as_tensor(np.asarray(seg)).to(dtype)
    f = torch.as_tensor(np.asarray(feat)).to(dtype).requires_grad_(True)
    loss, dis, pix, lab, cnt = feature_distance(s, f)
    (loss * upstream).backward()
    return float(loss.detach()), float(dis.detach()), float(pix.detach()), f.grad.numpy(), lab.numpy(), cnt.numpy()


def features(rng, shape, quantum=None):
    """relu(randn) without an all-zero pixel vector (at C = 8 about one pixel in 256 is one: the draw is repeated until none is);
    ``quantum``: values rounded to multiples of it"""
    while True:
        f = np.maximum(rng.standard_normal(shape), 0).astype(np.float32)
        if quantum:
            f = (np.round(f / quantum) * quantum).astype(np.float32)
        if (np.abs(f).sum(1) > 0).all():
            return f


def logits(rng, B, K, h, w, bg_boost=1.5):
    s = rng.standard_normal((B, K, h, w)).astype(np.float32)
    s[:, 0] += bg_boost                                           # some background in every image
    return s


def fixture_case(tag):
    """(seg, feat) float32 of a fixture case; every case is asserted to be what its name says"""
    B, K, C, h, w = CASES[tag]
    rng = np.random.default_rng(1000 + ord(tag))
    seg = logits(rng, B, K, h, w)
    if tag == "c":
        seg[:, 0] = -10
    elif tag == "d":
        seg[:, 0] = 10
    elif tag == "e":
        seg[0, 0] = -10
    elif tag == "f":
        seg[:] = 0
        seg[:, 0] = 1
        seg[0, 5, 0, 1] = seg[0, 5, 2, 2] = 2
    feat = features(rng, (B, C, h, w), quantum=1 / 64 if tag == "b" else None)      # b: short mantissas keep the file small
    lab = seg.argmax(1)
    bg = (lab == 0).reshape(B, -1).sum(1)
    assert (np.abs(feat).sum(1) > 0).all()
    if tag in "ab":
        assert (bg >= 1).all() and (lab > 0).any() and len(np.unique(lab)) > 3
    elif tag == "c":
        assert bg.sum() == 0
    elif tag == "d":
        assert (lab == 0).all()
    elif tag == "e":
        assert bg[0] == 0 and bg[1] >= 1 and (lab[1] > 0).any()
    else:
        assert (lab == 5).sum() == 2 and ((lab == 0) | (lab == 5)).all()
    return seg, feat


def seeded_case(B, K, C, h, w, seed, bg_boost=1.5, integer_logits=False):
    """(seg, feat) float32 for the device tests: random logits (small integers for exact ties) and relu(randn) features without an
    all-zero pixel"""
    rng = np.random.default_rng(seed)
    if integer_logits:
        seg = rng.integers(0, 3, (B, K, h, w)).astype(np.float32)
    else:
        seg = logits(rng, B, K, h, w, bg_boost)
    if C < 8:                                                     # relu would zero whole pixels: values of both signs away from 0 instead
        v = rng.standard_normal((B, C, h, w))
        return seg, (np.sign(v) * (np.abs(v) + 0.05)).astype(np.float32)
    return seg, features(rng, (B, C, h, w))
