"""Saliency-guided pseudo-labels on the device (csrc/pseudo_sal.hip behind acr_sal_pseudo_compose / acr_morph_open_u8) against
the reference's own runs (tests/golden/pseudo_sal_{a..d}.npz) and against the numpy restatement tests/pseudo_sal_ref.py -- pinned
to those runs by test_pseudo_sal_cpu.py -- on seeded inputs.  Outputs are uint8: every comparison is exact equality.  Seeded
inputs are checked to be decisive (pseudo_sal_ref.margin > 1e-5) before the device is asked, so that no comparison hangs on the
last bit of a pow."""
import os

import numpy as np
import pytest
import torch

import pseudo_sal_ref as R
from acr_wsss_amd import _lib as L
from acr_wsss_amd import pseudo as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = P.OPEN_TILE                                          # edge of the opening kernel's tile (test_pseudo_sal_cpu.py ties it to the source)


def _both(cams, present, sal, what, **kw):
    """device == restatement with and without the opening; returns the device's (label before, label after, saliency) as numpy"""
    outs = []
    for k in (0, kw.pop("open_size", 10)):
        got, got_sal = P.seg_label_saliency(cams, present, sal, open_size=k, device=DEV, **kw)
        assert got.dtype == got_sal.dtype == torch.uint8 and got.is_cuda and got_sal.is_cuda
        assert tuple(got.shape) == tuple(got_sal.shape) == sal.shape
        want, want_sal = R.seg_label(cams, present, sal, open_size=k, **kw)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg="%s open_size=%d" % (what, k))
        np.testing.assert_array_equal(got_sal.cpu().numpy(), want_sal, err_msg="%s open_size=%d saliency" % (what, k))
        outs.append(got.cpu().numpy())
    return outs[0], outs[1], got_sal.cpu().numpy()


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_fixtures_written_by_the_reference(tag):
    g = np.load(os.path.join(GOLDEN, "pseudo_sal_%s.npz" % tag))
    cams, sal = g["cams"][None], g["saliency"][None]
    present = (g["cam_label"].astype(np.uint8) > 1e-5)[None]
    for alpha, key in ((12, "label"), (32, "label32")):
        for k, name in ((0, key + "_pre"), (10, key)):
            got, got_sal = P.seg_label_saliency(cams, present, sal, bg_alpha=alpha, open_size=k, device=DEV)
            np.testing.assert_array_equal(got.cpu().numpy()[0], g[name], err_msg=name)
            np.testing.assert_array_equal(got_sal.cpu().numpy()[0], g["saliency_out"], err_msg=name)


SEEDED = {
    "1x1 7x9 (smaller than the window)": dict(seed=31, b=1, c=1, h=7, w=9, present=[[1]]),
    "3x20 33x35 (presence differs; image 1 has no class)": dict(seed=32, b=3, c=20, h=33, w=35,
                                                                 present=[[1 if c in (2, 7, 15) else 0 for c in range(20)], [0] * 20,
                                                                          [1 if c in (0, 19) else 0 for c in range(20)]]),
    "2x3 around the opening's tile": dict(seed=33, b=2, c=3, h=T - 1, w=T + 1, present=[[1, 1, 1], [1, 0, 1]]),
    "2x80 40x45": dict(seed=34, b=2, c=80, h=40, w=45, present=None),
    "2x20 60x70 rounded to 1/100": dict(seed=35, b=2, c=20, h=60, w=70, present=[[1] * 20, [1, 1, 1, 1] + [0] * 16], round_to=100),
}


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_device_equals_the_restatement(name):
    cams, present, sal, mg = R.decisive_case(**SEEDED[name])
    assert mg > 1e-5
    pre, lab, sal_out = _both(cams, present, sal, name)
    assert ((sal == 0) & (pre != 0)).any(), "no grabbed pixel"
    if name.startswith("3x20"):                          # no present class: 255 where salient, else 0; planes are never read
        np.testing.assert_array_equal(pre[1], np.where(sal[1] != 0, 255, 0))
        assert set(np.unique(lab[1])) <= {0, 255} and np.array_equal(sal_out[1], sal[1])
        assert ((pre != 0) & (lab == 0)).any() and (lab != 0).any()
    if "rounded" in name:                                # ties at the threshold
        thr = R.thresholds(cams[0], present[0].astype(bool))
        assert ((cams[0][0] == thr[0]).sum() > 1)


def test_a_fully_labelled_image_smaller_than_the_window_survives_whole():
    cams = np.full((1, 1, 7, 9), 0.9, np.float32)
    sal = np.full((1, 7, 9), 200, np.uint8)
    assert R.margin(cams[0], [1]) > 1e-5
    pre, lab, _ = _both(cams, np.ones((1, 1), np.uint8), sal, "7x9 all foreground")
    assert (pre == 1).all() and (lab == 1).all()


def test_other_cut_and_exponent():
    cams, present, sal, _ = R.decisive_case(seed=36, b=2, c=5, h=45, w=52, present=[[1, 0, 1, 1, 0], [0, 1, 0, 0, 1]], bg_alpha=32)
    assert min(R.margin(cams[i], present[i], 32) for i in range(2)) > 1e-5
    pre9, _, _ = _both(cams, present, sal, "bg_alpha=32", bg_alpha=32)
    pre5, _, _ = _both(cams, present, sal, "cut=0.5, bg_alpha=32", cut=0.5, bg_alpha=32)
    assert ((sal == 0) & (pre5 != 0)).sum() > ((sal == 0) & (pre9 != 0)).sum()       # a lower threshold grabs more
    _both(cams, present, sal, "cut=0", cut=0.0, bg_alpha=32)                          # pos == 0 everywhere: nothing is grabbed
    _both(cams, present, sal, "open_size=3", open_size=3, bg_alpha=32)


def test_device_equals_the_restatement_at_448x448_once():
    cams, present, sal, _ = R.decisive_case(seed=37, b=2, c=20, h=448, w=448, present=None)
    _both(cams, present, sal, "2x20 448x448")


def _blobs(rng, b, h, w):
    """masks with blocks that touch every image edge and straddle the tile borders, salted with holes and specks"""
    m = np.zeros((b, h, w), np.uint8)
    m[:, 0:40, T - 14:T + 16] = 255                      # top edge, across the first vertical tile border
    m[:, T - 15:T + 15, 0:30] = 255                      # left edge, across the first horizontal border
    m[:, h - 33:h, 20:55] = 255                          # bottom edge
    m[:, 30:h - 40, w - 21:w] = 255                      # right edge, across the horizontal borders
    m[:, T - 10:T + 12, T - 12:T + 10] = 255             # the corner where four tiles meet
    m[:, 2 * T - 6:2 * T + 5, 2 * T - 20:2 * T + 20] = 255
    m[0][rng.random((h, w)) < 0.004] = 0                 # holes
    m[-1][rng.random((h, w)) < 0.01] = 255               # specks
    return m


@pytest.mark.parametrize("k", [1, 2, 3, 10, 11, 32])
def test_morph_open_alone(k):
    rng = np.random.default_rng(40 + k)
    h, w = 2 * T + 9, 2 * T + 22                         # 3 x 3 tiles, the last ones narrow
    m = _blobs(rng, 2, h, w)
    got = P.morph_open(torch.from_numpy(m).to(DEV), k)
    assert got.dtype == torch.uint8 and tuple(got.shape) == m.shape
    for i in range(2):
        np.testing.assert_array_equal(got[i].cpu().numpy(), R.morph_open(m[i], k), err_msg="k=%d image %d" % (k, i))
    if k == 1:
        np.testing.assert_array_equal(got.cpu().numpy(), m)
    else:
        assert (got.cpu().numpy() != m).any() and got.any()
    full = np.full((h, w), 255, np.uint8)
    np.testing.assert_array_equal(P.morph_open(full, k, device=DEV).cpu().numpy(), full)
    assert not P.morph_open(np.zeros((h, w), np.uint8), k, device=DEV).any()
    small = _blobs(rng, 1, T - 1, T + 1)[0]
    np.testing.assert_array_equal(P.morph_open(small, k, device=DEV).cpu().numpy(), R.morph_open(small, k))


def test_two_calls_give_identical_bits_whatever_the_workspace_holds():
    cams, present, sal, _ = R.decisive_case(seed=38, b=3, c=20, h=70, w=90, present=None)
    a = P.seg_label_saliency(cams, present, sal, device=DEV)
    b = P.seg_label_saliency(cams, present, sal, device=DEV)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    lib = L.load()
    d_cams, d_pres, d_sal = (torch.from_numpy(x).to(DEV) for x in (cams, present, sal))
    nbytes = lib.acr_sal_pseudo_ws_bytes(3, 20, 70, 90)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    label, sal_out = torch.empty_like(d_sal), torch.empty_like(d_sal)
    L.check(lib.acr_sal_pseudo_compose(L.ptr(d_cams), L.ptr(d_pres), 3, 20, 70, 90, L.ptr(d_sal), 12.0, 0.9, 10, L.ptr(ws), nbytes, L.ptr(label),
                                       L.ptr(sal_out), L.stream_ptr()), "acr_sal_pseudo_compose")
    assert torch.equal(label, a[0]) and torch.equal(sal_out, a[1])
    # saliency_out may be the saliency map itself
    L.check(lib.acr_sal_pseudo_compose(L.ptr(d_cams), L.ptr(d_pres), 3, 20, 70, 90, L.ptr(d_sal), 12.0, 0.9, 10, L.ptr(ws), nbytes, L.ptr(label),
                                       L.ptr(d_sal), L.stream_ptr()), "acr_sal_pseudo_compose")
    assert torch.equal(label, a[0]) and torch.equal(d_sal, a[1])


def test_the_flow_from_cams_and_saliency_to_the_joint_loss():
    """shape and dtype contract only: segtrain.saliency_labels' label goes into segloss.joint_loss as seg_label and a finite loss
    comes back; nothing leaves the device"""
    from acr_wsss_amd import segloss, segtrain
    S, B = 64, 2
    cams, present, sal, _ = R.decisive_case(seed=39, b=B, c=20, h=S, w=S, present=None)
    labels = torch.from_numpy(present.astype(np.float32)).to(DEV)       # the loader's image-level labels are float
    label, sal_out = segtrain.saliency_labels(torch.from_numpy(cams).to(DEV), labels, torch.from_numpy(sal).to(DEV))
    assert label.dtype == torch.uint8 and label.is_cuda and tuple(label.shape) == (B, S, S) and tuple(sal_out.shape) == (B, S, S)
    np.testing.assert_array_equal(label.cpu().numpy(), R.seg_label(cams, present, sal)[0])
    torch.manual_seed(0)
    logits = torch.randn(B, 21, S // 4, S // 4, device=DEV, requires_grad=True)
    ori = torch.randint(0, 256, (B, 3, S, S), device=DEV, dtype=torch.uint8)
    croppings = torch.ones(S, S, B, device=DEV)
    ce, dl = segloss.joint_loss(ori, logits, label, croppings, False, segloss.DenseEnergyLoss(0.5, 15.0, 40.0, 1.0))
    assert torch.isfinite(ce + dl)
