"""Host side of the saliency-guided pseudo-labels: the numpy restatement (tests/pseudo_sal_ref.py) reproduces the reference's own
runs of compute_seg_label_3 and compute_seg_label_two_step recorded in tests/golden/pseudo_sal_{a..d}.npz (written by
tests/golden/make_pseudo_sal_golden.py), the restated opening is scipy's minimum filter followed by its maximum filter, the
fixtures are decisive, the C ABI is declared, bound and exported, bad arguments are refused with a message, and the product
refuses to run without a GPU.  Every comparison is exact."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_checks
import pseudo_sal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = {"a": (41, 50), "b": (40, 52), "c": (43, 49), "d": (38, 51)}
NAMES = ("acr_sal_pseudo_ws_bytes", "acr_sal_pseudo_compose", "acr_morph_open_u8")


def _load(tag):
    z = np.load(os.path.join(GOLDEN, "pseudo_sal_%s.npz" % tag))
    return {k: z[k] for k in z.files}


def _present(g):
    return g["cam_label"].astype(np.uint8) > 1e-5        # the reference's own test (myTool.py:190,195)


@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_restatement_reproduces_the_reference(tag):
    g = _load(tag)
    present = _present(g)
    assert g["cams"].shape == (20,) + SHAPES[tag] and g["cams"].dtype == np.float32 and g["saliency"].dtype == np.uint8
    for alpha, key in ((12, "label"), (32, "label32")):
        pre, sal_pre = R.seg_label_one(g["cams"], present, g["saliency"], bg_alpha=alpha, open_size=0)
        np.testing.assert_array_equal(pre, g[key + "_pre"])
        np.testing.assert_array_equal(sal_pre, g["saliency_out"])
        lab, sal = R.seg_label_one(g["cams"], present, g["saliency"], bg_alpha=alpha, open_size=10)
        np.testing.assert_array_equal(lab, g[key])
        np.testing.assert_array_equal(sal, g["saliency_out"])
    # what every case must contain: grabbed pixels, 255 pixels, pixels the opening removed and pixels it kept
    pre, lab = g["label_pre"], g["label"]
    grabbed = (g["saliency"] == 0) & (pre != 0)
    assert grabbed.any() and (lab == 255).any() and ((pre != 0) & (lab == 0)).any() and (lab != 0).any()
    np.testing.assert_array_equal(g["saliency_out"] != g["saliency"], grabbed)
    assert (g["label32"] != g["label"]).any()
    thr = R.thresholds(g["cams"], present)
    if present.sum() > 1:
        # pixels above the thresholds of two classes: the reference gave them to the lowest class (its conflict branch is dead)
        above = [(g["cams"][c] > thr[c]) for c in np.flatnonzero(present)]
        twice = grabbed & (np.sum(above, axis=0) >= 2)
        assert twice.any()
        lowest = np.zeros(pre.shape, np.int64)
        for c, a in list(zip(np.flatnonzero(present), above))[::-1]:
            lowest[a] = c + 1
        np.testing.assert_array_equal(pre[twice], lowest[twice])
        assert not (pre[twice] == 255).any()
    if tag == "c":                                       # values on the 1/100 grid: the threshold has duplicates
        assert np.array_equal(g["cams"], (np.round(g["cams"] * 100) / 100).astype(np.float32))
        order = np.sort(g["cams"][0][g["cams"][0] > 0])
        assert (order == thr[0]).sum() > 1
    if tag == "d":                                       # one positive value: pos == 0, skipped; an absent class with a plane
        assert (g["cams"][11] > 0).sum() == 1 and present[11] and thr[11] == np.inf
        assert not present[5] and g["cams"][5].any() and not (pre == 6).any()


@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_fixtures_are_decisive(tag):
    """bg is more than 1e-5 (relative) away from the largest present class value at every pixel, for both exponents: one pow or
    another (<= 1 ulp = 1.2e-7 apart) cannot change a comparison"""
    g = _load(tag)
    for alpha in (12, 32):
        mg = R.margin(g["cams"], _present(g), alpha)
        print("pseudo_sal_%s: bg_alpha %d margin %.3e" % (tag, alpha, mg))
        assert mg > 1e-5


@pytest.mark.parametrize("k", [1, 2, 3, 10, 11])
def test_restated_opening_is_scipys_minimum_then_maximum_filter(k):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(k)
    for h, w, p in ((37, 45, 0.97), (7, 9, 0.9), (30, 64, 0.995)):
        mask = np.where(rng.random((h, w)) < p, 255, 0).astype(np.uint8)
        mask[h // 2:, : w // 3] = 255                    # a block that touches two edges
        want = ndi.maximum_filter(ndi.minimum_filter(mask, size=k, mode="constant", cval=255), size=k, mode="constant", cval=0)
        np.testing.assert_array_equal(R.morph_open(mask, k), want)
    full = np.full((7, 9), 255, np.uint8)                # smaller than the window: a full image survives whole
    np.testing.assert_array_equal(R.morph_open(full, 10), full)
    assert not R.morph_open(np.zeros((7, 9), np.uint8), 10).any()


def test_an_even_opening_is_shifted_but_never_revives_a_label():
    """k = 10: O can hold where F does not (the pair of passes is shifted by one pixel) -- the label there is 0 already"""
    mask = np.zeros((30, 30), np.uint8)
    mask[5:15, 5:15] = 255                               # exactly one 10 x 10 box: it erodes to (10, 10), which dilates to 6..15
    O = R.morph_open(mask, 10)
    assert (O == 255).sum() == 100 and (O[6:16, 6:16] == 255).all() and ((O == 255) & (mask == 0)).any()


def test_symbols_are_declared_bound_and_exported():
    from acr_wsss_amd import _lib as L
    from acr_wsss_amd import pseudo
    abi_checks.check_bound(NAMES, L.SIGNATURES)
    lib = L.load()
    for name in NAMES:
        assert hasattr(lib, name)
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r" T %s$" % name, out, flags=re.M), name
    make = open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "Makefile")).read()
    assert "pseudo_sal.hip" in make
    src = open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "pseudo_sal.hip")).read()
    assert int(re.search(r"#define PSAL_TILE (\d+)", src).group(1)) == pseudo.OPEN_TILE
    assert int(re.search(r"#define PSAL_MAX_K (\d+)", src).group(1)) == pseudo.MAX_OPEN
    assert "#define PSAL_MAX_CLASSES ACR_SAL_PSEUDO_MAX_CLASSES\n" in src         # the kernels' limit is the header's
    assert int(abi_checks.defined("ACR_SAL_PSEUDO_MAX_CLASSES")) == pseudo.MAX_SAL_CLASSES == 127


def test_ws_bytes_is_a_host_only_query():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    f = lib.acr_sal_pseudo_ws_bytes
    small, big = f(1, 1, 7, 9), f(16, 20, 448, 448)
    assert 0 < small < big and big >= 16 * 20 * 4 * 256 * 4 + 16 * 448 * 448
    for bad in ((0, 20, 10, 10), (65536, 20, 10, 10), (1, 0, 10, 10), (1, 128, 10, 10), (1, 20, 0, 10), (1, 20, 10, 0), (1, 20, 1 << 16, 1 << 15)):
        assert f(*bad) < 0, bad
        assert b"acr_sal_pseudo_ws_bytes" in lib.acr_last_error()


def test_argument_errors_return_minus_one_with_a_message():
    """every refusal happens on the host before anything is launched: no GPU is needed, the pointers are never followed"""
    from acr_wsss_amd import _lib as L
    lib = L.load()
    p = L.c_void_p(4096)                                 # non-null, aligned; never dereferenced
    q, r, s = L.c_void_p(8192), L.c_void_p(12288), L.c_void_p(16384)
    ws = 1 << 40

    def compose(cams=p, present=p, B=2, C=20, h=30, w=40, sal=q, alpha=12.0, cut=0.9, k=10, wsp=p, wsb=ws, label=r, sal_out=s):
        return lib.acr_sal_pseudo_compose(cams, present, B, C, h, w, sal, alpha, cut, k, wsp, wsb, label, sal_out, None)
    bad = [dict(cams=None), dict(present=None), dict(sal=None), dict(label=None), dict(sal_out=None), dict(wsp=None),
           dict(wsp=L.c_void_p(4098)), dict(B=0), dict(B=65536), dict(C=0), dict(C=128), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15),
           dict(alpha=0.0), dict(cut=-0.1), dict(cut=1.0), dict(k=-1), dict(k=33), dict(wsb=lib.acr_sal_pseudo_ws_bytes(2, 20, 30, 40) - 1),
           dict(label=q), dict(label=s, sal_out=s)]
    for kw in bad:
        assert compose(**kw) == -1, kw
        assert b"acr_sal_pseudo_compose" in lib.acr_last_error(), kw
    for args in ((None, 1, 5, 5, 3, q), (p, 1, 5, 5, 3, None), (p, 1, 5, 5, 3, p), (p, 0, 5, 5, 3, q), (p, 1, 0, 5, 3, q), (p, 1, 5, 0, 3, q),
                 (p, 1, 5, 5, 0, q), (p, 1, 5, 5, 33, q), (p, 65535, 1 << 15, 1 << 15, 3, q)):
        assert lib.acr_morph_open_u8(args[0], *args[1:5], args[5], None) == -1, args
        assert b"acr_morph_open_u8" in lib.acr_last_error(), args


def test_python_validates_before_it_asks_for_a_device(monkeypatch):
    from acr_wsss_amd import pseudo, segtrain
    from acr_wsss_amd._lib import AcrHipError
    g = _load("a")
    cams, present, sal = g["cams"][None], _present(g)[None], g["saliency"][None]
    for kw in (dict(bg_alpha=0), dict(cut=1.0), dict(cut=-0.5), dict(open_size=33), dict(open_size=-1), dict(open_size=2.5)):
        with pytest.raises(ValueError):
            pseudo.seg_label_saliency(cams, present, sal, **kw)
    with pytest.raises(ValueError):
        pseudo.morph_open(sal[0], k=0)
    with pytest.raises(AcrHipError):                     # no CPU path
        pseudo.seg_label_saliency(cams, present, sal, device="cpu")
    with pytest.raises(AcrHipError):
        pseudo.seg_label_saliency(torch.from_numpy(cams), torch.from_numpy(present), torch.from_numpy(sal))
    with pytest.raises(AcrHipError):
        pseudo.morph_open(torch.from_numpy(sal[0]))
    with pytest.raises(AcrHipError):
        segtrain.saliency_labels(torch.from_numpy(cams), torch.from_numpy(g["cam_label"][None]), torch.from_numpy(sal))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(AcrHipError):
        pseudo.seg_label_saliency(cams, present, sal)
    with pytest.raises(AcrHipError):
        pseudo.morph_open(sal[0])
