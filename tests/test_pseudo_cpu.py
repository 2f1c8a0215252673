"""Host side of the pseudo-label composition: the numpy restatement (tests/pseudo_ref.py) reproduces the reference's own runs of
compute_seg_label_rrm recorded in tests/golden/pseudo_{a..d}.npz (written by tests/golden/make_pseudo_golden.py), the fixtures are
decisive, the C ABI is declared and bound, the PNG writer round-trips, and the product refuses to run without a GPU.  Every
comparison is exact."""
import inspect
import os

import numpy as np
import pytest
import torch

import abi_checks
import pseudo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = {"a": (3, 48, 64), "b": (1, 33, 35), "c": (20, 40, 52), "d": (2, 30, 44)}


def _load(tag):
    z = np.load(os.path.join(GOLDEN, "pseudo_%s.npz" % tag))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_restatement_reproduces_the_reference(tag):
    g = _load(tag)
    classes = g["classes"].tolist()
    assert g["cams"].shape == SHAPES[tag] and g["cams"].dtype == np.float32
    assert g["la"].shape == g["ha"].shape == (SHAPES[tag][0] + 1,) + SHAPES[tag][1:]
    np.testing.assert_array_equal(R.label_map(g["la"], classes), g["la_label"])
    np.testing.assert_array_equal(R.label_map(g["ha"], classes), g["ha_label"])
    np.testing.assert_array_equal(R.seg_label(g["cams"], classes, g["la"], g["ha"]), g["label"])
    np.testing.assert_array_equal(R.seg_label(g["cams"], classes, g["la"], g["ha"], ignore_uncertain=True), g["label_sure"])
    not_sure, M = R.not_sure(g["cams"], classes, g["la"], g["ha"])
    np.testing.assert_array_equal(M, g["cam_img"])
    np.testing.assert_array_equal(not_sure, g["not_sure_region"])
    # the two expectations differ (the rule is exercised) and the recorded one is the reference's arrays under its own line
    want = g["label"].copy()
    want[g["not_sure_region"]] = 255
    np.testing.assert_array_equal(want, g["label_sure"])
    assert (g["label"] != g["label_sure"]).any() and (g["label_sure"] != 255).any()
    if tag == "d":
        assert not g["la_label"].any()
    if tag == "c":                                       # values on the 1/100 grid: the selected value has duplicates
        assert np.array_equal(g["cams"], (np.round(g["cams"] * 100) / 100).astype(np.float32))


@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_fixtures_are_decisive(tag):
    """bg is more than 1e-5 (relative) away from the largest class value and from bg_sure at every pixel: one pow or another
    (<= 1 ulp = 1.2e-7 apart) cannot change a comparison.  Every label of L_la owns a value above the floor where it wins."""
    g = _load(tag)
    classes = g["classes"].tolist()
    mg = R.margin(g["cams"], classes)
    print("pseudo_%s: margin %.3e" % (tag, mg))
    assert mg > 1e-5
    for l in np.unique(g["la_label"]):
        if l:
            assert ((g["cam_img"] == l) & (g["cams"][classes.index(l - 1)] > np.float32(0.1))).sum() >= 1


def test_a_label_that_never_wins_the_cams_has_no_sure_pixel():
    """n == 0: class 4 takes part of L_la, but its CAM never wins M above the floor -- the reference raises IndexError there;
    here none of its pixels is sure, and the other labels are judged as usual"""
    w, h = 6, 8
    cams = np.zeros((2, w, h), np.float32)
    cams[0, :, :4] = np.linspace(0.5, 0.9, w * 4, dtype=np.float32).reshape(w, 4)      # class 2 wins the left half
    cams[1, :, 4:] = 0.05                                                              # class 4: below the floor everywhere
    la = np.zeros((3, w, h), np.float32)
    la[1, :, :4] = 0.95
    la[2, :, 4:] = 0.95
    ha = la.copy()
    classes = [2, 4]
    assert R.margin(cams, classes) > 1e-5
    out = R.seg_label(cams, classes, la, ha, ignore_uncertain=True)
    assert (out[:, 4:] == 255).all()
    left = np.sort(cams[0, :, :4].ravel())
    v = left[int(len(left) * 0.3)]
    np.testing.assert_array_equal(out[:, :4], np.where(cams[0, :, :4] > v, 3, 255))
    np.testing.assert_array_equal(R.seg_label(cams, classes, la, ha), np.where(np.arange(h)[None] < 4, 3, 5) * np.ones((w, 1), np.uint8))
    # an absent label in L_la (every present plane negative there) is such a label too
    la2 = la.copy()
    la2[:, :, 4:] = -1.0
    assert (R.label_map(la2, classes)[:, 4:] == 1).all()
    assert (R.seg_label(cams, classes, la2, ha, ignore_uncertain=True)[:, 4:] == 255).all()


def test_pseudo_symbols_are_declared_and_bound():
    from acr_wsss_amd import _lib as L
    for name in ("acr_pseudo_label_f32", "acr_pseudo_compose", "acr_pseudo_ws_bytes"):
        assert abi_checks.declared(name) and name in L.SIGNATURES
    assert len([n for n in L.SIGNATURES if n.startswith("acr_pseudo_")]) <= 4
    src = open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "Makefile")).read()
    assert "pseudo.hip" in src


def test_ws_bytes_is_a_host_only_query():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    small, big = lib.acr_pseudo_ws_bytes(1, 33, 35), lib.acr_pseudo_ws_bytes(20, 375, 500)
    assert 0 < small < big and big >= 4 * (4 * 20 * 256) + 375 * 500
    assert lib.acr_pseudo_ws_bytes(0, 10, 10) < 0 and lib.acr_pseudo_ws_bytes(128, 10, 10) < 0 and lib.acr_pseudo_ws_bytes(3, 0, 10) < 0


def test_png_round_trip_and_voc_palette(tmp_path):
    from PIL import Image
    from acr_wsss_amd import pseudo
    rng = np.random.default_rng(1)
    label = rng.choice(np.array(list(range(21)) + [255], np.uint8), (37, 53))
    path = str(tmp_path / "x.png")
    pseudo.save_label_png(path, label)
    im = Image.open(path)
    assert im.mode == "P"
    got = np.array(im)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, label)
    pal = np.asarray(im.getpalette(), np.uint8).reshape(-1, 3)
    assert pal.shape == (256, 3)
    for i, rgb in ((0, (0, 0, 0)), (1, (128, 0, 0)), (15, (192, 128, 128)), (255, (224, 224, 192))):
        assert tuple(pal[i]) == rgb, (i, pal[i])
    np.testing.assert_array_equal(pal, pseudo.voc_palette())
    with pytest.raises(ValueError):
        pseudo.save_label_png(path, label.astype(np.int64))


def test_infer_cam_list_rejects_an_unknown_pseudo_source(tmp_path):
    from acr_wsss_amd import infer_cam
    p = inspect.signature(infer_cam.infer_cam_list).parameters
    assert p["out_pseudo"].default is None and p["pseudo_source"].default == "crf"
    assert p["pseudo_uncertain"].default is False and p["pseudo_bg_alpha"].default == 36
    model = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="pseudo_source"):
        infer_cam.infer_cam_list(model, [], out_pseudo=str(tmp_path / "p"), pseudo_source="saliency")


def test_seg_label_raises_without_a_gpu(monkeypatch):
    from acr_wsss_amd import pseudo
    from acr_wsss_amd._lib import AcrHipError
    g = _load("b")
    args = (g["cams"], g["classes"].tolist(), g["la"], g["ha"])
    with pytest.raises(AcrHipError):
        pseudo.seg_label(*args, device="cpu")
    with pytest.raises(AcrHipError):
        pseudo.seg_label(torch.from_numpy(g["cams"]), args[1], torch.from_numpy(g["la"]), torch.from_numpy(g["ha"]))
    with pytest.raises(AcrHipError):
        pseudo.label_map(torch.from_numpy(g["la"]), [0, 6])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(AcrHipError):
        pseudo.seg_label(*args)
    with pytest.raises(AcrHipError):
        pseudo.seg_label(*args, ignore_uncertain=True)
    with pytest.raises(AcrHipError):
        pseudo.seg_label_from_dicts({5: g["cams"][0]}, {0: g["la"][0], 6: g["la"][1]}, {0: g["ha"][0], 6: g["ha"][1]})
    with pytest.raises(AcrHipError):
        pseudo.label_map(g["la"], [0, 6])
