"""Pseudo-label composition on the device (csrc/pseudo.hip behind acr_pseudo_label_f32 / acr_pseudo_compose) against the
reference's own runs (tests/golden/pseudo_{a..d}.npz) and against the numpy restatement tests/pseudo_ref.py -- pinned to those runs
by test_pseudo_cpu.py -- on seeded inputs.  Outputs are uint8 labels: every comparison is exact equality.  Seeded inputs are
checked to be decisive (pseudo_ref.margin > 1e-5) before the device is asked, so that no comparison hangs on the last bit of a pow."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pseudo_ref as R
from acr_wsss_amd import evaluation as E
from acr_wsss_amd import pseudo as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _both(cams, classes, la, ha, what, **kw):
    """device == restatement for both settings of ignore_uncertain; returns the two device maps (numpy)"""
    assert R.margin(cams, classes, kw.get("bg_alpha", 36), kw.get("bg_sure", 0.3), kw.get("num_classes", 20)) > 1e-5, what
    outs = []
    for unc in (False, True):
        got = P.seg_label(cams, classes, la, ha, ignore_uncertain=unc, device=DEV, **kw)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == cams.shape[1:]
        np.testing.assert_array_equal(got.cpu().numpy(), R.seg_label(cams, classes, la, ha, ignore_uncertain=unc, **kw),
                                      err_msg="%s ignore_uncertain=%s" % (what, unc))
        outs.append(got.cpu().numpy())
    return outs


@pytest.mark.parametrize("unc", [False, True])
@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_fixtures_written_by_the_reference(tag, unc):
    g = np.load(os.path.join(GOLDEN, "pseudo_%s.npz" % tag))
    classes = g["classes"].tolist()
    got = P.seg_label(g["cams"], classes, g["la"], g["ha"], ignore_uncertain=unc, device=DEV)
    np.testing.assert_array_equal(got.cpu().numpy(), g["label_sure" if unc else "label"])
    labels = [0] + [c + 1 for c in classes]
    np.testing.assert_array_equal(P.label_map(g["la"], labels, device=DEV).cpu().numpy(), g["la_label"])
    np.testing.assert_array_equal(P.label_map(g["ha"], labels, device=DEV).cpu().numpy(), g["ha_label"])


SEEDED = {
    "33x35 K=2": dict(seed=1, k=2, w=33, h=35, classes=[3, 11]),
    "120x130 K=20 rounded to 1/100": dict(seed=2, k=20, w=120, h=130, classes=list(range(20)), round_to=100),
    "61x67 K=3": dict(seed=3, k=3, w=61, h=67, classes=[0, 7, 19]),
    "all-background L_la": dict(seed=4, k=2, w=30, h=44, classes=[3, 19], bg_bias=5.0),
    "K=1 < C": dict(seed=5, k=1, w=40, h=50, classes=[14]),
    "K=C=80 (histograms above 64 KB of LDS)": dict(seed=15, k=80, w=40, h=45, classes=list(range(80)), num_classes=80),
}


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_device_equals_the_restatement(name):
    cams, classes, la, ha, _ = R.decisive_case(**SEEDED[name])
    plain, sure = _both(cams, classes, la, ha, name, num_classes=SEEDED[name].get("num_classes", 20))
    assert (sure == 255).any() and (sure != 255).any()
    if name.startswith("all-background"):
        assert not R.label_map(la, classes).any() and set(np.unique(plain)) == {0, 255}
    if "rounded" in name:                                # many workgroups (61 of 256 pixels), heavy ties at the selected value
        M = R.cam_label(cams, classes)[0]
        for j in (0, 7):
            S = np.sort(cams[j][(M == j + 1) & (cams[j] > np.float32(0.1))])
            assert (S == S[int(len(S) * 0.3)]).sum() > 1


def test_device_equals_the_restatement_at_375x500_once():
    cams, classes, la, ha, _ = R.decisive_case(seed=6, k=3, w=375, h=500, classes=[1, 8, 14])
    _both(cams, classes, la, ha, "375x500 K=3")


def test_quantile_parameters_and_other_thresholds():
    cams, classes, la, ha, _ = R.decisive_case(seed=7, k=3, w=45, h=52, classes=[2, 5, 9])
    _, sure0 = _both(cams, classes, la, ha, "fg_quantile=0", fg_quantile=0.0)
    _, sure3 = _both(cams, classes, la, ha, "defaults")
    assert (sure0 != 255).sum() > (sure3 != 255).sum()   # v = min(S): everything above the smallest value is sure
    _both(cams, classes, la, ha, "fg_quantile=0.999", fg_quantile=0.999)
    _both(cams, classes, la, ha, "other constants", bg_alpha=12, cam_floor=0.25, fg_quantile=0.6, bg_sure=0.5, crf_sure=0.6)
    _both(cams, classes, la, ha, "cam_floor=0", cam_floor=0.0)
    _both(cams, classes, la, ha, "coco", num_classes=80)


def test_a_class_in_l_la_that_never_wins_m_and_a_one_element_set():
    """n = 0: class 4 holds the right half of L_la but its CAM stays below the floor, so it never enters a selection set (the
    reference raises there; defined: not sure).  n = 1: class 9 wins M at one pixel only, v is that value and, the comparison
    being strict, that pixel is not sure either."""
    w, h = 24, 40
    rng = np.random.default_rng(8)
    cams = np.zeros((3, w, h), np.float32)
    cams[0, :, :20] = (0.5 + 0.4 * rng.random((w, 20))).astype(np.float32)            # class 2: the left half
    cams[1, :, 20:] = 0.05                                                             # class 4: below the floor everywhere
    cams[2, 3, 30] = 0.97                                                              # class 9: one pixel
    la = np.full((4, w, h), 0.01, np.float32)
    la[1, :, :20] = 0.95
    la[2, :, 20:] = 0.95
    la[2, 3, 30], la[3, 3, 30] = 0.02, 0.96
    ha = la.copy()
    classes = [2, 4, 9]
    M = R.cam_label(cams, classes)[0]
    assert (M == 10).sum() == 1 and not (M == 5).any() and set(np.unique(R.label_map(la, classes))) == {3, 5, 10}
    plain, sure = _both(cams, classes, la, ha, "n = 0 and n = 1")
    assert plain[3, 30] == 10 and sure[3, 30] == 255 and (sure[:, 20:] == 255).all() and (sure[:, :20] == 3).any()
    # with fg_quantile = 0 the one-element set still selects its own value, and nothing lies strictly above it
    assert _both(cams, classes, la, ha, "n = 1, q = 0", fg_quantile=0.0)[1][3, 30] == 255


def test_absent_labels_and_full_class_sets():
    """K = C = 20 (no absent label, no extra 0.0 in m) is the rounded case above and fixture c; here K = 1 < C with a stack whose
    present planes are all negative in a region, so that the zero plane of the smallest absent label wins, as in test_eval_gpu's
    'all negative' case -- for class 0 present (absent label 2) and class 0 absent (absent label 1)."""
    for classes in ([0], [6]):
        cams, classes, la, ha, _ = R.decisive_case(seed=9, k=1, w=33, h=35, classes=classes)
        la, ha = la.copy(), ha.copy()
        la[:, :10] = -la[:, :10]
        ha[:, :15] = -ha[:, :15] - 1
        cams = cams.copy()
        cams[:, 20:] = -0.25                                   # negative CAMs: the 0.0 of the absent classes is the maximum there
        absent = 2 if classes == [0] else 1
        assert (R.label_map(la, classes)[:10] == absent).all() and (R.label_map(ha, classes)[:15] == absent).all()
        plain, _ = _both(cams, classes, la, ha, "absent label, classes %s" % classes)
        assert (plain[:10] == absent).all()
        labels = [0] + [c + 1 for c in classes]
        for s in (la, ha):
            np.testing.assert_array_equal(P.label_map(s, labels, device=DEV).cpu().numpy(), R.label_map(s, classes))
    full = np.random.default_rng(10).standard_normal((21, 37, 41)).astype(np.float32)      # K = C: signs do not matter
    np.testing.assert_array_equal(P.label_map(full, list(range(21)), device=DEV).cpu().numpy(), full.argmax(0).astype(np.uint8))


def test_label_map_equals_evaluation_label_map_on_refined_dicts():
    for seed, classes in ((11, [2, 9]), (12, [0, 5, 17, 19])):
        cams, classes, la, ha, _ = R.decisive_case(seed=seed, k=len(classes), w=50, h=70, classes=classes)
        for s in (la, ha):
            d = {0: s[0]}
            d.update({c + 1: s[j + 1] for j, c in enumerate(classes)})
            got = P.label_map(torch.from_numpy(s).to(DEV), sorted(d))
            np.testing.assert_array_equal(got.cpu().numpy(), E.label_map(d))


def test_two_calls_give_identical_bytes_and_dicts_are_taken():
    cams, classes, la, ha, _ = R.decisive_case(seed=13, k=4, w=90, h=110, classes=[1, 4, 8, 15])
    dev = [torch.from_numpy(a).to(DEV) for a in (cams, la, ha)]
    a = P.seg_label(dev[0], classes, dev[1], dev[2], ignore_uncertain=True)
    b = P.seg_label(dev[0], classes, dev[1], dev[2], ignore_uncertain=True)
    assert torch.equal(a, b) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    cam_dict = {c: cams[j] for j, c in enumerate(classes)}
    la_dict, ha_dict = ({l: s[i] for i, l in enumerate([0] + [c + 1 for c in classes])} for s in (la, ha))
    got = P.seg_label_from_dicts(cam_dict, la_dict, ha_dict, ignore_uncertain=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, a.cpu().numpy())
    with pytest.raises(ValueError):
        P.seg_label_from_dicts(cam_dict, {0: la[0]}, ha_dict)
    with pytest.raises(ValueError):
        P.seg_label(dev[0], classes[::-1], dev[1], dev[2])
    with pytest.raises(ValueError):
        P.seg_label(dev[0], classes, dev[1][:4], dev[2])
    with pytest.raises(ValueError):
        P.seg_label(dev[0], classes, dev[1], dev[2], ignore_uncertain=True, fg_quantile=1.0)


def test_c_abi_launches_capture_into_a_hip_graph():
    """the entry points only enqueue work (the workspace is cleared on the stream): one chain, captured once, replays with the
    result of the eager call -- also after the outputs and the workspace were overwritten"""
    from acr_wsss_amd import _lib as L
    lib = L.load()
    cams_np, classes, la_np, ha_np, _ = R.decisive_case(seed=14, k=3, w=120, h=160, classes=[1, 8, 14])
    k, w, h = cams_np.shape
    arr = (ctypes.c_int32 * k)(*classes)
    cams, la, ha = (torch.from_numpy(a).to(DEV) for a in (cams_np, la_np, ha_np))
    nbytes = lib.acr_pseudo_ws_bytes(k, w, h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lab = torch.zeros((w, h), dtype=torch.uint8, device=DEV)
    plain = torch.zeros((w, h), dtype=torch.uint8, device=DEV)
    sure = torch.zeros((w, h), dtype=torch.uint8, device=DEV)

    def launch():
        st = L.stream_ptr()
        L.check(lib.acr_pseudo_label_f32(L.ptr(la), arr, k, w, h, 20, L.ptr(lab), st), "label")
        L.check(lib.acr_pseudo_compose(L.ptr(cams), arr, k, L.ptr(la), L.ptr(ha), w, h, 20, 0, 36.0, 0.1, 0.3, 0.3, 0.8, None, 0,
                                       L.ptr(plain), st), "compose")
        L.check(lib.acr_pseudo_compose(L.ptr(cams), arr, k, L.ptr(la), L.ptr(ha), w, h, 20, 1, 36.0, 0.1, 0.3, 0.3, 0.8, L.ptr(ws), nbytes,
                                       L.ptr(sure), st), "compose")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = (R.label_map(la_np, classes), R.seg_label(cams_np, classes, la_np, ha_np), R.seg_label(cams_np, classes, la_np, ha_np, True))
    for got, ref in zip((lab, plain, sure), want):
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for rep in range(2):
        lab.fill_(7); plain.fill_(7); sure.fill_(7); ws.fill_(0xAB)
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip((lab, plain, sure), want):
            np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg="replay %d" % rep)

    # bad arguments: negative code and a message, nothing launched
    def refused(rc, word):
        assert rc == -1 and word in lib.acr_last_error().decode(), lib.acr_last_error().decode()

    st = L.stream_ptr()
    before = sure.clone()
    refused(lib.acr_pseudo_label_f32(None, arr, k, w, h, 20, L.ptr(lab), st), "null pointer")
    refused(lib.acr_pseudo_label_f32(L.ptr(la), arr, k, w, h, 128, L.ptr(lab), st), "num_classes=128")
    refused(lib.acr_pseudo_label_f32(L.ptr(la), arr, 0, w, h, 20, L.ptr(lab), st), "K=0")
    refused(lib.acr_pseudo_label_f32(L.ptr(la), (ctypes.c_int32 * 3)(8, 1, 14), k, w, h, 20, L.ptr(lab), st), "ascending")
    refused(lib.acr_pseudo_label_f32(L.ptr(la), (ctypes.c_int32 * 3)(1, 8, 20), k, w, h, 20, L.ptr(lab), st), "outside")
    args = (L.ptr(cams), arr, k, L.ptr(la), L.ptr(ha), w, h, 20, 1)
    refused(lib.acr_pseudo_compose(*args, 36.0, -0.1, 0.3, 0.3, 0.8, L.ptr(ws), nbytes, L.ptr(sure), st), "cam_floor")
    refused(lib.acr_pseudo_compose(*args, 36.0, 0.1, 1.0, 0.3, 0.8, L.ptr(ws), nbytes, L.ptr(sure), st), "fg_quantile")
    refused(lib.acr_pseudo_compose(*args, 36.0, 0.1, 0.3, 0.3, 0.0, L.ptr(ws), nbytes, L.ptr(sure), st), "crf_sure")
    refused(lib.acr_pseudo_compose(*args, 36.0, 0.1, 0.3, 0.3, 0.8, None, nbytes, L.ptr(sure), st), "workspace")
    refused(lib.acr_pseudo_compose(*args, 36.0, 0.1, 0.3, 0.3, 0.8, L.ptr(ws), nbytes - 1, L.ptr(sure), st), "needed")
    torch.cuda.synchronize()
    assert torch.equal(sure, before)


def _tiny_model():
    from conftest import recipe_sd
    from acr_wsss_amd.DPT.ACR import ACR
    m = ACR(num_classes=20, backbone_name="vit_tiny", use_pretrain=False)
    missing = m.load_state_dict(recipe_sd("tiny"), strict=False)
    assert all(k.startswith("scratch.") for k in missing.missing_keys) and not missing.unexpected_keys
    return m.to(DEV)


@pytest.mark.parametrize("source", ["crf", "pamr"])
def test_infer_cam_list_writes_pseudo_labels(tmp_path, source):
    """out_pseudo: <out_pseudo>/<name>.png equals seg_label_from_dicts applied to the dictionaries the same call wrote with
    out_cam and out_crf / out_pamr; evaluate.pseudo equals LabelCounters fed those PNGs; an image without a positive class gets an
    all-background PNG and is not scored; without out_pseudo the call's files and return value are those of before"""
    from PIL import Image
    from recipe import make_inputs
    from acr_wsss_amd.infer_cam import infer_cam_list
    model = _tiny_model()
    rng = np.random.default_rng(0)
    items, gts = [], {}
    for i, (classes, hw) in enumerate((([2, 9], (40, 52)), ([0, 5, 17], (50, 70)), ([], (40, 52)))):
        img, _ = make_inputs(1, 64, 20, 20 + i)
        label = torch.zeros(1, 20)
        for c in classes:
            label[0, c] = 1
        items.append(("im%d" % i, img, label, hw, rng.integers(0, 256, hw + (3,)).astype(np.uint8)))
        gt = rng.integers(0, 21, hw).astype(np.uint8)
        gt[rng.random(hw) < 0.1] = 255
        gts["im%d" % i] = gt
    refine = "out_%s" % source
    outs = lambda tag: {"out_cam": str(tmp_path / tag / "cam"), refine: str(tmp_path / tag / source), "low_alpha": 1, "high_alpha": 12}
    plain = infer_cam_list(model, items, **outs("plain"))
    for unc in (False, True):
        tag = "unc%d" % unc
        ev = E.CamEvaluation(gts.__getitem__)
        res = infer_cam_list(model, items, evaluate=ev, out_pseudo=str(tmp_path / tag / "png"), pseudo_source=source,
                             pseudo_uncertain=unc, **outs(tag))
        assert sorted(os.listdir(str(tmp_path / tag / "png"))) == ["im0.png", "im1.png", "im2.png"]
        lc = E.LabelCounters(21)
        for name in ("im0", "im1"):
            load = lambda folder: np.load(str(tmp_path / tag / folder / (name + ".npy")), allow_pickle=True).item()
            want = P.seg_label_from_dicts(load("cam"), load("%s_1" % source), load("%s_12" % source), ignore_uncertain=unc)
            im = Image.open(str(tmp_path / tag / "png" / (name + ".png")))
            assert im.mode == "P"
            np.testing.assert_array_equal(np.array(im), want, err_msg="%s %s" % (tag, name))
            lc.add(np.array(im), gts[name])
        np.testing.assert_array_equal(np.array(Image.open(str(tmp_path / tag / "png" / "im2.png"))), np.zeros((40, 52), np.uint8))
        np.testing.assert_array_equal(ev.pseudo.to_host().conf, lc.conf)
        assert lc.conf.sum() == ((gts["im0"] < 21).sum() + (gts["im1"] < 21).sum())
        # the other outputs are those of the call without out_pseudo
        assert sorted(res) == sorted(plain)
        for name in res:
            assert sorted(res[name]) == sorted(plain[name])
            for c in res[name]:
                np.testing.assert_array_equal(res[name][c], plain[name][c])
        for folder in ("cam", "%s_1" % source, "%s_12" % source):
            files = sorted(os.listdir(str(tmp_path / "plain" / folder)))
            assert files == sorted(os.listdir(str(tmp_path / tag / folder)))
            for f in files:
                with open(str(tmp_path / "plain" / folder / f), "rb") as f0, open(str(tmp_path / tag / folder / f), "rb") as f1:
                    assert f0.read() == f1.read(), (folder, f)
    # out_pseudo alone runs the refinement by itself and writes the same masks; no refinement files appear
    infer_cam_list(model, items, out_pseudo=str(tmp_path / "alone" / "png"), pseudo_source=source, pseudo_uncertain=True, low_alpha=1,
                   high_alpha=12)
    assert os.listdir(str(tmp_path / "alone")) == ["png"]
    for name in ("im0", "im1", "im2"):
        with open(str(tmp_path / "alone" / "png" / (name + ".png")), "rb") as f0, open(str(tmp_path / "unc1" / "png" / (name + ".png")), "rb") as f1:
            assert f0.read() == f1.read(), name
    ev = E.CamEvaluation(gts.__getitem__)
    infer_cam_list(model, items, evaluate=ev)
    assert ev.pseudo is None
    with pytest.raises(ValueError):
        infer_cam_list(model, [items[0][:4]], out_pseudo=str(tmp_path / "x"))
