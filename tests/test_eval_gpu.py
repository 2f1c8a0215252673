"""Device CAM evaluation (csrc/eval.hip behind acr_eval_sweep_f32 / acr_eval_sweep_finish / acr_eval_confusion_u8) against the
numpy counters of ``evaluation.SweepCounters`` -- pinned by test_evaluation_cpu.py to the reference's per-threshold loop --, against
that loop itself (oracle.acr_oracle.seeds_from_cam_dict + iou_counts) and against tests/eval_ref.py.  All outputs are integers:
every comparison is exact equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eval_ref as R
from oracle import acr_oracle as O
from acr_wsss_amd import evaluation as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
T100 = np.arange(100, dtype=np.float32) / 100.0


def _assert_counters_equal(got, want, what=""):
    for name in ("TP", "P", "T"):
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg="%s %s" % (what, name))


def _host(images, thresholds=T100, num_cls=21):
    sc = E.SweepCounters(thresholds, num_cls)
    for cam_dict, gt in images:
        sc.add(cam_dict, gt)
    return sc


def _device(images, thresholds=T100, num_cls=21):
    dc = E.DeviceSweepCounters(thresholds, num_cls, DEV)
    for cam_dict, gt in images:
        cams, keys = R.stack(cam_dict)
        dc.add(torch.from_numpy(cams).to(DEV), keys, gt)
    return dc


def _gt(rng, h, w, num_cls=21, ignore=0.15):
    gt = rng.integers(0, num_cls, (h, w)).astype(np.uint8)
    gt[rng.random((h, w)) < ignore] = 255
    return gt


def _blobs(rng, classes, h, w):
    """A CAM-like case: exact zeros with a few smooth bumps per class, and a blocky ground truth."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    cams = {}
    for c in classes:
        plane = np.zeros((h, w), np.float32)
        for _ in range(2):
            cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.2) * min(h, w) + 1
            plane = np.maximum(plane, np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32))
        plane[plane < 0.05] = 0.0
        cams[c] = plane / max(float(plane.max()), 1e-6)
    gt = np.zeros((h, w), np.uint8)
    for c in classes:
        y0, x0 = int(rng.integers(0, max(h - 2, 1))), int(rng.integers(0, max(w - 2, 1)))
        gt[y0:y0 + h // 3 + 1, x0:x0 + w // 3 + 1] = c + 1
    gt[:, :2] = 255
    return cams, gt


def _seeded_cases():
    rng = np.random.default_rng(21)
    cases = {"four": R.four_cases()}
    for n, classes in ((1, [14]), (3, [1, 8, 14]), (20, list(range(20)))):
        cases["375x500 n=%d" % n] = [R.image_case(rng, 375, 500, classes)]
        cases["375x500 blobs n=%d" % n] = [_blobs(rng, classes, 375, 500)]
    neg = {c: (rng.random((60, 70)).astype(np.float32) - 0.5) for c in (0, 4, 5)}
    neg[4][:] = 0.0                                                          # an all-zero plane
    cases["negative and all-zero planes"] = [(neg, _gt(rng, 60, 70))]
    allneg = {c: -rng.random((33, 35)).astype(np.float32) for c in (0, 1)}   # class 2's absent plane wins everywhere
    cases["all negative"] = [(allneg, _gt(rng, 33, 35))]
    for step in (10, 100):
        d = {c: (np.round(rng.random((90, 110)).astype(np.float32) * step) / step).astype(np.float32) for c in (2, 3, 11, 19)}
        cases["rounded to 1/%d" % step] = [(d, _gt(rng, 90, 110))]
    d2 = {c: rng.choice(T100, (40, 50)).astype(np.float32) for c in (0, 1)}
    cases["on thresholds"] = [(d2, _gt(rng, 40, 50))]
    cases["all ignore"] = [({3: rng.random((20, 30)).astype(np.float32)}, np.full((20, 30), 255, np.uint8))]
    cases["1x1"] = [({5: np.array([[0.7]], np.float32)}, np.array([[6]], np.uint8)),
                    ({5: np.array([[0.0]], np.float32)}, np.array([[0]], np.uint8))]
    cases["7x13"] = [R.image_case(rng, 7, 13, [0, 19], ties=True)]
    return cases


CASES = _seeded_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_sweep_equals_numpy_counters(name):
    images = CASES[name]
    _assert_counters_equal(_device(images).to_host(), _host(images), name)


def test_device_sweep_coco_and_threshold_grids():
    rng = np.random.default_rng(22)
    coco = {c: rng.random((50, 64)).astype(np.float32) for c in range(80)}
    coco[7] = np.round(coco[7] * 10) / 10
    images = [(coco, _gt(rng, 50, 64, 81)), ({0: rng.random((31, 40)).astype(np.float32), 79: rng.random((31, 40)).astype(np.float32)},
                                             _gt(rng, 31, 40, 81))]
    _assert_counters_equal(_device(images, T100, 81).to_host(), _host(images, T100, 81), "coco")
    images = [R.image_case(rng, 64, 80, [0, 7, 19], ties=True), R.image_case(rng, 50, 50, [4])]
    for t in (np.array([0.3], np.float32), np.arange(256, dtype=np.float32) / 256.0, np.linspace(-0.2, 1.2, 57).astype(np.float32)):
        _assert_counters_equal(_device(images, t).to_host(), _host(images, t), "nt=%d" % len(t))
    # the default grid is evaluate_cam_dir's
    np.testing.assert_array_equal(E.DeviceSweepCounters(device=DEV).t, T100)
    # raw histograms themselves against the restatement of the header
    dc = _device(images)
    raw = None
    for cam_dict, gt in images:
        cams, keys = R.stack(cam_dict)
        raw = R.sweep_raw_fast(cams, keys, gt, T100, 21, raw)
    np.testing.assert_array_equal(dc._raw.cpu().numpy(), raw)


@pytest.mark.parametrize("nt,num_cls,path", [(199, 81, "the largest histogram kept in LDS (130728 bytes)"),
                                             (256, 81, "counted straight into the global counters"),
                                             (256, 128, "counted straight into the global counters, both limits")])
def test_device_sweep_large_histograms(nt, num_cls, path):
    """A histogram of 2 (nt + 1) num_cls + nt + num_cls + 2 counters lives in LDS up to 128 KB (32768 counters) and is counted
    straight into the global counters beyond: one case just under that size and two over it, structured and unstructured
    input, two images so that the counters accumulate."""
    words = R.raw_size(nt, num_cls)
    assert (words <= 32768) == path.startswith("the largest"), words
    rng = np.random.default_rng(25)
    t = np.arange(nt, dtype=np.float32) / nt
    n = num_cls - 1
    noise = {c: rng.random((70, 90)).astype(np.float32) for c in range(n)}
    noise[3] = np.round(noise[3] * 8) / 8                                          # values on thresholds (nt = 256), ties
    some = sorted(rng.choice(n, 5, replace=False).tolist())
    blobs, gt_b = _blobs(rng, some, 120, 150)
    images = [(noise, _gt(rng, 70, 90, num_cls)), (blobs, gt_b)]
    dc = _device(images, t, num_cls)
    _assert_counters_equal(dc.to_host(), _host(images, t, num_cls), path)
    raw = None
    for cam_dict, gt in images:
        cams, keys = R.stack(cam_dict)
        raw = R.sweep_raw_fast(cams, keys, gt, t, num_cls, raw)
    np.testing.assert_array_equal(dc._raw.cpu().numpy(), raw)
    assert torch.equal(dc._raw, _device(images, t, num_cls)._raw)                  # identical bits run to run


def test_device_sweep_equals_the_reference_loop():
    images = R.four_cases() + CASES["rounded to 1/10"] + CASES["negative and all-zero planes"]
    sc = _device(images).to_host()
    for k in (0, 1, 20, 40, 50, 77, 99):
        TP = np.zeros(21, np.int64); P = np.zeros(21, np.int64); T = np.zeros(21, np.int64)
        for cams, gt in images:
            pred = O.seeds_from_cam_dict(cams, T100[k])
            tp, p, t = O.iou_counts(pred, gt)
            TP += tp; P += p; T += t
        np.testing.assert_array_equal(sc.TP[k], TP, err_msg="TP t=%.2f" % T100[k])
        np.testing.assert_array_equal(sc.P[k], P, err_msg="P t=%.2f" % T100[k])
        np.testing.assert_array_equal(sc.T, T)
        assert abs(sc.miou()[0][k] - O.miou(TP, P, T)) < 1e-9


def test_accumulation_reset_merge_and_reproducible_bits():
    images = R.four_cases() + CASES["375x500 blobs n=3"] + CASES["7x13"]        # different sizes in sequence
    whole = _device(images)
    want = _host(images)
    _assert_counters_equal(whole.to_host(), want, "sequence")
    _assert_counters_equal(whole.to_host(), want, "to_host twice")                # finish does not accumulate
    separate = E.SweepCounters(T100)
    for im in images:
        separate.merge(_device([im]).to_host())
    _assert_counters_equal(separate, want, "sum of separate counters")
    a, b = _device(images[0::2]), _device(images[1::2])
    _assert_counters_equal(a.to_host().merge(b.to_host()), want, "halves merged")
    raw1 = whole._raw.clone()
    assert torch.equal(raw1, _device(images)._raw)                              # two runs, identical bits
    whole.reset()
    assert int(whole._raw.abs().sum()) == 0
    for im in images[:2]:
        cams, keys = R.stack(im[0])
        whole.add(torch.from_numpy(cams).to(DEV), keys, torch.from_numpy(im[1]).to(DEV))     # a device gt
    _assert_counters_equal(whole.to_host(), _host(images[:2]), "after reset")
    d = E.DeviceSweepCounters(device=DEV)
    for cam_dict, gt in images:
        d.add_dict(cam_dict, gt)
    _assert_counters_equal(d.to_host(), want, "add_dict")
    np.testing.assert_array_equal(d.miou()[0], want.miou()[0])


def test_device_label_counters():
    rng = np.random.default_rng(23)
    images = []
    for h, w in ((375, 500), (31, 27), (1, 1), (7, 13)):
        gt = rng.integers(0, 21, (h, w)).astype(np.uint8)
        gt[rng.random((h, w)) < 0.1] = 255
        gt[rng.random((h, w)) < 0.03] = 100                                      # ignored like 255 (documented deviation)
        pred = np.where(rng.random((h, w)) < 0.6, np.minimum(gt, 20), rng.integers(0, 21, (h, w))).astype(np.uint8)
        out = rng.random((h, w)) < 0.05
        pred[out] = rng.choice(np.array([21, 40, 254, 255], np.uint8), int(out.sum()))
        images.append((pred, gt))
    blocky = np.zeros((200, 300), np.uint8)
    blocky[50:120, 80:200] = 15
    images.append((blocky, np.roll(blocky, 9, axis=1)))
    dl = E.DeviceLabelCounters(21, DEV)
    conf = None
    TP = np.zeros(21, np.int64); P = np.zeros(21, np.int64); T = np.zeros(21, np.int64)
    for i, (pred, gt) in enumerate(images):
        if i % 2:
            dl.add(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
        else:
            dl.add(pred, gt)
        conf = R.confusion(pred, gt, 21, conf)
        tp, p, t = O.iou_counts(pred, np.where(gt < 21, gt, 255).astype(np.uint8))
        TP += tp; P += p; T += t
    lc = dl.to_host()
    np.testing.assert_array_equal(lc.conf, conf)
    np.testing.assert_array_equal(lc.TP, TP)
    np.testing.assert_array_equal(lc.P, P)
    np.testing.assert_array_equal(lc.T, T)
    assert lc.miou()[0] == O.miou(TP, P, T)
    assert lc.conf[:, 21].sum() > 0
    first = dl._conf.clone()
    dl.reset()
    assert int(dl._conf.sum()) == 0
    for pred, gt in images:
        dl.add(pred, gt)
    assert torch.equal(dl._conf, first)
    big = E.DeviceLabelCounters(128, DEV)                                        # the largest matrix the ABI takes
    pred = rng.integers(0, 256, (64, 64)).astype(np.uint8)
    gt = rng.integers(0, 256, (64, 64)).astype(np.uint8)
    big.add(pred, gt)
    np.testing.assert_array_equal(big.to_host().conf, R.confusion(pred, gt, 128))


def test_c_abi_launches_capture_into_a_hip_graph():
    """the three entry points only enqueue work: one chain, captured once; two replays accumulate twice, and finish after the
    replays equals the eager result"""
    from acr_wsss_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(24)
    n, h, w, nt, nc = 3, 120, 160, 100, 21
    classes = (ctypes.c_int32 * n)(1, 8, 14)
    cam_dict, gt_np = _blobs(rng, [1, 8, 14], h, w)
    cams = torch.from_numpy(R.stack(cam_dict)[0]).to(DEV)
    gt = torch.from_numpy(gt_np).to(DEV)
    pred = torch.from_numpy(rng.integers(0, 23, (h, w)).astype(np.uint8)).to(DEV)
    th = torch.from_numpy(T100).to(DEV)
    raw = torch.zeros(R.raw_size(nt, nc), dtype=torch.int64, device=DEV)
    conf = torch.zeros((nc, nc + 1), dtype=torch.int64, device=DEV)
    TP = torch.zeros((nt, nc), dtype=torch.int64, device=DEV)
    P = torch.zeros((nt, nc), dtype=torch.int64, device=DEV)

    def launch():
        st = L.stream_ptr()
        L.check(lib.acr_eval_sweep_f32(L.ptr(cams), classes, n, L.ptr(gt), h, w, L.ptr(th), nt, nc, L.ptr(raw), st), "sweep")
        L.check(lib.acr_eval_confusion_u8(L.ptr(pred), L.ptr(gt), h * w, nc, L.ptr(conf), st), "confusion")
        L.check(lib.acr_eval_sweep_finish(L.ptr(raw), nt, nc, L.ptr(TP), L.ptr(P), st), "finish")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    raw1, conf1, TP1, P1 = raw.clone(), conf.clone(), TP.clone(), P.clone()
    np.testing.assert_array_equal(raw1.cpu().numpy(), R.sweep_raw_fast(R.stack(cam_dict)[0], [1, 8, 14], gt_np, T100, nc))
    np.testing.assert_array_equal(conf1.cpu().numpy(), R.confusion(pred.cpu().numpy(), gt_np, nc))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    raw.zero_(); conf.zero_(); TP.zero_(); P.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(raw, raw1) and torch.equal(conf, conf1) and torch.equal(TP, TP1) and torch.equal(P, P1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(raw, 2 * raw1) and torch.equal(conf, 2 * conf1)
    assert torch.equal(TP, 2 * TP1) and torch.equal(P, 2 * P1)              # finish is linear in raw: it WROTE the doubled counters
    launch()                                                                 # eager, third accumulation
    torch.cuda.synchronize()
    assert torch.equal(raw, 3 * raw1) and torch.equal(TP, 3 * TP1) and torch.equal(P, 3 * P1)


def test_errors_are_loud():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    dc = E.DeviceSweepCounters(device=DEV)
    cams = torch.rand(2, 12, 16, device=DEV)
    gt = torch.zeros(12, 16, dtype=torch.uint8, device=DEV)
    dc.add(cams, [3, 5], gt)
    with pytest.raises(ValueError):
        dc.add(cams.double(), [3, 5], gt)                    # wrong dtype
    with pytest.raises(ValueError):
        dc.add(cams, [3, 5], gt.int())
    with pytest.raises(ValueError):
        dc.add(cams, [3, 5], np.zeros((12, 16), np.int64))
    with pytest.raises(ValueError):
        dc.add(cams.transpose(1, 2), [3, 5], gt.t())         # not contiguous
    with pytest.raises(ValueError):
        dc.add(cams, [3, 5], torch.zeros(16, 12, dtype=torch.uint8, device=DEV).t())
    with pytest.raises(ValueError):
        dc.add(cams, [3, 5], torch.zeros(12, 17, dtype=torch.uint8, device=DEV))     # shape mismatch
    with pytest.raises(ValueError):
        dc.add(cams, [3, 5, 7], gt)                          # planes and classes differ in number
    with pytest.raises(ValueError):
        dc.add(cams, [5, 3], gt)                             # unsorted
    with pytest.raises(ValueError):
        dc.add(cams, [3, 3], gt)                             # duplicate
    with pytest.raises(ValueError):
        dc.add(cams, [3, 20], gt)                            # out of range
    with pytest.raises(ValueError):
        dc.add(cams, [-1, 3], gt)
    with pytest.raises(ValueError):
        dc.add(cams[:0], [], gt)                             # empty
    with pytest.raises(L.AcrHipError):
        dc.add(cams.cpu(), [3, 5], gt)
    for bad in ([0.5, 0.2], [0.1, 0.1], [], list(np.arange(257) / 257.0)):
        with pytest.raises(ValueError):
            E.DeviceSweepCounters(bad, device=DEV)
    with pytest.raises(ValueError):
        E.DeviceSweepCounters(num_cls=129, device=DEV)
    dl = E.DeviceLabelCounters(device=DEV)
    with pytest.raises(ValueError):
        dl.add(gt.int(), gt)
    with pytest.raises(ValueError):
        dl.add(gt, gt.t())
    with pytest.raises(ValueError):
        dl.add(gt, torch.zeros(12, 17, dtype=torch.uint8, device=DEV))
    # nothing of the above was counted
    want = E.SweepCounters(T100)
    want.add({3: cams[0].cpu().numpy(), 5: cams[1].cpu().numpy()}, gt.cpu().numpy())
    _assert_counters_equal(dc.to_host(), want)
    assert int(dl._conf.sum()) == 0

    # the C entries, called directly: negative code and a message; valid pointers only, nothing is launched
    cl = (ctypes.c_int32 * 2)(3, 5)
    th, raw, st = dc._th, dc._raw, L.stream_ptr()
    out = torch.zeros(2 * 100 * 21, dtype=torch.int64, device=DEV)
    before = raw.clone()

    def refused(rc, word):
        assert rc == -1
        assert word in lib.acr_last_error().decode()

    refused(lib.acr_eval_sweep_f32(L.ptr(cams), cl, 0, L.ptr(gt), 12, 16, L.ptr(th), 100, 21, L.ptr(raw), st), "n=0")
    refused(lib.acr_eval_sweep_f32(L.ptr(cams), cl, 2, L.ptr(gt), 12, 16, L.ptr(th), 0, 21, L.ptr(raw), st), "nt=0")
    refused(lib.acr_eval_sweep_f32(None, cl, 2, L.ptr(gt), 12, 16, L.ptr(th), 100, 21, L.ptr(raw), st), "null pointer")
    refused(lib.acr_eval_sweep_f32(L.ptr(cams), None, 2, L.ptr(gt), 12, 16, L.ptr(th), 100, 21, L.ptr(raw), st), "null pointer")
    refused(lib.acr_eval_sweep_f32(L.ptr(cams), cl, 2, L.ptr(gt), 12, 16, L.ptr(th), 100, 21, None, st), "null pointer")
    refused(lib.acr_eval_sweep_f32(L.ptr(cams), (ctypes.c_int32 * 2)(5, 3), 2, L.ptr(gt), 12, 16, L.ptr(th), 100, 21, L.ptr(raw), st),
            "ascending")
    refused(lib.acr_eval_sweep_f32(L.ptr(cams), (ctypes.c_int32 * 2)(3, 20), 2, L.ptr(gt), 12, 16, L.ptr(th), 100, 21, L.ptr(raw), st),
            "outside")
    refused(lib.acr_eval_sweep_f32(L.ptr(cams), cl, 2, L.ptr(gt), 0, 16, L.ptr(th), 100, 21, L.ptr(raw), st), "geometry")
    refused(lib.acr_eval_sweep_f32(L.ptr(cams), cl, 2, L.ptr(gt), 12, 16, L.ptr(th), 257, 21, L.ptr(raw), st), "nt=257")
    refused(lib.acr_eval_sweep_f32(L.ptr(cams), cl, 2, L.ptr(gt), 12, 16, L.ptr(th), 100, 129, L.ptr(raw), st), "num_cls=129")
    refused(lib.acr_eval_sweep_finish(None, 100, 21, L.ptr(out), L.ptr(out), st), "null pointer")
    refused(lib.acr_eval_sweep_finish(L.ptr(raw), 0, 21, L.ptr(out), L.ptr(out), st), "nt=0")
    refused(lib.acr_eval_confusion_u8(None, L.ptr(gt), 12 * 16, 21, L.ptr(dl._conf), st), "null pointer")
    refused(lib.acr_eval_confusion_u8(L.ptr(gt), L.ptr(gt), 0, 21, L.ptr(dl._conf), st), "n_pixels=0")
    refused(lib.acr_eval_confusion_u8(L.ptr(gt), L.ptr(gt), 12 * 16, 0, L.ptr(dl._conf), st), "num_cls=0")
    torch.cuda.synchronize()
    assert torch.equal(raw, before) and int(dl._conf.sum()) == 0


def test_infer_cam_list_evaluates_on_the_device(tmp_path):
    """evaluate=CamEvaluation: the CAM sweep equals evaluate_cam_dir over the files the same call wrote (exactly: the hook sees the
    floats that are copied out), the CRF / PAMR label counters equal host argmax + iou_counts over the written dicts, every file
    is byte-identical to a run without evaluate, and two merged ranks equal the single run"""
    import sys
    from PIL import Image
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from __graft_entry__ import _recipe_model
    from recipe import make_inputs
    from acr_wsss_amd.infer_cam import infer_cam_list
    model, _ = _recipe_model(torch.device(DEV))
    rng = np.random.default_rng(0)
    items, gts = [], {}
    for i, (classes, hw) in enumerate((([2, 9], (40, 52)), ([], (40, 52)), ([0, 5, 17], (50, 70)))):
        img, _ = make_inputs(1, 64, 20, 20 + i)
        label = torch.zeros(1, 20)
        for c in classes:
            label[0, c] = 1
        items.append(("im%d" % i, img, label, hw, rng.integers(0, 256, hw + (3,)).astype(np.uint8)))
        gt = rng.integers(0, 21, hw).astype(np.uint8)
        for c in classes:                                    # some structure: blocks of the positive classes
            y0, x0 = int(rng.integers(0, hw[0] - 8)), int(rng.integers(0, hw[1] - 8))
            gt[y0:y0 + 12, x0:x0 + 12] = c + 1
        gt[rng.random(hw) < 0.1] = 255
        gts["im%d" % i] = gt
    os.makedirs(str(tmp_path / "gt"))
    for name, gt in gts.items():
        Image.fromarray(gt).save(str(tmp_path / "gt" / (name + ".png")))
    asked = []

    def gt_of(name):
        asked.append(name)
        return gts[name]

    outs = lambda tag: dict(out_cam=str(tmp_path / tag / "cam"), out_crf=str(tmp_path / tag / "crf"), out_pamr=str(tmp_path / tag / "pamr"),
                            low_alpha=1, high_alpha=12)
    plain = infer_cam_list(model, items, **outs("plain"))
    ev = E.CamEvaluation(gt_of)
    res = infer_cam_list(model, items, evaluate=ev, **outs("eval"))
    assert sorted(set(asked)) == ["im0", "im2"] and not ev._gts          # the image without a positive class is skipped

    # files and results are those of the run without evaluate
    assert sorted(res) == sorted(plain)
    for name in res:
        assert sorted(res[name]) == sorted(plain[name])
        for c in res[name]:
            np.testing.assert_array_equal(res[name][c], plain[name][c])
    folders = ["cam"] + ["%s_%d" % (k, a) for k in ("crf", "pamr") for a in (1, 12)]
    for folder in folders:
        files = sorted(os.listdir(str(tmp_path / "plain" / folder)))
        assert files == sorted(os.listdir(str(tmp_path / "eval" / folder)))
        assert files == (["im0.npy", "im1.npy", "im2.npy"] if folder == "cam" else ["im0.npy", "im2.npy"])
        for f in files:
            with open(str(tmp_path / "plain" / folder / f), "rb") as f0, open(str(tmp_path / "eval" / folder / f), "rb") as f1:
                assert f0.read() == f1.read(), (folder, f)

    # CAM sweep == the file-reading evaluator over what was written
    _, miou, want = E.evaluate_cam_dir(str(tmp_path / "eval" / "cam"), str(tmp_path / "gt"), ["im0", "im2"])
    got = ev.cam.to_host()
    _assert_counters_equal(got, want, "cam")
    np.testing.assert_array_equal(got.miou()[0], miou)
    assert want.T.sum() > 0

    # label counters == host argmax + iou_counts over the written dicts
    def label_counts(folder):
        TP = np.zeros(21, np.int64); P = np.zeros(21, np.int64); T = np.zeros(21, np.int64)
        for name in ("im0", "im2"):
            d = np.load(str(tmp_path / "eval" / folder / (name + ".npy")), allow_pickle=True).item()
            keys = sorted(d)
            pred = np.asarray(keys, np.uint8)[np.argmax(np.stack([d[k] for k in keys]), axis=0)]
            tp, p, t = O.iou_counts(pred, gts[name])
            TP += tp; P += p; T += t
        return TP, P, T

    assert sorted(ev.crf) == sorted(ev.pamr) == [1, 12]
    for kind, table in (("crf", ev.crf), ("pamr", ev.pamr)):
        for alpha in (1, 12):
            lc = table[alpha].to_host()
            TP, P, T = label_counts("%s_%d" % (kind, alpha))
            np.testing.assert_array_equal(lc.TP, TP, err_msg="%s %d" % (kind, alpha))
            np.testing.assert_array_equal(lc.P, P, err_msg="%s %d" % (kind, alpha))
            np.testing.assert_array_equal(lc.T, T, err_msg="%s %d" % (kind, alpha))
            assert lc.miou()[0] == O.miou(TP, P, T)

    # two ranks, merged on the host, equal the single run.  Both sides run with batch_size=1: sharding changes which images share
    # a batch, and a batch's composition moves the fp32 summation order of an image's CAMs (infer_cam_list's documented
    # behaviour, held to 1e-3 by test_infer_cam_images_batch_matches_single_images), which flips single pixels that sit on a
    # threshold (measured: 4 of 2100 P counters off by one at the default batch size).  Image by image the CAMs are the same
    # bits on every rank, and the counters must then be equal exactly.
    single = E.CamEvaluation(gt_of)
    infer_cam_list(model, items, evaluate=single, batch_size=1, **outs("single"))
    _assert_counters_equal(single.cam.to_host(), E.evaluate_cam_dir(str(tmp_path / "single" / "cam"), str(tmp_path / "gt"), ["im0", "im2"])[2],
                           "batch_size=1")
    # at the default batch size each rank's counters are still exactly those of the files that rank wrote
    for r, names in ((0, ["im0", "im2"]), (1, [])):
        ev_r = E.CamEvaluation(gt_of)
        infer_cam_list(model, items, evaluate=ev_r, rank=r, world=2, **outs("rank%d_default" % r))
        _assert_counters_equal(ev_r.cam.to_host(), E.evaluate_cam_dir(str(tmp_path / ("rank%d_default" % r) / "cam"), str(tmp_path / "gt"),
                                                                      names)[2], "rank %d, default batch size" % r)
    ranks = [E.CamEvaluation(gt_of), E.CamEvaluation(gt_of)]
    for r in (0, 1):
        infer_cam_list(model, items, evaluate=ranks[r], rank=r, world=2, batch_size=1, **outs("rank%d" % r))
    _assert_counters_equal(ranks[0].cam.to_host().merge(ranks[1].cam.to_host()), single.cam.to_host(), "two ranks")
    for kind in ("crf", "pamr"):
        for alpha in (1, 12):
            merged = E.LabelCounters(21)
            for r in (0, 1):
                if alpha in getattr(ranks[r], kind):
                    merged.merge(getattr(ranks[r], kind)[alpha].to_host())
            np.testing.assert_array_equal(merged.conf, getattr(single, kind)[alpha].to_host().conf)


def test_a_callers_own_hook_is_kept_next_to_evaluate():
    """on_device passed through infer_cam_list's keywords together with evaluate: both are served, with the same tensors"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from __graft_entry__ import _recipe_model
    from recipe import make_inputs
    from acr_wsss_amd.infer_cam import infer_cam_list
    model, _ = _recipe_model(torch.device(DEV))
    rng = np.random.default_rng(3)
    items, gts = [], {}
    for i, classes in enumerate(([4], [], [1, 6])):
        img, _ = make_inputs(1, 64, 20, 30 + i)
        label = torch.zeros(1, 20)
        for c in classes:
            label[0, c] = 1
        items.append(("im%d" % i, img, label, (30, 44)))
        gts["im%d" % i] = _gt(rng, 30, 44)
    seen = []
    own = E.DeviceSweepCounters(device=DEV)

    def hook(j, classes, cam):
        seen.append((j, list(classes), tuple(cam.shape)))
        own.add(cam, classes, gts["im%d" % j])               # one group here: the index in the group is the item's

    ev = E.CamEvaluation(gts.__getitem__)
    infer_cam_list(model, items, evaluate=ev, on_device=hook)
    assert seen == [(0, [4], (1, 30, 44)), (2, [1, 6], (2, 30, 44))]
    _assert_counters_equal(own.to_host(), ev.cam.to_host(), "own hook")
    assert ev.cam.to_host().T.sum() > 0
    # the pinned ground-truth buffers of released images are kept for reuse, one per image in flight at most
    assert not ev._gts and sum(len(v) for v in ev._free.values()) == 2
    infer_cam_list(model, items, evaluate=ev)                # a second list on the same object accumulates, reusing them
    assert sum(len(v) for v in ev._free.values()) == 2
    np.testing.assert_array_equal(ev.cam.to_host().T, 2 * own.to_host().T)
