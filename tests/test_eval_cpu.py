"""Host side of the device evaluation: the ABI's documented semantics (tests/eval_ref.py, a numpy restatement of include/acr_hip.h)
equal ``SweepCounters.add`` counter for counter; ``SweepCounters.merge``; ``LabelCounters`` against the oracle's counters; the
device classes refuse to run without a GPU; the new keywords default to None."""
import inspect

import numpy as np
import pytest
import torch

import eval_ref as R
from oracle import acr_oracle as O
from acr_wsss_amd import evaluation as E

T100 = np.arange(100, dtype=np.float32) / 100.0


def _extra_cases():
    rng = np.random.default_rng(5)
    neg = {c: (rng.random((19, 23)).astype(np.float32) - 0.5) for c in (1, 4)}             # negative values: absent planes win there
    neg[1][:5] = -0.25
    on = {c: rng.choice(T100, (21, 17)).astype(np.float32) for c in (0, 2, 9)}              # values exactly on thresholds
    gts = []
    for d in (neg, on):
        h, w = next(iter(d.values())).shape
        gt = rng.integers(0, 21, (h, w)).astype(np.uint8)
        gt[rng.random((h, w)) < 0.15] = 255
        gts.append(gt)
    return [(neg, gts[0]), (on, gts[1])]


CASES = R.four_cases() + _extra_cases()


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restated_abi_equals_sweep_counters(i):
    cam_dict, gt = CASES[i]
    cams, keys = R.stack(cam_dict)
    sc = E.SweepCounters(T100)
    sc.add(cam_dict, gt)
    raw = R.sweep_raw(cams, keys, gt, T100, 21)
    np.testing.assert_array_equal(raw, R.sweep_raw_fast(cams, keys, gt, T100, 21))
    TP, P, T = R.sweep_finish(raw, 100, 21)
    np.testing.assert_array_equal(TP, sc.TP)
    np.testing.assert_array_equal(P, sc.P)
    np.testing.assert_array_equal(T, sc.T)


def test_restated_abi_accumulates_over_images():
    sc = E.SweepCounters(T100)
    raw = None
    for cam_dict, gt in CASES:
        sc.add(cam_dict, gt)
        cams, keys = R.stack(cam_dict)
        raw = R.sweep_raw_fast(cams, keys, gt, T100, 21, raw)
    TP, P, T = R.sweep_finish(raw, 100, 21)
    np.testing.assert_array_equal(TP, sc.TP)
    np.testing.assert_array_equal(P, sc.P)
    np.testing.assert_array_equal(T, sc.T)


def test_sweep_counters_merge():
    one, a, b = E.SweepCounters(T100), E.SweepCounters(T100), E.SweepCounters(T100)
    for i, (cam_dict, gt) in enumerate(CASES):
        one.add(cam_dict, gt)
        (a if i % 2 == 0 else b).add(cam_dict, gt)
    assert a.merge(b) is a
    for name in ("TP", "P", "T"):
        np.testing.assert_array_equal(getattr(a, name), getattr(one, name))
    with pytest.raises(ValueError):
        a.merge(E.SweepCounters(T100[:50]))
    with pytest.raises(ValueError):
        a.merge(E.SweepCounters(T100 + np.float32(0.001)))
    with pytest.raises(ValueError):
        a.merge(E.SweepCounters(T100, num_cls=81))


def _label_images(rng, out_of_range):
    images = []
    for h, w in ((31, 27), (16, 40), (9, 9)):
        gt = rng.integers(0, 21, (h, w)).astype(np.uint8)
        gt[rng.random((h, w)) < 0.1] = 255
        pred = np.where(rng.random((h, w)) < 0.6, np.minimum(gt, 20), rng.integers(0, 21, (h, w))).astype(np.uint8)
        if out_of_range:
            out = rng.random((h, w)) < 0.05
            pred[out] = rng.choice(np.array([21, 40, 254, 255], np.uint8), int(out.sum()))
        images.append((pred, gt))
    return images


@pytest.mark.parametrize("out_of_range", [False, True])
def test_label_counters_equal_the_oracle_counters(out_of_range):
    """Predictions >= num_cls land in the last column: they count in T (the pixel is valid) and in no class's P, which is what
    oracle.iou_counts (the reference's loop) does as well."""
    rng = np.random.default_rng(11)
    images = _label_images(rng, out_of_range)
    conf = None
    TP = np.zeros(21, np.int64); P = np.zeros(21, np.int64); T = np.zeros(21, np.int64)
    host = E.LabelCounters(21)
    for pred, gt in images:
        conf = R.confusion(pred, gt, 21, conf)
        host.add(pred, gt)
        tp, p, t = O.iou_counts(pred, gt)
        TP += tp; P += p; T += t
    lc = E.LabelCounters(21, conf)
    np.testing.assert_array_equal(host.conf, conf)
    np.testing.assert_array_equal(lc.TP, TP)
    np.testing.assert_array_equal(lc.P, P)
    np.testing.assert_array_equal(lc.T, T)
    assert lc.miou()[0] == O.miou(TP, P, T)
    if out_of_range:
        assert lc.conf[:, 21].sum() > 0
    halves = E.LabelCounters(21, R.confusion(*images[0], 21)).merge(E.LabelCounters(21, R.confusion(*images[1], 21)))
    halves.merge(E.LabelCounters(21, R.confusion(*images[2], 21)))
    np.testing.assert_array_equal(halves.conf, conf)
    with pytest.raises(ValueError):
        lc.merge(E.LabelCounters(81))
    # the four summaries of the reference's Evaluator, restated on the square part of the matrix
    sq = conf[:, :21].astype(np.float64)
    iu = np.diag(sq) / (sq.sum(1) + sq.sum(0) - np.diag(sq))
    assert lc.pixel_accuracy() == np.trace(sq) / sq.sum()
    assert lc.pixel_accuracy_class() == np.nanmean(np.diag(sq) / sq.sum(1))
    assert lc.mean_iou() == np.nanmean(iu)
    freq = sq.sum(1) / sq.sum()
    assert lc.frequency_weighted_iou() == (freq[freq > 0] * iu[freq > 0]).sum()


def test_label_counters_on_a_hand_written_matrix():
    """Three classes, numbers worked out by hand: square part [[5,1,0],[2,3,1],[0,0,4]], out-of-range column [1,0,2]."""
    lc = E.LabelCounters(3, [[5, 1, 0, 1], [2, 3, 1, 0], [0, 0, 4, 2]])
    np.testing.assert_array_equal(lc.TP, [5, 3, 4])
    np.testing.assert_array_equal(lc.P, [7, 4, 5])                   # column sums of the square part
    np.testing.assert_array_equal(lc.T, [7, 6, 6])                   # row sums, the out-of-range column included
    assert lc.miou()[0] == pytest.approx(1400.0 / 27.0, rel=1e-9)    # (5/9 + 3/7 + 4/7) / 3 in percent (the 1e-10 is below 1e-9)
    assert lc.miou()[1] == pytest.approx([500.0 / 9, 300.0 / 7, 400.0 / 7], rel=1e-9)
    # the Evaluator's summaries see the square part only: rows 6, 6, 4, columns 7, 4, 5, 16 pixels, trace 12
    assert lc.pixel_accuracy() == pytest.approx(0.75, rel=1e-12)
    assert lc.pixel_accuracy_class() == pytest.approx(7.0 / 9.0, rel=1e-12)          # (5/6 + 3/6 + 4/4) / 3
    assert lc.mean_iou() == pytest.approx(519.0 / 840.0, rel=1e-12)                  # (5/8 + 3/7 + 4/5) / 3
    assert lc.frequency_weighted_iou() == pytest.approx(1333.0 / 2240.0, rel=1e-12)  # 3/8 * 5/8 + 3/8 * 3/7 + 1/4 * 4/5
    empty = E.LabelCounters(3, [[2, 0, 0, 0], [0, 0, 0, 0], [0, 1, 1, 0]])            # class 1 never occurs in the ground truth
    assert lc.merge(E.LabelCounters(3)) is lc
    assert empty.pixel_accuracy_class() == pytest.approx((1.0 + 0.5) / 2, rel=1e-12) # the mean skips the empty class
    assert empty.frequency_weighted_iou() == pytest.approx(0.5 * 1.0 + 0.5 * 0.5, rel=1e-12)


def test_ground_truth_labels_between_num_cls_and_254_are_ignored():
    """DEVIATION from the reference, documented in include/acr_hip.h and evaluation.py: a ground-truth label in num_cls..254 is
    ignored exactly like 255.  The reference's loop (oracle.iou_counts) keeps such a pixel 'valid' and so counts its prediction in
    P; this asserts the documented rule, i.e. the oracle's counters on the ground truth with those labels set to 255."""
    rng = np.random.default_rng(12)
    pred, gt = _label_images(rng, True)[0]
    odd = rng.random(gt.shape) < 0.1
    gt = gt.copy()
    gt[odd] = rng.integers(21, 255, int(odd.sum())).astype(np.uint8)
    as_ignore = np.where(gt < 21, gt, 255).astype(np.uint8)
    lc = E.LabelCounters(21, R.confusion(pred, gt, 21))
    tp, p, t = O.iou_counts(pred, as_ignore)
    np.testing.assert_array_equal(lc.TP, tp)
    np.testing.assert_array_equal(lc.P, p)
    np.testing.assert_array_equal(lc.T, t)
    assert not np.array_equal(O.iou_counts(pred, gt)[1], p)                  # the reference's P does differ here
    # the sweep follows the same rule
    cam_dict, _ = CASES[0]
    cams, keys = R.stack(cam_dict)
    gt2 = rng.integers(0, 255, cams.shape[1:]).astype(np.uint8)
    raw = R.sweep_raw(cams, keys, gt2, T100, 21)
    sc = E.SweepCounters(T100)
    sc.add(cam_dict, np.where(gt2 < 21, gt2, 255).astype(np.uint8))
    TP, P, T = R.sweep_finish(raw, 100, 21)
    np.testing.assert_array_equal(TP, sc.TP)
    np.testing.assert_array_equal(P, sc.P)
    np.testing.assert_array_equal(T, sc.T)


def test_label_map_takes_the_first_maximum_in_key_order():
    d = {3: np.array([[0.5, 0.1]], np.float32), 0: np.array([[0.5, 0.0]], np.float32), 7: np.array([[0.2, 0.1]], np.float32)}
    got = E.label_map(d)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, [[0, 3]])


def test_device_counters_raise_without_a_gpu(monkeypatch):
    from acr_wsss_amd._lib import AcrHipError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(AcrHipError):
        E.DeviceSweepCounters()
    with pytest.raises(AcrHipError):
        E.DeviceLabelCounters()


def test_device_counters_refuse_a_cpu_device():
    from acr_wsss_amd._lib import AcrHipError
    with pytest.raises(AcrHipError):
        E.DeviceSweepCounters(device="cpu")
    with pytest.raises(AcrHipError):
        E.DeviceLabelCounters(device="cpu")


def test_new_keywords_default_to_none():
    from acr_wsss_amd import infer_cam
    assert inspect.signature(infer_cam.infer_cam_list).parameters["evaluate"].default is None
    assert inspect.signature(infer_cam.launch_cam_images).parameters["on_device"].default is None
    ev = E.CamEvaluation(lambda name: None)
    assert ev.cam is None and ev.crf == {} and ev.pamr == {} and ev.num_cls == 21


def test_eval_symbols_are_declared_and_bound():
    import abi_checks
    from acr_wsss_amd import _lib as L
    for name in ("acr_eval_sweep_f32", "acr_eval_sweep_finish", "acr_eval_confusion_u8"):
        assert abi_checks.declared(name) and name in L.SIGNATURES
