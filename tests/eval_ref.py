"""Numpy restatement of the device evaluation ABI (include/acr_hip.h: acr_eval_sweep_f32, acr_eval_sweep_finish,
acr_eval_confusion_u8), written from the header's definitions, pixel by pixel where that is the clearest form.  The tests hold it
against ``evaluation.SweepCounters`` (itself pinned to the reference's loop by test_evaluation_cpu.py) and the kernels against both."""
import numpy as np


def raw_size(nt, num_cls):
    return 2 * (nt + 1) * num_cls + (nt + 1) + num_cls + 1


def split_raw(raw, nt, num_cls):
    """FG (nt + 1, num_cls), HIT (nt + 1, num_cls), BG (nt + 1), T (num_cls), NVALID -- views of raw."""
    nfg = (nt + 1) * num_cls
    FG = raw[:nfg].reshape(nt + 1, num_cls)
    HIT = raw[nfg:2 * nfg].reshape(nt + 1, num_cls)
    BG = raw[2 * nfg:2 * nfg + nt + 1]
    T = raw[2 * nfg + nt + 1:2 * nfg + nt + 1 + num_cls]
    return FG, HIT, BG, T, raw[-1:]


def sweep_raw(cams, classes, gt, thresholds, num_cls, raw=None):
    """cams (n, h, w) float32, classes: n ascending class indices, gt (h, w) uint8; accumulates into and returns raw (int64)."""
    thresholds = np.asarray(thresholds, np.float32)
    nt = len(thresholds)
    if raw is None:
        raw = np.zeros(raw_size(nt, num_cls), np.int64)
    FG, HIT, BG, T, NVALID = split_raw(raw, nt, num_cls)
    n, h, w = cams.shape
    full = np.zeros((num_cls - 1, h, w), np.float32)          # v_c: exactly 0.0 for a class without a plane
    for j, c in enumerate(classes):
        full[c] = cams[j]
    m = full.max(axis=0)
    a = 1 + full.argmax(axis=0)                               # the smallest c with v_c == m
    for y in range(h):
        for x in range(w):
            g = int(gt[y, x])
            if g >= num_cls:                                  # 255, and the documented deviation: num_cls..254 too
                continue
            kfg = int(np.sum(thresholds < m[y, x]))           # fp32 comparison
            NVALID[0] += 1
            T[g] += 1
            FG[kfg, a[y, x]] += 1
            if a[y, x] == g:
                HIT[kfg, a[y, x]] += 1
            if g == 0:
                BG[kfg] += 1
    return raw


def sweep_raw_fast(cams, classes, gt, thresholds, num_cls, raw=None):
    """``sweep_raw`` with bincounts instead of the pixel loop (for the large cases); test_eval_cpu.py holds the two equal."""
    thresholds = np.asarray(thresholds, np.float32)
    nt = len(thresholds)
    if raw is None:
        raw = np.zeros(raw_size(nt, num_cls), np.int64)
    FG, HIT, BG, T, NVALID = split_raw(raw, nt, num_cls)
    n, h, w = cams.shape
    full = np.zeros((num_cls - 1, h, w), np.float32)
    for j, c in enumerate(classes):
        full[c] = cams[j]
    keep = gt < num_cls
    m = full.max(axis=0)[keep]
    a = (1 + full.argmax(axis=0))[keep]
    g = gt[keep].astype(np.int64)
    kfg = (thresholds[None, :] < m[:, None]).sum(axis=1)
    NVALID[0] += len(g)
    T += np.bincount(g, minlength=num_cls)
    FG += np.bincount(kfg * num_cls + a, minlength=FG.size).reshape(FG.shape)
    hit = a == g
    HIT += np.bincount(kfg[hit] * num_cls + a[hit], minlength=HIT.size).reshape(HIT.shape)
    BG += np.bincount(kfg[g == 0], minlength=nt + 1)
    return raw


def sweep_finish(raw, nt, num_cls):
    """TP, P (nt, num_cls) from raw, by the sums of the header."""
    FG, HIT, BG, T, NVALID = split_raw(raw, nt, num_cls)
    TP = np.zeros((nt, num_cls), np.int64)
    P = np.zeros((nt, num_cls), np.int64)
    for k in range(nt):
        for c in range(1, num_cls):
            P[k, c] = FG[k + 1:, c].sum()
            TP[k, c] = HIT[k + 1:, c].sum()
        P[k, 0] = NVALID[0] - P[k, 1:].sum()
        TP[k, 0] = BG[:k + 1].sum()
    return TP, P, T.copy()


def confusion(pred, gt, num_cls, conf=None):
    """conf[gt][min(pred, num_cls)] += 1 over the pixels with gt < num_cls; (num_cls, num_cls + 1) int64."""
    if conf is None:
        conf = np.zeros((num_cls, num_cls + 1), np.int64)
    keep = gt < num_cls
    g = gt[keep].astype(np.int64)
    p = np.minimum(pred[keep].astype(np.int64), num_cls)
    conf += np.bincount(g * (num_cls + 1) + p, minlength=conf.size).reshape(conf.shape)
    return conf


def image_case(rng, h, w, classes, ties=False, num_cls=21):
    """The image cases of test_evaluation_cpu.py (same construction): uniform CAMs, optionally rounded to tenths with an all-zero
    region in the first class, random ground truth with 15 % ignore."""
    cams = {c: rng.random((h, w)).astype(np.float32) for c in classes}
    if ties:
        for c in classes:
            cams[c] = np.round(cams[c] * 10) / 10
        cams[classes[0]][: h // 3] = 0.0
    gt = rng.integers(0, num_cls, (h, w)).astype(np.uint8)
    gt[rng.random((h, w)) < 0.15] = 255
    return cams, gt


def four_cases(seed=0):
    rng = np.random.default_rng(seed)
    return [image_case(rng, 37, 53, [3, 11]), image_case(rng, 20, 31, [0], ties=True), image_case(rng, 25, 18, [0, 7, 19], ties=True),
            image_case(rng, 16, 16, list(range(20)))]


def stack(cam_dict):
    keys = sorted(cam_dict)
    return np.ascontiguousarray(np.stack([cam_dict[k] for k in keys]).astype(np.float32)), keys
