"""numpy restatement of the pseudo-label rule (include/acr_hip.h, acr_pseudo_label_f32 / acr_pseudo_compose; the reference's
compute_seg_label_rrm, myTool.py:674-744), written once for the tests: dense (C + 1)-plane arrays, np.argmax, np.sort.  Pinned to
the reference's own runs by tests/golden/pseudo_{a..d}.npz (test_pseudo_cpu.py); the device is compared with it exactly."""
import numpy as np


def dense(planes, labels, num_labels):
    """(num_labels, W, H) float32 with planes[i] at label labels[i] and 0.0 elsewhere"""
    planes = np.asarray(planes, np.float32)
    out = np.zeros((num_labels,) + planes.shape[1:], np.float32)
    for p, l in zip(planes, labels):
        out[l] = p
    return out


def label_map(scores, classes, num_classes=20):
    """step A: scores (K + 1, W, H), plane 0 label 0, plane j + 1 label classes[j] + 1"""
    return np.argmax(dense(scores, [0] + [c + 1 for c in classes], num_classes + 1), axis=0).astype(np.uint8)


def bg_score(cams, classes, bg_alpha=36, num_classes=20):
    m = np.asarray(cams, np.float32).max(axis=0)
    if len(classes) < num_classes:
        m = np.maximum(m, np.float32(0.0))
    return np.power((np.float32(1.0) - m).astype(np.float64), float(bg_alpha)).astype(np.float32)


def cam_label(cams, classes, bg_alpha=36, num_classes=20):
    """M and the dense (C + 1, W, H) array it is the argmax of"""
    allp = dense(cams, [c + 1 for c in classes], num_classes + 1)
    allp[0] = bg_score(cams, classes, bg_alpha, num_classes)
    return np.argmax(allp, axis=0), allp


def not_sure(cams, classes, la, ha, bg_alpha=36, cam_floor=0.1, fg_quantile=0.3, bg_sure=0.3, crf_sure=0.8, num_classes=20):
    """step C: (not_sure_region, M)"""
    assert cam_floor >= 0 and 0 <= fg_quantile < 1 and crf_sure > 0
    la, ha = np.asarray(la, np.float32), np.asarray(ha, np.float32)
    M, allp = cam_label(cams, classes, bg_alpha, num_classes)
    sure = np.zeros(M.shape, bool)
    for l in np.unique(label_map(la, classes, num_classes)):
        region = M == l
        if l == 0:
            sure |= region & (allp[0] > np.float32(bg_sure))
        else:
            S = np.sort(allp[l][region & (allp[l] > np.float32(cam_floor))])
            if len(S) == 0:
                continue                                 # defined here; the reference raises IndexError
            v = S[int(len(S) * float(fg_quantile))]
            sure |= region & (allp[l] > v)
    crf_unsure = np.maximum(ha[0], la[1:].max(axis=0)) < np.float32(crf_sure)
    return crf_unsure | ~sure, M


def seg_label(cams, classes, la, ha, ignore_uncertain=False, num_classes=20, **kw):
    l_la, l_ha = label_map(la, classes, num_classes), label_map(ha, classes, num_classes)
    out = l_la.copy()
    out[l_la == 0] = 255
    out[l_ha == 0] = 0
    if ignore_uncertain:
        out[not_sure(cams, classes, la, ha, num_classes=num_classes, **kw)[0]] = 255
    return out


def margin(cams, classes, bg_alpha=36, bg_sure=0.3, num_classes=20):
    """Decisiveness of an input: the smallest relative distance, over the pixels, of bg from the largest class value (dense, so
    0.0 counts when a class is absent) and from bg_sure.  Above 1e-5 the <= 1-ulp (1.2e-7) differences between one pow and
    another cannot change a comparison."""
    bg = bg_score(cams, classes, bg_alpha, num_classes).astype(np.float64)
    top = np.asarray(cams, np.float32).max(axis=0).astype(np.float64)
    if len(classes) < num_classes:
        top = np.maximum(top, 0.0)
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-30)
    return float(min(rel(bg, top).min(), rel(bg, np.float64(np.float32(bg_sure))).min()))


# ---- seeded inputs shared by the generator's cases and the GPU tests -------------------------------------------------------------
def bumps(rng, k, w, h, round_to=None):
    """(k, w, h) CAM-like planes: a few smooth bumps per class, exact zeros below 0.05, each plane's maximum 1"""
    yy, xx = np.mgrid[0:w, 0:h].astype(np.float32)
    cams = np.zeros((k, w, h), np.float32)
    for j in range(k):
        plane = np.zeros((w, h), np.float32)
        for _ in range(2):
            cy, cx = rng.uniform(0, w), rng.uniform(0, h)
            s = rng.uniform(0.08, 0.25) * min(w, h) / max(1.0, (k / 3.0) ** 0.5) + 1     # many classes: narrower bumps
            plane = np.maximum(plane, np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32))
        plane[plane < 0.05] = 0.0
        cams[j] = plane / max(float(plane.max()), 1e-6)
    if round_to:
        cams = (np.round(cams * round_to) / round_to).astype(np.float32)
    return cams


def refined(rng, cams, alpha, noise=0.15, bg_bias=0.0):
    """(k + 1, w, h) scores that look like a refinement of [(1 - max cam)^alpha; cams]: perturbed, positive, summing to one"""
    k, w, h = cams.shape
    s = np.concatenate((np.power(1 - cams.max(axis=0, keepdims=True), alpha), cams), axis=0).astype(np.float64)
    s = np.maximum(s + noise * rng.standard_normal((k + 1, 1, 1)) * rng.random((k + 1, w, h)), 1e-4)
    s[0] += bg_bias
    s = s ** 3                                           # sharpened, as a CRF's output is
    return (s / s.sum(axis=0, keepdims=True)).astype(np.float32)


def decisive_case(seed, k, w, h, classes, round_to=None, bg_bias=0.0, num_classes=20, tries=50):
    """(cams, classes, la, ha, margin) of the first seed at or after ``seed`` whose margin is above 1e-5; ``bg_bias`` lifts the
    background of la only (a large one makes L_la background everywhere while L_ha keeps its classes)"""
    for t in range(tries):
        rng = np.random.default_rng(seed + 1000 * t)
        cams = bumps(rng, k, w, h, round_to)
        mg = margin(cams, classes, num_classes=num_classes)
        if mg > 1e-5:
            return cams, list(classes), refined(rng, cams, 2, bg_bias=bg_bias), refined(rng, cams, 14), mg
    raise AssertionError("no decisive input in %d seeds" % tries)
