"""numpy restatement of the saliency-guided pseudo-label rule (include/acr_hip.h, acr_sal_pseudo_compose / acr_morph_open_u8; the
reference's compute_seg_label_3, myTool.py:188-264), written once for the tests: integers and comparisons, the pow in float64, a
brute-force opening over the k * k offsets.  Pinned to the reference's own runs by tests/golden/pseudo_sal_{a..d}.npz
(test_pseudo_sal_cpu.py); the device is compared with it exactly."""
import numpy as np


def bg_score(cams, present, bg_alpha=12):
    """(m, bg) of one image: cams (C, H, W) float32, present (C,) bool"""
    m = np.zeros(cams.shape[1:], np.float32)
    for c in np.flatnonzero(present):
        m = np.maximum(m, cams[c])
    return m, np.power((np.float32(1.0) - m).astype(np.float64), float(bg_alpha)).astype(np.float32)


def thresholds(cams, present, cut=0.9):
    """per class the pos-th smallest positive value, pos = int(n * cut); +inf for an absent class and for pos == 0"""
    thr = np.full(cams.shape[0], np.inf, np.float32)
    for c in np.flatnonzero(present):
        order = np.sort(cams[c][cams[c] > 0])
        pos = int(order.shape[0] * float(cut))
        if pos > 0:
            thr[c] = order[pos]
    return thr


def morph_open(mask, k=10):
    """O = dilate(erode(F)), F = mask != 0, both over the offsets -(k // 2) .. k - 1 - k // 2 on each axis, positions outside the
    image left out; 255 where O holds, 0 elsewhere.  mask (H, W)."""
    F = np.asarray(mask) != 0
    h, w = F.shape
    offs = range(-(k // 2), k - k // 2)

    def shifted(a, dy, dx, fill):
        out = np.full((h, w), fill, bool)
        ys, ye = max(0, -dy), min(h, h - dy)
        xs, xe = max(0, -dx), min(w, w - dx)
        if ys < ye and xs < xe:
            out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
        return out
    E = np.ones((h, w), bool)
    for dy in offs:
        for dx in offs:
            E &= shifted(F, dy, dx, True)
    O = np.zeros((h, w), bool)
    for dy in offs:
        for dx in offs:
            O |= shifted(E, dy, dx, False)
    return np.where(O, 255, 0).astype(np.uint8)


def seg_label_one(cams, present, saliency, bg_alpha=12, cut=0.9, open_size=10):
    """one image: cams (C, H, W) float32, present (C,), saliency (H, W) uint8 -> (label, saliency_out) uint8"""
    cams = np.asarray(cams, np.float32)
    present = np.asarray(present).astype(bool)
    m, bg = bg_score(cams, present, bg_alpha)
    L = np.zeros(m.shape, np.int64)
    best = bg.copy()
    for c in np.flatnonzero(present):                    # first maximum wins: strict >, ascending
        win = cams[c] > best
        L[win] = c + 1
        best[win] = cams[c][win]
    label = np.where(L == 0, 255, L)
    label[saliency == 0] = 0
    sal = np.array(saliency, np.uint8)
    thr = thresholds(cams, present, cut)
    grab = np.zeros(m.shape, np.int64)
    for c in np.flatnonzero(present)[::-1]:              # descending, so that the lowest class is written last
        grab[cams[c] > thr[c]] = c + 1
    take = (label == 0) & (grab > 0)
    label[take] = grab[take]
    sal[take] = 255
    if open_size:
        label[morph_open(label, open_size) != 255] = 0
    return label.astype(np.uint8), sal


def seg_label(cams, present, saliency, **kw):
    """the batch: cams (B, C, H, W), present (B, C), saliency (B, H, W)"""
    outs = [seg_label_one(cams[b], present[b], saliency[b], **kw) for b in range(len(cams))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def margin(cams, present, bg_alpha=12):
    """Decisiveness of one image: the smallest relative distance, over the pixels, of bg from the largest present class value --
    the only comparison a last-bit difference between one pow and another (<= 1 ulp = 1.2e-7) could flip.  Above 1e-5 it cannot."""
    m, bg = bg_score(np.asarray(cams, np.float32), np.asarray(present).astype(bool), bg_alpha)
    a, b = bg.astype(np.float64), m.astype(np.float64)
    return float((np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-30)).min())


# ---- seeded inputs shared by the generator's cases and the GPU tests -------------------------------------------------------------
def bumps(rng, c, h, w, round_to=None, width=0.35):
    """(c, h, w) CAM-like planes in [0, 1]: a few wide smooth bumps per class over a low noise floor, exact zeros below 0.05"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    cams = np.zeros((c, h, w), np.float32)
    for j in range(c):
        plane = (0.12 * rng.random((h, w))).astype(np.float32)
        for _ in range(2):
            cy, cx = rng.uniform(0, h), rng.uniform(0, w)
            s = rng.uniform(0.5, 1.0) * width * min(h, w) + 1
            plane = np.maximum(plane, np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32))
        plane[plane < 0.05] = 0.0
        cams[j] = plane / max(float(plane.max()), 1e-6)
    if round_to:
        cams = (np.round(cams * round_to) / round_to).astype(np.float32)
    return cams


def saliency_map(rng, h, w):
    """uint8 (h, w): a salient blob of values 1..255 with zero background, a few isolated salient specks outside it (the opening
    removes those) and a few zero holes inside"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    cy, cx = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w
    ry, rx = rng.uniform(0.25, 0.4) * h + 1, rng.uniform(0.25, 0.4) * w + 1
    sal = np.where(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
    sal[rng.random((h, w)) < 0.02] = 200
    sal[rng.random((h, w)) < 0.003] = 0
    return sal


def decisive_case(seed, b, c, h, w, present, round_to=None, bg_alpha=12, width=0.35, tries=50):
    """(cams (b, c, h, w), present (b, c) uint8, saliency (b, h, w), margin) of the first seed at or after ``seed`` whose margin
    is above 1e-5 in every image.  ``present``: (b, c) array-like, or None for three random classes per image."""
    for t in range(tries):
        rng = np.random.default_rng(seed + 1000 * t)
        pres = np.zeros((b, c), np.uint8)
        if present is None:
            for i in range(b):
                pres[i, rng.choice(c, min(3, c), replace=False)] = 1
        else:
            pres[:] = np.asarray(present)
        crowd = max(1.0, (int(pres.sum(axis=1).max()) / 3.0) ** 0.5)                  # many present classes: narrower bumps
        cams = np.stack([bumps(rng, c, h, w, round_to, width / crowd) for _ in range(b)])
        sal = np.stack([saliency_map(rng, h, w) for _ in range(b)])
        mg = min(margin(cams[i], pres[i], bg_alpha) for i in range(b))
        if mg > 1e-5:
            return cams, pres, sal, mg
    raise AssertionError("no decisive input in %d seeds" % tries)
