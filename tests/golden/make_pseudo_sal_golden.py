#!/usr/bin/env python3
"""Generate tests/golden/pseudo_sal_{a,b,c,d}.npz by running the *reference's own* ``compute_seg_label_3`` (myTool.py:188-264) and
``compute_seg_label_two_step`` (:313-385).

Run where the reference tree exists (``ACR_REFERENCE``, default /root/reference):   python tests/golden/make_pseudo_sal_golden.py
``myTool`` is imported UNMODIFIED from where it lies, under the throw-away stubs for cv2, torchvision and pydensecrf that
make_data_golden.py installs (taken from there); nothing of it is restated here.  Around the calls:
  * ``cv2.imwrite`` is a no-op (both functions write previews to fixed paths);
  * ``cv2.morphologyEx`` -- cv2 is not installed -- is stubbed twice per case: once returning all 255, so that the returned label
    is the reference's own map before the opening (``label_pre``, the expectation for open_size=0), and once with the opening as
    include/acr_hip.h defines it by OpenCV's documented formulas (tests/pseudo_sal_ref.morph_open; ``label``, the expectation for
    open_size=10).  The first half is pinned by the reference's code alone, the second also by that definition;
  * for ``two_step`` (bg_alpha = 32; it returns nothing), ``cv2.imread`` returns an image of the label's own size and
    ``cv2.resize`` hands its input back after keeping a copy: that copy is the label (``label32_pre`` / ``label32``).
Each file holds the inputs (cams (20, H, W) float32, cam_label (20,) float32, saliency (H, W) uint8), the labels and the saliency
map the reference returns / leaves modified (``saliency_out``).

Every case is asserted DECISIVE for both exponents: at every pixel bg = (1 - max cam)^alpha is more than 1e-5 (relative) away from
the largest present class value, so the <= 1-ulp (1.2e-7) differences between numpy's float32 power, the restatement's fp64 pow
and the device's cannot change a comparison; the seed moves on until that holds.  Every case must also contain grabbed pixels,
255 pixels, pixels the opening removed and pixels it kept.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("ACR_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_data_golden import install_stubs  # noqa: E402
import pseudo_sal_ref as R  # noqa: E402  (seeded inputs, the margin and the DEFINED opening; the rule's expectations come from the reference)

CASES = {
    # tag: (H, W, present classes, values rounded to 1/round_to, width of the bumps, seed)
    "a": (41, 50, [6], None, 0.35, 21),
    "b": (40, 52, [1, 8, 14], None, 0.2, 22),
    "c": (43, 49, list(range(20)), 100, 0.35, 23),
    "d": (38, 51, [3, 11, 19], None, 0.2, 24),               # class 11: one positive value; class 5: absent with a non-zero plane
}


def run_reference(myTool, cv2, cams, cam_label, sal, opening):
    h, w = sal.shape
    cv2.morphologyEx = (lambda frg, op, kernel: R.morph_open(frg, kernel.shape[0])) if opening else (lambda frg, op, kernel: np.full_like(frg, 255))
    ori = np.zeros((h, w, 3), np.uint8)
    s3 = sal.copy()
    label3, sal3 = myTool.compute_seg_label_3(ori, cam_label.copy(), cams.copy(), "x", s3)
    kept = []
    cv2.imread = lambda path, *a: np.zeros((h, w, 3), np.uint8)

    def resize(img, dsize, *a, **k):
        assert tuple(dsize) == (w, h)
        kept.append(np.array(img))
        return img
    cv2.resize = resize
    s32 = sal.copy()
    assert myTool.compute_seg_label_two_step(ori, cam_label.copy(), cams.copy(), "x", 0, s32, None, save_pseudo=False, cut=0.9) is None
    assert len(kept) == 1
    return np.array(label3), np.array(sal3), kept[0], s32


def main():
    install_stubs()
    cv2 = sys.modules["cv2"]
    cv2.imwrite = lambda *a, **k: True
    cv2.MORPH_OPEN = 2
    sys.path.insert(0, REF)
    import myTool                                                  # the reference, unmodified
    for tag, (h, w, classes, round_to, width, seed) in CASES.items():
        present = np.zeros((1, 20), np.uint8)
        present[0, classes] = 1
        for t in range(50):
            cams, _, sal, mg = R.decisive_case(seed + 100 * t, 1, 20, h, w, present, round_to, width=width)
            cams, sal = cams[0], sal[0]
            if tag == "d":
                one = np.zeros((h, w), np.float32)
                one[h // 2, w // 3] = 0.8
                cams[11] = one
            if tag != "c":                                         # absent classes keep non-zero planes only where it is a case
                for c in range(20):
                    if c not in classes and not (tag == "d" and c == 5):
                        cams[c] = 0
            cam_label = present[0].astype(np.float32)
            mg = min(R.margin(cams, present[0], 12), R.margin(cams, present[0], 32))
            if mg <= 1e-5:
                continue
            pre, sal_pre, pre32, sal_pre32 = run_reference(myTool, cv2, cams, cam_label, sal, opening=False)
            lab, sal_out, lab32, sal_out32 = run_reference(myTool, cv2, cams, cam_label, sal, opening=True)
            grabbed = (sal == 0) & (pre != 0)
            removed, kept = (pre != 0) & (lab == 0), lab != 0
            thr = R.thresholds(cams, present[0].astype(bool))
            above = sum((cams[c] > thr[c]).astype(int) for c in classes)
            twice = (above >= 2) & grabbed                         # above the thresholds of two classes: the lowest class keeps it
            if grabbed.any() and (lab == 255).any() and removed.any() and kept.any() and (lab32 != lab).any() and (twice.any() or len(classes) == 1):
                break
            print("  %s seed %d: grabbed %d (twice %d), 255 %d, removed %d, kept %d" % (tag, seed + 100 * t, grabbed.sum(), twice.sum(),
                                                                                    (lab == 255).sum(), removed.sum(), kept.sum()))
        else:
            raise AssertionError("case %s: no usable seed" % tag)
        # the saliency map does not depend on the opening or on the exponent; the grab leaves its mark there
        for s in (sal_pre, sal_pre32, sal_out32):
            assert np.array_equal(s, sal_out)
        assert np.array_equal(sal_out != sal, grabbed) and (sal_out[grabbed] == 255).all()
        if tag == "c":
            assert np.array_equal(cams, (np.round(cams * 100) / 100).astype(np.float32))
            order = np.sort(cams[0][cams[0] > 0])
            assert (order == thr[0]).sum() > 1                     # ties at the threshold
        if tag == "d":
            assert (cams[11] > 0).sum() == 1 and thr[11] == np.inf and cams[5].any() and not (pre == 6).any()
        out = {}
        for name, arr in (("label_pre", pre), ("label", lab), ("label32_pre", pre32), ("label32", lab32)):
            out[name] = arr.astype(np.uint8)
            assert np.array_equal(out[name], arr)
        path = os.path.join(HERE, "pseudo_sal_%s.npz" % tag)
        np.savez_compressed(path, cams=cams, cam_label=cam_label, saliency=sal, saliency_out=sal_out.astype(np.uint8), **out)
        print("pseudo_sal_%s: %dx%d present %s  margin %.3e  grabbed %d (above two thresholds %d)  removed %d  labels %s  (%d bytes)"
              % (tag, h, w, classes, mg, int(grabbed.sum()), int(twice.sum()), int(removed.sum()),
                 dict(zip(*np.unique(lab, return_counts=True))), os.path.getsize(path)))


if __name__ == "__main__":
    main()
