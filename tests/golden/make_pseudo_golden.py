#!/usr/bin/env python3
"""Generate tests/golden/pseudo_{a,b,c,d}.npz by running the *reference's own* ``compute_seg_label_rrm`` (myTool.py:674-744).

Run where the reference tree exists (``ACR_REFERENCE``, default /root/reference):   python tests/golden/make_pseudo_golden.py
``myTool`` is imported UNMODIFIED from where it lies, under the throw-away stubs for cv2, torchvision and pydensecrf that
make_data_golden.py installs (taken from there); nothing of it is restated here.  Around the call:
  * ``myTool._crf_with_alpha`` is set to a function that hands back prepared dense (21, W, H) arrays (the refinement is not under
    test: crf.py / pamr.py have their own fixtures), keyed by the alpha the function asks for (2 and 14, :703-704);
  * ``cv2.imwrite`` is a no-op (the function writes a colour preview to a fixed path, :740);
  * ``sys.setprofile`` copies ``crf_la_label``, ``crf_ha_label``, ``cam_img``, ``cam_sure_region`` and ``not_sure_region`` from the
    function's frame at its return event -- the confidence rule is computed there (:710-735) but its last line is kept commented
    (:737; live in the sibling function at :109).
Each file holds the inputs (present planes only, float32), the returned ``crf_label`` (``label`` -- the expectation for
ignore_uncertain=False), ``crf_label`` with ``[not_sure_region] = 255`` (``label_sure`` -- the reference's own arrays under its own
commented line, the expectation for True) and the copied locals.

Every case is asserted DECISIVE: at every pixel bg = (1 - max cam)^36 is more than 1e-5 (relative) away from the largest class
value and from 0.3, so the <= 1-ulp (1.2e-7) differences between numpy's float32 power, the restatement's fp64 pow and the
device's cannot change a comparison; the seed moves on until that holds.  Every label of the low-alpha map must also own at
least one CAM value above 0.1 where it wins (else the reference raises IndexError, :720).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("ACR_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_data_golden import install_stubs  # noqa: E402
import pseudo_ref as R  # noqa: E402  (seeded inputs and the margin only; the expectations come from the reference)

WANTED = ("crf_la_label", "crf_ha_label", "cam_img", "cam_sure_region", "not_sure_region")
CASES = {
    # tag: (W, H, classes, values rounded to 1/round_to, bias on the background score, seed)
    "a": (48, 64, [1, 8, 14], None, 0.0, 11),
    "b": (33, 35, [5], None, 0.0, 12),
    "c": (40, 52, list(range(20)), 100, 0.0, 13),
    "d": (30, 44, [3, 19], None, 5.0, 14),
}


def run_reference(myTool, cams, classes, la, ha):
    w, h = cams.shape[1:]
    norm_cam = R.dense(cams, classes, 20)
    cam_label = np.zeros(20, np.float32)
    cam_label[classes] = 1
    labels = [0] + [c + 1 for c in classes]
    prepared = {2: R.dense(la, labels, 21), 14: R.dense(ha, labels, 21)}
    myTool._crf_with_alpha = lambda ori_img, cam_dict, alpha: prepared[alpha].copy()
    seen = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "compute_seg_label_rrm":
            for name in WANTED:
                seen[name] = np.array(frame.f_locals[name])

    sys.setprofile(prof)
    try:
        crf_label = myTool.compute_seg_label_rrm(np.zeros((w, h, 3), np.uint8), cam_label, norm_cam, "x")
    finally:
        sys.setprofile(None)
    assert sorted(seen) == sorted(WANTED)
    return np.array(crf_label), seen


def main():
    install_stubs()
    sys.modules["cv2"].imwrite = lambda *a, **k: True
    sys.path.insert(0, REF)
    import myTool                                                  # the reference, unmodified
    for tag, (w, h, classes, round_to, bg_bias, seed) in CASES.items():
        for t in range(50):
            cams, classes, la, ha, mg = R.decisive_case(seed + 100 * t, len(classes), w, h, classes, round_to, bg_bias)
            try:
                crf_label, seen = run_reference(myTool, cams, classes, la, ha)
            except IndexError:                                     # a label of L_la with n = 0: the reference raises, next seed
                continue
            break
        else:
            raise AssertionError("case %s: no usable seed" % tag)
        assert mg > 1e-5
        # every label of L_la owns a value above the floor where it wins (the reference would have raised otherwise)
        for l in np.unique(seen["crf_la_label"]):
            if l:
                n = int(((seen["cam_img"] == l) & (cams[classes.index(l - 1)] > np.float32(0.1))).sum())
                assert n >= 1, (tag, l)
        if tag == "d":
            assert not seen["crf_la_label"].any()
        label = crf_label.astype(np.uint8)
        assert np.array_equal(label, crf_label)
        sure = label.copy()
        sure[seen["not_sure_region"]] = 255
        path = os.path.join(HERE, "pseudo_%s.npz" % tag)
        np.savez_compressed(path, cams=cams, classes=np.asarray(classes, np.int32), la=la, ha=ha, label=label, label_sure=sure,
                            la_label=seen["crf_la_label"].astype(np.uint8), ha_label=seen["crf_ha_label"].astype(np.uint8),
                            cam_img=seen["cam_img"].astype(np.uint8), cam_sure_region=seen["cam_sure_region"],
                            not_sure_region=seen["not_sure_region"])
        print("pseudo_%s: %dx%d K=%d  margin %.3e  labels %s  sure-map labels %s  L_la labels %s  (%d bytes)"
              % (tag, w, h, len(classes), mg, dict(zip(*np.unique(label, return_counts=True))),
                 dict(zip(*np.unique(sure, return_counts=True))), np.unique(seen["crf_la_label"]).tolist(), os.path.getsize(path)))


if __name__ == "__main__":
    main()
