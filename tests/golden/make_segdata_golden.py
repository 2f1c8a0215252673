#!/usr/bin/env python3
"""Pin the segmentation-loader restatement (tests/segdata_ref.py) against runs of the REFERENCE's own chunk functions.

Build container only (the reference tree does not travel):   python tests/golden/make_segdata_golden.py
writes tests/golden/segdata_chunk_{v4_a,v4_b,v4_c,v3_a}.npz.

What runs: ``myTool.get_data_from_chunk_v4`` (myTool.py:1257-1310) and ``myTool.get_data_from_chunk_v3`` (:1202-1253), imported
UNMODIFIED from the reference tree, with its real ``RandomResizeLong2`` (:1010-1023), ``flip2`` (:901-905), ``RandomCrop2``
(:957-993), normalisation, ``ori_images`` de-normalisation (:1293-1297), HWC->CHW and chunk assembly, driven by Python's ``random``
and ``np.random`` seeded here.

What is stubbed (the module-level stubs are make_data_golden.py's, reused)
--------------------------------------------------------------------------
  * ``cv2.imread``      a seeded BGR uint8 array per file stem: the decode is not under test;
  * ``cv2.resize``      oracle/data_oracle.cv2_resize_linear by default, and tests/segdata_ref.cv2_resize_nearest for
                        ``interpolation=cv2.INTER_NEAREST`` -- OpenCV's published rules.  The two resizes therefore stay the UNPINNED
                        steps (checked against themselves); draw order, target shape, flip of image AND map, float64 normalisation,
                        placement of image / map / cropping mask for images larger and smaller than the crop, the zero containers,
                        the float32 de-normalisation and its truncation, layouts -- all are the reference's own code;
  * ``PIL.Image.open``  a seeded uint8 map per file stem (np.asarray of it is what the reference takes, :1225,1280): values 0..20
                        with some 255 for v4 (a label map), 0 / 255 for v3 (a saliency map).  The hard-coded directories of
                        :1223,1278 therefore never matter;
  * ``voc12/cls_labels.npy`` is written to a temp dir with seeded multi-hot vectors and the script runs from there.
"""
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_data_golden as MD  # noqa: E402   (the cv2 / torchvision / pydensecrf stubs and the seeded "decoder")
import segdata_ref as SR  # noqa: E402        (only as the body of the INTER_NEAREST stub)

KIND = {"kind": "v4"}


def decoded_map(stem, kind):
    """The array np.asarray(PIL.Image.open(<stem>.png)) yields: uint8 (h, w), a pure function of the name and the kind."""
    h, w = MD.SIZES[stem]
    rs = np.random.RandomState((int.from_bytes(stem.encode(), "little") + (17 if kind == "v4" else 31)) % (2 ** 31))
    if kind == "v3":
        return (rs.randint(0, 2, (h, w)) * 255).astype(np.uint8)
    m = rs.randint(0, 21, (h, w)).astype(np.uint8)
    m[rs.rand(h, w) < 0.1] = 255
    return m


def install_stubs():
    MD.install_stubs()
    cv2 = sys.modules["cv2"]
    linear = cv2.resize

    def resize(img, dsize, interpolation=None, **kw):
        if interpolation == cv2.INTER_NEAREST:
            return SR.cv2_resize_nearest(img, int(dsize[0]), int(dsize[1]))
        return linear(img, dsize, interpolation=interpolation, **kw)
    cv2.resize = resize


def main():
    install_stubs()
    sys.path.insert(0, MD.REF)
    import myTool                                                  # the reference, unmodified
    myTool.PIL.Image.open = lambda path, *a, **k: decoded_map(os.path.splitext(os.path.basename(path))[0], KIND["kind"])
    work = tempfile.mkdtemp(prefix="acr_segdata_golden_")
    os.makedirs(os.path.join(work, "voc12"))
    four = [("2007_000001", 60, 90), ("2007_000002", 90, 60), ("2007_000003", 30, 40), ("2007_000004", 48, 48)]
    cases = {
        # kind, crop, [(stem, h, w)], seed -- images larger than the crop in both, one, or no dimension; odd sizes; a chunk of one.
        # v4 resizes the long side to exactly the crop, so one axis always pads; v3 draws it from [0.9 S, S / 0.875]: a draw above
        # S puts the crop box inside the image
        "v4_a": ("v4", 48, four, 3),
        "v4_b": ("v4", 64, [("2008_000011", 37, 113), ("2008_000012", 200, 150), ("2008_000013", 64, 80)], 12),
        "v4_c": ("v4", 32, [("2009_000021", 33, 31)], 5),
        "v3_a": ("v3", 48, four, 7),
    }
    labels = {}
    lr = np.random.RandomState(99)
    for _, (_, _, imgs, _) in cases.items():
        for stem, h, w in imgs:
            MD.SIZES[stem] = (h, w)
            if stem not in labels:
                labels[stem] = (lr.rand(20) > 0.8).astype(np.float32)
    np.save(os.path.join(work, "voc12", "cls_labels.npy"), labels)
    os.chdir(work)
    args = types.SimpleNamespace(IMpath=os.path.join(work, "JPEGImages"), crop_size=0)
    for name, (kind, crop, imgs, seed) in cases.items():
        chunk = [stem for stem, _, _ in imgs]
        args.crop_size = crop
        KIND["kind"] = kind
        random.seed(seed)
        np.random.seed(seed)
        fn = myTool.get_data_from_chunk_v4 if kind == "v4" else myTool.get_data_from_chunk_v3
        images, ori_images, lab, croppings, name_list, target = fn(chunk, args)
        assert list(name_list) == chunk and tuple(images.shape) == (len(chunk), 3, crop, crop)
        assert croppings.shape == (crop, crop, len(chunk)) and tuple(target.shape) == (len(chunk), crop, crop)
        out = {"crop": np.int64(crop), "seed": np.int64(seed), "images": images.numpy().astype(np.float32),
               "ori_images": np.asarray(ori_images, np.uint8), "croppings": np.asarray(croppings), "target": target.numpy(),
               "labels": lab.numpy().astype(np.float32)}
        for i, stem in enumerate(chunk):
            out["rgb_%d" % i] = np.ascontiguousarray(MD.decoded_bgr(stem)[:, :, ::-1])       # what cvtColor hands on: RGB uint8
            out["map_%d" % i] = decoded_map(stem, kind)
        full = [bool(croppings[:, :, i].all()) for i in range(len(chunk))]
        if kind == "v3":
            assert any(full) and not all(full), "v3 case must cover both the crop-inside-image and the padded branch: %s" % full
        path = os.path.join(HERE, "segdata_chunk_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%s: %s crop %d -> images %s, cropping fully inside %s, target values %s...  (%d bytes)" % (
            name, [MD.SIZES[s] for s in chunk], crop, tuple(images.shape), full, np.unique(target.numpy())[:6], os.path.getsize(path)))


if __name__ == "__main__":
    main()
