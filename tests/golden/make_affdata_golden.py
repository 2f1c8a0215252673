#!/usr/bin/env python3
"""Pin the affinity stage's input label against the REFERENCE's own ``VOC12AffDataset.__getitem__`` (voc12/data.py:241-278).

Build container only (the reference tree does not travel; ``ACR_REFERENCE`` or the first argument names it):
    python tests/golden/make_affdata_golden.py [/path/to/reference]
writes tests/golden/affdata_<tag>.npz (data only, tens of KB each).

What runs, imported UNMODIFIED under ``make_data_golden.install_stubs`` (tool/imutils.py imports cv2, pydensecrf and torchvision at
module top; none is called here): ``voc12.data.VOC12AffDataset.__getitem__`` -- the two ``np.load(...).item()``, the stack, the
joint-transform loop, the no-score region, the two argmaxes, the label rule and ``ExtractAffinityLabelInRadius(cropsize // 8)`` -- on
tiny synthetic images and dumps in a temporary VOC tree, with the transform lists of the PSA recipe built from the reference's own
functions:
    joint   ``tool.imutils.random_crop([x], S, [0])`` (box from ``get_random_crop_box`` :167-190), then
            ``tool.imutils.RandomHorizontalFlip()`` (``np.fliplr``, :239-246)
    image   ``np.asarray`` first (ColorJitter is torchvision's and out of scope; Normalize / HWC_to_CHW are not applied: the fixture
            keeps the cropped and flipped uint8-valued image, which pins the geometry of the image half of the joint transform)
    scores  ``tool.imutils.AvgPool2d(8)`` (:228-236)
Box and flip are RECORDED, not chosen: Python's ``random`` is seeded, ``get_random_crop_box`` and ``getrandbits(1)`` are called once to
read the draws, and the same seed is set again before ``__getitem__`` runs; the seed is searched until the flip wanted comes up.

What is shimmed in this process, and only here (throw-away, nothing of it is written anywhere):
  * ``voc12.data.VOC12ImageDataset.__getitem__`` returns four values in this tree (and needs ``transform2``) while
    ``VOC12AffDataset`` unpacks two: it is replaced at run time by a function returning ``(name, img)`` with ``img`` the RGB
    ``PIL.Image`` of ``get_img_path(name, voc12_root)``, which is what the class was written against.
  * ``skimage`` is absent: ``skimage.measure.block_reduce(image, block_size, func)`` is provided by its documented rule -- pad with
    zeros to whole blocks, view as blocks, ``func`` over the block axes.
  * ``scipy.misc`` (imported by voc12/data.py, never used on this path) is provided as an empty module where scipy has dropped it.
  * the dataset's ``extract_aff_lab_func`` attribute is wrapped by a recorder that keeps its argument -- the uint8 label grid, which
    ``__getitem__`` does not return -- and calls the reference's object unchanged.
The image files are PNG-encoded under the ``.jpg`` names the reference asks for (PIL decodes by content), so the decode is lossless.

Scores lie on a 2^-10 grid in [0, 1] (stored as their uint16 numerators), so every fp32 summation order, numpy's included, gives the
same block mean: equality with the reference is exact in every cell."""
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_data_golden import REF, install_stubs  # noqa: E402

S, RADIUS, GRID = 64, 3, 1024
# tag -> (h, w, n planes per dump, flip wanted)
CASES = {"40x56_n2": (40, 56, 2, 0), "40x56_n21_flip": (40, 56, 21, 1), "80x100_n3": (80, 100, 3, 0), "80x100_n2_flip": (80, 100, 2, 1),
         "40x100_n3_flip": (40, 100, 3, 1), "48x57_n3": (48, 57, 3, 0), "48x57_n2_flip": (48, 57, 2, 1)}


def block_reduce(image, block_size, func=np.sum, cval=0):
    pad = [(0, (-s) % b) for s, b in zip(image.shape, block_size)]
    image = np.pad(image, pad, mode="constant", constant_values=cval)
    shape, axes = [], []
    for i, (s, b) in enumerate(zip(image.shape, block_size)):
        shape += [s // b, b]
        axes.append(2 * i + 1)
    return func(image.reshape(shape), axis=tuple(axes))


def synthetic_scores(rng, h, w, n):
    """Two dumps {0: bg, class + 1: ...} of (h, w) float32 planes on the 2^-10 grid: per 8 x 8 cell one plane leads (the background
    in a third of them, the two dumps agreeing in most), small per-pixel noise, and a band of cells without any score."""
    gh, gw = (h + 7) // 8, (w + 7) // 8
    keys = [0] + sorted(rng.choice(np.arange(1, 21), n - 1, replace=False).tolist())
    lead_la = np.where(rng.rand(gh, gw) < 0.35, 0, rng.randint(0, n, (gh, gw)))
    lead_ha = np.where(rng.rand(gh, gw) < 0.7, lead_la, rng.randint(0, n, (gh, gw)))
    out = []
    for lead in (lead_la, lead_ha):
        base = rng.randint(0, 600, (n, gh, gw))
        top = rng.randint(700, GRID - 8, (gh, gw))
        base = np.where(np.arange(n)[:, None, None] == lead[None], top[None], base)
        full = np.kron(base, np.ones((8, 8), np.int64))[:, :h, :w] + rng.randint(-8, 9, (n, h, w))
        full = np.clip(full, 0, GRID)
        full[:, h // 3:h // 3 + 9, w // 4:w // 4 + 17] = 0                  # no score here in any plane
        out.append(full.astype(np.uint16))
    return keys, out[0], out[1]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    install_stubs()
    sk, skm = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
    skm.block_reduce, sk.measure = block_reduce, skm
    sys.modules["skimage"], sys.modules["skimage.measure"] = sk, skm
    try:
        import scipy.misc  # noqa: F401
    except Exception:
        sys.modules["scipy.misc"] = types.ModuleType("scipy.misc")
    sys.path.insert(0, ref)
    import PIL.Image
    from tool import imutils                                        # the reference, unmodified
    from voc12 import data as vdata

    def parent_getitem(self, idx):
        name = self.img_name_list[idx]
        return name, PIL.Image.open(vdata.get_img_path(name, self.voc12_root)).convert("RGB")
    vdata.VOC12ImageDataset.__getitem__ = parent_getitem

    work = tempfile.mkdtemp(prefix="acr_affdata_golden_")
    for d in ("JPEGImages", "la", "ha"):
        os.makedirs(os.path.join(work, d))
    names = {tag: "2007_%06d" % (i + 1) for i, tag in enumerate(sorted(CASES))}
    with open(os.path.join(work, "list.txt"), "w") as f:
        for tag in sorted(CASES):
            f.write("/JPEGImages/%s.jpg /SegmentationClassAug/%s.png\n" % (names[tag], names[tag]))
    inputs = {}
    for i, tag in enumerate(sorted(CASES)):
        h, w, n, _ = CASES[tag]
        rng = np.random.RandomState(500 + i)
        image = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        keys, la, ha = synthetic_scores(rng, h, w, n)
        PIL.Image.fromarray(image).save(os.path.join(work, "JPEGImages", names[tag] + ".jpg"), format="PNG")
        for d, num in (("la", la), ("ha", ha)):
            np.save(os.path.join(work, d, names[tag] + ".npy"), {k: (p.astype(np.float32) / np.float32(GRID)) for k, p in zip(keys, num)})
        inputs[tag] = (image, keys, la, ha)

    ds = vdata.VOC12AffDataset(os.path.join(work, "list.txt"), os.path.join(work, "la"), os.path.join(work, "ha"), cropsize=S,
                               voc12_root=work, radius=RADIUS,
                               joint_transform_list=[None, lambda x: imutils.random_crop([x], S, [0])[0], imutils.RandomHorizontalFlip()],
                               img_transform_list=[np.asarray, None, None],
                               label_transform_list=[None, None, imutils.AvgPool2d(8)])
    seen = []
    extract = ds.extract_aff_lab_func

    def recorder(label):
        seen.append(label.copy())
        return extract(label)
    ds.extract_aff_lab_func = recorder
    assert [names[t] for t in sorted(CASES)] == ds.img_name_list

    for idx, tag in enumerate(sorted(CASES)):
        h, w, n, want_flip = CASES[tag]
        image, keys, la, ha = inputs[tag]
        for seed in range(1000, 1200):                              # read the draws of this seed, keep it when the flip fits
            random.seed(seed)
            box = imutils.get_random_crop_box((h, w), S)
            flip = int(random.getrandbits(1))
            if flip == want_flip:
                break
        assert flip == want_flip, tag
        random.seed(seed)
        img, (bg, fg, neg) = ds[idx]
        label = seen.pop()
        assert not seen and label.dtype == np.uint8 and label.shape == (S // 8, S // 8)
        img = np.asarray(img)
        assert img.shape == (S, S, 3) and np.array_equal(img, img.astype(np.uint8))
        ct, cb, cl, cr, it, ib, il, ir = box
        np.savez_compressed(os.path.join(HERE, "affdata_%s.npz" % tag), S=np.int32(S), radius=np.int32(RADIUS), grid=np.int32(GRID),
                            image=image, keys=np.asarray(keys, np.int32), la_num=la, ha_num=ha,
                            box=np.asarray([ct, cl, it, il, cb - ct, cr - cl], np.int32), flip=np.int32(flip), ref_image=img.astype(np.uint8),
                            label=label, bg=bg.numpy().astype(np.uint8), fg=fg.numpy().astype(np.uint8), neg=neg.numpy().astype(np.uint8))
        print(tag, "box", box, "flip", flip, "label values", np.unique(label).tolist(), "pairs", int(bg.sum()), int(fg.sum()), int(neg.sum()))


if __name__ == "__main__":
    main()
