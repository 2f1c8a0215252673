"""The affinity stage's input label restated in numpy, step by step as ``VOC12AffDataset.__getitem__`` takes it (voc12/data.py:241-278
under the joint RandomCrop / RandomHorizontalFlip and AvgPool2d(8), tool/imutils.py:167-246; pinned to fixtures written by that code
in tests/test_affdata_cpu.py): stack, crop into a zero container, flip the container, pool 8 x 8, no-score region, two argmaxes,
label.  It crops and THEN flips, as the reference does; the kernel reads flip-then-crop records with the box mirrored
(``data.aff_record``), so the two share no index arithmetic.

The mean is the exact one wherever a float64 sum of 64 float32 values is exact (values 0 or in [2^-20, 1]): summed in float64,
divided by 64, rounded to float32 once."""
import numpy as np

NO_SCORE = np.float32(1e-5)


def stack(la, ha):
    """step 1: {key: (h, w)} dicts or (n, h, w) stacks -> (h, w, 2n) float32, the low-alpha planes first"""
    planes = [np.asarray(p) for s in (la, ha) for p in (s.values() if isinstance(s, dict) else s)]
    return np.transpose(np.stack(planes).astype(np.float32, copy=False), (1, 2, 0))


def crop_flip(x, SH, SW, box, flip):
    """step 2: x (h, w, C) -> the (SH, SW, C) zero container with box = (cont_top, cont_left, img_top, img_left, ch, cw) copied in,
    then mirrored left-right when ``flip``"""
    ct, cl, it, il, ch, cw = (int(v) for v in box)
    cont = np.zeros((SH, SW, x.shape[2]), x.dtype)
    cont[ct:ct + ch, cl:cl + cw] = x[it:it + ch, il:il + cw]
    return cont[:, ::-1].copy() if flip else cont


def pool8(cont):
    """step 3: (SH, SW, C) -> (SH / 8, SW / 8, C) float32 block means"""
    SH, SW, C = cont.shape
    assert SH % 8 == 0 and SW % 8 == 0
    s = cont.reshape(SH // 8, 8, SW // 8, 8, C).astype(np.float64).sum(axis=(1, 3))
    return (s / 64.0).astype(np.float32)


def label_of_pooled(pooled):
    """steps 4-6: (gh, gw, 2n) float32 -> (gh, gw) uint8"""
    n = pooled.shape[2] // 2
    no_score = pooled.max(axis=-1) < NO_SCORE
    la = np.argmax(pooled[..., :n], axis=-1).astype(np.uint8)
    ha = np.argmax(pooled[..., n:], axis=-1).astype(np.uint8)
    label = la.copy()
    label[la == 0] = 255
    label[ha == 0] = 0
    label[no_score] = 255
    return label


def aff_label(la, ha, SH, SW, box, flip):
    """steps 1-6 for one image; ``box`` is the crop box on the UNFLIPPED image, ``flip`` mirrors the container afterwards"""
    return label_of_pooled(pool8(crop_flip(stack(la, ha), SH, SW, box, flip)))


def aff_label_whole(la, ha):
    """the uncropped form: the image zero-padded bottom / right to multiples of 8"""
    x = stack(la, ha)
    h, w = x.shape[:2]
    return aff_label(la, ha, (h + 7) // 8 * 8, (w + 7) // 8 * 8, (0, 0, 0, 0, h, w), False)


def record_crop_flip(x, SH, SW, rec):
    """The container an ``acr_pre_image`` record describes (flip the image, then crop): for the mirrored-box identity"""
    f = x[:, ::-1] if rec["flip"] else x
    cont = np.zeros((SH, SW, x.shape[2]), x.dtype)
    ct, cl, it, il, ch, cw = (int(rec[k]) for k in ("cont_top", "cont_left", "img_top", "img_left", "ch", "cw"))
    cont[ct:ct + ch, cl:cl + cw] = f[it:it + ch, il:il + cw]
    return cont
