#!/usr/bin/env python3
"""Writes tests/golden/colorjitter_*.npz with Pillow itself: torchvision's ColorJitter on a PIL image is ``ImageEnhance.Brightness``,
``ImageEnhance.Contrast``, ``ImageEnhance.Color`` and, for the hue, ``convert("HSV")``, a uint8 wrap-around add on the H band and
``merge(...).convert("RGB")`` (torchvision/transforms/_functional_pil.py adjust_hue).  Every file records ``PIL.__version__``.

    python tests/golden/make_colorjitter_golden.py

  colorjitter_orders.npz   a 5 x 7 random image and a 33 x 65 image of random pixels from a 32-colour palette (black, white, greys and
                           primaries among them: the palette keeps the compressed file small) under all 24 operation orders with
                           the factors (1.27, 0.74, 1.3) and hue -0.05
  colorjitter_single.npz   each operation alone on the 5 x 7 image and on an 8 x 32 image of ramps, at the factors 0, 0.3, 0.9999, 1,
                           1.0001, 1.3 and 2.5 (2.5 clips at both ends); hue at -0.5, 0.5, 0 and -0.05
  colorjitter_mean.npz     contrast 0 on a 1 x 2 and a 1 x 3 grey image whose mean lies on and just beside x.5: (10, 11) -> 11,
                           (10, 10, 11) -> 10
"""
import itertools
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
FACTORS = (1.27, 0.74, 1.3)
HUE = -0.05
SINGLE = (0.0, 0.3, 0.9999, 1.0, 1.0001, 1.3, 2.5)
HUES = (-0.5, 0.5, 0.0, -0.05)


def adjust_hue(img, hue_factor):
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(int(hue_factor * 255) % 256)          # the uint8 wrap-around of torchvision's adjust_hue
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


OPS = (lambda im, f: ImageEnhance.Brightness(im).enhance(f), lambda im, f: ImageEnhance.Contrast(im).enhance(f),
       lambda im, f: ImageEnhance.Color(im).enhance(f), adjust_hue)


def jitter(arr, order, factors):
    im = Image.fromarray(arr, "RGB")
    for op in order:
        im = OPS[op](im, factors[op])
    return np.asarray(im)


def images():
    small = np.random.default_rng(3).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    rng = np.random.default_rng(4)
    palette = rng.integers(0, 256, (32, 3), dtype=np.uint8)
    palette[:10] = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (1, 1, 1), (254, 254, 254), (255, 0, 0), (0, 255, 0), (0, 0, 255),
                    (255, 255, 0), (0, 255, 255)]
    large = palette[rng.integers(0, 32, (33, 65))]
    x = np.arange(32, dtype=np.int64)
    ramp = np.zeros((8, 32, 3), np.uint8)
    ramp[0] = (x * 255 // 31)[:, None]                        # grey ramp 0..255
    ramp[1, :, 0], ramp[2, :, 1], ramp[3, :, 2] = x * 255 // 31, x * 255 // 31, x * 255 // 31
    ramp[4, :, 0], ramp[4, :, 1] = 255, x * 8                # red -> yellow: the hue sectors' edges
    ramp[5, :, 1], ramp[5, :, 2] = 255 - x * 8, 255
    ramp[6] = np.stack([x * 8, 255 - x * 8, (x * 37) % 256], -1)
    ramp[7] = np.stack([255 - x, 254 - x // 2, 253 + 0 * x], -1)     # nearly white, low saturation
    return small, large, ramp


def main():
    small, large, ramp = images()
    version = np.array(PIL.__version__)
    orders = np.array(list(itertools.permutations(range(4))), np.int32)
    out = {"pil_version": version, "orders": orders, "factors": np.array(FACTORS + (HUE,), np.float64), "small": small, "large": large}
    for name, img in (("small", small), ("large", large)):
        out[name + "_out"] = np.stack([jitter(img, o, FACTORS + (HUE,)) for o in orders])
    np.savez_compressed(os.path.join(HERE, "colorjitter_orders.npz"), **out)

    out = {"pil_version": version, "small": small, "ramp": ramp, "factors": np.array(SINGLE, np.float64), "hues": np.array(HUES, np.float64)}
    for name, img in (("small", small), ("ramp", ramp)):
        for op in range(3):
            out["%s_op%d" % (name, op)] = np.stack([jitter(img, (op,), {op: f}) for f in SINGLE])
        out["%s_op3" % name] = np.stack([jitter(img, (3,), {3: f}) for f in HUES])
    np.savez_compressed(os.path.join(HERE, "colorjitter_single.npz"), **out)

    two, three = np.array([[10, 11]], np.uint8), np.array([[10, 10, 11]], np.uint8)
    out = {"pil_version": version}
    for name, g in (("two", two), ("three", three)):
        img = np.repeat(g[..., None], 3, -1)
        out[name], out[name + "_out"] = img, jitter(img, (1,), {1: 0.0})
    np.savez_compressed(os.path.join(HERE, "colorjitter_mean.npz"), **out)


if __name__ == "__main__":
    main()
