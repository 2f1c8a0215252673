"""numpy restatement of the colour jitter include/acr_hip.h defines ("colour jitter"): torchvision's ColorJitter on a PIL image, i.e.
Pillow's ImageEnhance.Brightness / Contrast / Color and an HSV round trip, uint8 in and uint8 out.  Every operation below is of the
type written (float32 where the C is ``float``, float64 where it is ``double``); tests/test_colorjitter_cpu.py holds it against live
Pillow and against the fixtures Pillow wrote, tests/test_colorjitter_gpu.py holds the kernels against it, bit for bit."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
F32, F64 = np.float32, np.float64


def gray(img):
    """(h, w, 3) uint8 -> (h, w) uint8: ``(r 19595 + g 38470 + b 7471 + 0x8000) >> 16``."""
    x = img.astype(np.int64)
    return ((x[..., 0] * 19595 + x[..., 1] * 38470 + x[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, a):
    """``deg + a (img - deg)`` in float32, truncated; clipped to 0..255 only for ``a`` outside [0, 1], as Pillow's ImagingBlend."""
    a = F32(a)
    deg, img = np.asarray(deg).astype(np.int32), np.asarray(img).astype(np.int32)
    t = deg.astype(F32) + a * (img - deg).astype(F32)       # a float32 product, then a float32 sum
    if F32(0) <= a <= F32(1):
        return t.astype(np.int32).astype(np.uint8)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32)))
    return out.astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def saturation(img, f):
    return blend(gray(img)[..., None], img, f)


def contrast_mean(img):
    """``int(mean of gray + 0.5)`` as the exact integer ``(2 sum + n) // (2 n)``."""
    g = gray(img)
    s, n = int(g.astype(np.int64).sum()), g.size
    return (2 * s + n) // (2 * n)


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def rgb2hsv(img):
    """Pillow's rgb2hsv_row on a (..., 3) uint8 array."""
    r, g, b = (img[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    flat = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc, gc, bc = ((maxc - x).astype(F32) / cr for x in (r, g, b))
        h = np.where(r == maxc, (bc - gc).astype(F64),                                       # a float32 difference, widened
                     np.where(g == maxc, 2.0 + rc.astype(F64) - bc.astype(F64), 4.0 + gc.astype(F64) - rc.astype(F64))).astype(F32)
        h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
        H = np.clip((h.astype(F64) * 255.0).astype(np.int32), 0, 255)
        S = np.clip((s.astype(F64) * 255.0).astype(np.int32), 0, 255)
    H, S = np.where(flat, 0, H), np.where(flat, 0, S)
    return np.stack([H, S, maxc], -1).astype(np.uint8)


def _round_clip(x):
    """C's round (half away from zero; the values here are >= 0), clipped to 0..255."""
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.int32)


def hsv2rgb(hsv):
    """Pillow's hsv2rgb_row on a (..., 3) uint8 array."""
    H, S, V = (hsv[..., k].astype(np.int32) for k in range(3))
    hf = H.astype(F32).astype(F64) * 6.0 / 255.0
    i = np.floor(hf).astype(F32)
    f = (hf - i.astype(F64)).astype(F32)
    fs = (S.astype(F32).astype(F64) / 255.0).astype(F32)
    Vd = V.astype(F64)
    p = _round_clip(Vd * (1.0 - fs.astype(F64)))
    q = _round_clip(Vd * (1.0 - (fs * f).astype(F64)))                                      # fs f: a float32 product
    t = _round_clip(Vd * (1.0 - fs.astype(F64) * (1.0 - f.astype(F64))))
    k = i.astype(np.int32) % 6
    table = (((V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)))
    out = [np.select([k == j for j in range(6)], [table[j][c] for j in range(6)]) for c in range(3)]
    gray_px = S == 0
    return np.stack([np.where(gray_px, V, o) for o in out], -1).astype(np.uint8)


def hue_shift(hue_factor):
    """``trunc(hue_factor 255) mod 256``: -0.05 -> 244."""
    return int(float(hue_factor) * 255) % 256


def hue(img, hue_factor):
    hsv = rgb2hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + hue_shift(hue_factor)) % 256).astype(np.uint8)
    return hsv2rgb(hsv)


OPS = {BRIGHTNESS: brightness, CONTRAST: contrast, SATURATION: saturation, HUE: hue}


def color_jitter(img, params):
    """``params`` = (order, b, c, s, hue_factor) as ``data.ColorJitter.draw`` returns it: the operations of ``order`` whose factor
    is not None, in that order, on the whole image."""
    order, factors = params[0], params[1:]
    for op in order:
        if factors[int(op)] is not None:
            img = OPS[int(op)](img, factors[int(op)])
    return img
