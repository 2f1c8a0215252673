"""numpy restatement of the segmentation-training loaders -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restates myTool.py:1257-1310 (`get_data_from_chunk_v4`: image + target map) and :1202-1253 (`get_data_from_chunk_v3`: image +
saliency map; the same code with another resize range) over already decoded arrays, on top of oracle/data_oracle.py
(`cv2_resize_linear`, `normalise`, the crop draws).  Added here: `RandomResizeLong2`'s nearest resize of the map (:1021),
`flip2` (:901-905), `RandomCrop2`'s placement of image, map and cropping mask (:957-993), `ori_images` in the float32 the
reference's container has (:981, :1293-1297) and the draw order.

Parity status: everything is a literal restatement except the two resizes.  `cv2_resize_nearest` restates OpenCV's published
INTER_NEAREST rule (modules/imgproc/src/resize.cpp, `resizeNN`): destination pixel d reads source min(floor(d * src/dst), src-1).
OpenCV evaluates d * (src/dst) in double; the restatement uses exact integer division, which can differ where the exact quotient
is an integer and the double product falls just below it.  cv2 is not installed here: PARITY UNPINNED for that step, in the same
sense as `cv2_resize_linear`.  tests/golden/make_segdata_golden.py pins the rest against the reference's own functions.
"""
import os

import numpy as np

from oracle import data_oracle as DO

MEAN, STD = DO.MEAN, DO.STD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["v4_a", "v4_b", "v4_c", "v3_a"]                  # tests/golden/segdata_chunk_<name>.npz (make_segdata_golden.py)


def load_fixture(name):
    """(fixture dict, decoded RGB arrays, maps, kind) of one reference run"""
    fx = dict(np.load(os.path.join(GOLDEN, "segdata_chunk_%s.npz" % name)))
    n = fx["images"].shape[0]
    return fx, [fx["rgb_%d" % i] for i in range(n)], [fx["map_%d" % i] for i in range(n)], name[:2]


def cv2_resize_nearest(img, new_w, new_h):
    """cv2.resize(img, (new_w, new_h), interpolation=cv2.INTER_NEAREST) for an (h, w[, c]) array of any dtype."""
    h, w = img.shape[:2]
    sy = np.minimum(np.arange(new_h, dtype=np.int64) * h // new_h, h - 1)
    sx = np.minimum(np.arange(new_w, dtype=np.int64) * w // new_w, w - 1)
    return img[sy][:, sx]


def long_range(dim, kind):
    """The (min_long, max_long) RandomResizeLong2 is called with: v4 :1284, v3 :1228."""
    return (int(dim), int(dim)) if kind == "v4" else (int(dim * 0.9), int(dim / 0.875))


def draw_geometry(h, w, dim, lo_hi, pyrandom, nprandom):
    """Per-image draws in the reference's order: flip_p (:1275), randint of RandomResizeLong2 (:1011), RandomCrop2 w before h (:967-979)."""
    flip_p = nprandom.uniform(0, 1)
    target_long = pyrandom.randint(lo_hi[0], lo_hi[1])
    new_w, new_h = DO.resize_long_shape(h, w, target_long)
    g = dict(rw=new_w, rh=new_h, flip=int(flip_p > 0.5))
    g.update(DO.random_crop_boxes(new_h, new_w, dim, pyrandom))
    return g


def ori_from_image(img_f32):
    """:1293-1297 on a (dim, dim, 3) float32 container: numpy evaluates multiply, add, multiply in float32, astype truncates."""
    img_f32 = np.asarray(img_f32, np.float32)
    out = np.zeros_like(img_f32)
    for c in range(3):
        out[:, :, c] = (img_f32[:, :, c] * np.float32(STD[c]) + np.float32(MEAN[c])) * np.float32(255.0)
    return np.clip(out, 0, 255).astype(np.uint8)


def seg_image(rgb_u8, map_u8, dim, geom, map_fill=0):
    """One image of v3 / v4 with the draws in `geom` -> (image (3,dim,dim) float32, ori (3,dim,dim) uint8, cropping (dim,dim) bool,
    map (dim,dim) uint8).  `map_fill` = 0 is the reference's zero container (:982)."""
    img = DO.cv2_resize_linear(rgb_u8.astype(np.float64), geom["rw"], geom["rh"])
    m = cv2_resize_nearest(map_u8, geom["rw"], geom["rh"])
    if geom["flip"]:
        img, m = np.fliplr(img), np.fliplr(m)
    img = DO.normalise(img)
    ct, cl, it, il, ch, cw = (geom[k] for k in ("cont_top", "cont_left", "img_top", "img_left", "ch", "cw"))
    box = np.zeros((dim, dim, 3), np.float32)
    mbox = np.full((dim, dim), map_fill, np.uint8)
    cropping = np.zeros((dim, dim), bool)
    box[ct:ct + ch, cl:cl + cw] = img[it:it + ch, il:il + cw]
    mbox[ct:ct + ch, cl:cl + cw] = m[it:it + ch, il:il + cw]
    cropping[ct:ct + ch, cl:cl + cw] = True
    return box.transpose(2, 0, 1), ori_from_image(box).transpose(2, 0, 1), cropping, mbox


def get_data_from_chunk(decoded, maps, dim, kind, pyrandom, nprandom, map_fill=0):
    """v3 / v4 over decoded RGB uint8 arrays and uint8 maps: the per-chunk `scale` draw (:1260, never used), then per image the
    draws and the arithmetic above.  Returns a dict in the reference's layouts -- images (B,3,dim,dim) float32, ori_images
    (B,3,dim,dim) uint8, croppings (dim,dim,B) float64, target (B,dim,dim) float32 -- plus the geometry list."""
    nprandom.uniform(0.7, 1.3)
    lo_hi = long_range(dim, kind)
    images, oris, crops, targets, geoms = [], [], [], [], []
    for rgb, m in zip(decoded, maps):
        g = draw_geometry(rgb.shape[0], rgb.shape[1], dim, lo_hi, pyrandom, nprandom)
        a, o, c, t = seg_image(rgb, m, dim, g, map_fill)
        images.append(a)
        oris.append(o)
        crops.append(c.astype(np.float64))
        targets.append(t.astype(np.float32))
        geoms.append(g)
    return dict(images=np.stack(images), ori_images=np.stack(oris), croppings=np.stack(crops, axis=2), target=np.stack(targets),
                geoms=geoms)


def box_of(cropping):
    """(cont_top, cont_left, ch, cw) of a (dim, dim) cropping mask that is one filled rectangle."""
    ys, xs = np.nonzero(cropping)
    ct, cl, ch, cw = int(ys.min()), int(xs.min()), int(ys.max() - ys.min() + 1), int(xs.max() - xs.min() + 1)
    assert int(np.count_nonzero(cropping)) == ch * cw
    return ct, cl, ch, cw
