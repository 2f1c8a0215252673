"""Input pipeline of the ACR training / CAM steps on the device.

Counterpart of myTool.py:1158-1199 (`get_data_from_chunk_v2`) and :1364-1403 (`get_data_from_chunk_val`): the
reference decodes with cv2 on the training process's CPU and does resize / flip / normalise / crop in numpy float64,
one image at a time, synchronously; at >100 img/s/GPU that starves the device.  Here the host only decodes (any
decoder -- PIL is what this image has) and draws the geometry; ONE H2D copy of the packed uint8 pixels and ONE kernel
launch (`acr_preprocess_batch`, include/acr_hip.h) produce the (B,3,S,S) network input:

  random resize-long to [0.9*S, S/0.875]   (RandomResizeLong :995-1008; cv2.resize float-path bilinear)
  horizontal flip with probability 1/2     (flip :895-899)
  (x/255 - mean) / std                     (:1180-1182)
  zero-padded random crop to S x S         (RandomCrop :923-955)

and returns the same contract as the reference: images (B,3,S,S) + labels (B,C) from the `cls_labels.npy` dict
(voc12/make_cls_labels.py:18-22).  The draws follow the reference's order (np.random.uniform for the flip, then
random.randint / random.randrange) from SEEDABLE generators (the reference's are the unseeded globals, train_acr.py:23).
There is no CPU path: tensors land on the GPU through the HIP kernel or the call raises.

Segmentation training (myTool.py:1257-1310 `get_data_from_chunk_v4`: image + target map; :1202-1253 `_v3`: image + saliency map)
puts a single-channel uint8 map through the image's own resize (nearest) / flip / crop: `preprocess_seg_batch`, `SegTrainBatcher`
and `ChunkLoader.get_data_from_chunk_v4 / _v3` give images, the de-normalised uint8 `ori_images`, the `croppings` masks and the map
from ONE launch (`acr_preprocess_seg_batch`), on the device and shaped for `segloss.joint_loss`.

Affinity training (voc12/data.py:222-278 `VOC12AffDataset`: image + the two CRF score dumps) crops and flips the 2n score planes with
the image, pools them 8 x 8 and reduces them to the label grid the pair masks are cut from: `preprocess_aff_batch`, `AffTrainBatcher`
and `ChunkLoader.get_data_from_chunk_aff` give images (the existing `acr_preprocess_batch`) and that label (ONE launch of
`acr_aff_label_batch`), shaped for `affinity.aff_train_step`.  PSA's transform list puts torchvision's ColorJitter in front of all that,
on the PIL image: `ColorJitter` draws its parameters, `acr_color_jitter_batch` (include/acr_hip.h, "colour jitter") applies them to the
packed uint8 pixels on the device, between the H2D copy and `acr_preprocess_batch`, bit for bit what Pillow computes.
"""
import concurrent.futures
import ctypes
import os
import random as _pyrandom

import numpy as np
import torch

from . import _abi
from . import _args as A
from . import _lib as L

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

PRE_IMAGE = _abi.record_dtype("acr_pre_image")


def load_cls_labels(path, names, num_classes=20):
    """`cls_labels.npy`: pickled {image name: float32 (C,)} (voc12/make_cls_labels.py)."""
    d = np.load(path, allow_pickle=True).item()
    return torch.from_numpy(np.stack([np.asarray(d[n], dtype=np.float32) for n in names]))


def resize_long_target(h, w, target_long):
    """myTool.py:995-1005: the longer side becomes target_long, the other is rounded.  Returns (new_h, new_w)."""
    if w < h:
        return target_long, int(round(w * target_long / h))
    return int(round(h * target_long / w)), target_long


def random_crop_boxes(h, w, crop, rng):
    """myTool.py:923-948 -> (cont_top, cont_left, img_top, img_left, ch, cw); w is drawn before h, like the reference.
    ``rng``: a ``random.Random``."""
    ch, cw = min(crop, h), min(crop, w)
    w_space, h_space = w - crop, h - crop
    if w_space > 0:
        cont_left, img_left = 0, rng.randrange(w_space + 1)
    else:
        cont_left, img_left = rng.randrange(-w_space + 1), 0
    if h_space > 0:
        cont_top, img_top = 0, rng.randrange(h_space + 1)
    else:
        cont_top, img_top = rng.randrange(-h_space + 1), 0
    return cont_top, cont_left, img_top, img_left, ch, cw


def _check_images(who, images_uint8, records, S):
    """Everything the preprocess kernels trust about the images and their geometry records, judged on the host before any device
    is asked for: the kernels index the packed pixels by the table alone."""
    if len(images_uint8) == 0 or len(records) != len(images_uint8):
        raise ValueError("need one record per image (got %d images, %d records)" % (len(images_uint8), len(records)))
    if not 0 < int(S) <= 32768:
        raise ValueError("crop size %r outside 1..32768" % (S,))
    for i, (a, rec) in enumerate(zip(images_uint8, records)):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
            raise ValueError("image %d must be a (h, w, 3) uint8 RGB array, got %s %s" % (i, getattr(a, "dtype", type(a)), getattr(a, "shape", "")))
        ok = (rec["h"] == a.shape[0] and rec["w"] == a.shape[1] and rec["rh"] > 0 and rec["rw"] > 0
              and 0 <= rec["cont_top"] and rec["cont_top"] + rec["ch"] <= S and 0 <= rec["cont_left"] and rec["cont_left"] + rec["cw"] <= S
              and 0 <= rec["img_top"] and rec["img_top"] + rec["ch"] <= rec["rh"] and 0 <= rec["img_left"]
              and rec["img_left"] + rec["cw"] <= rec["rw"] and rec["ch"] >= 0 and rec["cw"] >= 0 and rec["flip"] in (0, 1)
              and 2 * int(rec["rh"]) * int(rec["h"]) < 2 ** 31 and 2 * int(rec["rw"]) * int(rec["w"]) < 2 ** 31)     # the kernel's int32 sample positions
        if not ok:
            raise L.AcrHipError("%s: inconsistent geometry record %s for a %s image" % (who, rec, a.shape))


def _upload_packed(arrays, device):
    """The uint8 arrays back to back, each at a 16-byte aligned offset of ONE pinned staging buffer, and its one H2D copy.
    Returns (offsets, staging buffer, device buffer); the staging buffer must outlive the asynchronous copy."""
    sizes = [int(a.size) for a in arrays]
    offs = np.concatenate([[0], np.cumsum([(s + 15) // 16 * 16 for s in sizes])])
    stage = torch.empty(int(offs[-1]), dtype=torch.uint8).pin_memory()
    sn = stage.numpy()
    for a, o, s in zip(arrays, offs[:-1], sizes):
        sn[o:o + s] = np.ascontiguousarray(a).reshape(-1)
    return offs[:-1], stage, stage.to(device, non_blocking=True)


def table_bytes(records, offsets, extra=()):
    """The bytes of the record table with its ``offset`` column filled in and, right behind it, the int64 values ``extra``."""
    table = np.zeros(len(records), PRE_IMAGE)              # not records.copy(): a structured copy leaves the struct's padding unset
    table[:] = records
    table["offset"] = offsets
    return np.concatenate([table.view(np.uint8), np.asarray(extra, dtype=np.int64).view(np.uint8)])


def _upload_table(records, offsets, device, extra=()):
    """``table_bytes`` on the device: one pinned buffer (a pageable source would make the "asynchronous" copy drain the stream on
    the host), one copy."""
    raw = table_bytes(records, offsets, extra)
    table_host = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
    table_host.numpy()[:] = raw
    return table_host.to(device, non_blocking=True)


# ------------------------------------------------------------------------------------------------------------------
# Colour jitter on the packed uint8 batch (PSA's transform list in front of VOC12AffDataset, voc12/data.py:241-278)
# ------------------------------------------------------------------------------------------------------------------
JITTER_OPS = ("brightness", "contrast", "saturation", "hue")      # the operation codes ACR_JITTER_* of the header, in order
assert [_abi.constants["ACR_JITTER_" + k.upper()] for k in JITTER_OPS] == [0, 1, 2, 3] and _abi.constants["ACR_JITTER_NONE"] == -1


def _jitter_range(name, value):
    """torchvision's ``ColorJitter._check_input``: a number v is [max(0, 1 - v), 1 + v] ([-v, v] for the hue), a pair is the range
    itself; the hue lies within [-0.5, 0.5], the others are >= 0.  None for a range that disables the operation."""
    hue = name == "hue"
    center, lo_bound, hi_bound = (0.0, -0.5, 0.5) if hue else (1.0, 0.0, float("inf"))
    if isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool):
        v = float(value)
        if not 0 <= v < float("inf"):
            raise ValueError("%s=%r: a single number must be finite and non-negative" % (name, value))
        lo, hi = center - v, center + v
        if not hue:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        lo, hi = float(value[0]), float(value[1])
    else:
        raise ValueError("%s=%r must be a number or a (min, max) pair" % (name, value))
    if not lo_bound <= lo <= hi <= hi_bound or hi == float("inf"):
        raise ValueError("%s range (%r, %r) must be ordered and lie within [%s, %s]" % (name, lo, hi, lo_bound, hi_bound))
    return None if lo == hi == center else (lo, hi)


class ColorJitter:
    """torchvision's ``ColorJitter(brightness, contrast, saturation, hue)`` as a drawer of parameters; PSA's affinity stage uses
    (0.3, 0.3, 0.3, 0.1).  It owns its OWN ``np.random.RandomState(seed)``, so a batcher's geometry for a given seed is the same with
    and without jitter.  The stream is this project's: torchvision draws from torch's global generator (``randperm(4)``, then
    ``Tensor.uniform_``), and no parity of streams is claimed -- only the ranges, the order of the draws and what the drawn
    parameters do to the pixels (include/acr_hip.h, "colour jitter") are torchvision's."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, seed=None):
        self.ranges = tuple(_jitter_range(k, v) for k, v in zip(JITTER_OPS, (brightness, contrast, saturation, hue)))
        self.nprandom = np.random.RandomState(seed)

    def draw(self):
        """One image's parameters ``(order, b, c, s, hue_factor)``: ``permutation(4)``, then one ``uniform(lo, hi)`` per enabled
        operation in the order b, c, s, h; None for a disabled one, which draws nothing."""
        order = tuple(int(k) for k in self.nprandom.permutation(4))
        return (order,) + tuple(None if r is None else float(self.nprandom.uniform(r[0], r[1])) for r in self.ranges)


def jitter_tables(params, n_images):
    """The per-image tables of ``acr_color_jitter_batch`` from one ``(order, b, c, s, hue_factor)`` per image, judged on the host:
    -> (order (B, 4) int32, slot 0 first and ACR_JITTER_NONE behind the enabled ones; factors (B, 3) float32; hue_shift (B) int32).
    A factor of None disables its operation.  ``order`` is a permutation of the enabled operations' codes or of all four (the
    disabled ones are then skipped)."""
    if params is None or len(params) != n_images or n_images == 0:
        raise ValueError("need one set of jitter parameters per image (got %d images, %s sets)" % (n_images, "no" if params is None else len(params)))
    order, factors, shift = np.full((n_images, 4), -1, np.int32), np.zeros((n_images, 3), np.float32), np.zeros(n_images, np.int32)
    for i, p in enumerate(params):
        if not isinstance(p, (tuple, list)) or len(p) != 5:
            raise ValueError("jitter parameters %d must be (order, brightness, contrast, saturation, hue), got %r" % (i, p))
        enabled = [k for k in range(4) if p[1 + k] is not None]
        try:
            codes = [int(k) for k in p[0]]
        except (TypeError, ValueError):
            raise ValueError("jitter parameters %d: order %r is not a sequence of operation codes" % (i, p[0])) from None
        if sorted(codes) != enabled and sorted(codes) != [0, 1, 2, 3]:
            raise ValueError("jitter parameters %d: order %r is no permutation of the enabled operations %s" % (i, p[0], enabled))
        for k in enabled:
            v = float(p[1 + k])
            lo, hi = (-0.5, 0.5) if k == 3 else (0.0, float(np.finfo(np.float32).max))
            if not lo <= v <= hi:                           # a NaN fails too
                raise ValueError("jitter parameters %d: %s factor %r outside [%s, %s]" % (i, JITTER_OPS[k], p[1 + k], lo, hi))
            if k == 3:
                shift[i] = int(v * 255) % 256               # trunc(hue_factor * 255) mod 256: -0.05 -> 244
            else:
                factors[i, k] = v                           # Pillow narrows the Python float to a C float
        codes = [k for k in codes if k in enabled]
        order[i, :len(codes)] = codes
    return order, factors, shift


def _check_jitter_images(images_uint8):
    if len(images_uint8) == 0:
        raise ValueError("need at least one image")
    for i, a in enumerate(images_uint8):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
            raise ValueError("image %d must be a (h, w, 3) uint8 RGB array, got %s %s" % (i, getattr(a, "dtype", type(a)), getattr(a, "shape", "")))


def color_jitter_launch(packed, offsets, shapes, tables):
    """Run acr_color_jitter_batch IN PLACE on ``packed``, a uint8 device buffer (16-byte aligned) that holds image b, ``shapes[b]`` =
    (h, w) and h w 3 bytes, at the byte offset ``offsets[b]`` (a multiple of 16: what ``_upload_packed`` produces).  ``tables``: what
    ``jitter_tables`` returned.  The five per-image arrays go up in one pinned copy; the mean pass and its workspace are left out
    when no image has contrast.  The callers have validated images and parameters.  Returns what must outlive the launches."""
    order, factors, shift = tables
    B, device = len(shapes), packed.device
    hw = np.asarray([(int(h), int(w)) for h, w in shapes], np.int32).reshape(B, 2)
    raw = np.concatenate([np.asarray(offsets, np.int64).view(np.uint8), hw.view(np.uint8).reshape(-1), order.view(np.uint8).reshape(-1),
                          factors.view(np.uint8).reshape(-1), shift.view(np.uint8)])
    host = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = raw
    table = host.to(device, non_blocking=True)
    with torch.cuda.device(device):
        ws = L.workspace("acr_color_jitter_ws_bytes", B, device=device)[0] if bool((order == 1).any()) else None
        L.check(L.load().acr_color_jitter_batch(L.ptr(packed), L.ptr(table), L.ptr(table[8 * B:]), L.ptr(table[16 * B:]), L.ptr(table[32 * B:]),
                                                L.ptr(table[44 * B:]), B, L.ptr(ws), L.stream_ptr()), "acr_color_jitter_batch")
    return host, table, ws


def color_jitter_batch(images_uint8, params, device="cuda"):
    """The colour jitter alone: ``images_uint8`` = list of (h, w, 3) uint8 RGB arrays, ``params`` = one ``(order, b, c, s,
    hue_factor)`` per image (``ColorJitter.draw``) -> the list of jittered (h, w, 3) uint8 arrays, on the host again.  One H2D copy
    of the packed pixels, the two launches of ``acr_color_jitter_batch``, one copy back."""
    _check_jitter_images(images_uint8)
    tables = jitter_tables(params, len(images_uint8))
    device = A.gpu_device(device, "acr_color_jitter_batch")
    offs, stage, packed = _upload_packed(images_uint8, device)
    keep = color_jitter_launch(packed, offs, [a.shape[:2] for a in images_uint8], tables)
    out = packed.cpu().numpy()                              # synchronises: stage and keep have done their work
    del keep, stage
    return [out[o:o + a.size].reshape(a.shape).copy() for o, a in zip(offs, images_uint8)]


def preprocess_batch(images_uint8, records, S, device, dtype=torch.float32, jitter=None):
    """Run acr_preprocess_batch: ``images_uint8`` = list of (h,w,3) uint8 RGB arrays, ``records`` = PRE_IMAGE array with
    everything but ``offset`` filled in.  One pinned staging buffer, one H2D copy, one launch.  ``jitter``: one ``(order, b, c, s,
    hue_factor)`` per image (``ColorJitter.draw``); the colour jitter then runs on the packed uint8 pixels on the device
    (``acr_color_jitter_batch``) between the copy and the launch.  With None nothing of it is called."""
    _check_images("acr_preprocess_batch", images_uint8, records, S)
    tables = None if jitter is None else jitter_tables(jitter, len(images_uint8))
    device = A.gpu_device(device, "acr_preprocess_batch")
    offs, stage, packed = _upload_packed(images_uint8, device)
    keep = () if tables is None else color_jitter_launch(packed, offs, [a.shape[:2] for a in images_uint8], tables)
    table = _upload_table(records, offs, device)
    out = torch.empty((len(images_uint8), 3, S, S), dtype=dtype, device=device)
    mean = (ctypes.c_float * 3)(*MEAN)
    std = (ctypes.c_float * 3)(*STD)
    with torch.cuda.device(device):
        L.check(L.load().acr_preprocess_batch(L.ptr(packed), L.ptr(table), len(images_uint8), S, mean, std, L.dtype_code(dtype)
                                              if dtype != torch.bfloat16 else L.ACR_BF16, L.ptr(out), L.stream_ptr()),
                "acr_preprocess_batch")
    # the staging buffer and the table must outlive the asynchronous copies: tie them to the output
    out._acr_keep = (stage, packed, table) + tuple(keep)
    return out


class TrainBatcher:
    """get_data_from_chunk_v2 for a chunk of decoded images.  ``seed`` seeds both generators the reference draws from."""

    def __init__(self, crop_size, device="cuda", seed=None, dtype=torch.float32):
        self.S = crop_size
        self.device = torch.device(device)
        self.dtype = dtype
        self.pyrandom = _pyrandom.Random(seed)
        self.nprandom = np.random.RandomState(seed)

    def draw(self, h, w):
        """The per-image draws in the reference's order: flip_p (:1175), target_long (:996), crop boxes (:935-945)."""
        S = self.S
        flip_p = self.nprandom.uniform(0, 1)
        target_long = self.pyrandom.randint(int(S * 0.9), int(S / 0.875))
        nh, nw = resize_long_target(h, w, target_long)
        ct, cl, it, il, ch, cw = random_crop_boxes(nh, nw, S, self.pyrandom)
        return (0, h, w, nh, nw, int(flip_p > 0.5), ct, cl, it, il, ch, cw)

    def __call__(self, images_uint8, labels):
        """images_uint8: list of (h,w,3) uint8 RGB arrays; labels: (B,C) tensor.  Returns (img, label) on the device."""
        self.nprandom.uniform(0.7, 1.3)                     # myTool.py:1161: `scale`, drawn once per chunk and never used
        rec = np.zeros(len(images_uint8), PRE_IMAGE)
        for i, a in enumerate(images_uint8):
            rec[i] = self.draw(int(a.shape[0]), int(a.shape[1]))
        self.last_records = rec
        return preprocess_batch(images_uint8, rec, self.S, self.device, self.dtype), labels.to(self.device, non_blocking=True)


def val_batch(images_uint8, crop_size, device="cuda", dtype=torch.float32):
    """myTool.py:1364-1403: plain resize to crop x crop + normalise (no augmentation)."""
    S = crop_size
    rec = np.zeros(len(images_uint8), PRE_IMAGE)
    for i, a in enumerate(images_uint8):
        rec[i] = (0, int(a.shape[0]), int(a.shape[1]), S, S, 0, 0, 0, 0, 0, S, S)
    return preprocess_batch(images_uint8, rec, S, device, dtype)


# ------------------------------------------------------------------------------------------------------------------
# Segmentation training: image + companion map through one geometry (myTool.py:1202-1253 v3, :1257-1310 v4)
# ------------------------------------------------------------------------------------------------------------------
def _check_seg_inputs(images_uint8, maps_uint8, records, S):
    """Everything acr_preprocess_seg_batch trusts, judged on the host before any device is asked for."""
    if len(images_uint8) != len(maps_uint8):
        raise ValueError("need one map per image (got %d images, %d maps)" % (len(images_uint8), len(maps_uint8)))
    _check_images("acr_preprocess_seg_batch", images_uint8, records, S)
    for i, (a, m) in enumerate(zip(images_uint8, maps_uint8)):
        if not isinstance(m, np.ndarray) or m.dtype != np.uint8:
            raise ValueError("map %d must be a uint8 array, got %s" % (i, getattr(m, "dtype", type(m))))
        if m.ndim != 2:
            raise ValueError("map %d must be 2-D (h, w), got shape %s" % (i, m.shape))
        if m.shape != a.shape[:2]:
            raise ValueError("map %d is %s, its image %s" % (i, m.shape, a.shape[:2]))


def preprocess_seg_batch(images_uint8, maps_uint8, records, S, device, dtype=torch.float32, map_fill=0, with_ori=True, *,
                         with_croppings=True, with_map=True):
    """Run acr_preprocess_seg_batch (include/acr_hip.h): ``images_uint8`` = list of (h,w,3) uint8 RGB arrays, ``maps_uint8`` = list of
    (h,w) uint8 maps, one per image and of its size, ``records`` = PRE_IMAGE array with everything but ``offset`` filled in.  Images
    and maps share one pinned staging buffer: one H2D copy, one launch.  Returns device tensors
    ``(images (B,3,S,S) dtype, ori_images (B,3,S,S) uint8, croppings (B,S,S) float32, maps (B,S,S) uint8)``; an output that was not
    asked for is None.  ``map_fill`` is what the map holds outside the crop box: 0 as in the reference (myTool.py:982), or 255 (this
    project's extension) so that a cross-entropy with ignore skips the padding."""
    _check_seg_inputs(images_uint8, maps_uint8, records, S)
    if not 0 <= int(map_fill) <= 255:
        raise ValueError("map_fill=%r outside 0..255" % (map_fill,))
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("dtype must be float32 or bfloat16, got %s" % (dtype,))
    device = A.gpu_device(device, "acr_preprocess_seg_batch")
    B = len(images_uint8)
    offs, stage, packed = _upload_packed(list(images_uint8) + list(maps_uint8), device)      # images and maps share the buffer
    table = _upload_table(records, offs[:B], device, extra=offs[B:])                        # ... and the map offsets the table's
    map_offs = table[B * PRE_IMAGE.itemsize:]
    images = torch.empty((B, 3, S, S), dtype=dtype, device=device)
    ori = torch.empty((B, 3, S, S), dtype=torch.uint8, device=device) if with_ori else None
    crop = torch.empty((B, S, S), dtype=torch.float32, device=device) if with_croppings else None
    maps = torch.empty((B, S, S), dtype=torch.uint8, device=device) if with_map else None
    mean = (ctypes.c_float * 3)(*MEAN)
    std = (ctypes.c_float * 3)(*STD)
    with torch.cuda.device(device):
        L.check(L.load().acr_preprocess_seg_batch(L.ptr(packed), L.ptr(table), L.ptr(map_offs), B, S, mean, std,
                                                  L.ACR_BF16 if dtype == torch.bfloat16 else L.ACR_F32, int(map_fill), L.ptr(images),
                                                  L.ptr(ori), L.ptr(crop), L.ptr(maps), L.stream_ptr()), "acr_preprocess_seg_batch")
    images._acr_keep = (stage, packed, table)               # the staging buffers must outlive the asynchronous copies
    return images, ori, crop, maps


class SegTrainBatcher(TrainBatcher):
    """get_data_from_chunk_v4 / _v3 (myTool.py:1257-1310, :1202-1253) for a chunk of decoded images and their maps.  The draws
    follow the reference's order: per chunk the unused ``scale`` (:1260), then per image flip_p (:1275), ``randint(lo, hi)`` of
    RandomResizeLong2 (:1011) and the RandomCrop2 draws, w before h (:967-979).  ``long_range`` = (lo, hi): None means (S, S), which is
    v4 (:1284; ``randint(S, S)`` still consumes a draw); v3 uses ``(int(0.9 * S), int(S / 0.875))`` (:1228).  ``map_fill``: see
    ``preprocess_seg_batch``."""

    def __init__(self, crop_size, device="cuda", seed=None, dtype=torch.float32, long_range=None, map_fill=0):
        super().__init__(crop_size, device, seed, dtype)
        lo, hi = (crop_size, crop_size) if long_range is None else (int(long_range[0]), int(long_range[1]))
        if not 0 < lo <= hi:
            raise ValueError("long_range %r must be 0 < lo <= hi" % (long_range,))
        self.long_range, self.map_fill = (lo, hi), map_fill

    def draw(self, h, w):
        flip_p = self.nprandom.uniform(0, 1)
        target_long = self.pyrandom.randint(*self.long_range)
        nh, nw = resize_long_target(h, w, target_long)
        ct, cl, it, il, ch, cw = random_crop_boxes(nh, nw, self.S, self.pyrandom)
        return (0, h, w, nh, nw, int(flip_p > 0.5), ct, cl, it, il, ch, cw)

    def __call__(self, images_uint8, maps_uint8, labels, with_ori=True):
        """images_uint8: list of (h,w,3) uint8 RGB arrays; maps_uint8: list of (h,w) uint8 maps; labels: (B,C) tensor.  Returns
        ``(images, ori_images, labels, croppings, target)`` on the device, shaped for ``segloss.joint_loss``: ori_images (B,3,S,S)
        uint8, croppings the (S,S,B) view of a contiguous (B,S,S) float32 buffer (the reference's layout, :1267; joint_loss permutes
        it back without a copy), target (B,S,S) uint8 (the reference returns float: ``target.float()`` gives that)."""
        for a, m in zip(images_uint8, maps_uint8):           # before any draw: a refused chunk leaves the generators alone
            if getattr(a, "ndim", 0) != 3 or getattr(m, "shape", None) != a.shape[:2]:
                raise ValueError("every map must be (h, w) like its (h, w, 3) image, got %s for %s" % (getattr(m, "shape", None), getattr(a, "shape", None)))
        self.nprandom.uniform(0.7, 1.3)                     # :1260 / :1205: `scale`, drawn once per chunk and never used
        rec = np.zeros(len(images_uint8), PRE_IMAGE)
        for i, a in enumerate(images_uint8):
            rec[i] = self.draw(int(a.shape[0]), int(a.shape[1]))
        self.last_records = rec
        images, ori, crop, target = preprocess_seg_batch(images_uint8, maps_uint8, rec, self.S, self.device, self.dtype, self.map_fill, with_ori)
        return images, ori, labels.to(self.device, non_blocking=True), crop.permute(1, 2, 0), target


# ------------------------------------------------------------------------------------------------------------------
# Affinity-stage training input: image + the label grid cut from the two CRF score dumps (voc12/data.py:241-278)
# ------------------------------------------------------------------------------------------------------------------
AFF_MIN_PLANES, AFF_MAX_PLANES = 2, 81


def score_planes(s, who="scores"):
    """One score dump as ``acr_aff_label_batch`` takes it: a {key: (h, w) float32} dict (what ``infer_cam_list(out_crf=...)`` writes:
    key 0 the background, then class + 1) or an (n, h, w) float32 stack -> (keys or None, (n, h, w) float32 C-contiguous numpy array,
    the planes in the dict's own order).  Raises ValueError for anything else: nothing is cast."""
    if isinstance(s, dict):
        keys, planes = list(s.keys()), [np.asarray(v) for v in s.values()]
        if len(planes) < AFF_MIN_PLANES:
            raise ValueError("%s: %d planes, need at least %d (background and one class)" % (who, len(planes), AFF_MIN_PLANES))
        for k, p in zip(keys, planes):
            if p.dtype != np.float32 or p.ndim != 2:
                raise ValueError("%s[%r] must be a (h, w) float32 array, got %s %s" % (who, k, p.dtype, p.shape))
            if p.shape != planes[0].shape:
                raise ValueError("%s[%r] is %s, the first plane %s" % (who, k, p.shape, planes[0].shape))
        a = np.stack(planes)
    else:
        keys, a = None, np.asarray(s)
        if a.dtype != np.float32:
            raise ValueError("%s must be float32, got %s" % (who, a.dtype))
        if a.ndim != 3:
            raise ValueError("%s must be an (n, h, w) stack or a {key: (h, w)} dict, got shape %s" % (who, a.shape))
    if not AFF_MIN_PLANES <= a.shape[0] <= AFF_MAX_PLANES or a.size == 0:
        raise ValueError("%s: %d planes of %s outside %d..%d non-empty planes" % (who, a.shape[0], a.shape[1:], AFF_MIN_PLANES, AFF_MAX_PLANES))
    return keys, np.ascontiguousarray(a)


def score_pair(la, ha, hw=None, who="scores"):
    """The low- and the high-alpha dump of one image -> their two (n, h, w) float32 stacks, after the checks the kernel relies on: the
    same keys in the same order, the same n, and planes of ``hw`` (the image's size) where that is given."""
    kl, a = score_planes(la, who + " la")
    kh, b = score_planes(ha, who + " ha")
    if (kl is not None and kh is not None and kl != kh) or a.shape != b.shape:
        raise ValueError("%s: the low-alpha dump (keys %s, %s) and the high-alpha dump (keys %s, %s) differ" % (who, kl, a.shape, kh, b.shape))
    if hw is not None and tuple(a.shape[1:]) != tuple(hw):
        raise ValueError("%s: planes of %s for an image of %s" % (who, a.shape[1:], tuple(hw)))
    return a, b


def aff_record(h, w, S, cont_top, cont_left, img_top, img_left, ch, cw, flip):
    """The PRE_IMAGE record (no resize) of the reference's joint crop-THEN-flip: the box is the one ``get_random_crop_box``
    (tool/imutils.py:167-190; ``random_crop_boxes`` here) draws on the unflipped image, the flip is ``np.fliplr`` of the S-wide
    container.  The record describes flip-then-crop, so a flip mirrors the box: cont_left' = S - cont_left - cw,
    img_left' = w - img_left - cw."""
    if flip:
        cont_left, img_left = S - cont_left - cw, w - img_left - cw
    return (0, h, w, h, w, int(bool(flip)), cont_top, cont_left, img_top, img_left, ch, cw)


def _check_aff_records(records, shapes, SH, SW):
    """What acr_aff_label_batch trusts about its table: one record per image, no resize, both boxes inside image and container."""
    if len(records) != len(shapes) or len(shapes) == 0:
        raise ValueError("need one record per image (got %d score pairs, %d records)" % (len(shapes), len(records)))
    if SH <= 0 or SW <= 0 or SH % 8 or SW % 8 or SH > 32768 or SW > 32768:
        raise ValueError("container %r x %r must be multiples of 8 up to 32768" % (SH, SW))
    for rec, (h, w) in zip(records, shapes):
        ok = (rec["h"] == h and rec["w"] == w and rec["rh"] == h and rec["rw"] == w and rec["flip"] in (0, 1) and rec["ch"] >= 0 and rec["cw"] >= 0
              and 0 <= rec["cont_top"] and rec["cont_top"] + rec["ch"] <= SH and 0 <= rec["cont_left"] and rec["cont_left"] + rec["cw"] <= SW
              and 0 <= rec["img_top"] and rec["img_top"] + rec["ch"] <= h and 0 <= rec["img_left"] and rec["img_left"] + rec["cw"] <= w)
        if not ok:
            raise L.AcrHipError("acr_aff_label_batch: inconsistent geometry record %s for planes of %s in a %d x %d container" % (rec, (h, w), SH, SW))


def aff_label_launch(scores, records, la_off, ha_off, n_planes, SH, SW):
    """Run acr_aff_label_batch on ``scores``, a device buffer that holds every image's two stacks at the byte offsets ``la_off`` /
    ``ha_off``: the table, the offsets and the plane counts go up in one pinned copy, one launch writes the (B, SH / 8, SW / 8) uint8
    label.  The callers have validated records and offsets (``_check_aff_records``, ``score_pair``)."""
    B, device = len(records), scores.device
    n32 = np.zeros(B + (B & 1), "<i4")                      # int32 counts, padded to whole int64 words of the table's tail
    n32[:B] = n_planes
    tail = np.concatenate([np.asarray(la_off, np.int64), np.asarray(ha_off, np.int64), n32.view(np.int64)])
    table = _upload_table(records, np.zeros(B, np.int64), device, extra=tail)
    base = B * PRE_IMAGE.itemsize
    label = torch.empty((B, SH // 8, SW // 8), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        L.check(L.load().acr_aff_label_batch(L.ptr(scores), L.ptr(table), L.ptr(table[base:]), L.ptr(table[base + 8 * B:]),
                                             L.ptr(table[base + 16 * B:]), B, SH, SW, L.ptr(label), L.stream_ptr()), "acr_aff_label_batch")
    label._acr_keep = (scores, table)
    return label


def preprocess_aff_batch(images_uint8, la, ha, records, S, device, dtype=torch.float32, jitter=None):
    """The affinity stage's batch under given geometry records (PRE_IMAGE, no resize: rh = h, rw = w; ``aff_record`` writes them):
    ``images_uint8`` = list of (h, w, 3) uint8 RGB arrays, ``la`` / ``ha`` = per image the low- / high-alpha score dict or (n, h, w)
    float32 stack.  Images go through the existing ``preprocess_batch`` (an identity resize has integer sample positions and weights
    0 / 1, hence exact values; the zero padding after the normalisation is the recipe's fill), all scores through ONE pinned
    staging buffer, one H2D copy and one ``acr_aff_label_batch`` launch (include/acr_hip.h, "affinity-stage input").  Returns
    ``(images (B, 3, S, S), label (B, S / 8, S / 8) uint8)`` on the device; ``label`` is a stride-1 grid for ``affinity.pair_codes``.
    ``jitter``: per image the colour-jitter parameters ``preprocess_batch`` takes; they change the image alone, never the label.
    Everything is validated on the host before any device is asked for."""
    if not (len(images_uint8) == len(la) == len(ha)):
        raise ValueError("need one low- and one high-alpha dump per image (got %d images, %d, %d)" % (len(images_uint8), len(la), len(ha)))
    if int(S) <= 0 or int(S) % 32:
        raise ValueError("crop size %r must be a positive multiple of 32" % (S,))
    _check_images("acr_aff_label_batch", images_uint8, records, S)
    stacks = [score_pair(l, h, a.shape[:2], "image %d" % i) for i, (a, l, h) in enumerate(zip(images_uint8, la, ha))]
    _check_aff_records(records, [a.shape[:2] for a in images_uint8], S, S)
    if jitter is not None:
        jitter_tables(jitter, len(images_uint8))
    device = A.gpu_device(device, "acr_aff_label_batch")
    images = preprocess_batch(images_uint8, records, S, device, dtype, jitter)
    flat = [s.view(np.uint8).reshape(-1) for pair in stacks for s in pair]
    offs, stage, packed = _upload_packed(flat, device)
    label = aff_label_launch(packed, records, offs[0::2], offs[1::2], [p[0].shape[0] for p in stacks], S, S)
    label._acr_keep += (stage,)                             # the staging buffer must outlive the asynchronous copy
    return images, label


class AffTrainBatcher(TrainBatcher):
    """``VOC12AffDataset.__getitem__`` (voc12/data.py:241-278) under PSA's transforms -- joint RandomCrop(S) and RandomHorizontalFlip,
    Normalize + HWC_to_CHW on the image, AvgPool2d(8) on the scores -- for a chunk of decoded images and their two score dumps.
    Flip and box are drawn as ``TrainBatcher`` draws them, without its resize draw: per image ``uniform(0, 1) > 0.5`` from the numpy
    generator, then ``random_crop_boxes`` (w before h) from Python's; the box is mirrored where a flip was drawn (``aff_record``).
    ``color_jitter``: a ``ColorJitter``, PSA's first transform; its parameters are drawn per image from ITS generator, so the geometry
    of a seed does not depend on it."""

    def __init__(self, crop_size, device="cuda", seed=None, dtype=torch.float32, color_jitter=None):
        super().__init__(crop_size, device, seed, dtype)
        if color_jitter is not None and not isinstance(color_jitter, ColorJitter):
            raise ValueError("color_jitter must be a data.ColorJitter or None, got %s" % type(color_jitter).__name__)
        self.color_jitter, self.last_jitter = color_jitter, None

    def draw(self, h, w):
        flip_p = self.nprandom.uniform(0, 1)
        return aff_record(h, w, self.S, *random_crop_boxes(h, w, self.S, self.pyrandom), flip_p > 0.5)

    def __call__(self, images_uint8, la, ha, records=None, jitter=None):
        """images_uint8: list of (h, w, 3) uint8 RGB arrays; la, ha: per image the low- / high-alpha {key: (h, w)} dict or (n, h, w)
        float32 stack.  ``records``: a PRE_IMAGE array to replay instead of drawing; ``jitter``: per image the colour-jitter parameters
        to replay instead of drawing (``last_jitter`` of an earlier call).  Returns (images (B, 3, S, S), label (B, S / 8, S / 8) uint8)
        on the device."""
        if jitter is not None and len(jitter) != len(images_uint8):      # before any draw: a refused chunk leaves the generators alone
            raise ValueError("need one set of jitter parameters per image (got %d images, %d sets)" % (len(images_uint8), len(jitter)))
        if records is None:
            for a in images_uint8:
                if getattr(a, "ndim", 0) != 3:
                    raise ValueError("every image must be a (h, w, 3) array, got %s" % (getattr(a, "shape", None),))
            records = np.zeros(len(images_uint8), PRE_IMAGE)
            for i, a in enumerate(images_uint8):
                records[i] = self.draw(int(a.shape[0]), int(a.shape[1]))
        if jitter is None and self.color_jitter is not None:
            jitter = [self.color_jitter.draw() for _ in images_uint8]
        self.last_records, self.last_jitter = records, jitter
        return preprocess_aff_batch(images_uint8, la, ha, records, self.S, self.device, self.dtype, jitter)


# ------------------------------------------------------------------------------------------------------------------
# The reference's own call contract: names in, tensors out (myTool.py:1158-1199, :1364-1403)
# ------------------------------------------------------------------------------------------------------------------
def decode_rgb(path):
    """One image file -> (h, w, 3) uint8 RGB (what cv2.imread + cvtColor(BGR2RGB) hand to the reference, :1176-1177).  PIL
    is the decoder this image ships (cv2 is absent); it releases the GIL while it decodes, so a thread pool scales."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def decode_map(path):
    """One single-channel map file -> (h, w) uint8 (myTool.py:1224-1225, :1279-1280: ``np.asarray(PIL.Image.open(path))``).  A palette
    PNG yields its indices, which is what ``pseudo.save_label_png`` writes."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im)


def load_score_dump(path):
    """One ``<out_crf>_<alpha>/<name>.npy`` file -> its {key: (h, w) float32} dict (voc12/data.py:248-249)."""
    return np.load(path, allow_pickle=True).item()


class ChunkLoader:
    """`get_data_from_chunk_v2(chunk, args)` / `get_data_from_chunk_val(chunk, args)` for a training process that must not
    wait for its input: files are read and decoded by a small thread pool, geometry is drawn on the host in the reference's
    RNG order, and ONE pinned H2D copy + ONE `acr_preprocess_batch` launch build the (B,3,S,S) batch on the GPU.

        loader = ChunkLoader(img_dir, cls_labels, crop_size, device="cuda", seed=None, workers=8)
        images, ori_images, labels, names = loader.get_data_from_chunk_v2(chunk)        # one chunk, synchronous decode
        for images, ori_images, labels, names in loader.iterate(chunks, train=True):    # decode of chunk i+1 overlaps step i

    `cls_labels`: the `voc12/cls_labels.npy` dict {name: float32 (C,)} (myTool.py:916-920) or its path.  `ori_images`
    (de-normalised uint8 crops, :1186-1190, which no caller of the training loop reads) is None unless `with_ori=True`.

    With `map_dir` (and `map_ext`, default ".png") the loader also serves segmentation training:
        images, ori_images, labels, croppings, names, target = loader.get_data_from_chunk_v4(chunk)    # or _v3: saliency maps
        for batch in loader.iterate(chunks, kind="v4"): ...
    where the map of image <name> is <map_dir>/<name><map_ext> and `map_fill` is what the map holds outside the crop box.

    With `la_dir` and `ha_dir` (the ``<out_crf>_<low_alpha>`` / ``<out_crf>_<high_alpha>`` folders ``infer_cam_list`` writes) it serves
    the affinity stage (voc12/data.py:222-278 VOC12AffDataset; `cls_labels` is not read on this path):
        images, label, names = loader.get_data_from_chunk_aff(chunk)
        for images, label, names in loader.iterate(chunks, kind="aff"): ...
    and `color_jitter` (a ``ColorJitter``; PSA's is ``ColorJitter(0.3, 0.3, 0.3, 0.1)``) is applied to that stage's images, on the
    device; the other loaders' recipes have none."""

    def __init__(self, img_dir, cls_labels, crop_size, device="cuda", seed=None, workers=8, dtype=torch.float32, ext=".jpg",
                 with_ori=False, map_dir=None, map_ext=".png", map_fill=0, la_dir=None, ha_dir=None, color_jitter=None):
        self.img_dir, self.S, self.ext, self.with_ori = img_dir, crop_size, ext, with_ori
        self.map_dir, self.map_ext, self.map_fill = map_dir, map_ext, map_fill
        self.la_dir, self.ha_dir, self._aff = la_dir, ha_dir, None
        if color_jitter is not None and not isinstance(color_jitter, ColorJitter):
            raise ValueError("color_jitter must be a data.ColorJitter or None, got %s" % type(color_jitter).__name__)
        self.color_jitter = color_jitter
        self._seg_batchers = {}
        self.device, self.dtype = torch.device(device), dtype
        if isinstance(cls_labels, (str, os.PathLike)):
            cls_labels = np.load(cls_labels, allow_pickle=True).item()
        self.cls_labels = cls_labels
        self.batcher = TrainBatcher(crop_size, device, seed, dtype)
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, workers), thread_name_prefix="acr-decode")

    def close(self):
        self.pool.shutdown(wait=True)

    def _submit(self, chunk):
        return [self.pool.submit(decode_rgb, os.path.join(self.img_dir, name + self.ext)) for name in chunk]

    def _labels(self, chunk):
        return torch.from_numpy(np.stack([np.asarray(self.cls_labels[n], dtype=np.float32) for n in chunk]))

    def _ori(self, images):
        if not self.with_ori:
            return None
        mean = torch.tensor(MEAN, device=images.device).view(1, 3, 1, 1)
        std = torch.tensor(STD, device=images.device).view(1, 3, 1, 1)
        return ((images.float() * std + mean) * 255.0).clamp(0, 255).to(torch.uint8).cpu().numpy()     # :1186-1190 (astype truncates)

    def _finish(self, chunk, futures, train):
        decoded = [f.result() for f in futures]
        labels = self._labels(chunk)
        if train:
            images, labels = self.batcher(decoded, labels)
        else:
            self.batcher.nprandom.uniform(0.7, 1.3)         # :1367: the val function draws `scale` too
            images, labels = val_batch(decoded, self.S, self.device, self.dtype), labels.to(self.device, non_blocking=True)
        return images, self._ori(images), labels, list(chunk)

    def get_data_from_chunk_v2(self, chunk):
        """myTool.py:1158-1199 -> (images (B,3,S,S) on the device, ori_images, labels (B,C), name_list)."""
        return self._finish(chunk, self._submit(chunk), True)

    def get_data_from_chunk_val(self, chunk):
        """myTool.py:1364-1403: plain resize to S x S + normalise."""
        return self._finish(chunk, self._submit(chunk), False)

    # ---- segmentation training: image + map (myTool.py:1257-1310 v4, :1202-1253 v3) ----
    def _seg_batcher(self, kind):
        """One SegTrainBatcher per kind, all drawing from this loader's two generators (the reference's are the process globals)."""
        if kind not in ("v3", "v4"):
            raise ValueError("kind must be 'v2', 'v3' or 'v4', got %r" % (kind,))
        if self.map_dir is None:
            raise ValueError("get_data_from_chunk_%s needs ChunkLoader(map_dir=...)" % kind)
        b = self._seg_batchers.get(kind)
        if b is None:
            S = self.S
            b = SegTrainBatcher(S, self.device, None, self.dtype, None if kind == "v4" else (int(S * 0.9), int(S / 0.875)), self.map_fill)
            b.pyrandom, b.nprandom = self.batcher.pyrandom, self.batcher.nprandom
            self._seg_batchers[kind] = b
        return b

    def _submit_seg(self, chunk):
        return (self._submit(chunk), [self.pool.submit(decode_map, os.path.join(self.map_dir, name + self.map_ext)) for name in chunk])

    def _finish_seg(self, chunk, futures, kind):
        decoded = [f.result() for f in futures[0]]
        maps = [f.result() for f in futures[1]]
        images, ori, labels, croppings, target = self._seg_batcher(kind)(decoded, maps, self._labels(chunk))
        return images, ori, labels, croppings, list(chunk), target

    def get_data_from_chunk_v4(self, chunk):
        """myTool.py:1257-1310 -> (images (B,3,S,S), ori_images (B,3,S,S) uint8, labels (B,C), croppings (S,S,B) float32, name_list,
        target (B,S,S) uint8), all tensors on the device and shaped for ``segloss.joint_loss`` (see ``SegTrainBatcher.__call__``;
        the reference's target is float: ``target.float()``).  The map of image <name> is ``<map_dir>/<name><map_ext>`` (the
        reference hard-codes its directory, :1278); the long side is resized to exactly S (:1284)."""
        self._seg_batcher("v4")
        return self._finish_seg(chunk, self._submit_seg(chunk), "v4")

    def get_data_from_chunk_v3(self, chunk):
        """myTool.py:1202-1253: the same tuple with the saliency map of ``map_dir`` as the last element and the long side drawn from
        [int(0.9 * S), int(S / 0.875)] (:1228)."""
        self._seg_batcher("v3")
        return self._finish_seg(chunk, self._submit_seg(chunk), "v3")

    # ---- affinity stage: image + the label grid of its two CRF score dumps (voc12/data.py:241-278) ----
    def _aff_batcher(self):
        """The AffTrainBatcher of this loader, drawing from the loader's two generators"""
        if self.la_dir is None or self.ha_dir is None:
            raise ValueError("get_data_from_chunk_aff needs ChunkLoader(la_dir=..., ha_dir=...)")
        if self._aff is None:
            self._aff = AffTrainBatcher(self.S, self.device, None, self.dtype, self.color_jitter)
            self._aff.pyrandom, self._aff.nprandom = self.batcher.pyrandom, self.batcher.nprandom
        return self._aff

    def _submit_aff(self, chunk):
        return (self._submit(chunk), [self.pool.submit(load_score_dump, os.path.join(self.la_dir, name + ".npy")) for name in chunk],
                [self.pool.submit(load_score_dump, os.path.join(self.ha_dir, name + ".npy")) for name in chunk])

    def _finish_aff(self, chunk, futures):
        decoded, la, ha = ([f.result() for f in fs] for fs in futures)
        images, label = self._aff_batcher()(decoded, la, ha)
        return images, label, list(chunk)

    def get_data_from_chunk_aff(self, chunk):
        """voc12/data.py:241-278 for a chunk of names -> (images (B,3,S,S), label (B,S/8,S/8) uint8, name_list), the tensors on the
        device: the image <img_dir>/<name><ext> and the pickled score dicts <la_dir>/<name>.npy and <ha_dir>/<name>.npy, read by the
        worker threads, through ``AffTrainBatcher``.  ``label`` is a stride-1 grid: ``affinity.aff_train_step(model, head, optimizer,
        images, label)`` takes it as it is."""
        self._aff_batcher()
        return self._finish_aff(chunk, self._submit_aff(chunk))

    def iterate(self, chunks, train=True, depth=2, kind="v2"):
        """Yield the batches of `chunks` in order while the pool already decodes the next `depth` chunks (the previous step's
        GPU work and this thread's Python run meanwhile; the RNG draws stay in chunk order because they happen here).  ``kind``:
        "v2" (classification: get_data_from_chunk_v2 / _val), "v3" / "v4" (the segmentation tuples; training only) or "aff" (the
        affinity stage's; training only)."""
        chunks = list(chunks)
        if kind == "v2":
            submit, finish = self._submit, lambda c, f: self._finish(c, f, train)
        elif kind == "aff":
            self._aff_batcher()
            if not train:
                raise ValueError("kind='aff' has no validation form; use train=True")
            submit, finish = self._submit_aff, self._finish_aff
        else:
            self._seg_batcher(kind)
            if not train:
                raise ValueError("kind=%r has no validation form; use train=True" % (kind,))
            submit, finish = self._submit_seg, lambda c, f: self._finish_seg(c, f, kind)
        pending = [submit(c) for c in chunks[:depth]]
        for i, chunk in enumerate(chunks):
            futures = pending.pop(0)
            if i + depth < len(chunks):
                pending.append(submit(chunks[i + depth]))
            yield finish(chunk, futures)


def chunker(seq, size):
    """myTool.py:882-883."""
    return (seq[pos:pos + size] for pos in range(0, len(seq), size))


def read_file(path_to_file):
    """myTool.py:867-873: one image id per line."""
    with open(path_to_file) as f:
        return [line.rstrip("\n") for line in f]
