"""Pseudo-label masks from refined CAMs on the GPU: the reference's ``compute_seg_label_rrm`` (myTool.py:674-744) -- the label
maps of the low- and high-alpha refinements (:705-706), their combination (:707-708, :732) and, with ``ignore_uncertain``, the
confidence rule (:694-701, :710-735) applied by the line the reference keeps commented at :737 (live in its sibling at :109).
All of it runs in csrc/pseudo.hip behind the C ABI (``acr_pseudo_label_f32``, ``acr_pseudo_compose``, ``acr_pseudo_ws_bytes``,
include/acr_hip.h states the rule in full); there is no CPU path -- without the HIP library and a GPU these raise.  The result is
an exact function of the inputs: uint8 labels 0..C and 255 (ignore), identical bits run to run.  One definition beyond the
reference: a label of the low-alpha map whose class never wins the CAM argmax above ``cam_floor`` has no sure pixel (the reference
raises IndexError there).

``seg_label_saliency`` is the saliency-guided rule the reference marks "# use this" (``compute_seg_label_3``, myTool.py:188-264;
``bg_alpha=32`` gives the label ``compute_seg_label_two_step`` composes, :313-367): a whole batch at once in csrc/pseudo_sal.hip
behind ``acr_sal_pseudo_compose``, its 10 x 10 opening also on its own as ``morph_open`` (``acr_morph_open_u8``).  The
CRF-based siblings (``compute_seg_label`` / ``compute_seg_label_2``, :57-185) are ``segtrain.crf_labels`` (without their saliency
line); of the reference's saliency variants the COCO ones are not covered, nor ``two_step``'s resize and PNG writes."""
import numpy as np
import torch

from . import _abi
from . import _args as A
from . import _lib as L

MAX_LABELS = _abi.constants["ACR_PSEUDO_MAX_LABELS"]            # C + 1 <= 128
_WHAT = "pseudo-label composition"


def _classes(classes, num_classes):
    if not 1 <= int(num_classes) <= MAX_LABELS - 1:
        raise ValueError("num_classes=%d outside 1..%d" % (num_classes, MAX_LABELS - 1))
    arr, cl = A.class_array(classes, num_classes, "no scores to label")
    return arr, len(cl)


def label_map(scores, labels, num_classes=20, device="cuda"):
    """Step A on the device (myTool.py:705-706): scores (n, W, H) float32, plane i the score of label ``labels[i]`` -- ascending,
    ``labels[0] == 0`` the background, label c + 1 class c, the layout of a refined dict -- -> the uint8 (W, H) argmax over the
    labels 0..num_classes, a label without a plane counting as 0.0 and the smallest label among the maxima winning (``np.argmax``
    over the reference's dense array; on a refined dict, whose scores are positive, this is ``evaluation.label_map``)."""
    labels = [int(l) for l in labels]
    if not labels or labels[0] != 0:
        raise ValueError("labels %s must start with the background label 0" % (labels,))
    arr, k = _classes([l - 1 for l in labels[1:]], num_classes)
    dev = A.first_device((scores,), device, _WHAT)
    lib = L.load()
    scores = A.tensor_arg(scores, "scores", torch.float32, shape=(k + 1, "W", "H"), device=dev, upload=True)
    _, w, h = scores.shape
    with torch.cuda.device(dev):
        out = torch.empty((w, h), dtype=torch.uint8, device=dev)
        L.check(lib.acr_pseudo_label_f32(L.ptr(scores), arr, k, w, h, int(num_classes), L.ptr(out), L.stream_ptr()), "acr_pseudo_label_f32")
    return out


def seg_label(cams, classes, la, ha, *, ignore_uncertain=False, bg_alpha=36, cam_floor=0.1, fg_quantile=0.3, bg_sure=0.3,
              crf_sure=0.8, num_classes=20, device="cuda"):
    """``compute_seg_label_rrm`` for one image: cams (K, W, H) float32, plane j the CAM of class ``classes[j]`` (0-based,
    strictly ascending); la / ha (K + 1, W, H) float32, the scores refined at the low / high background alpha (plane 0 the
    background, plane j + 1 class ``classes[j]``).  Device tensors, or numpy arrays (uploaded to ``device``).  Returns the uint8
    (W, H) pseudo-label on the device: the low-alpha label, 255 where that is background, 0 where the high-alpha label is
    background; with ``ignore_uncertain`` also 255 wherever the refined score or the CAM is not confident (defaults: the
    reference's constants).  Nothing here synchronises."""
    arr, k = _classes(classes, num_classes)
    if not (cam_floor >= 0 and 0 <= fg_quantile < 1 and crf_sure > 0):
        raise ValueError("need cam_floor >= 0, 0 <= fg_quantile < 1, crf_sure > 0 (got %r, %r, %r)" % (cam_floor, fg_quantile, crf_sure))
    dev = A.first_device((cams, la, ha), device, _WHAT)
    lib = L.load()
    cams = A.tensor_arg(cams, "cams", torch.float32, shape=(k, "W", "H"), device=dev, upload=True)
    _, w, h = cams.shape
    la = A.tensor_arg(la, "la", torch.float32, shape=(k + 1, w, h), device=dev, upload=True)
    ha = A.tensor_arg(ha, "ha", torch.float32, shape=(k + 1, w, h), device=dev, upload=True)
    with torch.cuda.device(dev):
        out = torch.empty((w, h), dtype=torch.uint8, device=dev)
        ws, nbytes = (None, 0) if not ignore_uncertain else L.workspace("acr_pseudo_ws_bytes", k, w, h, device=dev)
        L.check(lib.acr_pseudo_compose(L.ptr(cams), arr, k, L.ptr(la), L.ptr(ha), w, h, int(num_classes), 1 if ignore_uncertain else 0,
                                       float(bg_alpha), float(cam_floor), float(fg_quantile), float(bg_sure), float(crf_sure),
                                       L.ptr(ws), nbytes, L.ptr(out), L.stream_ptr()), "acr_pseudo_compose")
    return out


MAX_SAL_CLASSES = _abi.constants["ACR_SAL_PSEUDO_MAX_CLASSES"]  # labels c + 1 next to 255
OPEN_TILE = 64                            # edge of the opening kernel's output tile (PSAL_TILE, csrc/pseudo_sal.hip)
MAX_OPEN = 32                             # largest opening box


def seg_label_saliency(cams, present, saliency, *, bg_alpha=12, cut=0.9, open_size=10, device="cuda"):
    """``compute_seg_label_3`` (myTool.py:188-264) for a batch: cams (B, C, H, W) float32 in [0, 1]; present (B, C) uint8 or bool,
    nonzero where the image has the class (the reference's ``cam_label.astype(uint8) > 1e-5``; the plane of an absent class is
    ignored); saliency (B, H, W) uint8.  Device tensors, or numpy arrays (uploaded to ``device``).  Returns (label, saliency_out),
    both uint8 (B, H, W) on the device: the CAM label with its background as 255, 0 where the saliency is 0, except that such a
    pixel takes the lowest present class whose CAM lies above the class's ``cut`` quantile of its positive values (and 255 in
    saliency_out); then the ``open_size`` x ``open_size`` opening of the labelled area clears what it removes (0 skips it).
    ``bg_alpha=32`` is ``compute_seg_label_two_step``'s label before its resize.  The inputs are left as they are.  With device
    inputs nothing here synchronises (a numpy input is uploaded from pageable memory, which holds the host until it is copied)."""
    if not (bg_alpha > 0 and 0 <= cut < 1 and int(open_size) == open_size and 0 <= open_size <= MAX_OPEN):
        raise ValueError("need bg_alpha > 0, 0 <= cut < 1, open_size an integer in 0..%d (got %r, %r, %r)" % (MAX_OPEN, bg_alpha, cut, open_size))
    dev = A.first_device((cams, present, saliency), device, _WHAT)
    lib = L.load()
    cams = A.tensor_arg(cams, "cams", torch.float32, shape=("B", "C", "H", "W"), device=dev, upload=True)
    b, c, h, w = cams.shape
    if c > MAX_SAL_CLASSES:
        raise ValueError("C=%d outside 1..%d" % (c, MAX_SAL_CLASSES))
    present = A.tensor_arg(present, "present", torch.uint8, shape=(b, c), device=dev, upload=True, bool_as_u8=True)
    saliency = A.tensor_arg(saliency, "saliency", torch.uint8, shape=(b, h, w), device=dev, upload=True, bool_as_u8=True)
    with torch.cuda.device(dev):
        ws, nbytes = L.workspace("acr_sal_pseudo_ws_bytes", b, c, h, w, device=dev)
        label = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
        sal_out = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
        L.check(lib.acr_sal_pseudo_compose(L.ptr(cams), L.ptr(present), b, c, h, w, L.ptr(saliency), float(bg_alpha), float(cut),
                                           int(open_size), L.ptr(ws), nbytes, L.ptr(label), L.ptr(sal_out), L.stream_ptr()),
                "acr_sal_pseudo_compose")
    return label, sal_out


def morph_open(mask_u8, k=10, device="cuda"):
    """The opening of ``seg_label_saliency`` alone (``cv2.morphologyEx(mask, cv2.MORPH_OPEN, np.ones((k, k)))`` by OpenCV's
    documented rule, myTool.py:254): mask_u8 (H, W) or (B, H, W) uint8, foreground where nonzero; returns 255 where the dilation of
    the erosion holds and 0 elsewhere, both taken over the offsets -(k // 2) .. k - 1 - k // 2 with positions outside the image
    left out.  1 <= k <= 32."""
    if not (int(k) == k and 1 <= k <= MAX_OPEN):
        raise ValueError("k=%r outside 1..%d" % (k, MAX_OPEN))
    dev = A.first_device((mask_u8,), device, _WHAT)
    lib = L.load()
    mask = A.tensor_arg(mask_u8, "mask_u8", torch.uint8, device=dev, upload=True, bool_as_u8=True)
    if mask.dim() not in (2, 3):
        raise ValueError("mask_u8 %s must be (H, W) or (B, H, W)" % (tuple(mask.shape),))
    b = mask.shape[0] if mask.dim() == 3 else 1
    h, w = mask.shape[-2:]
    with torch.cuda.device(dev):
        out = torch.empty_like(mask)
        L.check(lib.acr_morph_open_u8(L.ptr(mask), b, h, w, int(k), L.ptr(out), L.stream_ptr()), "acr_morph_open_u8")
    return out


def stack_dicts(cam_dict, la_dict, ha_dict):
    """The wire formats infer_cam_list writes -- {class: (W, H)} and two refined {0: background, class + 1: ...} dicts -- as
    (cams (K, W, H), ascending classes, la (K + 1, W, H), ha (K + 1, W, H)) float32 numpy arrays."""
    classes = sorted(int(c) for c in cam_dict)
    if not classes:
        raise ValueError("empty cam_dict: an image without a positive class has no pseudo-label to compose")
    want = [0] + [c + 1 for c in classes]
    for name, d in (("la_dict", la_dict), ("ha_dict", ha_dict)):
        if sorted(int(k) for k in d) != want:
            raise ValueError("%s holds the labels %s, the CAMs ask for %s" % (name, sorted(d), want))
    cams = np.stack([np.asarray(cam_dict[c]) for c in classes]).astype(np.float32, copy=False)
    la = np.stack([np.asarray(la_dict[l]) for l in want]).astype(np.float32, copy=False)
    ha = np.stack([np.asarray(ha_dict[l]) for l in want]).astype(np.float32, copy=False)
    return cams, classes, la, ha


def seg_label_from_dicts(cam_dict, la_dict, ha_dict, **kw):
    """``seg_label`` on the dictionaries infer_cam_list writes with out_cam and out_crf / out_pamr; returns a numpy uint8 (W, H)."""
    cams, classes, la, ha = stack_dicts(cam_dict, la_dict, ha_dict)
    return seg_label(cams, classes, la, ha, **kw).cpu().numpy()


def voc_palette():
    """The 256 x 3 uint8 PASCAL VOC colour map: bit b of label i goes to bit 7 - b // 3 of channel b % 3."""
    pal = np.zeros((256, 3), np.uint8)
    for i in range(256):
        for b in range(8):
            if (i >> b) & 1:
                pal[i, b % 3] |= 1 << (7 - b // 3)
    return pal


def save_label_png(path, label):
    """Write a uint8 (W, H) label map as a ``P``-mode PNG with the VOC colour map; ``np.array(PIL.Image.open(path))`` returns the
    map unchanged (what the reference's evaluation.py reads with input_type='png')."""
    from PIL import Image
    label = np.asarray(label)
    if label.dtype != np.uint8 or label.ndim != 2:
        raise ValueError("label must be a 2-d uint8 array, got %s %s" % (label.dtype, label.shape))
    im = Image.fromarray(np.ascontiguousarray(label))     # mode L; attaching a palette makes it P, the pixel bytes stay
    im.putpalette(voc_palette().reshape(-1).tolist())
    im.save(path, format="PNG")
