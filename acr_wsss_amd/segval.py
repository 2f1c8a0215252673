"""Segmentation validation on the GPU: the reference's ``validation(model, use_crf)`` (myTool.py:1826-1895) with
``_crf_with_alpha_2`` (:1819-1823) -- per image the plain resize to ``test_size`` and normalisation (:1859-1866, ``data.val_batch``),
``forward_seg`` (:1869), the bilinear resize of the logits to the image's own size (:1881), the softmax (:1883) and the argmax
(:1891) or, with ``use_crf``, ``imutils.crf_inference_inf`` on the probabilities and then the argmax (:1886-1888), counted into the
confusion matrix of tool/metrics.py.  Resize, softmax and argmax are ONE kernel (csrc/segpred.hip behind ``acr_segpred_f32``;
include/acr_hip.h states the rule in full): the (K, H, W) tensor ``F.interpolate`` would write never exists, and label maps are
counted where they were computed (``evaluation.DeviceLabelCounters``).  There is no CPU path -- without the HIP library and a GPU
these raise.  Results are bit-identical run to run.

``scales`` and ``flip`` (test-time augmentation: the probabilities of several passes summed before the argmax) are this project's
extension; the reference runs one pass at 384 x 384."""
import os

import numpy as np
import torch

from . import _args as A
from . import _lib as L
from . import crf, data, decoder, pseudo
from .evaluation import DeviceLabelCounters
from .infer_cam import shard_indices


def forward_seg(model, head, x):
    """The reference's ``forward_seg`` (:1869): x (B, 3, h, w) float32 on the GPU, h and w multiples of 32 -> the logits
    (B, num_classes + 1, h, w) of an ``ACR(..., seg=True)`` (any of the reference's backbones) and its ``decoder.SegmentationHead``.
    A bf16 x with a bf16 model and head (vitb_hybrid) runs the pass in bf16 storage; the logits are float32 in either mode."""
    return head(decoder.decode(model, x))


def _out_hw(out_hw):
    try:
        H, W = (int(v) for v in out_hw)
    except (TypeError, ValueError):
        raise ValueError("out_hw must be (H, W), got %r" % (out_hw,))
    if H < 1 or W < 1:
        raise ValueError("out_hw %r must be positive" % (out_hw,))
    return H, W


def predict(logits, out_hw, *, hflip=False, probs=None, accumulate=False, want_label=True):
    """acr_segpred_f32: logits (B, K, h, w) contiguous float32 on the GPU -> the uint8 (B, H, W) label map at ``out_hw`` = (H, W),
    the smallest class among the maxima of the bilinearly resized (``align_corners=False``) logits; None without ``want_label``.
    ``probs``: a contiguous (B, K, H, W) float32 buffer on the same device, WRITTEN with the softmax of the resized logits, or with
    ``accumulate`` ADDED to -- the label is then the argmax of the updated buffer (the last pass of a sum over scales and flips
    leaves the final map).  ``hflip``: the logits are those of the mirrored image; the result is that of ``logits.flip(-1)``.
    Any ratio per axis works, enlarging or shrinking.  Nothing here synchronises."""
    logits = A.tensor_arg(logits, "logits", torch.float32, shape=("B", "K", "h", "w"), on_gpu=False)
    b, k, h, w = logits.shape
    if not 2 <= k <= A.MAX_SEG_CLASSES:
        raise ValueError("K=%d outside 2..%d" % (k, A.MAX_SEG_CLASSES))
    H, W = _out_hw(out_hw)
    if k * h * w >= 2 ** 31 or k * H * W >= 2 ** 31:
        raise ValueError("K * h * w and K * H * W must stay below 2^31 (K=%d, %d x %d -> %d x %d)" % (k, h, w, H, W))
    if probs is None:
        if accumulate:
            raise ValueError("accumulate needs the probs buffer it adds to")
        if not want_label:
            raise ValueError("nothing to compute: neither a label map nor probs was asked for")
    else:
        probs = A.tensor_arg(probs, "probs", torch.float32, shape=(b, k, H, W), on_gpu=False)
    L.require_gpu(logits)
    if probs is not None:
        A.on_device(probs, "probs", logits.device)
    lib = L.load()
    with torch.cuda.device(logits.device):
        label = torch.empty((b, H, W), dtype=torch.uint8, device=logits.device) if want_label else None
        L.check(lib.acr_segpred_f32(L.ptr(logits), b, k, h, w, H, W, 1 if hflip else 0, 1 if accumulate else 0, L.ptr(probs), L.ptr(label),
                                    L.stream_ptr()), "acr_segpred_f32")
    return label


def _sizes(test_size, scales):
    scales = tuple(float(s) for s in scales)
    if not scales:
        raise ValueError("no scales")
    sizes = [int(round(test_size * s)) for s in scales]
    for s, n in zip(scales, sizes):
        if n < 32 or n % 32:
            raise ValueError("scale %g of test_size %d gives %d, not a positive multiple of 32" % (s, test_size, n))
    return sizes


def _image(img, name="img_uint8"):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.size == 0:
        raise ValueError("%s must be a (H, W, 3) uint8 RGB image, got %s %s" % (name, img.dtype, img.shape))
    return img


def _predict_group(model, head, imgs, sizes, flip, use_crf, dev):
    """The uint8 (H, W) device label maps of a group of images that share the network passes."""
    passes = [(s, f) for s in sizes for f in ((False, True) if flip else (False,))]     # the fixed order the probabilities add in
    plain = len(passes) == 1 and not use_crf
    probs = [None] * len(imgs)
    labels = [None] * len(imgs)
    x, at = None, None
    for n, (size, flipped) in enumerate(passes):
        if at != size:
            x, at = data.val_batch(imgs, size, dev), size
            if model.cls_head.weight.dtype == torch.bfloat16:
                x = x.bfloat16()                             # a bf16 model (model.bfloat16()) takes bf16 images; the logits come back fp32
        logits = forward_seg(model, head, x.flip(-1).contiguous() if flipped else x)
        last = n == len(passes) - 1
        for i, img in enumerate(imgs):
            hw = img.shape[:2]
            if plain:                                        # the reference's path: the argmax of the resized logits
                labels[i] = predict(logits[i:i + 1], hw)[0]
                continue
            if probs[i] is None:
                probs[i] = torch.empty((1, logits.shape[1]) + tuple(hw), dtype=torch.float32, device=dev)
            labels[i] = predict(logits[i:i + 1], hw, hflip=flipped, probs=probs[i], accumulate=n > 0, want_label=last and not use_crf)
            if last and not use_crf:
                labels[i] = labels[i][0]
    if use_crf:
        for i, img in enumerate(imgs):
            p = probs[i][0]
            if len(passes) > 1:
                p = p / float(len(passes))                   # the mean probabilities
            k = p.shape[0]
            q = crf.crf_inference_inf_device(img, p.contiguous(), labels=k, device=dev)
            labels[i] = pseudo.label_map(q, list(range(k)), num_classes=k - 1, device=dev)
    return labels


def _device_of(model):
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise L.AcrHipError("segmentation validation runs on the GPU only (the model lies on %s); there is no CPU path" % dev)
    return dev


def predict_image(model, head, img_uint8, *, test_size=384, scales=(1.0,), flip=False, use_crf=False):
    """One image of the reference's ``validation`` loop: img_uint8 (H, W, 3) uint8 RGB -> the uint8 (H, W) label map on the
    model's device.  The image is resized to ``round(test_size * s)`` squared for every scale s (each a multiple of 32, else
    ValueError), passed through ``forward_seg`` and predicted at its own size.  With one scale, no flip and no CRF this is the
    argmax of the resized logits, exactly the reference's :1881,1891.  Otherwise the softmax probabilities of the passes are summed
    in a fixed order (scales as given, each plain and then mirrored) and the argmax of the sum is taken; with ``use_crf`` the
    mean probabilities go through ``crf.crf_inference_inf_device`` with the original image first (:1886-1888).  ``scales`` and
    ``flip`` are this project's extension: the reference runs (1.0,) without flip.  The caller sets eval mode and ``no_grad``."""
    sizes = _sizes(test_size, scales)
    img = _image(img_uint8)
    dev = _device_of(model)
    return _predict_group(model, head, [img], sizes, bool(flip), bool(use_crf), dev)[0]


def validate(model, head, items, *, rank=0, world=1, batch_size=8, test_size=384, scales=(1.0,), flip=False, use_crf=False,
             out_png=None, num_cls=21):
    """``validation(model, use_crf)`` over ``items``, an indexable of (name, uint8 RGB image (H, W, 3), gt uint8 (H, W) or None;
    255 = ignore), sharded over ranks like ``infer_cam.infer_cam_list``.  Model and head run in eval mode under ``no_grad`` (their
    modes are restored afterwards); the network pass is batched (every input is ``test_size`` squared, so batches always form;
    a batch that does not fit in memory is halved for the rest of the list), each image is predicted at its own size as
    ``predict_image`` does and counted on the device without reading the labels back.  With ``out_png`` every label map is also
    written to ``<out_png>/<name>.png`` (``pseudo.save_label_png``); an image without gt is written but not counted.  Returns this
    rank's ``evaluation.LabelCounters``: ``.mean_iou()`` is the reference's return value, ``merge`` adds another rank's."""
    sizes = _sizes(test_size, scales)
    if int(batch_size) < 1:
        raise ValueError("batch_size=%r must be at least 1" % (batch_size,))
    todo = shard_indices(len(items), rank, world)
    counters = None
    modes = [(m, m.training) for m in (model, head) if isinstance(m, torch.nn.Module)]
    batch_size, pos = int(batch_size), 0
    try:
        for m, _ in modes:
            m.eval()
        with torch.no_grad():
            while pos < len(todo):
                grp = [items[i] for i in todo[pos:pos + batch_size]]
                imgs, gts = [], []
                for name, img, gt in grp:
                    img = _image(img, "the image of %r" % (name,))
                    if gt is not None:
                        gt = np.asarray(gt)
                        if gt.dtype != np.uint8 or gt.shape != img.shape[:2]:
                            raise ValueError("the gt of %r must be uint8 %s like its image, got %s %s" % (name, img.shape[:2], gt.dtype, gt.shape))
                    imgs.append(img)
                    gts.append(gt)
                dev = _device_of(model)
                if counters is None:
                    counters = DeviceLabelCounters(num_cls, dev)
                try:
                    labels = _predict_group(model, head, imgs, sizes, bool(flip), bool(use_crf), dev)
                except torch.cuda.OutOfMemoryError:
                    if len(grp) == 1:
                        raise
                    labels = None                            # nothing of this group is counted yet: halve the batch, take it again
                    torch.cuda.empty_cache()
                    batch_size = max(1, len(grp) // 2)
                    continue
                for (name, _, _), gt, label in zip(grp, gts, labels):
                    if gt is not None:
                        counters.add(label, gt)
                    if out_png is not None:
                        os.makedirs(out_png, exist_ok=True)
                        pseudo.save_label_png(os.path.join(out_png, "%s.png" % name), label.cpu().numpy())
                pos += len(grp)
    finally:
        for m, was in modes:
            m.train(was)
    if counters is None:                                     # an empty shard
        counters = DeviceLabelCounters(num_cls, _device_of(model))
    return counters.to_host()
