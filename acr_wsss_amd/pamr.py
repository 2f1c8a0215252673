"""Pixel-adaptive mask refinement (PAMR) of CAMs on the GPU: the host mirror of the reference's ``pamr.py`` (``PAMR``, :115-144,
with ``LocalAffinityAbs`` / ``LocalStDev`` / ``LocalAffinityCopy`` :10-110; imported by infer_cam.py:14 and
train_acr_coco.py:15), same names, arguments and defaults.  All arithmetic runs in csrc/pamr.hip (and the mask resize in
csrc/cam.hip) behind the C ABI (``acr_pamr_affinity``, ``acr_pamr_propagate``, ``acr_bilinear_resize``); there is no CPU path --
without the HIP library and a GPU these raise.  No autograd: the reference's users refine detached masks, and an input that
requires grad is refused rather than answered with a constant."""
import ctypes

import numpy as np
import torch

from . import _args as A
from . import _lib as L


def _dilation_array(dilations):
    dil = [int(d) for d in dilations]
    return (ctypes.c_int32 * len(dil))(*dil), len(dil)


def _check_input(t, name):
    A.tensor_arg(t, name, torch.float32, shape=("B", "C", "H", "W"))
    if t.requires_grad:
        raise ValueError("%s requires grad: pamr has no backward (detach it, as the reference's callers do)" % name)


def affinity(x, dilations=(1,)):
    """pamr.py:133-137: x (B, K, H, W) -> the (B, 8 * len(dilations), H, W) softmax weights of every pixel's neighbours."""
    lib = L.load()
    _check_input(x, "x")
    B, K, H, W = x.shape
    dil, nd = _dilation_array(dilations)
    w = torch.empty((B, 8 * nd, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(lib.acr_pamr_affinity(L.ptr(x), B, K, H, W, dil, nd, L.ptr(w), L.stream_ptr()), "acr_pamr_affinity")
    return w


def propagate(w, mask, num_iter, dilations=(1,)):
    """pamr.py:139-141: ``num_iter`` gathers of mask (B, C, H, W) under the weights w; ``mask`` itself is left untouched."""
    lib = L.load()
    _check_input(mask, "mask")
    B, C, H, W = mask.shape
    dil, nd = _dilation_array(dilations)
    if tuple(w.shape) != (B, 8 * nd, H, W):
        raise ValueError("w %s does not fit mask %s and %d dilations" % (tuple(w.shape), tuple(mask.shape), nd))
    bufs = [torch.empty_like(mask) for _ in range(min(int(num_iter), 2))]
    src = mask
    with torch.cuda.device(mask.device):
        for it in range(int(num_iter)):
            dst = bufs[it % 2]
            L.check(lib.acr_pamr_propagate(L.ptr(w), L.ptr(src), L.ptr(dst), B, C, H, W, dil, nd, L.stream_ptr()), "acr_pamr_propagate")
            src = dst
    return src


def pamr(x, mask, num_iter=1, dilations=(1,)):
    """``PAMR(num_iter, dilations)(x, mask)``: x (B, K, H, W) image, mask (B, C, h, w), both contiguous float32 device tensors ->
    the refined (B, C, H, W) float32 mask.  The mask is first resized to (H, W), bilinear with align_corners=True (:126)."""
    lib = L.load()
    _check_input(x, "x")
    _check_input(mask, "mask")
    if mask.device != x.device or mask.shape[0] != x.shape[0]:
        raise ValueError("x %s on %s and mask %s on %s do not belong together" % (tuple(x.shape), x.device, tuple(mask.shape), mask.device))
    B, _, H, W = x.shape
    _, C, h, w = mask.shape
    if (h, w) != (H, W):
        full = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            L.check(lib.acr_bilinear_resize(L.ptr(mask), h * w, 1, B * C, h, w, L.ptr(full), H, W, 1, None, 0, 0, L.stream_ptr()),
                    "acr_bilinear_resize")
        mask = full
    if int(num_iter) <= 0:
        return mask.clone() if (h, w) == (H, W) else mask
    return propagate(affinity(x, dilations), mask, num_iter, dilations)


class PAMR(torch.nn.Module):
    """Drop-in for the reference's ``PAMR`` (pamr.py:115-144): ``PAMR(num_iter, dilations)(x, mask)``."""

    def __init__(self, num_iter=1, dilations=[1]):
        super().__init__()
        self.num_iter = num_iter
        self.dilations = list(dilations)

    def forward(self, x, mask):
        return pamr(x, mask, self.num_iter, self.dilations)


def pamr_with_alpha(cam_dict, alphas, orig_img, num_iter=1, dilations=(1,), device="cuda"):
    """The twin of ``crf.crf_with_alpha`` (infer_cam.py:27-40) with PAMR as the refinement: {class: cam (h, w)} ->
    {alpha: {0: background, class + 1: ...}}, background score (1 - max_c cam)^alpha.  Takes ALL alphas at once: the affinity
    depends on the image only and is computed once, and the planes of every alpha ride as channels through the same
    iterations.  orig_img: (h, w, 3) uint8, uploaded as it is and converted on the device (the weights are invariant under a
    positive per-channel affine map of the image, so the raw 0..255 values serve as well as the normalised ones)."""
    alphas = list(alphas)
    classes, refined = pamr_with_alpha_device(cam_dict, alphas, orig_img, num_iter, dilations, device)
    refined = refined.cpu().numpy()
    n = 1 + len(classes)
    out = {}
    for ai, a in enumerate(alphas):
        d = {0: refined[ai * n]}
        for i, c in enumerate(classes):
            d[c + 1] = refined[ai * n + i + 1]
        out[a] = d
    return out


def pamr_with_alpha_device(cam_dict, alphas, orig_img, num_iter=1, dilations=(1,), device="cuda"):
    """``pamr_with_alpha`` with the refined scores left on the device: (classes in the dict's order, (len(alphas) * n, h, w)
    float32 tensor with n = 1 + len(classes): planes [ai * n, (ai + 1) * n) are the background and the classes at alphas[ai]) --
    what pseudo.seg_label takes."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.AcrHipError("pamr_with_alpha needs a GPU (no CPU path in the product)")
    L.load()
    alphas = list(alphas)
    classes = list(cam_dict.keys())
    cams = np.stack([cam_dict[c] for c in classes], axis=0).astype(np.float32, copy=False)
    top = 1 - cams.max(axis=0, keepdims=True)
    scores = np.concatenate([np.concatenate((np.power(top, a), cams), axis=0) for a in alphas], axis=0).astype(np.float32, copy=False)
    img = torch.as_tensor(np.ascontiguousarray(orig_img))
    if img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8 or tuple(img.shape[:2]) != cams.shape[1:]:
        raise ValueError("orig_img must be (h, w, 3) uint8 matching the cams %s, got %s %s" % (cams.shape[1:], tuple(img.shape), img.dtype))
    with torch.cuda.device(dev):
        x = img.to(dev).permute(2, 0, 1).to(torch.float32).contiguous()[None]
        return classes, pamr(x, torch.as_tensor(scores).to(dev)[None], num_iter, dilations)[0]
