"""Training-time CAM targets on the HIP path: the patch CAMs ``forward_cam`` returns as (B, T - 1, C) tokens become the normalised
(B, C, S, S) stack ``segtrain.saliency_labels`` / ``pseudo.seg_label_saliency`` take -- the reference's ``compute_cam_up``
(myTool.py:860-864: bilinear upsampling to the crop, times the image-level label) and the two-view sum and min-max normalisation
it applies to patch CAMs (infer_cam.py:156-162, 201-202) -- in one entry point, ``acr_train_cam_f32`` (csrc/traincam.hip), that
writes the largest tensor of the loop once.  include/acr_hip.h states the rule."""
import torch

from . import _args as A
from . import _lib as L

MAX_PLANES = 1 << 22          # B * C (TC_MAX_PLANES, csrc/traincam.hip)


def _int_pair(v, name):
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError("%s must be a pair of integers, got %r" % (name, v))
    if isinstance(a, bool) or isinstance(b, bool) or int(a) != a or int(b) != b:
        raise ValueError("%s must be a pair of integers, got %r" % (name, v))
    return int(a), int(b)


def training_cams(patch_cam, labels, out_hw, *, grid=None, patch_cam_flipped=None, eps=1e-5, normalize=True, out=None):
    """patch_cam (B, N, C) float32 on the GPU: the patch CAMs of view 1 (``forward_cam``'s ``x_patch_cam``), class stride 1, any
    token and batch stride -- a slice ``cams[:, skip:]`` of a (B, T, C) tensor is taken as it lies.  labels (B, C): the image-level
    labels, any real dtype (they multiply as float32).  out_hw = (oh, ow): the crop, any positive size.  ``grid`` = (gh, gw) with
    gh * gw == N, by default (oh // 16, ow // 16).  ``patch_cam_flipped``: the CAMs of the h-flipped view, same shape and strides;
    its upsampled map is mirrored back and added (infer_cam.py:156-162).  ``normalize``: (s - min) / (max - min + eps) per plane
    over the upsampled map (:201-202); False gives ``compute_cam_up``'s product alone.  A plane whose label is 0 is +0.
    Returns (B, C, oh, ow) float32 (``out`` when given: contiguous, on the same device), every element written.  The result is a
    target, not part of the graph: the inputs are detached.  Every argument is checked before the library is touched
    (ValueError); with device inputs nothing synchronises (``labels`` given on the host are uploaded first)."""
    oh, ow = _int_pair(out_hw, "out_hw")
    if oh < 1 or ow < 1:
        raise ValueError("out_hw must be positive, got %r" % (out_hw,))
    if not isinstance(normalize, (bool, int)) or normalize not in (0, 1):
        raise ValueError("normalize must be True or False, got %r" % (normalize,))
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 1e-45 < eps < 3e38:       # positive and finite as float32
        raise ValueError("eps must be a positive finite float32 number, got %r" % (eps,))
    patch_cam = A.tensor_arg(patch_cam, "patch_cam", torch.float32, shape=("B", "N", "C"), contiguous=False, on_gpu=False)
    B, N, C = patch_cam.shape
    gh, gw = _int_pair(grid, "grid") if grid is not None else (oh // 16, ow // 16)
    if gh < 1 or gw < 1 or gh * gw != N:
        raise ValueError("%d patch tokens are not a %d x %d grid (grid=%r, out_hw=%r)" % (N, gh, gw, grid, (oh, ow)))
    if patch_cam.stride(2) != 1 and C > 1:
        raise ValueError("patch_cam must have class stride 1, got strides %s" % (tuple(patch_cam.stride()),))
    if min(patch_cam.stride()) < 0:
        raise ValueError("patch_cam has a negative stride: %s" % (tuple(patch_cam.stride()),))
    if patch_cam_flipped is not None:
        f = patch_cam_flipped
        if not torch.is_tensor(f) or f.dtype != torch.float32 or f.shape != patch_cam.shape or f.device != patch_cam.device:
            raise ValueError("patch_cam_flipped must be a float32 tensor of patch_cam's shape %s and device, got %s" % (
                tuple(patch_cam.shape), "%s %s on %s" % (f.dtype, tuple(f.shape), f.device) if torch.is_tensor(f) else type(f).__name__))
        if (f.stride(0), f.stride(1)) != (patch_cam.stride(0), patch_cam.stride(1)) or (f.stride(2) != 1 and C > 1):
            raise ValueError("patch_cam_flipped must have patch_cam's strides %s, got %s" % (tuple(patch_cam.stride()), tuple(f.stride())))
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(labels)
    if labels.is_complex() or tuple(labels.shape) != (B, C):
        raise ValueError("labels must be a real (B, C) = (%d, %d) tensor, got %s %s" % (B, C, labels.dtype, tuple(labels.shape)))
    if B * C > MAX_PLANES or oh * ow >= 1 << 31 or gh * gw >= 1 << 31:
        raise ValueError("B * C = %d planes (at most %d) of %d x %d from a %d x %d grid (each below 2^31 values) are outside the "
                         "supported range" % (B * C, MAX_PLANES, oh, ow, gh, gw))
    if (B - 1) * patch_cam.stride(0) + (N - 1) * patch_cam.stride(1) + C >= 1 << 62 or B * C * oh * ow >= 1 << 60:
        raise ValueError("index range: B * C * oh * ow = %d values, strides %s" % (B * C * oh * ow, tuple(patch_cam.stride())))
    if out is not None:
        A.tensor_arg(out, "out", torch.float32, shape=(B, C, oh, ow), on_gpu=False)
        if out.device != patch_cam.device:                  # a ValueError like every refusal here, the host included (below)
            raise ValueError("out must be on %s like patch_cam, got %s" % (patch_cam.device, out.device))
    if not patch_cam.is_cuda:
        raise ValueError("training_cams runs on the GPU only (got a %s tensor); there is no CPU path" % patch_cam.device)
    dev = patch_cam.device
    lib = L.load()
    cam1 = patch_cam.detach()
    cam2 = patch_cam_flipped.detach() if patch_cam_flipped is not None else None
    lab = labels.detach().to(device=dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(dev):
        ws, nbytes = None, 0
        if normalize:
            ws, nbytes = L.workspace("acr_train_cam_ws_bytes", B, C, oh, ow, device=dev)
        if out is None:
            out = torch.empty((B, C, oh, ow), dtype=torch.float32, device=dev)
        L.check(lib.acr_train_cam_f32(L.ptr(cam1), L.ptr(cam2), cam1.stride(1), cam1.stride(0), L.ptr(lab), B, C, gh, gw, oh, ow,
                                      float(eps), int(normalize), L.ptr(ws), nbytes, L.ptr(out), L.stream_ptr()), "acr_train_cam_f32")
    return out


def cam_up(patch_cam, labels, out_hw, *, grid=None, patch_cam_flipped=None, out=None):
    """``compute_cam_up`` (myTool.py:860-864) for the batch, on the device: ``training_cams`` with ``normalize=False``."""
    return training_cams(patch_cam, labels, out_hw, grid=grid, patch_cam_flipped=patch_cam_flipped, normalize=False, out=out)
