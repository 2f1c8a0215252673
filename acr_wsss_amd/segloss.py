"""The loss a segmentation head trains with on the pseudo-labels, on the GPU: the reference's ``compute_joint_loss``
(myTool.py:825-857) -- the logits upsampled to label size (:831), the background-only and the foreground-only cross-entropy with
ignore (:845-855; ``nn.CrossEntropyLoss(ignore_index=255)`` or ``SegmentationLosses.CrossEntropyLoss``, tool/loss.py:21-33) and a
dense-energy term on the bilateral lattice (``bilateralfilter_batch``, wrapper/bilateralfilter/bilateralfilter.cpp:42-55; the
``--densecrfloss / --rloss-scale / --sigma-rgb / --sigma-xy`` flags of infer_cam.py:58-65).  The arithmetic runs in
csrc/segloss.hip and csrc/crf.hip behind the C ABI (``acr_segloss_fwd``, ``acr_segloss_bwd``, ``acr_dense_energy_dot``,
``acr_lattice_*``; include/acr_hip.h states both rules in full); there is no CPU path -- without the HIP library and a GPU these
raise.  Forward and backward are bit-identical run to run.

The reference receives its ``DenseEnergyLosslayer`` as an argument and does not contain the class, so the energy is this project's
own definition: ``AS = roi * F[roi * S]``, ``E = -(weight / B) * sum S * AS`` and ``dE/dS := -(2 * weight / B) * AS`` (the filter
treated as symmetric, as the regularised-loss layer does).

"h, w" and "W, H" are the first and second spatial axis.  The cross-entropy calls enqueue kernels only; building a lattice reads
its point count back once per image (``acr_lattice_info``), as in crf.py."""
import numpy as np
import torch
import torch.nn.functional as F

from . import _abi
from . import _args as A
from . import _lib as L

_ENERGY_WS_BYTES = _abi.constants["ACR_DENSE_ENERGY_WS_BYTES"]


def _logits(logits):
    logits = A.tensor_arg(logits, "logits", torch.float32, shape=("B", "K", "h", "w"), contiguous=False, on_gpu=False)
    if not 2 <= logits.shape[1] <= A.MAX_SEG_CLASSES:
        raise ValueError("K=%d outside 2..%d" % (logits.shape[1], A.MAX_SEG_CLASSES))
    return logits


def _label(label, logits):
    """(B, W, H) contiguous uint8 on the device of ``logits``; numpy arrays and host tensors are uploaded; a single (W, H) map
    serves a batch of one.  The arguments are judged before the device is asked for: a bad shape is a ValueError with or without a
    GPU."""
    b = logits.shape[0]
    label = A.tensor_arg(label, "label", torch.uint8, contiguous=False, upload=True, on_gpu=False)
    if label.dim() == 2 and b == 1:
        label = label.unsqueeze(0)
    if label.dim() != 3 or label.shape[0] != b:
        raise ValueError("label %s must be (%d, W, H)" % (tuple(label.shape), b))
    if logits.shape[2] > label.shape[1] or logits.shape[3] > label.shape[2]:
        raise ValueError("logits %s must be no larger than the label %s" % (tuple(logits.shape[2:]), tuple(label.shape[1:])))
    L.require_gpu(logits)
    return A.on_device(label, "label", logits.device, upload=True).contiguous()


class _SplitCE(torch.autograd.Function):
    """(loss (3) = celoss, bg, fg; probs (B, K, W, H) or None; sums (B, 2); counts (B + 1, 2)) of acr_segloss_fwd."""

    @staticmethod
    def forward(ctx, logits, label, batch_average, want_probs):
        lib = L.load()
        ctx.set_materialize_grads(False)                 # an unused output's gradient stays None: no zero (B, K, W, H) d_probs
        logits = logits.contiguous()
        b, k, h, w = logits.shape
        _, W, H = label.shape
        dev = logits.device
        with torch.cuda.device(dev):
            ws, nbytes = L.workspace("acr_segloss_ws_bytes", b, k, h, w, W, H, device=dev)
            probs = torch.empty((b, k, W, H), dtype=torch.float32, device=dev) if want_probs else None
            rowstat = torch.empty((b, W, H, 2), dtype=torch.float32, device=dev)
            sums = torch.empty((b, 2), dtype=torch.float32, device=dev)
            counts = torch.empty((b + 1, 2), dtype=torch.int64, device=dev)
            loss = torch.empty(3, dtype=torch.float32, device=dev)
            L.check(lib.acr_segloss_fwd(L.ptr(logits), L.ptr(label), b, k, h, w, W, H, 1 if batch_average else 0, L.ptr(ws), nbytes,
                                        L.ptr(probs), L.ptr(rowstat), L.ptr(sums), L.ptr(counts), L.ptr(loss), L.stream_ptr()),
                    "acr_segloss_fwd")
        ctx.save_for_backward(logits, label, rowstat, counts, probs)
        ctx.batch_average = bool(batch_average)
        ctx.ws = ws
        ctx.mark_non_differentiable(sums, counts)
        if probs is None:
            return loss, None, sums, counts
        return loss, probs, sums, counts

    @staticmethod
    def backward(ctx, g_loss, g_probs, _g_sums, _g_counts):
        lib = L.load()
        logits, label, rowstat, counts, probs = ctx.saved_tensors
        b, k, h, w = logits.shape
        _, W, H = label.shape
        dev = logits.device
        with torch.cuda.device(dev):
            g = torch.zeros(3, dtype=torch.float32, device=dev) if g_loss is None else g_loss.to(torch.float32).contiguous()
            if g_probs is not None:
                g_probs = g_probs.to(torch.float32).contiguous()
            d_logits = torch.empty_like(logits)
            L.check(lib.acr_segloss_bwd(L.ptr(logits), L.ptr(label), L.ptr(rowstat), L.ptr(counts), L.ptr(g), L.ptr(probs),
                                        L.ptr(g_probs), b, k, h, w, W, H, 1 if ctx.batch_average else 0, L.ptr(ctx.ws),
                                        ctx.ws.numel(), L.ptr(d_logits), L.stream_ptr()), "acr_segloss_bwd")
        return d_logits, None, None, None


def _split_ce(logits, label, batch_average, want_probs):
    logits = _logits(logits)
    label = _label(label, logits)
    return _SplitCE.apply(logits, label, bool(batch_average), want_probs)


def split_cross_entropy(logits, label, batch_average=False, return_stats=False):
    """myTool.py:831,845-855 in one pass: logits (B, K, h, w) float32 on the GPU are upsampled to the label's (W, H) with
    bilinear ``align_corners=False`` and meet the background-only label (every label but 0 ignored) and the foreground-only label
    (0 ignored) in a cross-entropy with ignore.  label (B, W, H) uint8 -- the device tensor ``pseudo.seg_label`` returned, or
    numpy (uploaded) -- holds 0..K-1 and 255; a value in K..254 is ignored too.  Returns (celoss, bg, fg), celoss = bg + fg, each
    the mean over its pixels of the whole batch (``nn.CrossEntropyLoss(ignore_index=255)``), with ``batch_average`` also divided
    by B (tool/loss.py:21-33).  A term without a pixel is NaN, as torch's is.  Differentiable in ``logits``.  With
    ``return_stats`` also (sums (B, 2) float32, counts (B + 1, 2) int64): per image sum_bg, sum_fg and n_bg, n_fg, the last row
    of counts the batch totals.  Nothing here synchronises."""
    loss, _, sums, counts = _split_ce(logits, label, batch_average, False)
    out = (loss[0], loss[1], loss[2])
    return out + (sums, counts) if return_stats else out


def _placed(x, name, dev, shape, np_dtype=None):
    """``x`` -- a tensor of any dtype, or a numpy array (uploaded, as ``np_dtype`` if given) -- on ``dev`` and of ``shape``"""
    host = not torch.is_tensor(x)
    if host:
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np_dtype))
    x = A.on_device(x, name, dev, upload=host)
    if tuple(x.shape) != shape:
        raise ValueError("%s %s must be %s" % (name, tuple(x.shape), shape))
    return x


def filtered_probs(images, probs, roi, sigma_rgb, sigma_xy):
    """AS = roi * F_b[roi * S] per image: images (B, W, H, 3) uint8, probs (B, K, W, H) float32, roi (B, W, H) float32, all
    contiguous on one GPU; F_b the bilateral lattice of image b (bilateralfilter.cpp:4-20).  Returns (B, K, W, H)."""
    from .crf import PermutohedralLattice
    b, k, W, H = probs.shape
    out = torch.empty_like(probs)
    for i in range(b):
        lat = PermutohedralLattice(W, H, sigma_xy, rgb=images[i], srgb=sigma_rgb, device=probs.device)
        r = roi[i].reshape(-1)
        lat.filter(probs[i].reshape(k, W * H), pre=r, post=r, out=out[i].reshape(k, W * H))
    return out


class _DenseEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, probs, images, roi, weight, sigma_rgb, sigma_xy):
        lib = L.load()
        probs = probs.contiguous()
        b, k, W, H = probs.shape
        dev = probs.device
        with torch.cuda.device(dev):
            filtered = filtered_probs(images, probs, roi, sigma_rgb, sigma_xy)
            grad = torch.empty_like(probs)
            dots = torch.empty(b, dtype=torch.float32, device=dev)
            ws = torch.empty(_ENERGY_WS_BYTES, dtype=torch.uint8, device=dev)
            for i in range(b):
                L.check(lib.acr_dense_energy_dot(L.ptr(probs[i]), L.ptr(filtered[i]), k * W * H, -2.0 * weight / b, L.ptr(grad[i]),
                                                 L.ptr(ws), _ENERGY_WS_BYTES, L.ptr(dots[i:]), L.stream_ptr()), "acr_dense_energy_dot")
        ctx.save_for_backward(grad)
        return dots.sum() * (-float(weight) / b)

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return grad * g, None, None, None, None, None


class DenseEnergyLoss(torch.nn.Module):
    """The dense-energy (regularised) term of ``compute_joint_loss``, called as the reference calls its layer (:836):
    ``layer(ori_img, probs, croppings, seg_label)`` with ori_img (B, 3, W, H) values 0..255, probs (B, K, W, H) float32 on the
    GPU, croppings (B, W, H) in [0, 1]; ``seg_label`` is accepted and unused.  Returns the scalar
    ``E = -(weight / B) * sum S * (roi * F[roi * S])``; its gradient in probs is DEFINED as ``-(2 * weight / B) * roi * F[roi * S]``.
    ``scale_factor`` in (0, 1] (``--rloss-scale``): image and croppings are resized with nearest, the probabilities with bilinear
    ``align_corners=False``, to (floor(W * factor), floor(H * factor)), and ``sigma_xy`` is multiplied by the factor."""

    def __init__(self, weight, sigma_rgb, sigma_xy, scale_factor):
        super().__init__()
        if not (sigma_rgb > 0 and sigma_xy > 0 and 0 < scale_factor <= 1):
            raise ValueError("need sigma_rgb > 0, sigma_xy > 0, 0 < scale_factor <= 1 (got %r, %r, %r)" % (sigma_rgb, sigma_xy, scale_factor))
        self.weight, self.sigma_rgb, self.sigma_xy, self.scale_factor = float(weight), float(sigma_rgb), float(sigma_xy), float(scale_factor)

    def inputs(self, ori_img, probs, croppings):
        """What the kernels are given: (images (B, W', H', 3) uint8, probs (B, K, W', H'), roi (B, W', H'), sigma_xy') after the
        ``scale_factor`` plumbing"""
        probs = A.tensor_arg(probs, "probs", torch.float32, shape=("B", "K", "W", "H"), contiguous=False)
        b, _, W, H = probs.shape
        img = _placed(ori_img, "ori_img", probs.device, (b, 3, W, H))                    # values 0..255, uint8 or a float type
        roi = _placed(croppings, "croppings", probs.device, (b, W, H), np.float32).to(torch.float32)
        sxy = self.sigma_xy
        if self.scale_factor != 1.0:
            size = (max(1, int(W * self.scale_factor)), max(1, int(H * self.scale_factor)))
            img = F.interpolate(img.to(torch.float32), size=size, mode="nearest")
            roi = F.interpolate(roi.unsqueeze(1), size=size, mode="nearest").squeeze(1)
            probs = F.interpolate(probs, size=size, mode="bilinear", align_corners=False)
            sxy = sxy * self.scale_factor
        return img.to(torch.uint8).permute(0, 2, 3, 1).contiguous(), probs.contiguous(), roi.contiguous(), sxy

    def forward(self, ori_img, probs, croppings, seg_label=None):
        images, probs, roi, sxy = self.inputs(ori_img, probs, croppings)
        return _DenseEnergy.apply(probs, images, roi, self.weight, self.sigma_rgb, sxy)


def joint_loss(ori_img, seg, seg_label, croppings, criterion_batch_average, dense_energy_layer):
    """``compute_joint_loss`` (myTool.py:825-857): ori_img (B, 3, W, H), seg (B, K, h, w) float32 logits on the GPU, seg_label
    (B, W, H) uint8 -- device tensors as ``pseudo.seg_label`` returns them (no host trip; a single (W, H) map for B = 1) or
    numpy --, croppings (W, H, B) as the reference's loader hands them (:835 moves the batch axis to the front).
    ``criterion_batch_average`` stands for the reference's ``critersion``: False for ``nn.CrossEntropyLoss(ignore_index=255)``,
    True for ``SegmentationLosses(batch_average=True).CrossEntropyLoss``.  Returns (celoss, dloss); both differentiable in seg."""
    loss, probs, _, _ = _split_ce(seg, seg_label, criterion_batch_average, True)
    if torch.is_tensor(croppings):
        croppings = croppings.permute(2, 0, 1)
    else:
        croppings = np.asarray(croppings, dtype=np.float32).transpose(2, 0, 1)
    dloss = dense_energy_layer(ori_img, probs, croppings, seg_label)
    return loss[0], dloss
