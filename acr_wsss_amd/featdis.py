"""The class-centre feature-distance loss of the single-stage recipe, on the GPU: the reference's ``compute_dis_no_batch(seg,
seg_feature)`` (myTool.py:1624-1710, with ``compute_cos`` :1616-1622).  Every pixel's feature vector is pulled towards the centre
of the class the head predicts for it (the background centre per image, the foreground centres over the whole batch), the
foreground centres are pushed apart from one another and away from each image's background centre.  The arithmetic runs in
csrc/featdis.hip behind the C ABI (``acr_featdis_fwd``, ``acr_featdis_bwd``; include/acr_hip.h states the definition and the
gradient in full); there is no CPU path -- without the HIP library and a GPU these raise.  Forward and backward are bit-identical
run to run, and nothing here synchronises.

The reference hard-codes the classes 1..20 and 1024 channels; here the classes are 1..K-1 of a (B, K, h, w) ``seg`` and C is free.
The features are read as they lie (NCHW): no (B N, C) copy and no per-class masked copy exists."""
import torch

from . import _abi
from . import _args as A
from . import _lib as L

MAX_CLASSES = _abi.constants["ACR_FEATDIS_MAX_K"]   # 2 <= K <= 128
MAX_CHANNELS = 1 << 20
SLAB = 2048                               # FD_SLAB: pixels of a slab per 32 classes (csrc/featdis.hip)


def slab_pixels(k):
    """the pixels of one image whose class sums form one partial: above it an image has more than one slab"""
    return SLAB * ((k + 31) // 32)


def _inputs(seg, feat):
    """The arguments are judged before the device is asked for: a bad dtype, rank, shape or K is a ValueError with or without a GPU."""
    seg = A.tensor_arg(seg, "seg", torch.float32, shape=("B", "K", "h", "w"), contiguous=False, on_gpu=False)
    feat = A.tensor_arg(feat, "feat", torch.float32, shape=("B", "C", "h", "w"), contiguous=False, on_gpu=False)
    if not 2 <= seg.shape[1] <= MAX_CLASSES:
        raise ValueError("K=%d outside 2..%d" % (seg.shape[1], MAX_CLASSES))
    if feat.shape[1] > MAX_CHANNELS:
        raise ValueError("C=%d above %d" % (feat.shape[1], MAX_CHANNELS))
    if seg.shape[0] != feat.shape[0] or seg.shape[2:] != feat.shape[2:]:
        raise ValueError("seg %s and feat %s must share B, h and w" % (tuple(seg.shape), tuple(feat.shape)))
    if seg.shape[0] * seg.shape[2] * seg.shape[3] >= 1 << 31:
        raise ValueError("B h w = %d must stay below 2^31" % (seg.shape[0] * seg.shape[2] * seg.shape[3]))
    L.require_gpu(feat)
    A.on_device(seg, "seg", feat.device)


class _FeatDis(torch.autograd.Function):
    """(total, loss (3) = total, dis, pixel_dis; labels (B, h, w) uint8; counts (B + K - 1) int64) of acr_featdis_fwd"""

    @staticmethod
    def forward(ctx, seg, feat):
        lib = L.load()
        seg, feat = seg.detach().contiguous(), feat.contiguous()
        b, k, h, w = seg.shape
        c = feat.shape[1]
        dev = feat.device
        with torch.cuda.device(dev):
            ws, nbytes = L.workspace("acr_featdis_ws_bytes", b, k, c, h, w, device=dev)
            loss = torch.empty(3, dtype=torch.float32, device=dev)
            labels = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
            counts = torch.empty(b + k - 1, dtype=torch.int64, device=dev)
            pix = torch.empty((b, h * w, 2), dtype=torch.float64, device=dev)
            cst = torch.empty((2, b + k - 1, c), dtype=torch.float64, device=dev)
            L.check(lib.acr_featdis_fwd(L.ptr(seg), L.ptr(feat), b, k, c, h, w, L.ptr(ws), nbytes, L.ptr(loss), L.ptr(labels), L.ptr(counts),
                                        L.ptr(pix), L.ptr(cst), L.stream_ptr()), "acr_featdis_fwd")
            total = loss[0].clone()
        ctx.save_for_backward(feat, labels, pix, cst)
        ctx.k = k
        ctx.mark_non_differentiable(loss, labels, counts)
        return total, loss, labels, counts

    @staticmethod
    def backward(ctx, g_total, _g_loss, _g_labels, _g_counts):
        lib = L.load()
        feat, labels, pix, cst = ctx.saved_tensors
        b, c, h, w = feat.shape
        with torch.cuda.device(feat.device):
            g = g_total.to(torch.float32).contiguous()
            d_feat = torch.empty_like(feat)
            L.check(lib.acr_featdis_bwd(L.ptr(feat), L.ptr(labels), L.ptr(pix), L.ptr(cst), L.ptr(g), b, ctx.k, c, h, w, L.ptr(d_feat),
                                        L.stream_ptr()), "acr_featdis_bwd")
        return None, d_feat


def feature_distance_loss(seg, feat, return_stats=False):
    """``compute_dis_no_batch`` (myTool.py:1624-1710): seg (B, K, h, w) float32 logits and feat (B, C, h, w) float32 features on
    the GPU, the same h, w.  Every pixel takes the label ``argmax`` gives it (the first index of the maximum); the loss is
    ``dis + pixel_dis`` as include/acr_hip.h defines them -- the mean, over the B background centres and the F foreground centres
    with a pixel, of the mean ``1 - cos`` between a centre and its pixels, plus half the mean ``1 + cos`` between two foreground
    centres and half that between a foreground and a background centre.  Returns the scalar loss; ``feat`` receives its gradient,
    ``seg`` none (the labels are an argmax).  An all-zero feature vector has a gradient of order 1e7, as in the reference.
    With ``return_stats`` also (dis, pixel_dis, labels (B, h, w) uint8, counts (B + K - 1) int64: the background pixels per image,
    then the pixels per class 1..K-1 over the batch).  2 <= K <= 128; K = 21 is the reference."""
    _inputs(seg, feat)
    total, loss, labels, counts = _FeatDis.apply(seg, feat)
    if return_stats:
        return total, loss[1], loss[2], labels, counts
    return total


compute_dis_no_batch = feature_distance_loss
