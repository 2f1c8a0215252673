"""CAM evaluation -- single-pass counterpart of the reference's evaluation.py.

The reference sweeps the background threshold t = 0.00 ... 0.99 (`evaluation.py:127-133`) by re-reading every
`<name>.npy` dict and redoing `argmax([t, cam_0, ...])` per threshold (`:19-33`), 100 passes over the dataset.
Because plane 0 holds the constant t and `np.argmax` returns the first maximum, the prediction at threshold t is

    pred(t) = 0            if t >= m        (m = max_c cam_c at the pixel; ties go to index 0 = background)
              1 + argmax_c cam_c   otherwise

so all thresholds follow from (m, argmax) computed ONCE per pixel: a histogram of m over the threshold grid per
(gt class, argmax class) pair gives every TP/P/T counter of `evaluation.py:37-49` for every t.  Same wire format
in (pickled `{class: float32 (h,w)}` dicts, `infer_cam.py:227-228`), same counters and mIoU out
(`evaluation.py:59-85`).  ``SweepCounters`` / ``evaluate_cam_dir`` are pure numpy and read the files.

On the device (csrc/eval.hip behind ``acr_eval_sweep_f32`` / ``acr_eval_sweep_finish`` / ``acr_eval_confusion_u8``, include/acr_hip.h):
``DeviceSweepCounters`` keeps the same histograms for CAMs that already sit on the GPU -- scoring one 375x500 image on the host
costs more than generating its CAMs -- and ``DeviceLabelCounters`` the confusion matrix of uint8 label maps (the reference's
``--type png`` mode, tool/metrics.py:36-41).  Both hand back the host classes ``SweepCounters`` / ``LabelCounters`` with exactly
the integers the numpy code would hold; there is no CPU path behind them.  ``CamEvaluation`` is what
``infer_cam.infer_cam_list(..., evaluate=...)`` fills.  One deviation, shared by every class here: a ground-truth label that is
neither < num_cls nor 255 is ignored like 255 (the reference counts such a pixel in P only; VOC and COCO hold none).
"""
import os

import numpy as np

from . import _abi
from . import _args as A

CATEGORIES = ['background', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
              'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']


class SweepCounters:
    """TP/P/T per class for every threshold of ``thresholds`` (ascending)."""

    def __init__(self, thresholds, num_cls=21):
        self.t = np.asarray(thresholds, dtype=np.float32)
        assert np.all(np.diff(self.t) > 0)
        self.num_cls = num_cls
        nt = len(self.t)
        self.TP = np.zeros((nt, num_cls), np.int64)
        self.P = np.zeros((nt, num_cls), np.int64)
        self.T = np.zeros(num_cls, np.int64)

    def add(self, cam_dict, gt):
        """cam_dict: {class index (0-based, without background): float32 (h,w)}, gt: uint8 (h,w), 255 = ignore."""
        num_cls, nt = self.num_cls, len(self.t)
        keys = sorted(cam_dict.keys())
        cams = np.stack([cam_dict[k] for k in keys]).astype(np.float32)           # (n,h,w)
        # argmax over the (21,h,w) tensor of evaluation.py:27-31: absent classes are zero planes
        m_present = cams.max(axis=0)
        a_present = np.asarray(keys)[cams.argmax(axis=0)] + 1                       # first max among present, label space
        # a zero plane of an absent class wins/ties only if every present cam <= 0 there; first index wins ties
        absent = [c for c in range(num_cls - 1) if c not in cam_dict]
        if absent:
            first_absent = absent[0] + 1
            lower = (m_present < 0) | ((m_present == 0) & (first_absent < a_present))
            m = np.where(lower, 0.0, m_present).astype(np.float32)
            a = np.where(lower, first_absent, a_present)
        else:
            m, a = m_present, a_present
        valid = gt < 255
        m, a, g = m[valid], a[valid], gt[valid].astype(np.int64)
        # number of thresholds with t < m  -> for those the pixel is predicted `a`, for the rest background
        kfg = np.searchsorted(self.t, m, side="left")                                # t[k] < m  <=>  k < kfg
        np.add.at(self.T, g, 1)
        # P: foreground prediction `a` for thresholds [0, kfg), background for [kfg, nt)
        fg = np.zeros((nt + 1, num_cls), np.int64)
        np.add.at(fg, (kfg, a), 1)                     # pixels whose foreground range ends at kfg
        fg_cum = fg[::-1].cumsum(axis=0)[::-1]         # fg_cum[k] = #pixels with kfg >= k
        self.P += fg_cum[1:]                           # threshold index k is foreground iff kfg > k  -> kfg >= k+1
        self.P[:, 0] += (len(m) - fg_cum[1:].sum(axis=1))
        hit = a == g
        tp = np.zeros((nt + 1, num_cls), np.int64)
        np.add.at(tp, (kfg[hit], a[hit]), 1)
        self.TP += tp[::-1].cumsum(axis=0)[::-1][1:]
        bg = g == 0                                    # background pixels are TP whenever predicted background
        bgk = np.bincount(kfg[bg], minlength=nt + 1)
        self.TP[:, 0] += np.cumsum(bgk)[:nt]           # kfg <= k  <=> background at threshold k

    def miou(self):
        """(nt,) mIoU in percent and (nt, num_cls) IoU, evaluation.py:59-74."""
        iou = self.TP / (self.T[None, :] + self.P - self.TP + 1e-10)
        return iou.mean(axis=1) * 100.0, iou * 100.0

    def merge(self, other):
        """Add the counters of ``other`` (same threshold grid and class count, e.g. another rank's shard); returns self."""
        if other.num_cls != self.num_cls or other.t.shape != self.t.shape or not np.array_equal(other.t, self.t):
            raise ValueError("cannot merge sweep counters of different threshold grids or class counts")
        self.TP += other.TP
        self.P += other.P
        self.T += other.T
        return self


class LabelCounters:
    """Confusion matrix of label maps against ground truth: ``conf[gt][min(pred, num_cls)]`` over the pixels with gt < num_cls,
    (num_cls, num_cls + 1) int64 -- the last column collects predictions outside the label range.  Its first num_cls columns are
    tool/metrics.py:36-41; TP / P / T are the counters of evaluation.py:40-52 in ``--type png`` mode."""

    def __init__(self, num_cls=21, conf=None):
        self.num_cls = int(num_cls)
        self.conf = np.zeros((self.num_cls, self.num_cls + 1), np.int64)
        if conf is not None:
            conf = np.asarray(conf)
            if conf.shape != self.conf.shape:
                raise ValueError("conf %s is not (num_cls, num_cls + 1) = %s" % (conf.shape, self.conf.shape))
            self.conf += conf.astype(np.int64)

    def add(self, pred, gt):
        """pred, gt: integer label maps of one shape (host arrays)."""
        pred, gt = np.asarray(pred), np.asarray(gt)
        if pred.shape != gt.shape:
            raise ValueError("pred %s and gt %s differ in shape" % (pred.shape, gt.shape))
        keep = (gt >= 0) & (gt < self.num_cls)
        g = gt[keep].astype(np.int64)
        p = pred[keep].astype(np.int64)
        if np.any(p < 0):
            raise ValueError("negative predicted labels")
        p = np.minimum(p, self.num_cls)
        self.conf += np.bincount(g * (self.num_cls + 1) + p, minlength=self.conf.size).reshape(self.conf.shape)

    def merge(self, other):
        if other.num_cls != self.num_cls:
            raise ValueError("cannot merge label counters of %d and %d classes" % (self.num_cls, other.num_cls))
        self.conf += other.conf
        return self

    @property
    def TP(self):
        return np.diag(self.conf[:, :self.num_cls]).copy()

    @property
    def P(self):
        return self.conf[:, :self.num_cls].sum(axis=0)

    @property
    def T(self):
        return self.conf.sum(axis=1)

    def miou(self):
        """mIoU in percent and (num_cls,) IoU in percent, evaluation.py:66-76."""
        TP, P, T = self.TP, self.P, self.T
        iou = TP / (T + P - TP + 1e-10)
        return float(iou.mean() * 100.0), iou * 100.0

    # the four summaries of tool/metrics.py:10-34, on the square part of the matrix (plain ratios: an empty class gives nan,
    # which the means skip, as there)
    def _square(self):
        return self.conf[:, :self.num_cls].astype(np.float64)

    def pixel_accuracy(self):
        m = self._square()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.trace(m) / m.sum()

    def pixel_accuracy_class(self):
        m = self._square()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.nanmean(np.diag(m) / m.sum(axis=1))

    def _iu(self):
        m = self._square()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(m) / (m.sum(axis=1) + m.sum(axis=0) - np.diag(m))

    def mean_iou(self):
        return np.nanmean(self._iu())

    def frequency_weighted_iou(self):
        m = self._square()
        with np.errstate(divide="ignore", invalid="ignore"):
            freq = m.sum(axis=1) / m.sum()
        iu = self._iu()
        seen = freq > 0
        return (freq[seen] * iu[seen]).sum()


def evaluate_cam_dir(predict_dir, gt_dir, name_list, thresholds=None, num_cls=21):
    """Single pass over ``<predict_dir>/<name>.npy`` + ``<gt_dir>/<name>.png`` for all thresholds.
    Returns (thresholds, mIoU per threshold, SweepCounters)."""
    from PIL import Image
    if thresholds is None:
        thresholds = np.arange(100, dtype=np.float32) / 100.0                       # evaluation.py:128-130
    sc = SweepCounters(thresholds, num_cls)
    for name in name_list:
        cam_dict = np.load(os.path.join(predict_dir, name + ".npy"), allow_pickle=True).item()
        gt = np.array(Image.open(os.path.join(gt_dir, name + ".png")))
        sc.add(cam_dict, gt)
    return sc.t, sc.miou()[0], sc


# ---- device side ---------------------------------------------------------------------------------------------------------------
MAX_CLS, MAX_THRESHOLDS = _abi.constants["ACR_EVAL_MAX_CLS"], _abi.constants["ACR_EVAL_MAX_NT"]        # limits of the ABI


def _device(device):
    """torch.device of a GPU with the library loaded, else AcrHipError: nothing below has a CPU path."""
    from . import _lib as L
    dev = A.gpu_device(device, "device-side evaluation (SweepCounters / LabelCounters count on the host)")
    L.load()
    return dev


class DeviceSweepCounters:
    """``SweepCounters`` for CAMs that sit on the GPU: ``add`` enqueues one pass over the image on the current stream
    (acr_eval_sweep_f32) and nothing here synchronises but ``to_host()``."""

    def __init__(self, thresholds=None, num_cls=21, device="cuda"):
        import torch
        self.device = _device(device)
        if thresholds is None:
            thresholds = np.arange(100, dtype=np.float32) / 100.0                   # evaluation.py:128-130
        self.t = np.asarray(thresholds, dtype=np.float32).reshape(-1)
        self.num_cls = int(num_cls)
        if not 2 <= self.num_cls <= MAX_CLS:
            raise ValueError("num_cls=%d outside 2..%d" % (self.num_cls, MAX_CLS))
        if not 1 <= len(self.t) <= MAX_THRESHOLDS:
            raise ValueError("%d thresholds: 1..%d are supported" % (len(self.t), MAX_THRESHOLDS))
        if not np.all(np.isfinite(self.t)) or not np.all(np.diff(self.t) > 0):
            raise ValueError("thresholds must be finite and strictly ascending")
        nt = len(self.t)
        self._nfg = (nt + 1) * self.num_cls
        with torch.cuda.device(self.device):
            self._th = torch.from_numpy(self.t.copy()).to(self.device)
            self._raw = torch.zeros(2 * self._nfg + (nt + 1) + self.num_cls + 1, dtype=torch.int64, device=self.device)

    def reset(self):
        self._raw.zero_()

    def add(self, cams, classes, gt):
        """cams: (n, h, w) contiguous float32 device tensor, plane j the CAM of class ``classes[j]`` (0-based, without
        background, strictly ascending); gt: (h, w) uint8, a device tensor or a numpy array (uploaded), 255 = ignore."""
        import torch
        from . import _lib as L
        lib = L.load()
        arr, cl = A.class_array(classes, self.num_cls - 1, "no CAM to score")
        cams = A.tensor_arg(cams, "cams", torch.float32, shape=(len(cl), "h", "w"), device=self.device)
        n, h, w = cams.shape
        gt = A.tensor_arg(gt, "gt", torch.uint8, shape=(h, w), device=self.device, upload=True)
        with torch.cuda.device(self.device):
            L.check(lib.acr_eval_sweep_f32(L.ptr(cams), arr, n, L.ptr(gt), h, w, L.ptr(self._th), len(self.t), self.num_cls,
                                           L.ptr(self._raw), L.stream_ptr()), "acr_eval_sweep_f32")

    def add_dict(self, cam_dict, gt):
        """The wire format of ``SweepCounters.add``: {class: float32 (h, w) numpy array}, uploaded."""
        import torch
        keys = sorted(cam_dict.keys())
        if not keys:
            raise ValueError("empty cam_dict")
        cams = np.stack([np.asarray(cam_dict[k]) for k in keys]).astype(np.float32, copy=False)
        with torch.cuda.device(self.device):
            self.add(torch.from_numpy(np.ascontiguousarray(cams)).to(self.device), keys, gt)

    def to_host(self):
        """Run acr_eval_sweep_finish, copy once, and return a ``SweepCounters`` with the TP / P / T the numpy class would hold."""
        import torch
        from . import _lib as L
        lib = L.load()
        nt, nc = len(self.t), self.num_cls
        with torch.cuda.device(self.device):
            out = torch.empty(2 * nt * nc + nc, dtype=torch.int64, device=self.device)
            TP, P = out[:nt * nc], out[nt * nc:2 * nt * nc]
            L.check(lib.acr_eval_sweep_finish(L.ptr(self._raw), nt, nc, L.ptr(TP), L.ptr(P), L.stream_ptr()), "acr_eval_sweep_finish")
            o_t = 2 * self._nfg + nt + 1
            out[2 * nt * nc:].copy_(self._raw[o_t:o_t + nc])
            host = out.cpu().numpy()
        sc = SweepCounters(self.t, nc)
        sc.TP[...] = host[:nt * nc].reshape(nt, nc)
        sc.P[...] = host[nt * nc:2 * nt * nc].reshape(nt, nc)
        sc.T[...] = host[2 * nt * nc:]
        return sc

    def miou(self):
        return self.to_host().miou()


class DeviceLabelCounters:
    """``LabelCounters`` on the GPU: ``add`` enqueues acr_eval_confusion_u8 on the current stream; only ``to_host()`` waits."""

    def __init__(self, num_cls=21, device="cuda"):
        import torch
        self.device = _device(device)
        self.num_cls = int(num_cls)
        if not 1 <= self.num_cls <= MAX_CLS:
            raise ValueError("num_cls=%d outside 1..%d" % (self.num_cls, MAX_CLS))
        with torch.cuda.device(self.device):
            self._conf = torch.zeros((self.num_cls, self.num_cls + 1), dtype=torch.int64, device=self.device)

    def reset(self):
        self._conf.zero_()

    def add(self, pred, gt):
        """pred, gt: uint8 label maps of one shape, each a contiguous device tensor or a numpy array (uploaded)."""
        import torch
        from . import _lib as L
        lib = L.load()
        pred = A.tensor_arg(pred, "pred", torch.uint8, device=self.device, upload=True)
        gt = A.tensor_arg(gt, "gt", torch.uint8, shape=tuple(pred.shape), device=self.device, upload=True)
        with torch.cuda.device(self.device):
            L.check(lib.acr_eval_confusion_u8(L.ptr(pred), L.ptr(gt), pred.numel(), self.num_cls, L.ptr(self._conf), L.stream_ptr()),
                    "acr_eval_confusion_u8")

    def to_host(self):
        return LabelCounters(self.num_cls, self._conf.cpu().numpy())

    def miou(self):
        return self.to_host().miou()


def label_map(score_dict):
    """uint8 label map of a refined {label: float32 (h, w)} dict (crf_with_alpha / pamr_with_alpha): the argmax over its planes in
    ascending key order, the first maximum wins, label = key."""
    keys = sorted(score_dict.keys())
    planes = np.stack([np.asarray(score_dict[k]) for k in keys])
    return np.asarray(keys, dtype=np.uint8)[planes.argmax(axis=0)]


class CamEvaluation:
    """What ``infer_cam_list(..., evaluate=...)`` fills while it walks its list: ``cam``, the threshold sweep of the CAMs scored on
    the device before they are copied out, ``crf`` / ``pamr``, {alpha: DeviceLabelCounters} of the refined label maps (created
    when the first one arrives), and ``pseudo``, the DeviceLabelCounters of the pseudo-labels written with ``out_pseudo`` (None
    without it; a pseudo-label of 255 falls into the counters' last column, outside every class).  ``gt_of(name)`` returns the
    uint8 (W, H) ground truth of an item, 255 = ignore.  Counters live on the model's device; a sharded run gives each rank its own
    and the caller merges their ``to_host()`` results."""

    def __init__(self, gt_of, thresholds=None, num_cls=21):
        self.gt_of = gt_of
        self.thresholds = thresholds
        self.num_cls = int(num_cls)
        self.cam = None
        self.crf, self.pamr = {}, {}
        self.pseudo = None
        self._gts = {}
        self._free = {}        # shape -> [(pinned buffer, event after its last upload)]: buffers of released images, reused

    def bind(self, device):
        """Create the CAM counters on ``device`` (once; infer_cam_list calls this with the model's device).  Counters stay on
        the device they were created on: binding to another one raises."""
        if self.cam is None:
            self.cam = DeviceSweepCounters(self.thresholds, self.num_cls, device)
        elif self.cam.device != _device(device):
            raise ValueError("this CamEvaluation counts on %s and cannot score a model on %s (use one per device and merge)"
                             % (self.cam.device, device))
        return self

    def gt_device(self, name):
        """The ground truth of ``name`` on the counters' device, uploaded once from pinned memory without blocking and kept
        until ``release(name)``.  Pinned buffers are pooled by shape (allocating one costs more than the upload): a released
        buffer is written again only after the event behind its last upload, which has long passed by then."""
        import torch
        if name not in self._gts:
            gt = np.asarray(self.gt_of(name))
            if gt.dtype != np.uint8 or gt.ndim != 2:
                raise ValueError("gt_of(%r) must be a 2-d uint8 array, got %s %s" % (name, gt.dtype, gt.shape))
            free = self._free.get(gt.shape)
            if free:
                pinned, ev = free.pop()
                ev.synchronize()
            else:
                pinned = torch.empty(gt.shape, dtype=torch.uint8, pin_memory=True)
            pinned.copy_(torch.from_numpy(np.ascontiguousarray(gt)))
            with torch.cuda.device(self.cam.device):
                dev_gt = pinned.to(self.cam.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
            self._gts[name] = (pinned, dev_gt, ev)
        return self._gts[name][1]

    def release(self, name):
        held = self._gts.pop(name, None)
        if held is not None:
            self._free.setdefault(tuple(held[0].shape), []).append((held[0], held[2]))

    def score_cam(self, name, classes, norm_cam):
        self.cam.add(norm_cam, classes, self.gt_device(name))

    def score_labels(self, which, alpha, name, score_dict):
        table = self.crf if which == "crf" else self.pamr
        if alpha not in table:
            table[alpha] = DeviceLabelCounters(self.num_cls, self.cam.device)
        table[alpha].add(label_map(score_dict), self.gt_device(name))

    def bind_pseudo(self):
        """Create the pseudo-label counters next to the CAM counters (once; infer_cam_list calls this with ``out_pseudo``)."""
        if self.pseudo is None:
            self.pseudo = DeviceLabelCounters(self.num_cls, self.cam.device)
        return self.pseudo

    def score_pseudo(self, name, label):
        """label: the uint8 (W, H) pseudo-label as it sits on the device (pseudo.seg_label)."""
        self.bind_pseudo().add(label, self.gt_device(name))
