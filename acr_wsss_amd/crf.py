"""Dense-CRF refinement of CAMs on the GPU: the host mirror of ``imutils.crf_inference``
(tool/imutils.py:345-362 -- pydensecrf's ``DenseCRF2D`` with ``addPairwiseGaussian(sxy=3, compat=3)``,
``addPairwiseBilateral(sxy=80, srgb=13, compat=10)`` and ``inference(t)``), of ``imutils.crf_inference_inf`` (:365-384, the
validation's parameter set: bilateral sxy=83, srgb=5, compat=4) and of ``_crf_with_alpha``
(infer_cam.py:27-40), same names, arguments and return layout; ``crf_with_alphas`` puts several background alphas through one
pair of lattices, and ``crf_inference_label`` mirrors tool/imutils.py:387-400 (unaries from a label map).  All arithmetic runs in csrc/crf.hip behind the C ABI
(``acr_lattice_*``, ``acr_crf_*``); there is no CPU path -- without the HIP library and a GPU these raise."""
import ctypes

import numpy as np
import torch

from . import _args as A
from . import _lib as L


class PermutohedralLattice:
    """One pairwise kernel of the CRF: the lattice of an H x W image with spatial (rgb=None, d = 2) or bilateral
    (rgb = (H, W, 3) uint8, d = 5) features; ``filter`` applies Permutohedral::compute
    (wrapper/bilateralfilter/permutohedral.cpp:441-520) to K planes."""

    def __init__(self, h, w, sxy, rgb=None, srgb=1.0, device="cuda"):
        lib = L.load()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.AcrHipError("PermutohedralLattice needs a GPU (no CPU path in the product)")
        self.h, self.w, self.n = int(h), int(w), int(h) * int(w)
        self.d = 2 if rgb is None else 5
        self.device = dev
        if rgb is not None:
            rgb = torch.as_tensor(np.ascontiguousarray(rgb)) if not torch.is_tensor(rgb) else rgb
            if tuple(rgb.shape) != (self.h, self.w, 3) or rgb.dtype != torch.uint8:
                raise ValueError("rgb must be (H, W, 3) uint8, got %s %s" % (tuple(rgb.shape), rgb.dtype))
            rgb = rgb.to(dev).contiguous()
        with torch.cuda.device(dev):
            self.ws, nbytes = L.workspace("acr_lattice_ws_bytes", self.n, self.d, device=dev)
            L.check(lib.acr_lattice_build(L.ptr(rgb) if rgb is not None else None, self.h, self.w, float(sxy), float(srgb),
                                          L.ptr(self.ws), nbytes, L.stream_ptr()), "acr_lattice_build")
            m, ovf = ctypes.c_int32(0), ctypes.c_int32(0)
            L.check(lib.acr_lattice_info(L.ptr(self.ws), ctypes.byref(m), ctypes.byref(ovf), L.stream_ptr()), "acr_lattice_info")
        self.n_points = int(m.value)
        self._vals = None

    def filter(self, x, pre=None, post=None, scale=None, out=None):
        """x (K, n) float32 on the device -> scale * post * filter(pre * x), (K, n)."""
        lib = L.load()
        A.tensor_arg(x, "x", torch.float32, shape=("K", self.n))
        k = x.shape[0]
        need = 2 * k * (self.n_points + 2)
        if self._vals is None or self._vals.numel() < need:
            self._vals = torch.empty(need, dtype=torch.float32, device=self.device)
        out = torch.empty_like(x) if out is None else out
        with torch.cuda.device(self.device):
            L.check(lib.acr_lattice_filter(L.ptr(self.ws), self.n, self.d, self.n_points, L.ptr(x), L.ptr(pre) if pre is not None else None,
                                           L.ptr(out), L.ptr(post) if post is not None else None,
                                           float(scale) if scale is not None else 1.0, 0 if scale is None else 1, k,
                                           L.ptr(self._vals), L.stream_ptr()), "acr_lattice_filter")
        return out

    def tables(self):
        """(offsets (n, d+1) int32, weights (n, d+1) float32, point keys (n_points, d) int16) as numpy arrays."""
        lib = L.load()
        po, pw, pk = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        L.check(lib.acr_lattice_tables(L.ptr(self.ws), self.n, self.d, ctypes.byref(po), ctypes.byref(pw), ctypes.byref(pk)), "acr_lattice_tables")
        base = self.ws.data_ptr()
        e = self.n * (self.d + 1)
        off = self.ws[po.value - base: po.value - base + 4 * e].view(torch.int32).reshape(self.n, self.d + 1).cpu().numpy()
        wts = self.ws[pw.value - base: pw.value - base + 4 * e].view(torch.float32).reshape(self.n, self.d + 1).cpu().numpy()
        packed = self.ws[pk.value - base: pk.value - base + 8 * self.n_points].view(torch.int64).cpu().numpy()
        keys = np.stack([((packed >> (12 * (self.d - 1 - c))) & 4095) - 2048 for c in range(self.d)], axis=1).astype(np.int16)
        return off, wts, keys


class _Kernel:
    """DenseKernel (DIAG_KERNEL, NORMALIZE_SYMMETRIC: pydensecrf's defaults) with a Potts weight."""

    def __init__(self, lattice, compat):
        lib = L.load()
        self.lat = lattice
        self.compat = float(compat)
        ones = torch.ones((1, lattice.n), dtype=torch.float32, device=lattice.device)
        self.norm = lattice.filter(ones).reshape(-1).contiguous()
        with torch.cuda.device(lattice.device):
            L.check(lib.acr_crf_norm(L.ptr(self.norm), lattice.n, L.stream_ptr()), "acr_crf_norm")

    def apply(self, q, out=None):
        return self.lat.filter(q, pre=self.norm, post=self.norm, scale=self.compat, out=out)


def crf_inference(img, probs, t=10, scale_factor=1, labels=21, device="cuda"):
    """tool/imutils.py:345-362.  img (h, w, 3) uint8, probs (labels, h, w) -> Q (labels, h, w) float32 numpy array."""
    return crf_inference_device(img, probs, t, scale_factor, labels, device).cpu().numpy()


def crf_inference_device(img, probs, t=10, scale_factor=1, labels=21, device="cuda"):
    """``crf_inference`` with Q left where it was computed: a (labels, h, w) float32 tensor on ``device``."""
    return _mean_field(img, probs, t, labels, device, (3 / scale_factor, 3), (80 / scale_factor, 13, 10))


def crf_inference_inf(img, probs, t=10, scale_factor=1, labels=21, device="cuda"):
    """tool/imutils.py:365-384, the parameter set the reference's validation refines its probabilities with
    (myTool.py:1819-1823): ``addPairwiseGaussian(sxy=3, compat=3)``, ``addPairwiseBilateral(sxy=83, srgb=5, compat=4)``.
    img (h, w, 3) uint8, probs (labels, h, w) -> Q (labels, h, w) float32 numpy array."""
    return crf_inference_inf_device(img, probs, t, scale_factor, labels, device).cpu().numpy()


def crf_inference_inf_device(img, probs, t=10, scale_factor=1, labels=21, device="cuda"):
    """``crf_inference_inf`` with Q left on the device.  ``probs`` may also be a contiguous (labels, h, w) float32 tensor that
    already sits on the GPU (what ``segval.predict`` accumulated): it is then read in place, with no host round trip, and the
    result has the bits the same values give as a numpy array."""
    return _mean_field(img, probs, t, labels, device, (3 / scale_factor, 3), (83 / scale_factor, 5, 4))


def _mean_field(img, probs, t, labels, device, gaussian, bilateral):
    """The loop all parameter sets share: unary_from_softmax, a Gaussian kernel ``(sxy, compat)`` and a bilateral kernel
    ``(sxy, srgb, compat)``, ``t`` iterations -> Q (labels, h, w) float32 on ``device``."""
    lib = L.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.AcrHipError("crf_inference needs a GPU (no CPU path in the product)")
    img = np.ascontiguousarray(img)
    h, w = img.shape[:2]
    n = h * w
    if torch.is_tensor(probs):
        A.tensor_arg(probs, "probs", torch.float32, shape=(labels, h, w))
        dev = probs.device
        p = probs.reshape(labels, n)
    else:
        p = torch.as_tensor(np.ascontiguousarray(probs, dtype=np.float32)).reshape(labels, n).to(dev)
    unary = torch.empty_like(p)
    q = torch.empty_like(p)
    with torch.cuda.device(dev):
        L.check(lib.acr_crf_unary(L.ptr(p), L.ptr(unary), labels * n, 1e-5, L.stream_ptr()), "acr_crf_unary")
        kernels = [_Kernel(PermutohedralLattice(h, w, gaussian[0], device=dev), gaussian[1]),
                   _Kernel(PermutohedralLattice(h, w, bilateral[0], rgb=img, srgb=bilateral[1], device=dev), bilateral[2])]
        L.check(lib.acr_crf_update(L.ptr(unary), None, None, L.ptr(q), n, labels, L.stream_ptr()), "acr_crf_update")
        msg = [torch.empty_like(p), torch.empty_like(p)]
        for _ in range(t):
            for k, m in zip(kernels, msg):
                k.apply(q, out=m)
            L.check(lib.acr_crf_update(L.ptr(unary), L.ptr(msg[0]), L.ptr(msg[1]), L.ptr(q), n, labels, L.stream_ptr()), "acr_crf_update")
    return q.reshape(labels, h, w)


def crf_with_alpha(cam_dict, alpha, orig_img, device="cuda"):
    """infer_cam.py:27-40: {class: cam (h, w)} -> {0: background, class + 1: ...} after the CRF, background score
    (1 - max_c cam)^alpha."""
    classes, refined = crf_with_alpha_device(cam_dict, alpha, orig_img, device=device)
    return score_dict(classes, refined.cpu().numpy())


def crf_with_alpha_device(cam_dict, alpha, orig_img, device="cuda"):
    """``crf_with_alpha`` with the refined scores left on the device: (classes in the dict's order, (1 + len(classes), h, w)
    float32 tensor, plane 0 the background and plane i + 1 class ``classes[i]``) -- what pseudo.seg_label takes."""
    classes = list(cam_dict.keys())
    cams = np.stack([cam_dict[c] for c in classes], axis=0)
    background = np.power(1 - cams.max(axis=0, keepdims=True), alpha)
    scores = np.concatenate((background, cams), axis=0)
    return classes, crf_inference_device(orig_img, scores, labels=scores.shape[0], device=device)


def score_dict(classes, refined):
    """{0: background, class + 1: ...} of a host (1 + len(classes), h, w) array: the layout infer_cam.py:38-40 writes."""
    out = {0: refined[0]}
    for i, c in enumerate(classes):
        out[c + 1] = refined[i + 1]
    return out


# ---- several alphas through one pair of lattices ----------------------------------------------------------------------------
def _iterate(kernels, unary, q, t, n, k, groups):
    """``t`` mean-field updates of ``groups`` stacks of ``k`` planes held in one (groups * k, n) tensor: one filter call per
    kernel over all planes and one grouped normalisation per iteration.  ``q`` holds the initial Q and is updated in place."""
    lib = L.load()
    msg = [torch.empty_like(q), torch.empty_like(q)] if t > 0 else None
    for _ in range(t):
        for kern, m in zip(kernels, msg):
            kern.apply(q, out=m)
        L.check(lib.acr_crf_update_groups(L.ptr(unary), L.ptr(msg[0]), L.ptr(msg[1]), L.ptr(q), n, k, groups, L.stream_ptr()),
                "acr_crf_update_groups")
    return q


def _alpha_list(alphas, t):
    alphas = [a for a in alphas]
    if not alphas or any(isinstance(a, bool) or not isinstance(a, (int, float, np.integer, np.floating)) or not np.isfinite(a) or a < 0
                         for a in alphas):
        raise ValueError("alphas must be a non-empty sequence of numbers >= 0, got %r" % (alphas,))
    if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0:
        raise ValueError("t must be an integer >= 0, got %r" % (t,))
    return alphas


def crf_with_alphas(cam_dict, alphas, orig_img, t=10, device="cuda"):
    """``crf_with_alpha`` for ALL ``alphas`` at once, the twin of ``pamr.pamr_with_alpha``: {class: cam (h, w)} ->
    {alpha: {0: background, class + 1: ...}}.  Every array has the bits ``crf_with_alpha(cam_dict, alpha, orig_img)`` returns."""
    alphas = list(alphas)
    classes, refined = crf_with_alphas_device(cam_dict, alphas, orig_img, t=t, device=device)
    refined = refined.cpu().numpy()
    n = 1 + len(classes)
    return {a: score_dict(classes, refined[ai * n:(ai + 1) * n]) for ai, a in enumerate(alphas)}


def crf_with_alphas_device(cams, alphas, orig_img, classes=None, t=10, device="cuda", return_scores=False):
    """The CRF of ``crf_with_alpha_device`` at several background alphas in one mean field: returns (classes, (len(alphas) * n,
    h, w) float32 tensor on the device) with n = 1 + len(classes); planes [ai * n, (ai + 1) * n) are the background and the
    classes at ``alphas[ai]`` (duplicates allowed) -- what pseudo.seg_label takes.  The Gaussian and the bilateral lattice depend
    on the image only and are built once (``crf_inference``'s parameters); each of the ``t`` iterations filters all planes in one
    call per kernel and normalises them in one launch.  Planes never interact outside their group, so every plane has the bits
    of the separate run.
    ``cams``: a {class: cam (h, w)} dict, or a (K, h, w) numpy array with ``classes`` (K ids) -- the backgrounds are then formed as
    ``crf_with_alpha_device`` forms them (numpy's ``np.power``, one upload) and the result equals that function's bit for bit; or
    a contiguous (K, h, w) float32 tensor on the GPU with ``classes`` -- then the backgrounds powf(1 - max_c cam, alpha), the
    unaries and the initial Q are made by one kernel (``acr_crf_alpha_unary``) and nothing leaves the device.
    ``orig_img``: (h, w, 3) uint8, a numpy array or a tensor on the GPU.  ``return_scores``: also return the (len(alphas) * n, h, w)
    score stack the unaries were taken from."""
    alphas = _alpha_list(alphas, t)
    on_device = torch.is_tensor(cams)
    if isinstance(cams, dict):
        if classes is not None and list(classes) != list(cams.keys()):
            raise ValueError("classes %r given next to a cam_dict with the keys %r" % (list(classes), list(cams.keys())))
        classes = list(cams.keys())
        if not classes:
            raise ValueError("empty cam_dict: an image without a positive class has nothing to refine")
        cams = np.stack([cams[c] for c in classes], axis=0)
    elif classes is None:
        raise ValueError("classes must name the planes of cams unless cams is a cam_dict")
    classes = list(classes)
    if on_device:
        cams = A.tensor_arg(cams, "cams", torch.float32, shape=(len(classes), "h", "w"), on_gpu=False)
    else:
        cams = np.asarray(cams)
        if cams.ndim != 3 or cams.shape[0] != len(classes) or cams.size == 0 or cams.dtype.kind != "f":
            raise ValueError("cams must be a non-empty (%d, h, w) floating-point array, got %s %s" % (len(classes), cams.shape, cams.dtype))
    k, (h, w) = 1 + len(classes), tuple(cams.shape[1:])
    n, groups = h * w, len(alphas)
    img = A.tensor_arg(orig_img, "orig_img", torch.uint8, shape=(h, w, 3), upload=True, on_gpu=False)
    if groups * k * n >= 2 ** 31:
        raise ValueError("%d alphas x %d planes x %d pixels exceed 2^31 - 1 elements" % (groups, k, n))
    dev = A.first_device((cams, orig_img) if on_device else (orig_img,), device, "crf_with_alphas")
    lib = L.load()
    if on_device:
        cams = A.on_device(cams, "cams", dev)
    with torch.cuda.device(dev):
        img = A.on_device(img, "orig_img", dev, upload=True)
        unary = torch.empty((groups * k, n), dtype=torch.float32, device=dev)
        q = torch.empty_like(unary)
        if on_device:
            scores = torch.empty_like(unary) if return_scores else None
            alpha_t = torch.tensor(alphas, dtype=torch.float32).to(dev)
            L.check(lib.acr_crf_alpha_unary(L.ptr(cams), k - 1, n, L.ptr(alpha_t), groups, 1e-5, L.ptr(scores), L.ptr(unary), L.ptr(q),
                                            L.stream_ptr()), "acr_crf_alpha_unary")
        else:
            stacks = []
            for alpha in alphas:                                 # crf_with_alpha_device's expressions, alpha by alpha
                background = np.power(1 - cams.max(axis=0, keepdims=True), alpha)
                stacks.append(np.ascontiguousarray(np.concatenate((background, cams), axis=0), dtype=np.float32))
            scores = torch.as_tensor(np.concatenate(stacks, axis=0)).reshape(groups * k, n).to(dev)
            L.check(lib.acr_crf_unary(L.ptr(scores), L.ptr(unary), groups * k * n, 1e-5, L.stream_ptr()), "acr_crf_unary")
            L.check(lib.acr_crf_update_groups(L.ptr(unary), None, None, L.ptr(q), n, k, groups, L.stream_ptr()), "acr_crf_update_groups")
        kernels = [_Kernel(PermutohedralLattice(h, w, 3, device=dev), 3),
                   _Kernel(PermutohedralLattice(h, w, 80, rgb=img, srgb=13, device=dev), 10)]
        _iterate(kernels, unary, q, int(t), n, k, groups)
    refined = q.reshape(groups * k, h, w)
    return (classes, refined, scores.reshape(groups * k, h, w)) if return_scores else (classes, refined)


# ---- unaries from a label map -----------------------------------------------------------------------------------------------
def label_energies(n_labels, gt_prob):
    """(e_label, e_other, e_unsure) of pydensecrf's ``unary_from_labels(labels, n_labels, gt_prob, zero_unsure=False)``: evaluated in
    double and rounded to float32, as numpy fills its float32 unary.  ValueError outside 2 <= n_labels <= 255, 0 < gt_prob < 1."""
    if isinstance(n_labels, bool) or not isinstance(n_labels, (int, np.integer)) or not 2 <= n_labels <= 255:
        raise ValueError("n_labels must be an integer in 2..255 (the label map is uint8), got %r" % (n_labels,))
    if not 0 < gt_prob < 1:
        raise ValueError("gt_prob must lie in (0, 1), got %r" % (gt_prob,))
    return (float(np.float32(-np.log(gt_prob))), float(np.float32(-np.log((1.0 - gt_prob) / (n_labels - 1)))),
            float(np.float32(-np.log(1.0 / n_labels))))


def _label_args(img, labels, t, n_labels, gt_prob, device):
    """The arguments of the label CRF judged (ValueError) before a device is asked for; ``img`` None: the unary alone."""
    energies = label_energies(n_labels, gt_prob)
    given = (labels, img)
    if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0:
        raise ValueError("t must be an integer >= 0, got %r" % (t,))
    if not torch.is_tensor(labels):
        labels = np.asarray(labels)
        if labels.dtype.kind not in "iu" or labels.ndim != 2 or labels.size == 0 or labels.min() < 0 or labels.max() > 255:
            raise ValueError("labels must be a non-empty (h, w) integer array with values in 0..255, got %s %s" % (labels.shape, labels.dtype))
        labels = labels.astype(np.uint8)
    labels = A.tensor_arg(labels, "labels", torch.uint8, shape=("h", "w"), upload=True, on_gpu=False)
    h, w = labels.shape
    if img is not None:
        img = A.tensor_arg(img, "img", torch.uint8, shape=(h, w, 3), upload=True, on_gpu=False)
    dev = A.first_device(given, device, "crf_inference_label")
    return energies, labels, img, dev


def label_unary_device(labels, n_labels=21, gt_prob=0.7, device="cuda"):
    """(unary, q): the (n_labels, h, w) float32 unary energies of a (h, w) label map and softmax(-unary), on the device.  A pixel's
    own label gets -log(gt_prob), every other label -log((1 - gt_prob) / (n_labels - 1)); a label >= n_labels (255 included) is
    unsure and gets -log(1 / n_labels) on every plane -- this project's extension: pydensecrf raises there."""
    (e_label, e_other, e_unsure), labels, _, dev = _label_args(None, labels, 0, n_labels, gt_prob, device)
    return _label_unary(labels, n_labels, e_label, e_other, e_unsure, dev)


def _label_unary(labels, n_labels, e_label, e_other, e_unsure, dev):
    lib = L.load()
    h, w = labels.shape
    with torch.cuda.device(dev):
        labels = A.on_device(labels, "labels", dev, upload=True)
        unary = torch.empty((n_labels, h, w), dtype=torch.float32, device=dev)
        q = torch.empty_like(unary)
        L.check(lib.acr_crf_label_unary(L.ptr(labels), h * w, n_labels, e_label, e_other, e_unsure, L.ptr(unary), L.ptr(q), L.stream_ptr()),
                "acr_crf_label_unary")
    return unary, q


def crf_inference_label(img, labels, t=10, n_labels=21, gt_prob=0.7, device="cuda"):
    """tool/imutils.py:387-400.  img (h, w, 3) uint8, labels (h, w) integers -> the refined label map, (h, w) int64 numpy array."""
    return crf_inference_label_device(img, labels, t, n_labels, gt_prob, device).cpu().numpy().astype(np.int64)


def crf_inference_label_device(img, labels, t=10, n_labels=21, gt_prob=0.7, device="cuda", return_q=False):
    """``crf_inference_label`` with the (h, w) uint8 label map left on the device: ``unary_from_labels(zero_unsure=False)``,
    ``addPairwiseGaussian(sxy=3, compat=3)``, ``addPairwiseBilateral(sxy=50, srgb=5, compat=10)``, ``t`` mean-field iterations and the
    argmax.  ``labels``: a numpy integer array or a uint8 tensor on the GPU; a value >= n_labels (255 included) marks an unsure
    pixel (all labels equally likely before the first iteration; the reference raises there).  The last iteration takes the
    argmax of the logits directly (``acr_crf_update_argmax``: no exp, no Q) -- the first index of the largest, which is
    ``np.argmax(Q)`` unless two distinct logits give probabilities that round to the same float.  ``t = 0`` is the argmax of
    softmax(-unary): the input labels when gt_prob > 1 / n_labels, with unsure pixels as 0.  ``return_q``: also run the plain
    update last and return (labels, Q (n_labels, h, w) float32)."""
    (e_label, e_other, e_unsure), labels, img, dev = _label_args(img, labels, t, n_labels, gt_prob, device)
    lib = L.load()
    h, w = labels.shape
    n = h * w
    with torch.cuda.device(dev):
        img = A.on_device(img, "img", dev, upload=True)
        unary, q = _label_unary(labels, n_labels, e_label, e_other, e_unsure, dev)
        unary, q = unary.reshape(n_labels, n), q.reshape(n_labels, n)
        out = torch.empty((h, w), dtype=torch.uint8, device=dev)
        if t == 0:
            L.check(lib.acr_crf_update_argmax(L.ptr(unary), None, None, n, n_labels, L.ptr(out), L.stream_ptr()), "acr_crf_update_argmax")
        else:
            kernels = [_Kernel(PermutohedralLattice(h, w, 3, device=dev), 3),
                       _Kernel(PermutohedralLattice(h, w, 50, rgb=img, srgb=5, device=dev), 10)]
            _iterate(kernels, unary, q, int(t) - 1, n, n_labels, 1)
            msg = [kern.apply(q) for kern in kernels]
            L.check(lib.acr_crf_update_argmax(L.ptr(unary), L.ptr(msg[0]), L.ptr(msg[1]), n, n_labels, L.ptr(out), L.stream_ptr()),
                    "acr_crf_update_argmax")
            if return_q:
                L.check(lib.acr_crf_update(L.ptr(unary), L.ptr(msg[0]), L.ptr(msg[1]), L.ptr(q), n, n_labels, L.stream_ptr()), "acr_crf_update")
    return (out, q.reshape(n_labels, h, w)) if return_q else out
