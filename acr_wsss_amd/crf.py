"""Dense-CRF refinement of CAMs on the GPU: the host mirror of ``imutils.crf_inference``
(tool/imutils.py:345-362 -- pydensecrf's ``DenseCRF2D`` with ``addPairwiseGaussian(sxy=3, compat=3)``,
``addPairwiseBilateral(sxy=80, srgb=13, compat=10)`` and ``inference(t)``), of ``imutils.crf_inference_inf`` (:365-384, the
validation's parameter set: bilateral sxy=83, srgb=5, compat=4) and of ``_crf_with_alpha``
(infer_cam.py:27-40), same names, arguments and return layout.  All arithmetic runs in csrc/crf.hip behind the C ABI
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
