"""TEST INFRASTRUCTURE ONLY -- CPU restatement of what the shared-lattice CRF stage adds to oracle/crf_oracle.py: pydensecrf's
``unary_from_labels(zero_unsure=False)`` by its formula (the package is not installed), a mean field with free kernel parameters,
``crf_inference_label`` (tool/imutils.py:387-400) on top of both, and the scenes the CPU and GPU tests of the stage share.  The
lattice, the kernels and the normalisation are the oracle's own (``_Kernel``, ``spatial_features``, ``bilateral_features``,
``_exp_and_normalize``).  Like the oracle's mean field this part is "parity unpinned": nothing runs pydensecrf here."""
import functools

import numpy as np

from oracle.crf_oracle import _Kernel, _exp_and_normalize, bilateral_features, spatial_features

F = np.float32
LABEL_GAUSSIAN = (3, 3)                 # addPairwiseGaussian(sxy, compat) of crf_inference_label
LABEL_BILATERAL = (50, 5, 10)           # addPairwiseBilateral(sxy, srgb, compat) of crf_inference_label


def label_energies(n_labels, gt_prob):
    """(own label, other label, unsure) energies as float32, evaluated in double as numpy evaluates them before the fill."""
    return F(-np.log(gt_prob)), F(-np.log((1.0 - gt_prob) / (n_labels - 1))), F(-np.log(1.0 / n_labels))


def label_unary(labels, n_labels, gt_prob, own_ulps=0):
    """unary_from_labels(labels, n_labels, gt_prob, zero_unsure=False): (n_labels, n) float32, the own label's energy
    -log(gt_prob), every other -log((1 - gt_prob) / (n_labels - 1)).  A label >= n_labels (255 included) is unsure: -log(1 / n_labels)
    on every plane (the project's extension; pydensecrf's fancy index raises there).  ``own_ulps``: move the own-label energy by that
    many float32 ulps (the tests' probe of how far a last-bit difference travels)."""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    e_own, e_other, e_unsure = label_energies(n_labels, gt_prob)
    for _ in range(own_ulps):
        e_own = np.nextafter(e_own, F(np.inf))
    u = np.full((n_labels, lab.size), e_other, dtype=F)
    sure = lab < n_labels
    u[lab[sure], np.flatnonzero(sure)] = e_own
    u[:, ~sure] = e_unsure
    return u


def label_kernels(img):
    h, w = img.shape[:2]
    return [_Kernel(spatial_features(h, w, LABEL_GAUSSIAN[0]), LABEL_GAUSSIAN[1]),
            _Kernel(bilateral_features(img, LABEL_BILATERAL[0], LABEL_BILATERAL[1]), LABEL_BILATERAL[2])]


def mean_field(unary, kernels, t):
    """DenseCRF::inference(t) on a (K, n) float32 unary with the given kernels: Q (K, n) float32 (crf_oracle.crf_inference's loop)."""
    q = _exp_and_normalize(-unary)
    for _ in range(t):
        tmp = -unary
        for k in kernels:
            tmp = tmp + k.apply(q)
        q = _exp_and_normalize(tmp)
    return q


def crf_inference_label(img, labels, t=10, n_labels=21, gt_prob=0.7, kernels=None, own_ulps=0):
    """tool/imutils.py:387-400 -> (label map (h, w) int64, Q (n_labels, h, w) float32)."""
    h, w = img.shape[:2]
    q = mean_field(label_unary(labels, n_labels, gt_prob, own_ulps), kernels or label_kernels(img), t).reshape(n_labels, h, w)
    return np.argmax(q, axis=0), q


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def scene_image(h, w, seed):
    """The image of tests/test_crf_gpu.py::_scene (seed >= 0), or its uniform-noise image (seed < 0)."""
    if seed < 0:
        return np.random.default_rng(9).integers(0, 256, (h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 3) % 256, (yy * 2) % 256, (xx * yy) % 256], -1).astype(np.uint8)
    img[h // 4: 3 * h // 4, w // 3: 2 * w // 3] = (230, 40, 40)
    return img


def scene_cams(h, w, k, seed):
    """k CAM planes in [0, 1): noise, with the box of the scene raised in plane 0."""
    rng = np.random.default_rng(100 + abs(seed))
    cams = rng.random((k, h, w)).astype(F) * 0.4
    cams[0, h // 4: 3 * h // 4, w // 3: 2 * w // 3] += 0.55
    return cams


SCENES = ((48, 64, 0), (61, 47, 1), (33, 70, 2), (40, 52, -1))          # (h, w, seed); the last is the noise image
LABEL_SCENES = tuple(s + (k,) for s, k in zip(SCENES, (3, 5, 21, 3)))   # + n_labels


def label_scene(h, w, seed, k):
    """(img, labels uint8): a box of class 1, a band of class 2 where k > 2, 15 % of the pixels relabelled at random, 3 % unsure."""
    rng = np.random.default_rng(200 + abs(seed))
    labels = np.zeros((h, w), np.uint8)
    labels[h // 4: 3 * h // 4, w // 3: 2 * w // 3] = 1
    if k > 2:
        labels[: h // 8] = 2
    noisy = rng.random((h, w)) < 0.15
    labels[noisy] = rng.integers(0, k, int(noisy.sum()))
    labels[rng.random((h, w)) < 0.03] = 255
    return scene_image(h, w, seed), labels


@functools.lru_cache(maxsize=None)
def label_case(h, w, seed, k, t=10, gt_prob=0.7):
    """One label scene with everything the tests compare against, computed once per process and shared (treat as read-only):
    dict(img, labels, unary, ref_label, ref_q, probe, bound, margin).  ``probe``: max |dQ| when the own-label energy moves by one
    float32 ulp; ``bound`` = max(1e-4, 16 * probe), tests/test_crf_gpu.py's rule; ``margin``: the smallest top-2 margin of Q."""
    img, labels = label_scene(h, w, seed, k)
    kernels = label_kernels(img)
    ref_label, ref_q = crf_inference_label(img, labels, t, k, gt_prob, kernels)
    _, moved = crf_inference_label(img, labels, t, k, gt_prob, kernels, own_ulps=1)
    probe = float(np.abs(moved - ref_q).max())
    top = np.sort(ref_q, axis=0)
    return dict(img=img, labels=labels, unary=label_unary(labels, k, gt_prob).reshape(k, h, w), ref_label=ref_label, ref_q=ref_q,
                probe=probe, bound=max(1e-4, 16.0 * probe), margin=float((top[-1] - top[-2]).min()))
