"""The shared-lattice CRF stage without a GPU: its four entry points are declared and bound, every argument error of the new
Python functions is raised before a device is asked for (here there is none, so a ValueError proves the order), the
restatement's label unary is the formula, and the label scenes of test_crf_stage_gpu.py are decided by a margin."""
import numpy as np
import pytest
import torch

import abi_checks
import crf_stage_ref as R

NEW = ("acr_crf_alpha_unary", "acr_crf_update_groups", "acr_crf_label_unary", "acr_crf_update_argmax")


def test_prototypes_are_declared_and_bound():
    from acr_wsss_amd import _abi
    abi_checks.check_bound(NEW, _abi.prototypes)
    assert [len(abi_checks.declared(n)[1]) for n in NEW] == [10, 8, 9, 7]
    assert all(abi_checks.declared(n)[1][-1] == "void* stream" and abi_checks.declared(n)[0] == "int" for n in NEW)
    assert "IndexError" in abi_checks.HEADER and "round to the same float" in abi_checks.HEADER    # the two stated deviations


def test_argument_errors_come_before_the_device():
    from acr_wsss_amd import crf, segtrain
    from acr_wsss_amd._lib import AcrHipError
    img = np.zeros((4, 5, 3), np.uint8)
    cam = np.full((4, 5), 0.5, np.float32)
    bad = [lambda: crf.crf_with_alphas({}, (1,), img),
           lambda: crf.crf_with_alphas({1: cam}, (), img),
           lambda: crf.crf_with_alphas({1: cam}, (1, -2), img),
           lambda: crf.crf_with_alphas({1: cam}, (1, "4"), img),
           lambda: crf.crf_with_alphas({1: cam}, (1,), img, t=-1),
           lambda: crf.crf_with_alphas({1: cam}, (1,), img[:3]),
           lambda: crf.crf_with_alphas({1: cam}, (1,), img.astype(np.float32)),
           lambda: crf.crf_with_alphas_device({1: cam}, (1,), img, classes=[2]),
           lambda: crf.crf_with_alphas_device(cam[None], (1,), img),                                  # no classes
           lambda: crf.crf_with_alphas_device(cam[None], (1,), img, classes=[1, 2]),
           lambda: crf.crf_with_alphas_device(cam[None].astype(np.int32), (1,), img, classes=[1]),
           lambda: crf.crf_with_alphas_device(torch.zeros(1, 4, 5, dtype=torch.float64), (1,), img, classes=[1]),
           lambda: crf.crf_with_alphas_device(torch.zeros(4, 5, 1).permute(2, 0, 1), (1,), np.zeros((4, 6, 3), np.uint8), classes=[1]),
           lambda: crf.crf_inference_label(img, np.zeros((4, 5), np.int64), n_labels=1),
           lambda: crf.crf_inference_label(img, np.zeros((4, 5), np.int64), n_labels=256),
           lambda: crf.crf_inference_label(img, np.zeros((4, 5), np.int64), n_labels=3.0),
           lambda: crf.crf_inference_label(img, np.zeros((4, 5), np.int64), gt_prob=0.0),
           lambda: crf.crf_inference_label(img, np.zeros((4, 5), np.int64), gt_prob=1.0),
           lambda: crf.crf_inference_label(img, np.zeros((4, 5), np.int64), t=-1),
           lambda: crf.crf_inference_label(img, np.zeros((4, 5), np.float32)),
           lambda: crf.crf_inference_label(img, np.full((4, 5), 256)),
           lambda: crf.crf_inference_label(img, np.zeros((4, 6), np.int64)),
           lambda: crf.crf_inference_label_device(img, torch.zeros(4, 5, dtype=torch.int64)),
           lambda: crf.label_unary_device(np.zeros((20,), np.uint8)),
           lambda: segtrain.crf_labels(torch.zeros(2, 3, 8, 8, dtype=torch.float64), torch.zeros(2, 3), torch.zeros(2, 3, 8, 8, dtype=torch.uint8)),
           lambda: segtrain.crf_labels(torch.zeros(2, 3, 8, 8), torch.zeros(2, 3), torch.zeros(2, 3, 8, 8)),
           lambda: segtrain.crf_labels(torch.zeros(2, 3, 8, 8), torch.zeros(2, 4), torch.zeros(2, 3, 8, 8, dtype=torch.uint8))]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d raised nothing" % i)
    if not torch.cuda.is_available():                            # well-formed arguments: there is no CPU path
        for call in (lambda: crf.crf_with_alphas({1: cam}, (1, 12), img), lambda: crf.crf_inference_label(img, np.zeros((4, 5), np.int64)),
                     lambda: crf.crf_with_alphas_device(torch.zeros(1, 4, 5), (1,), img, classes=[1]),
                     lambda: segtrain.crf_labels(torch.zeros(2, 3, 8, 8), torch.zeros(2, 3), torch.zeros(2, 3, 8, 8, dtype=torch.uint8))):
            with pytest.raises(AcrHipError):
                call()


def test_label_unary_is_the_formula():
    labels = np.array([[0, 2, 255], [1, 1, 4]], np.uint8)
    for k, p in ((3, 0.7), (2, 0.5), (21, 0.9)):
        u = R.label_unary(labels, k, p)
        assert u.shape == (k, 6) and u.dtype == np.float32
        for i, lab in enumerate(labels.reshape(-1)):
            for j in range(k):
                if lab >= k:
                    want = -np.log(1.0 / k)
                else:
                    want = -np.log(p) if j == lab else -np.log((1.0 - p) / (k - 1))
                assert u[j, i] == np.float32(want)
        sure = labels.reshape(-1) < k
        assert np.allclose(np.exp(-u.astype(np.float64)).sum(0)[sure], 1.0, atol=1e-6)        # a distribution per sure pixel
    from acr_wsss_amd.crf import label_energies
    assert label_energies(21, 0.7) == tuple(float(e) for e in R.label_energies(21, 0.7))


@pytest.mark.parametrize("scene", R.LABEL_SCENES + ((48, 64, 0, 2),))
def test_label_scenes_are_decided_by_a_margin(scene):
    """What lets test_crf_stage_gpu.py demand equal labels at every pixel: each pixel's top-2 margin of the restatement's Q exceeds
    twice the bound on |dQ|; and the CRF changes labels, so that test is not vacuous."""
    h, w, seed, k = scene
    c = R.label_case(h, w, seed, k)
    print("\nlabel scene %dx%d, %d labels: margin %.2e, one-ulp probe %.2e, bound %.2e" % (h, w, k, c["margin"], c["probe"], c["bound"]))
    assert c["bound"] == max(1e-4, 16.0 * c["probe"]) and c["margin"] > 2 * c["bound"]
    assert (c["ref_label"] != np.where(c["labels"] < k, c["labels"], 0)).mean() > 0.01
    assert np.allclose(c["ref_q"].sum(axis=0), 1.0, atol=1e-5) and (c["labels"] == 255).any()
