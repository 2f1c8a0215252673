"""Host side of segmentation validation: the float64 restatement (tests/segval_ref.py) agrees with torch's CPU
``F.interpolate`` + ``softmax`` + ``argmax`` on every shape the GPU tests use, its CRF assembly reproduces ``crf_oracle.crf_inference``
exactly under that function's parameters, the C ABI is declared, bound and exported and refuses bad arguments on the host, and the
product judges its arguments before the device is asked for and refuses to run without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_checks
import segval_ref as R
from oracle import crf_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hflip", [False, True])
@pytest.mark.parametrize("scale", [1, 30])
@pytest.mark.parametrize("tag", sorted(R.SHAPES))
def test_restatement_against_torch_cpu(tag, scale, hflip):
    """torch computes in fp32, the restatement in double.  A source coordinate below n_in, formed in three fp32 roundings, is off
    by at most 2 * 2^-23 * n_in, and so is its weight; a weight error e moves a value by e * |difference of two neighbours| <=
    2 e max|logit|; the four products and three sums add 8 ulps.  Together: |dv| <= max|logit| * 2^-23 * (4 (h + w) + 8) -- loose
    (the measured figure is printed), but a wrong rule is off by the size of the logits.  A probability follows its exponent:
    |d(v_k - m)| <= 2 |dv| moves it by at most that share of itself, numerator and denominator, plus K + 4 fp32 roundings.
    Labels must agree wherever the restatement's top-two margin exceeds 2 |dv|: two values that each move by |dv| cannot swap."""
    B, K, h, w, H, W = R.SHAPES[tag]
    logits = R.logits_case(tag, scale)
    assert logits.shape == (B, K, h, w)
    ref = R.predict(logits, H, W, hflip)
    x = torch.from_numpy(logits)
    tv = F.interpolate(x.flip(-1) if hflip else x, (H, W), mode="bilinear", align_corners=False)
    tp = tv.softmax(1)
    verr = np.abs(tv.double().numpy() - ref["v"]).max()
    perr = np.abs(tp.double().numpy() - ref["p"]).max()
    vmax = np.abs(logits).max()
    print("%s x%d flip%d: torch fp32 vs restatement |dv| %.3e (max|logit| %.3e), |dp| %.3e" % (tag, scale, hflip, verr, vmax, perr))
    assert verr <= vmax * 2.0 ** -23 * (4 * (h + w) + 8)
    assert perr <= 4.0 * verr + (K + 4) * 2.0 ** -23
    np.testing.assert_allclose(ref["p"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    decided = R.top_two_margin(ref["v"]) > 2 * verr
    assert decided.mean() >= 0.995
    assert np.array_equal(tv.argmax(1).numpy()[decided], ref["label"][decided])


def test_restatement_edge_rules():
    x = np.random.default_rng(3).standard_normal((2, 5, 6, 7))
    assert np.array_equal(R.interpolate(x, 6, 7), x)                                     # the identity resize
    assert np.array_equal(R.interpolate(x, 6, 7, hflip=True), x[..., ::-1])
    one = R.interpolate(x[:, :, :1, :1], 3, 2)
    assert np.allclose(one, np.broadcast_to(x[:, :, :1, :1], one.shape), rtol=1e-15, atol=0)   # h = w = 1: the constant (weights sum to 1)
    i0, i1, lam = R.source_index(5, 37)
    assert i0.min() == 0 and i1.max() == 4 and lam.min() >= 0 and lam.max() < 1 and lam[0] == 0
    i0, i1, lam = R.source_index(40, 13)                                                 # shrinking: two neighbours, not an average
    assert np.array_equal(i1 - i0, np.ones(13)) and i1.max() <= 39
    # accumulation: the label follows the updated sum, ties go to the smallest class
    acc = np.zeros((1, 3, 1, 1))
    acc[0, 2] = 5.0
    r = R.predict(np.array([4.0, 4.0, 0.0]).reshape(1, 3, 1, 1), 1, 1)
    assert r["label"][0, 0, 0] == 0
    assert R.predict(np.array([4.0, 4.0, 0.0]).reshape(1, 3, 1, 1), 1, 1, acc=acc)["label"][0, 0, 0] == 2


def test_restated_crf_reproduces_the_oracle_under_its_parameters():
    img, probs = R.smooth_scene(17, 22, 3, 0)
    assert img.dtype == np.uint8 and probs.dtype == np.float32 and np.allclose(probs.sum(0), 1.0, atol=1e-6)
    for log_dtype in (np.float64, np.float32):
        want = C.crf_inference(img, probs, t=3, labels=3, log_dtype=log_dtype)
        got = R.crf_mean_field(img, probs, (3, 3), (80, 13, 10), t=3, labels=3, log_dtype=log_dtype)
        assert np.array_equal(got, want)
    inf = R.crf_inference_inf(img, probs, t=3, labels=3)
    assert inf.shape == (3, 17, 22) and np.allclose(inf.sum(0), 1.0, atol=1e-5) and not np.array_equal(inf, want)


def test_segpred_symbol_is_declared_bound_and_exported():
    from acr_wsss_amd import _lib as L
    assert "myTool.py:1826-1895" in abi_checks.HEADER
    assert "acr_segpred_f32" in L.SIGNATURES
    assert len(abi_checks.declared("acr_segpred_f32")[1]) == len(L.SIGNATURES["acr_segpred_f32"][1]) == 12
    assert getattr(L.load(), "acr_segpred_f32") is not None
    assert "segpred.hip" in open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "Makefile")).read()


def test_c_abi_refuses_bad_arguments_on_the_host():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    one = ctypes.c_void_p(8)                             # never dereferenced: the arguments are refused first

    def refused(args, word):
        assert lib.acr_segpred_f32(*args) == -1 and word in lib.acr_last_error().decode(), (args, lib.acr_last_error().decode())

    # (logits, B, K, h, w, H, W, hflip, accumulate, probs, label, stream)
    refused((one, 0, 21, 5, 7, 37, 41, 0, 0, one, one, None), "B=0")
    refused((one, 65536, 21, 5, 7, 37, 41, 0, 0, one, one, None), "B=65536")
    refused((one, 2, 1, 5, 7, 37, 41, 0, 0, one, one, None), "K=1")
    refused((one, 2, 129, 5, 7, 37, 41, 0, 0, one, one, None), "K=129")
    for sizes in ((0, 7, 37, 41), (5, 0, 37, 41), (5, 7, 0, 41), (5, 7, 37, 0), (-1, 7, 37, 41)):
        refused((one, 2, 21) + sizes + (0, 0, one, one, None), "empty size")
    refused((one, 1, 2, 32768, 32768, 4, 4, 0, 0, one, one, None), "logits too large")
    refused((one, 1, 2, 4, 4, 32768, 32768, 0, 0, one, one, None), "output too large")
    refused((one, 1, 128, 4, 4, 4096, 4096, 0, 0, one, one, None), "output too large")
    refused((None, 2, 21, 5, 7, 37, 41, 0, 0, one, one, None), "null pointer")
    refused((one, 2, 21, 5, 7, 37, 41, 0, 0, None, None, None), "no output")
    refused((one, 2, 21, 5, 7, 37, 41, 0, 1, None, one, None), "accumulate")


def test_python_argument_errors_and_no_cpu_path():
    from acr_wsss_amd import segval as V
    from acr_wsss_amd._lib import AcrHipError
    x = torch.zeros(2, 21, 5, 7)
    for bad in (x.numpy(), x.double(), x[:, :1], torch.zeros(2, 129, 5, 7), torch.zeros(2, 21, 5), x.transpose(2, 3)):
        with pytest.raises(ValueError):
            V.predict(bad, (37, 41))
    for bad_hw in ((37,), (0, 41), (37, -1), None):
        with pytest.raises(ValueError):
            V.predict(x, bad_hw)
    with pytest.raises(ValueError):
        V.predict(x, (37, 41), accumulate=True)                                         # nothing to add to
    with pytest.raises(ValueError):
        V.predict(x, (37, 41), want_label=False)                                        # nothing to compute
    for bad_probs in (torch.zeros(2, 21, 37, 40), torch.zeros(2, 21, 37, 41, dtype=torch.float64), np.zeros((2, 21, 37, 41), np.float32),
                      torch.zeros(2, 21, 41, 37).transpose(2, 3)):
        with pytest.raises(ValueError):
            V.predict(x, (37, 41), probs=bad_probs)
    # well-formed arguments on the CPU: there is no CPU path
    with pytest.raises(AcrHipError):
        V.predict(x, (37, 41))
    with pytest.raises(AcrHipError):
        V.predict(x, (37, 41), probs=torch.zeros(2, 21, 37, 41), accumulate=True, hflip=True)
    # validate / predict_image judge their arguments before any model or device is touched
    img = np.zeros((50, 67, 3), np.uint8)
    gt = np.zeros((50, 67), np.uint8)
    for scales in ((1.1,), (1.0, 0.7), (), (0.0,)):
        with pytest.raises(ValueError):
            V.validate(None, None, [("a", img, gt)], test_size=64, scales=scales)
        with pytest.raises(ValueError):
            V.predict_image(None, None, img, test_size=64, scales=scales)
    with pytest.raises(ValueError):
        V.validate(None, None, [("a", img, gt)], test_size=48)                          # 48 is no multiple of 32
    for bad_gt in (gt[:, :66], gt.T, gt.astype(np.int32), np.zeros((50, 67, 1), np.uint8)):
        with pytest.raises(ValueError):
            V.validate(None, None, [("a", img, bad_gt)], test_size=64)
    for bad_img in (img.astype(np.float32), img[:, :, :2], img[:, :, 0]):
        with pytest.raises(ValueError):
            V.validate(None, None, [("a", bad_img, None)], test_size=64)
        with pytest.raises(ValueError):
            V.predict_image(None, None, bad_img, test_size=64)
    with pytest.raises(ValueError):
        V.validate(None, None, [("a", img, gt)], rank=2, world=2)
    with pytest.raises(ValueError):
        V.validate(None, None, [("a", img, gt)], batch_size=0)
    # a model on the CPU: refused, no quiet fallback
    lin = torch.nn.Linear(2, 2)
    with pytest.raises(AcrHipError):
        V.validate(lin, lin, [("a", img, gt)], test_size=64)
    with pytest.raises(AcrHipError):
        V.predict_image(lin, lin, img, test_size=64)
    assert lin.training                                                                  # the mode is restored
    from acr_wsss_amd import crf
    with pytest.raises(AcrHipError):
        crf.crf_inference_inf(img, np.zeros((3, 50, 67), np.float32), labels=3, device="cpu")
    with pytest.raises(AcrHipError):
        crf.crf_inference_inf_device(img, torch.zeros(3, 50, 67), labels=3)
