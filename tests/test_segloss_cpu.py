"""Host side of the pseudo-label segmentation loss: the float64 restatement (tests/segloss_ref.py) reproduces what torch's CPU
kernels and the reference's own SegmentationLosses gave (tests/golden/segloss_{a..c}.npz, written by
tests/golden/make_segloss_golden.py) and is consistent with itself (its gradient is the derivative of its loss), the C ABI is
declared, bound and exported, arguments are judged before the device is asked for, and the product refuses to run without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_checks
import segloss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = {"a": (2, 21, 5, 7, 37, 41), "b": (1, 2, 1, 1, 3, 2), "c": (3, 21, 9, 4, 70, 33)}
NAMES = ("acr_segloss_ws_bytes", "acr_segloss_fwd", "acr_segloss_bwd", "acr_dense_energy_dot")
# fixtures are fp32 results; the restatement is float64.  A log-softmax over K <= 21 terms and a mean over n <= 7000 pixels in
# fp32 stay within (K + log2 n) * 2^-24 < 35 * 6e-8 of the value: 4e-6 relative covers it, and a wrong rule is off by percents
RTOL = 4e-6


def _load(tag):
    z = np.load(os.path.join(GOLDEN, "segloss_%s.npz" % tag))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_restatement_reproduces_torch_and_the_reference(tag):
    g = _load(tag)
    B, K, h, w, W, H = SHAPES[tag]
    assert g["logits"].shape == (B, K, h, w) and g["logits"].dtype == np.float32
    assert g["label"].shape == (B, W, H) and g["label"].dtype == np.uint8
    for ba in (0, 1):
        r = R.split_ce(g["logits"], g["label"], bool(ba))
        for name in ("celoss", "bg", "fg"):
            want = float(g["%s_ba%d" % (name, ba)])
            print("segloss_%s ba%d %s: %.9g vs torch %.9g (rel %.2e)" % (tag, ba, name, r[name], want, abs(r[name] - want) / abs(want)))
            assert abs(r[name] - want) <= RTOL * abs(want)
        d = g["d_logits_ba%d" % ba]
        assert d.shape == g["logits"].shape and np.abs(d).max() > 0
        assert np.abs(r["d_logits"] - d).max() <= RTOL * np.abs(d).max()
        np.testing.assert_array_equal(r["counts"][B], g["counts"])
    assert float(g["celoss_ba0"]) == pytest.approx(B * float(g["celoss_ba1"]), rel=1e-6)
    if tag != "b":                                       # the fixtures exercise the ignore rules
        lab = g["label"]
        assert (lab == 255).any() and ((lab >= K) & (lab < 255)).any() and (lab == 0).any()


def test_restatement_gradient_is_the_derivative_of_its_loss():
    """central differences in float64 on the restatement itself: the cross-entropy part under output gradients g, and the d_probs
    path against sum(probs * d_probs)"""
    rng = np.random.default_rng(5)
    B, K, h, w, W, H = 2, 4, 3, 2, 7, 5
    x = rng.standard_normal((B, K, h, w))
    lab = R.labels_case(rng, B, K, W, H)
    dp = rng.standard_normal((B, K, W, H))
    g = (0.5, 2.0, -1.0)
    for ba in (False, True):
        def f(x):
            r = R.split_ce(x, lab, ba)
            return g[0] * r["celoss"] + g[1] * r["bg"] + g[2] * r["fg"] + (r["probs"] * dp).sum()
        d = R.split_ce(x, lab, ba, g=g, d_probs=dp)["d_logits"]
        num = np.zeros_like(x)
        for i in np.ndindex(*x.shape):
            e = np.zeros_like(x)
            e[i] = 1e-6
            num[i] = (f(x + e) - f(x - e)) / 2e-6
        assert np.abs(num - d).max() <= 1e-7 * max(1.0, np.abs(d).max())


def test_restatement_edge_rules():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((1, 3, 2, 2))
    r = R.split_ce(x, R.labels_case(rng, 1, 3, 4, 4, "bg"))
    assert np.isnan(r["fg"]) and np.isnan(r["celoss"]) and np.isfinite(r["bg"]) and np.isfinite(r["d_logits"]).all()
    r = R.split_ce(x, R.labels_case(rng, 1, 3, 4, 4, "ignore"))
    assert np.isnan(r["bg"]) and np.isnan(r["fg"]) and not r["d_logits"].any() and not r["counts"].any()
    lab = R.labels_case(rng, 1, 3, 4, 4)
    lab[0, 0, 0] = 100
    lab2 = lab.copy()
    lab2[lab >= 3] = 255
    assert R.split_ce(x, lab)["celoss"] == R.split_ce(x, lab2)["celoss"]
    # the identity resize leaves the logits alone; the bilinear rows sum to one; nearest picks torch's pixel
    assert np.array_equal(R.upsample(x, 2, 2), x)
    assert np.allclose(R.bilinear_matrix(5, 37).sum(axis=1), 1.0, atol=1e-6)
    assert R.nearest_index(33, 16).tolist() == [int(np.floor(i * 33 / 16)) for i in range(16)]
    E, dE = R.energy(np.ones((2, 3, 4, 5)), 2 * np.ones((2, 3, 4, 5)), 0.5)
    assert E == -0.25 * 240 and (dE == -1.0).all()


def test_segloss_symbols_are_declared_bound_and_exported():
    from acr_wsss_amd import _lib as L
    hdr = abi_checks.HEADER
    assert "myTool.py:825-857" in hdr and "tool/loss.py:21-33" in hdr and "bilateralfilter.cpp:42-55" in hdr
    lib = L.load()
    for name in NAMES:
        assert name in L.SIGNATURES
        assert len(abi_checks.declared(name)[1]) == len(L.SIGNATURES[name][1]), name       # one ctypes type per declared parameter
        assert getattr(lib, name) is not None
    assert abi_checks.defined("ACR_DENSE_ENERGY_WS_BYTES") == "2048"
    src = open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "Makefile")).read()
    assert "segloss.hip" in src


def test_c_abi_refuses_bad_arguments_on_the_host():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    ok = lib.acr_segloss_ws_bytes(2, 21, 5, 7, 37, 41)
    assert ok >= 4 * 2 * 37 * 41 and lib.acr_segloss_ws_bytes(16, 21, 112, 112, 448, 448) > ok
    for bad in ((0, 21, 5, 7, 37, 41), (2, 1, 5, 7, 37, 41), (2, 129, 5, 7, 37, 41), (2, 21, 38, 7, 37, 41), (2, 21, 5, 42, 37, 41),
                (2, 21, 0, 7, 37, 41), (1, 21, 5, 7, 65536, 65536)):
        assert lib.acr_segloss_ws_bytes(*bad) < 0, bad
    one = ctypes.c_void_p(8)                             # never dereferenced: the arguments are refused first

    def refused(rc, word):
        assert rc == -1 and word in lib.acr_last_error().decode(), lib.acr_last_error().decode()

    refused(lib.acr_segloss_fwd(one, one, 2, 1, 5, 7, 37, 41, 0, one, 1 << 20, None, None, one, one, one, None), "K=1")
    refused(lib.acr_segloss_fwd(one, one, 2, 21, 38, 7, 37, 41, 0, one, 1 << 20, None, None, one, one, one, None), "no larger")
    refused(lib.acr_segloss_fwd(None, one, 2, 21, 5, 7, 37, 41, 0, one, 1 << 20, None, None, one, one, one, None), "null pointer")
    refused(lib.acr_segloss_fwd(one, one, 2, 21, 5, 7, 37, 41, 0, one, 8, None, None, one, one, one, None), "needed")
    refused(lib.acr_segloss_bwd(one, one, one, one, one, None, None, 2, 200, 5, 7, 37, 41, 0, None, 0, one, None), "K=200")
    refused(lib.acr_segloss_bwd(one, one, None, one, one, None, None, 2, 21, 5, 7, 37, 41, 0, None, 0, one, None), "null pointer")
    refused(lib.acr_segloss_bwd(one, one, one, one, one, None, one, 2, 21, 5, 7, 37, 41, 0, one, 1 << 20, one, None), "d_probs")
    refused(lib.acr_dense_energy_dot(one, one, 0, 1.0, None, one, 2048, one, None), "count")
    refused(lib.acr_dense_energy_dot(one, one, 10, 1.0, None, one, 2047, one, None), "needed")
    refused(lib.acr_dense_energy_dot(one, None, 10, 1.0, None, one, 2048, one, None), "null pointer")


def test_python_argument_errors_and_no_cpu_path():
    from acr_wsss_amd import segloss as S
    from acr_wsss_amd._lib import AcrHipError
    x = torch.zeros(2, 21, 5, 7)
    lab = np.zeros((2, 37, 41), np.uint8)
    for bad_x in (torch.zeros(2, 1, 5, 7), torch.zeros(2, 129, 5, 7), torch.zeros(2, 21, 5), x.double(), x.numpy()):
        with pytest.raises(ValueError):
            S.split_cross_entropy(bad_x, lab)
    for bad_lab in (lab.astype(np.int64), lab[:1], lab[:, :4], lab[:, :, :6], torch.zeros(2, 37, 41, dtype=torch.int64)):
        with pytest.raises(ValueError):
            S.split_cross_entropy(x, bad_lab)
    with pytest.raises(ValueError):
        S.DenseEnergyLoss(1.0, 15.0, 100.0, 0.0)
    with pytest.raises(ValueError):
        S.DenseEnergyLoss(1.0, 0.0, 100.0, 1.0)
    # well-formed arguments on the CPU: there is no CPU path
    with pytest.raises(AcrHipError):
        S.split_cross_entropy(x, lab)
    with pytest.raises(AcrHipError):
        S.split_cross_entropy(x, torch.from_numpy(lab), batch_average=True)
    layer = S.DenseEnergyLoss(1.0, 15.0, 100.0, 0.5)
    with pytest.raises(AcrHipError):
        layer(np.zeros((2, 3, 37, 41), np.uint8), torch.zeros(2, 21, 37, 41), np.ones((2, 37, 41), np.float32), lab)
    with pytest.raises(AcrHipError):
        S.joint_loss(np.zeros((2, 3, 37, 41), np.uint8), x, lab, np.ones((37, 41, 2)), False, layer)
