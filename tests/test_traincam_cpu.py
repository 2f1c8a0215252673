"""The rule of ``acr_train_cam_f32`` without a GPU: tests/traincam_ref.py's float64 restatement against torch's float64 operators
composed as the reference composes them (compute_cam_up, myTool.py:860-864; infer_cam.py:156-162, 201-202), its float32
restatement (the kernel's arithmetic) against the float64 one, the shortcut the rule forbids, ``training_cams``' argument checks and
the C ABI's bookkeeping.  The bounds are derived below from the rounding unit and each plane's denominator, not tuned."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_checks
import traincam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("acr_train_cam_ws_bytes", "acr_train_cam_f32")
EPS = 1e-5
SHAPES = [(1, 1, 1, 1, 16, 16), (2, 3, 2, 3, 32, 48), (3, 20, 5, 7, 80, 112), (2, 80, 4, 4, 61, 37)]


make_case = R.make_case


def bounds(cam1, cam2, lab, shape, u, normalize):
    """|restatement a - restatement b| per plane, (B, C, 1, 1).  Both sample the piecewise-linear interpolant of the plane, whose
    slope per source index is at most 2 M (M = the plane's largest |value * label|): a source position computed with rounding unit
    u is off by at most 3 u g on an axis of g texels (scale, product, difference), which moves the value by 6 u g M per axis; the
    interpolation itself, the label product and the view sum commit fewer than 16 roundings of values <= M.  So per view
        ds <= M u (16 + 6 (gh + gw)).
    Normalised, out = (s - mn) / D with D = (mx - mn) + eps and 0 <= out <= 1: numerator and denominator each move by at most 2 ds,
    the subtraction, the sum with eps and the quotient round once each:
        d_out <= 4 ds / D + 4 u."""
    B, C, gh, gw, oh, ow = shape
    views = 1 if cam2 is None else 2
    M = np.abs(cam1).max(axis=1)
    if cam2 is not None:
        M = np.maximum(M, np.abs(cam2).max(axis=1))
    M = (M * np.abs(lab)).astype(np.float64)[:, :, None, None]
    ds = views * M * u * (16 + 6 * (gh + gw))
    if not normalize:
        return ds
    s = R.cams_f64(cam1, cam2, lab, (gh, gw), (oh, ow), EPS, normalize=False)
    D = (s.max(axis=(2, 3), keepdims=True) - s.min(axis=(2, 3), keepdims=True)) + float(np.float32(EPS))
    return 4 * ds / D + 4 * u


def torch_f64(cam1, cam2, lab, shape, normalize):
    B, C, gh, gw, oh, ow = shape
    label = torch.from_numpy(lab).double()

    def view(cam, flip):
        x = torch.from_numpy(cam).double().permute(0, 2, 1).reshape(B, C, gh, gw)
        up = F.interpolate(x, (oh, ow), mode="bilinear", align_corners=False) * label.clone().view(B, C, 1, 1)    # compute_cam_up
        return up.flip(-1) if flip else up                                                                           # infer_cam.py:159-160
    s = view(cam1, False)
    if cam2 is not None:
        s = s + view(cam2, True)                                                                                     # :201
    if normalize:
        mn, mx = s.amin((2, 3), keepdim=True), s.amax((2, 3), keepdim=True)
        s = (s - mn) / (mx - mn + float(np.float32(EPS)))                                                            # :202
    return s.numpy()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
def test_float64_restatement_equals_torch_float64(shape, two, normalize):
    cam1, cam2, lab = make_case(shape, 11)
    cam2 = cam2 if two else None
    got = R.cams_f64(cam1, cam2, lab, shape[2:4], shape[4:], EPS, normalize)
    ref = torch_f64(cam1, cam2, lab, shape, normalize)
    bound = bounds(cam1, cam2, lab, shape, 2.0 ** -53, normalize)
    err = np.abs(got - ref)
    print("f64 vs torch: max err %.3e, max bound %.3e" % (err.max(), bound.max()))
    assert (err <= bound).all()
    assert (got[lab == 0] == 0).all()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
def test_float32_restatement_is_within_its_rounding_of_float64(shape, two, normalize):
    cam1, cam2, lab = make_case(shape, 12)
    cam2 = cam2 if two else None
    got = R.cams_f32(cam1, cam2, lab, shape[2:4], shape[4:], EPS, normalize)
    assert got.dtype == np.float32
    ref = R.cams_f64(cam1, cam2, lab, shape[2:4], shape[4:], EPS, normalize)
    bound = bounds(cam1, cam2, lab, shape, 2.0 ** -24, normalize)
    err = np.abs(got.astype(np.float64) - ref)
    print("f32 vs f64: max err %.3e, max bound %.3e" % (err.max(), bound.max()))
    assert (err <= bound).all()
    if normalize:
        assert got.min() >= 0 and got.max() <= 1


def test_the_extremes_are_those_of_the_upsampled_plane_not_of_the_source():
    """2 x 3 -> 32 x 48 with the maximum in the middle column: no output column samples that texel's centre, so the upsampled
    maximum lies strictly below the source's, and normalising by the source's extremes is another function."""
    cam = np.array([[1.0, 5.0, 2.0], [0.5, 3.0, 1.5]], np.float32).reshape(1, 6, 1)
    lab = np.ones((1, 1), np.float32)
    s = R.cams_f32(cam, None, lab, (2, 3), (32, 48), EPS, normalize=False)
    assert s.max() < cam.max() and s.min() == cam.min()                  # the minimum sits in a corner, which IS sampled (clamped)
    rule = R.cams_f32(cam, None, lab, (2, 3), (32, 48), EPS, normalize=True)
    shortcut = ((s - cam.min()) / np.float32(np.float32(cam.max() - cam.min()) + np.float32(EPS))).astype(np.float32)
    assert rule.max() > shortcut.max() and not np.array_equal(rule, shortcut)
    assert rule.max() == np.float32(s.max() - s.min()) / np.float32(np.float32(s.max() - s.min()) + np.float32(EPS))


def test_absent_planes_are_zero_whatever_their_source_holds():
    cam1, cam2, lab = make_case((2, 3, 2, 3, 32, 48), 13)
    cam1[:, :, lab[0] == 0] = np.nan
    for normalize in (False, True):
        out = R.cams_f32(cam1[:1], cam2[:1], lab[:1], (2, 3), (32, 48), EPS, normalize)
        assert np.isfinite(out).all() and (out[lab[:1] == 0] == 0).all() and not np.signbit(out[lab[:1] == 0]).any()


def test_training_cams_checks_every_argument_before_the_library(monkeypatch):
    from acr_wsss_amd import _lib as L
    from acr_wsss_amd import traincam as T

    def no_library(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(L, "load", no_library)
    cam = torch.zeros(2, 6, 3)
    lab = torch.ones(2, 3)
    wide = torch.zeros(2, 6, 6)[:, :, ::2]                                 # class stride 2
    bad = [
        (dict(patch_cam=cam.double()), "float32"),
        (dict(patch_cam=cam.numpy()), "torch tensor"),
        (dict(patch_cam=cam[0]), "(B, N, C)"),
        (dict(patch_cam=torch.zeros(0, 6, 3)), "non-empty"),
        (dict(patch_cam=cam[:, :5]), "grid"),                               # N != gh * gw
        (dict(grid=(3, 3)), "grid"),
        (dict(grid=(0, 6)), "grid"),
        (dict(grid=(2.5, 3)), "pair of integers"),
        (dict(grid=None, out_hw=(32, 32)), "grid"),                         # the default grid (2, 2) has 4 tokens
        (dict(patch_cam=wide), "class stride 1"),
        (dict(labels=torch.ones(2, 4)), "labels"),
        (dict(labels=torch.ones(3)), "labels"),
        (dict(labels=torch.ones(2, 3, dtype=torch.complex64)), "labels"),
        (dict(patch_cam_flipped=torch.zeros(2, 6, 4)), "patch_cam_flipped"),
        (dict(patch_cam_flipped=cam.double()), "patch_cam_flipped"),
        (dict(patch_cam_flipped=cam.numpy()), "patch_cam_flipped"),
        (dict(patch_cam_flipped=torch.zeros(2, 7, 3)[:, 1:]), "strides"),   # same shape, another batch stride
        (dict(eps=0.0), "eps"),
        (dict(eps=-1e-5), "eps"),
        (dict(eps=float("nan")), "eps"),
        (dict(eps=float("inf")), "eps"),
        (dict(eps=1e-60), "eps"),                                           # 0 as float32
        (dict(eps="1e-5"), "eps"),
        (dict(normalize=2), "normalize"),
        (dict(normalize=None), "normalize"),
        (dict(out_hw=(0, 48)), "positive"),
        (dict(out_hw=(32, -1)), "positive"),
        (dict(out_hw=32), "pair of integers"),
        (dict(out_hw=(32.5, 48)), "pair of integers"),
        (dict(out_hw=(1 << 16, 1 << 15)), "supported range"),                # oh * ow = 2^31
        (dict(out=torch.zeros(2, 3, 32, 47)), "out must be"),
        (dict(out=torch.zeros(2, 3, 32, 48, dtype=torch.float64)), "out must be"),
        (dict(out=torch.zeros(2, 3, 48, 32).transpose(2, 3)), "out must be"),
        (dict(), "GPU only"),                                               # everything in order, but on the host
    ]
    for change, word in bad:
        kw = dict(patch_cam=cam, labels=lab, out_hw=(32, 48), grid=(2, 3))
        kw.update(change)
        pc, lb, hw = kw.pop("patch_cam"), kw.pop("labels"), kw.pop("out_hw")
        with pytest.raises(ValueError) as e:
            T.training_cams(pc, lb, hw, **kw)
        assert word in str(e.value), (change, str(e.value))
    big = torch.zeros(1, 1, 1).expand((1 << 22) + 1, 1, 1)                    # B * C above the launch's range, no memory behind it
    with pytest.raises(ValueError) as e:
        T.training_cams(big, torch.ones(1, 1).expand((1 << 22) + 1, 1), (16, 16))
    assert "supported range" in str(e.value)
    with pytest.raises(ValueError) as e:
        T.cam_up(cam, lab, (32, 48), grid=(2, 3))
    assert "GPU only" in str(e.value)
    with pytest.raises(TypeError):
        T.cam_up(cam, lab, (32, 48), grid=(2, 3), normalize=True)             # compute_cam_up has no normalisation


def test_symbols_are_declared_bound_and_exported():
    import subprocess
    import __graft_entry__ as g
    g.build()
    from acr_wsss_amd import _lib as L
    from acr_wsss_amd import traincam as T
    for ref in ("myTool.py:860-864", "infer_cam.py:156-162, 201-202", "WITHOUT READING ITS SOURCE", "acr_resample.h"):
        assert ref in abi_checks.HEADER, ref
    abi_checks.check_bound(NAMES, L.SIGNATURES)
    lib = L.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert hasattr(lib, name) and re.search(r" T %s$" % name, exported, flags=re.M), name
    assert "traincam.hip" in open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "traincam.hip")).read()
    assert '#include "acr_resample.h"' in src and "acr_taps_of" in src and "acr_bilerp" in src          # the shared rule, not a restatement
    assert "atomic" not in src
    assert 1 << int(re.search(r"#define TC_MAX_PLANES \(1 << (\d+)\)", src).group(1)) == T.MAX_PLANES


def test_c_abi_refuses_bad_arguments_on_the_host():
    import ctypes
    import __graft_entry__ as g
    g.build()
    from acr_wsss_amd import _lib as L
    lib = L.load()
    assert lib.acr_train_cam_ws_bytes(16, 20, 256, 256) >= 16 * 20 * 8
    assert lib.acr_train_cam_ws_bytes(1, 1, 1, 1) == 8
    for bad in ((0, 20, 16, 16), (1, 0, 16, 16), (1, 1, 0, 16), (1, 1, 16, 0), ((1 << 22) + 1, 1, 16, 16), (1, 1, 1 << 16, 1 << 15)):
        assert lib.acr_train_cam_ws_bytes(*bad) < 0, bad
    one = ctypes.c_void_p(16)                                               # never dereferenced: every call below is refused
    ok = dict(cam1=one, cam2=None, st=3, sb=18, label=one, B=2, C=3, gh=2, gw=3, oh=32, ow=48, eps=1e-5, normalize=1, ws=one,
              ws_bytes=1 << 20, out=one, stream=None)
    for change, word in ((dict(cam1=None), "null pointer"), (dict(label=None), "null pointer"), (dict(out=None), "null pointer"),
                         (dict(B=0), "supported range"), (dict(C=(1 << 22) + 1), "supported range"), (dict(oh=0), "supported range"),
                         (dict(gh=0), "bad grid"), (dict(gw=-1), "bad grid"), (dict(st=-1), "negative stride"),
                         (dict(eps=0.0), "eps"), (dict(eps=-1.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(normalize=2), "normalize"),
                         (dict(ws=None), "null workspace"), (dict(ws=ctypes.c_void_p(18)), "aligned"), (dict(ws_bytes=8), "workspace of")):
        a = dict(ok)
        a.update(change)
        rc = lib.acr_train_cam_f32(*a.values())
        assert rc < 0 and word in lib.acr_last_error().decode(), (change, rc, lib.acr_last_error().decode())
