"""``traincam.training_cams`` (``acr_train_cam_f32``) on the device, bit for bit: against tests/traincam_ref.py's float32 restatement
of the rule, against the existing ``acr_bilinear_resize`` (both apply csrc/acr_resample.h), on the planes where a reduction or a
fill can go wrong, and against itself."""
import functools

import numpy as np
import pytest
import torch

import traincam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
# (B, C, gh, gw, oh, ow): one pixel source; two slabs' worth of nothing; several planes per image; odd sizes, a width that is no
# multiple of 4 (the 4-byte store path) and the COCO class count; one production-size image (50 slabs per plane); and a five-fold
# REDUCTION whose slab reads 77 source rows of 80 -- more than the kernel stages in LDS, so its taps come from global memory
SHAPES = [(1, 1, 1, 1, 16, 16), (2, 3, 2, 3, 32, 48), (3, 20, 5, 7, 80, 112), (2, 80, 4, 4, 61, 37), (1, 20, 28, 28, 448, 448),
          (1, 2, 80, 80, 16, 16)]


@functools.lru_cache(maxsize=None)
def case(shape):
    return R.make_case(shape, 21 + shape[1])


@functools.lru_cache(maxsize=None)
def expected(shape, two, normalize):
    cam1, cam2, lab = case(shape)
    out = R.cams_f32(cam1, cam2 if two else None, lab, shape[2:4], shape[4:], EPS, normalize)
    out.setflags(write=False)
    return out


def embedded(cam, skip):
    """cam (B, N, C) on the device as it lies (skip 0) or as the slice [:, skip:] of a (B, skip + N, C) tensor whose leading
    tokens hold NaN: they must not be read"""
    t = torch.from_numpy(cam).to(DEV)
    if skip == 0:
        return t
    full = torch.full((cam.shape[0], skip + cam.shape[1], cam.shape[2]), float("nan"), device=DEV)
    full[:, skip:] = t
    return full[:, skip:]


def same_bytes(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    if got.tobytes() != want.tobytes():
        diff = got.view(np.uint32) != want.view(np.uint32)
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError("%d of %d values differ, first at %s: %r != %r" % (diff.sum(), diff.size, at, got[at], want[at]))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
def test_equals_the_float32_restatement_bit_for_bit(shape, two, normalize):
    from acr_wsss_amd import traincam as T
    cam1, cam2, lab = case(shape)
    want = expected(shape, two, normalize)
    labels = torch.from_numpy(lab).to(DEV)
    for skip in (0, 1, 2):
        got = T.training_cams(embedded(cam1, skip), labels, shape[4:], grid=shape[2:4], eps=EPS, normalize=normalize,
                              patch_cam_flipped=embedded(cam2, skip) if two else None)
        same_bytes(got, want)


@pytest.mark.parametrize("shape", SHAPES[1:4])
def test_cam_up_equals_the_existing_resize_kernel(shape):
    """normalize=False against ``ops.bilinear_resize(channels_last=True, chan_mul=label[b])`` per image, view 2 by the
    ``hflip=True, out=`` accumulating call (infer_cam.py:156-162 as infer_cam.py runs it)"""
    from acr_wsss_amd import ops
    from acr_wsss_amd import traincam as T
    B, C, gh, gw, oh, ow = shape
    cam1, cam2, lab = case(shape)
    d1, d2, labels = torch.from_numpy(cam1).to(DEV), torch.from_numpy(cam2).to(DEV), torch.from_numpy(lab).to(DEV)
    for two in (False, True):
        got = T.cam_up(d1, labels, (oh, ow), grid=(gh, gw), patch_cam_flipped=d2 if two else None)
        for b in range(B):
            ref = ops.bilinear_resize(d1[b].reshape(gh, gw, C).contiguous(), (oh, ow), False, chan_mul=labels[b], channels_last=True)
            if two:
                ops.bilinear_resize(d2[b].reshape(gh, gw, C).contiguous(), (oh, ow), False, chan_mul=labels[b], hflip=True, out=ref,
                                    channels_last=True)
            same_bytes(got[b], ref.cpu().numpy())


@pytest.mark.parametrize("shape", [(1, 3, 2, 3, 32, 48), (1, 3, 4, 4, 61, 37), (1, 3, 28, 28, 448, 448)])
def test_zero_constant_absent_and_corner_planes(shape):
    """class 0: present, source all zero -> +0.  class 1: ABSENT, source NaN -> +0.  class 2: present, its maximum 8 at texel
    (gh - 1, gw - 1) and its minimum 0.25 at (0, 0), both powers of two, so both corners of the upsampled plane hold them exactly
    (a clamped tap pair has weights hx + lx = 1 and the products are exact): out[0, 0] == 0 and out[-1, -1] == D / (D + eps) --
    the extremes' reduction covers the first and the last element, row and column.  A second call with a constant plane."""
    from acr_wsss_amd import traincam as T
    B, C, gh, gw, oh, ow = shape
    rng = np.random.default_rng(5)
    cam = np.zeros((1, gh * gw, 3), np.float32)
    cam[0, :, 1] = np.nan
    plane = (0.5 + rng.random(gh * gw)).astype(np.float32)               # in [0.5, 1.5)
    plane[0], plane[-1] = 0.25, 8.0
    cam[0, :, 2] = plane
    lab = np.array([[1, 0, 1]], np.float32)
    out = T.training_cams(torch.from_numpy(cam).to(DEV), torch.from_numpy(lab).to(DEV), (oh, ow), grid=(gh, gw), eps=EPS).cpu().numpy()
    zero = np.zeros((oh, ow), np.float32).tobytes()
    assert out[0, 0].tobytes() == zero and out[0, 1].tobytes() == zero   # +0 everywhere, bit for bit
    same_bytes(torch.from_numpy(out), R.cams_f32(cam, None, lab, (gh, gw), (oh, ow), EPS, True))
    D = np.float32(8.0) - np.float32(0.25)
    assert out[0, 2, 0, 0] == 0 and out[0, 2, -1, -1] == D / np.float32(D + np.float32(EPS))
    assert out[0, 2].max() == out[0, 2, -1, -1] and out[0, 2].min() == 0
    raw = T.cam_up(torch.from_numpy(cam).to(DEV), torch.from_numpy(lab).to(DEV), (oh, ow), grid=(gh, gw)).cpu().numpy()
    assert raw[0, 2, 0, 0] == np.float32(0.25) and raw[0, 2, -1, -1] == np.float32(8.0) and raw[0, 1].tobytes() == zero
    flat = np.full((1, gh * gw, 3), 3.0, np.float32)                       # constant planes, both views: s - mn == 0 everywhere
    d = torch.from_numpy(flat).to(DEV)
    const = T.training_cams(d, torch.ones(1, 3, device=DEV), (oh, ow), grid=(gh, gw), patch_cam_flipped=d, eps=EPS).cpu().numpy()
    assert const.tobytes() == np.zeros((1, 3, oh, ow), np.float32).tobytes()


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]])
def test_out_is_fully_overwritten_and_a_second_call_gives_the_same_bytes(shape):
    from acr_wsss_amd import traincam as T
    B, C, gh, gw, oh, ow = shape
    cam1, cam2, lab = case(shape)
    d1, d2, labels = torch.from_numpy(cam1).to(DEV), torch.from_numpy(cam2).to(DEV), torch.from_numpy(lab).to(DEV)
    for normalize in (False, True):
        outs = []
        for _ in range(2):
            out = torch.full((B, C, oh, ow), float("nan"), device=DEV)
            ret = T.training_cams(d1, labels, (oh, ow), grid=(gh, gw), patch_cam_flipped=d2, eps=EPS, normalize=normalize, out=out)
            assert ret is out and torch.isfinite(out).all()
            outs.append(out.cpu().numpy())
        assert outs[0].tobytes() == outs[1].tobytes()
        same_bytes(torch.from_numpy(outs[0]), expected(shape, True, normalize))


def test_labels_of_any_real_dtype_and_inputs_with_grad():
    """labels as the loader hands them (uint8, bool, float64, a host array) multiply as float32; the result is no part of the graph"""
    from acr_wsss_amd import traincam as T
    shape = SHAPES[1]
    cam1, _, lab = case(shape)
    want = expected(shape, False, True)
    d1 = torch.from_numpy(cam1).to(DEV).requires_grad_(True)
    for labels in (torch.from_numpy(lab).to(DEV).to(torch.uint8), torch.from_numpy(lab).to(DEV).bool(), torch.from_numpy(lab).double(), lab):
        got = T.training_cams(d1, labels, shape[4:], grid=shape[2:4], eps=EPS)
        assert not got.requires_grad
        same_bytes(got, want)
