"""Host side of the segmentation-training input pipeline: the numpy restatement (tests/segdata_ref.py) reproduces fixtures written by
the REFERENCE's own get_data_from_chunk_v4 / _v3 (tests/golden/make_segdata_golden.py), ``data.SegTrainBatcher`` draws the geometry
those fixtures encode, the C ABI is declared, bound and exported, and the product judges its arguments before the device is asked
for and refuses to run without a GPU."""
import random

import numpy as np
import pytest
import torch

import abi_checks
import segdata_ref as R
from conftest import ROOT
from segdata_ref import FIXTURES, load_fixture


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_chunk_functions(name):
    """Both sides run the same float64 path (the resize stubs ARE the restatement's resizes), so everything is exact: images,
    the truncated float32 ``ori_images``, the cropping masks and the map."""
    fx, decoded, maps, kind = load_fixture(name)
    crop, seed = int(fx["crop"]), int(fx["seed"])
    got = R.get_data_from_chunk(decoded, maps, crop, kind, random.Random(seed), np.random.RandomState(seed))
    assert fx["croppings"].shape == (crop, crop, len(decoded)) and fx["target"].shape == (len(decoded), crop, crop)
    assert np.array_equal(got["target"], fx["target"])
    assert np.array_equal(got["croppings"], fx["croppings"])
    assert np.array_equal(got["images"], fx["images"])
    assert np.array_equal(got["ori_images"], fx["ori_images"])
    # the padding of ori_images is the de-normalised zero: (123, 116, 103)
    out = fx["croppings"].transpose(2, 0, 1) == 0
    if out.any():
        assert [set(fx["ori_images"][:, c][out].tolist()) for c in range(3)] == [{123}, {116}, {103}]


def test_fixtures_cover_the_branches_the_issue_names():
    """Sources larger than the crop in both, one and no dimension; a chunk of one; an odd-sized image; v4 always pads one axis;
    v3 has a resized image larger than the crop (the crop box lies inside the image) and a padded one; both flip states."""
    seen = set()
    for name in FIXTURES:
        fx, decoded, maps, kind = load_fixture(name)
        crop, seed = int(fx["crop"]), int(fx["seed"])
        geoms = R.get_data_from_chunk(decoded, maps, crop, kind, random.Random(seed), np.random.RandomState(seed))["geoms"]
        if len(decoded) == 1:
            seen.add("chunk of one")
        for rgb, g in zip(decoded, geoms):
            h, w = rgb.shape[:2]
            seen.add("source larger in %d" % ((h > crop) + (w > crop)))
            if h % 2 and w % 2:
                seen.add("odd")
            seen.add("flip %d" % g["flip"])
            if kind == "v4":
                assert max(g["rh"], g["rw"]) == crop
            else:
                seen.add("v3 resized %s crop" % ("above" if max(g["rh"], g["rw"]) > crop else "within"))
            if g["img_top"] > 0 or g["img_left"] > 0:
                seen.add("offset into the image")
            if g["cont_top"] > 0 or g["cont_left"] > 0:
                seen.add("offset into the container")
    want = {"chunk of one", "source larger in 0", "source larger in 1", "source larger in 2", "odd", "flip 0", "flip 1",
            "v3 resized above crop", "v3 resized within crop", "offset into the image", "offset into the container"}
    assert want <= seen, want - seen


def test_nearest_rule():
    a = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)
    assert np.array_equal(R.cv2_resize_nearest(a, 7, 5), a)                              # the identity resize
    up = R.cv2_resize_nearest(a, 14, 10)
    assert np.array_equal(up, a.repeat(2, axis=0).repeat(2, axis=1))                     # floor(d / 2)
    down = R.cv2_resize_nearest(a, 3, 2)                                                 # floor(d * 7 / 3) = 0, 2, 4; floor(d * 5 / 2) = 0, 2
    assert np.array_equal(down, a[[0, 2]][:, [0, 2, 4]])


@pytest.mark.parametrize("name", FIXTURES)
def test_seg_train_batcher_draws_the_reference_geometry(name):
    """``SegTrainBatcher.draw`` on the fixture's sizes and seed: the container box equals the one the reference's croppings show."""
    from acr_wsss_amd import data
    fx, decoded, maps, kind = load_fixture(name)
    crop, seed = int(fx["crop"]), int(fx["seed"])
    b = data.SegTrainBatcher(crop, device="cuda", seed=seed, long_range=None if kind == "v4" else R.long_range(crop, "v3"))
    assert b.long_range == R.long_range(crop, kind)
    b.nprandom.uniform(0.7, 1.3)                          # the per-chunk `scale` draw (myTool.py:1260) __call__ makes
    pr, nr = random.Random(seed), np.random.RandomState(seed)
    nr.uniform(0.7, 1.3)
    for i, rgb in enumerate(decoded):
        rec = np.zeros(1, data.PRE_IMAGE)
        rec[0] = b.draw(rgb.shape[0], rgb.shape[1])
        rec = rec[0]
        ct, cl, ch, cw = R.box_of(fx["croppings"][:, :, i])
        assert (int(rec["cont_top"]), int(rec["cont_left"]), int(rec["ch"]), int(rec["cw"])) == (ct, cl, ch, cw)
        g = R.draw_geometry(rgb.shape[0], rgb.shape[1], crop, R.long_range(crop, kind), pr, nr)
        for k in ("rh", "rw", "flip", "cont_top", "cont_left", "img_top", "img_left", "ch", "cw"):
            assert int(rec[k]) == g[k], (i, k)
        assert (int(rec["h"]), int(rec["w"])) == rgb.shape[:2]


def test_symbol_is_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from acr_wsss_amd import _lib as L
    hdr = abi_checks.HEADER
    assert "myTool.py:1257-1310" in hdr and "UNPINNED" in hdr and "map_fill" in hdr
    assert "acr_preprocess_seg_batch" in L.SIGNATURES
    assert len(abi_checks.declared("acr_preprocess_seg_batch")[1]) == len(L.SIGNATURES["acr_preprocess_seg_batch"][1]) == 14
    lib = L.load()
    assert getattr(lib, "acr_preprocess_seg_batch") is not None
    # the C ABI refuses bad arguments on the host (the pointers are never dereferenced)
    import ctypes
    one = ctypes.c_void_p(8)
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    for args, word in (((None, one, one, 1, 32, f3, f3, 0, 0, one, one, one, one, None), "null pointer"),
                       ((one, one, one, 1, 32, f3, f3, 0, 0, None, one, one, one, None), "null pointer"),
                       ((one, one, one, 0, 32, f3, f3, 0, 0, one, one, one, one, None), "batch=0"),
                       ((one, one, one, 1, 0, f3, f3, 0, 0, one, one, one, one, None), "S=0"),
                       ((one, one, None, 1, 32, f3, f3, 0, 0, one, one, one, one, None), "map offsets"),
                       ((one, one, one, 1, 32, f3, f3, 0, 256, one, one, one, one, None), "map_fill=256")):
        assert lib.acr_preprocess_seg_batch(*args) == -1 and word in lib.acr_last_error().decode(), (word, lib.acr_last_error().decode())


def _good():
    from acr_wsss_amd import data
    img = np.zeros((30, 40, 3), np.uint8)
    m = np.zeros((30, 40), np.uint8)
    rec = np.zeros(1, data.PRE_IMAGE)
    rec[0] = (0, 30, 40, 24, 32, 1, 4, 0, 0, 0, 24, 32)      # 24 x 32 resized image at rows 4..27 of a 32 x 32 container
    return img, m, rec


def test_host_validation_needs_no_gpu():
    from acr_wsss_amd import data
    from acr_wsss_amd._lib import AcrHipError
    img, m, rec = _good()
    for bad_map in (np.zeros((30, 41), np.uint8),                # another size than its image
                    np.zeros((40, 30), np.uint8),
                    np.zeros((30, 40), np.int32),                # not uint8
                    np.zeros((30, 40), np.float32),
                    np.zeros((30, 40, 1), np.uint8),             # 3-D
                    np.zeros((30, 40, 3), np.uint8)):
        with pytest.raises(ValueError):
            data.preprocess_seg_batch([img], [bad_map], rec, 32, "cuda")
    for bad_img in (img.astype(np.float32), img[:, :, :2], img[:, :, 0]):
        with pytest.raises(ValueError):
            data.preprocess_seg_batch([bad_img], [m], rec, 32, "cuda")
    with pytest.raises(ValueError):
        data.preprocess_seg_batch([img, img], [m], rec, 32, "cuda")
    for field, value in (("img_top", 1),                         # rows 1..24 of a 24-row image
                         ("img_left", 1), ("cont_top", 9),       # rows 9..32 of a 32-row container
                         ("cont_left", 1), ("ch", 25), ("cw", 33), ("h", 31), ("w", 39), ("rh", 0), ("cont_top", -1), ("flip", 2)):
        bad = rec.copy()
        bad[field] = value
        with pytest.raises(AcrHipError, match="inconsistent geometry"):
            data.preprocess_seg_batch([img], [m], bad, 32, "cuda")
    for fill in (-1, 256):
        with pytest.raises(ValueError):
            data.preprocess_seg_batch([img], [m], rec, 32, "cuda", map_fill=fill)
    with pytest.raises(ValueError):
        data.preprocess_seg_batch([img], [m], rec, 32, "cuda", dtype=torch.float16)
    # well-formed arguments, no GPU device: there is no CPU path
    with pytest.raises(AcrHipError, match="no CPU path"):
        data.preprocess_seg_batch([img], [m], rec, 32, "cpu")
    with pytest.raises(ValueError):
        data.SegTrainBatcher(32, long_range=(40, 30))
    b = data.SegTrainBatcher(32, device="cpu", seed=1)
    state = b.nprandom.get_state()[1].copy()
    with pytest.raises(ValueError):
        b([img], [np.zeros((30, 41), np.uint8)], torch.zeros(1, 20))
    assert np.array_equal(b.nprandom.get_state()[1], state)      # a refused chunk consumed no draw
    with pytest.raises(AcrHipError):
        b([img], [m], torch.zeros(1, 20))


def test_chunk_loader_argument_errors(tmp_path):
    from acr_wsss_amd import data
    loader = data.ChunkLoader(str(tmp_path), {}, 32, device="cpu", workers=1)
    with pytest.raises(ValueError, match="map_dir"):
        loader.get_data_from_chunk_v4(["a"])
    with pytest.raises(ValueError, match="map_dir"):
        next(loader.iterate([["a"]], kind="v3"))
    loader.close()
    loader = data.ChunkLoader(str(tmp_path), {}, 32, device="cpu", workers=1, map_dir=str(tmp_path))
    with pytest.raises(ValueError, match="kind"):
        next(loader.iterate([["a"]], kind="v5"))
    with pytest.raises(ValueError, match="validation"):
        next(loader.iterate([["a"]], train=False, kind="v4"))
    assert loader._seg_batcher("v3").long_range == (28, 36) and loader._seg_batcher("v4").long_range == (32, 32)
    assert loader._seg_batcher("v3").pyrandom is loader.batcher.pyrandom       # one stream of draws, like the reference's globals
    loader.close()
