"""The affinity stage's input label without a GPU: the restatement (tests/affdata_ref.py) against fixtures written by the reference's
own ``VOC12AffDataset.__getitem__`` (tests/golden/make_affdata_golden.py) bit for bit, the mirrored-box identity the kernel's records
rest on, the ABI's names, and what the host refuses before any device is asked for."""
import glob
import os
import random

import numpy as np
import pytest
import torch

import abi_checks
import affdata_ref as R
import affinity_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TAGS = ("40x56_n2", "40x56_n21_flip", "80x100_n3", "80x100_n2_flip", "40x100_n3_flip", "48x57_n3", "48x57_n2_flip")


def gold(tag):
    """One fixture with its scores back as the float32 dicts the reference read: numerator / 2^10 is exact"""
    g = dict(np.load(os.path.join(GOLD, "affdata_%s.npz" % tag)))
    scale = np.float32(int(g["grid"]))
    for half in ("la", "ha"):
        g[half] = {int(k): p.astype(np.float32) / scale for k, p in zip(g["keys"], g[half + "_num"])}
    return g


def test_every_fixture_is_listed():
    assert sorted("affdata_%s.npz" % t for t in TAGS) == sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "affdata_*.npz")))
    seen = {(gold(t)["image"].shape[:2], len(gold(t)["keys"]), int(gold(t)["flip"])) for t in TAGS}
    assert {s[0] for s in seen} == {(40, 56), (80, 100), (40, 100), (48, 57)}
    assert {s[1] for s in seen} == {2, 3, 21} and {s[2] for s in seen} == {0, 1}


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_reference(tag):
    g = gold(tag)
    S, radius = int(g["S"]), int(g["radius"])
    label = R.aff_label(g["la"], g["ha"], S, S, g["box"], int(g["flip"]))
    assert label.dtype == np.uint8 and np.array_equal(label, g["label"])            # every cell, none excluded
    assert (g["label"] == 255).any() and (g["label"] == 0).any() and ((g["label"] > 0) & (g["label"] < 255)).any()
    bg, fg, neg = AR.pair_masks(torch.from_numpy(label), radius)
    for name, m in (("bg", bg), ("fg", fg), ("neg", neg)):
        assert g[name].any(), name
        assert np.array_equal(m.numpy().astype(np.uint8), g[name]), name
    # the image half of the joint transform: the reference's cropped and flipped image is what the mirrored record describes
    from acr_wsss_amd import data as D
    h, w = g["image"].shape[:2]
    rec = np.zeros(1, D.PRE_IMAGE)
    rec[0] = D.aff_record(h, w, S, *(int(v) for v in g["box"]), int(g["flip"]))
    assert np.array_equal(R.record_crop_flip(g["image"], S, S, rec[0]), g["ref_image"])
    assert np.array_equal(R.crop_flip(g["image"], S, S, g["box"], int(g["flip"])), g["ref_image"])


def test_mirrored_box_identity_for_random_boxes():
    """crop-then-flip (the reference) == flip-then-crop with cont_left' = S - cont_left - cw, img_left' = w - img_left - cw"""
    from acr_wsss_amd import data as D
    rng, py = np.random.RandomState(7), random.Random(7)
    for _ in range(200):
        S = int(rng.choice([8, 16, 64]))
        h, w = int(rng.randint(1, 2 * S + 1)), int(rng.randint(1, 2 * S + 1))
        x = rng.randint(1, 1 << 20, (h, w, 2)).astype(np.float32)
        box = D.random_crop_boxes(h, w, S, py)
        for flip in (0, 1):
            rec = np.zeros(1, D.PRE_IMAGE)
            rec[0] = D.aff_record(h, w, S, *box, flip)
            D._check_aff_records(rec, [(h, w)], S, S)
            assert np.array_equal(R.record_crop_flip(x, S, S, rec[0]), R.crop_flip(x, S, S, box, flip)), (S, h, w, box, flip)
            assert (rec[0]["cont_left"], rec[0]["img_left"]) == ((S - box[1] - box[5], w - box[3] - box[5]) if flip else (box[1], box[3]))


def test_uncropped_form_pads_like_block_reduce():
    rng = np.random.RandomState(3)
    la, ha = (rng.randint(0, 1025, (3, 37, 61)).astype(np.float32) / np.float32(1024) for _ in range(2))
    pad = [np.pad(s, ((0, 0), (0, 3), (0, 3))) for s in (la, ha)]
    want = R.label_of_pooled(R.pool8(R.stack(*pad)))
    assert want.shape == (5, 8) and np.array_equal(R.aff_label_whole(la, ha), want)


def test_abi_names_in_signatures_header_and_makefile():
    from acr_wsss_amd import _lib
    assert "voc12/data.py:241-278" in abi_checks.HEADER and "tool/imutils.py:167-190" in abi_checks.HEADER
    declared = abi_checks.PROTOTYPES
    assert "acr_aff_label_batch" in declared and "acr_aff_label_batch" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["acr_aff_label_batch"][1]) == len(abi_checks.declared("acr_aff_label_batch")[1]) == 10
    assert "acr_aff_label_ws_bytes" not in declared and "acr_aff_label_ws_bytes" not in _lib.SIGNATURES     # the kernel needs no workspace
    assert "affdata.hip" in open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "Makefile")).read()


def _batch(n=2, h=40, w=56, dtype=np.float32):
    img = np.zeros((h, w, 3), np.uint8)
    la = {k: np.zeros((h, w), dtype) for k in range(n)}
    ha = {k: np.zeros((h, w), dtype) for k in range(n)}
    return img, la, ha


def test_host_validation_errors_before_any_device():
    from acr_wsss_amd import data as D
    b = D.AffTrainBatcher(64, "cuda", seed=0)              # no device is touched before the checks have passed
    img, la, ha = _batch()
    with pytest.raises(ValueError, match="differ"):
        b([img], [la], [{0: ha[0], 5: ha[1]}])             # differing key lists
    with pytest.raises(ValueError, match="differ"):
        b([img], [la], [{1: ha[1], 0: ha[0]}])             # the same keys in another order
    with pytest.raises(ValueError, match="for an image of"):
        b([img], [{k: p[:, :55] for k, p in la.items()}], [{k: p[:, :55] for k, p in ha.items()}])     # plane shape != image's
    with pytest.raises(ValueError, match="at least 2"):
        b([img], [{0: la[0]}], [{0: ha[0]}])               # n < 2
    with pytest.raises(ValueError, match="outside 2..81"):
        b([img], [np.zeros((1, 40, 56), np.float32)], [np.zeros((1, 40, 56), np.float32)])
    with pytest.raises(ValueError, match="outside 2..81"):
        b([img], [np.zeros((82, 40, 56), np.float32)], [np.zeros((82, 40, 56), np.float32)])
    with pytest.raises(ValueError, match="float32"):
        b([img], [np.zeros((2, 40, 56), np.float64)], [np.zeros((2, 40, 56), np.float64)])             # a non-float32 stack
    with pytest.raises(ValueError, match="float32"):
        b([img], [_batch(dtype=np.float64)[1]], [ha])
    with pytest.raises(ValueError, match="multiple of 32"):
        D.AffTrainBatcher(72, "cuda", seed=0)([img], [la], [ha])                                       # S % 32 != 0
    with pytest.raises(ValueError):
        b([img, img], [la], [ha])
    state = (b.pyrandom.getstate(), b.nprandom.get_state()[1].tolist())
    with pytest.raises(ValueError):
        b([img[0]], [la], [ha])                            # a refused chunk leaves the generators alone
    assert state == (b.pyrandom.getstate(), b.nprandom.get_state()[1].tolist())
    rec = np.zeros(1, D.PRE_IMAGE)
    rec[0] = (0, 40, 56, 40, 64, 0, 0, 0, 0, 0, 40, 56)                                              # a resize: not this stage's record
    with pytest.raises(D.L.AcrHipError, match="inconsistent geometry"):
        b([img], [la], [ha], records=rec)
    from acr_wsss_amd import affinity as A
    t = torch.zeros(2, 8, 8)
    with pytest.raises(ValueError):
        A.aff_label(t, torch.zeros(3, 8, 8))
    with pytest.raises(ValueError):
        A.aff_label(t.double(), t.double())
    with pytest.raises(ValueError):
        A.aff_label(t[:1], t[:1])
    with pytest.raises(ValueError):
        A.aff_label({0: t[0], 1: t[1]}, {0: t[0], 2: t[1]})
    with pytest.raises(D.L.AcrHipError):
        A.aff_label(t, t, box=(8, 8, 0, 0, 0, 0, 8, 9, 0))                                             # the box leaves the image


def test_no_cpu_path():
    from acr_wsss_amd import affinity as A
    from acr_wsss_amd import data as D
    img, la, ha = _batch()
    with pytest.raises(D.L.AcrHipError, match="no CPU path"):
        D.AffTrainBatcher(64, "cpu", seed=0)([img], [la], [ha])
    with pytest.raises(D.L.AcrHipError):
        A.aff_label(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8))
    loader = D.ChunkLoader("/nonexistent", {}, 64, device="cpu", workers=1)
    try:
        with pytest.raises(ValueError, match="la_dir"):
            loader.get_data_from_chunk_aff(["a"])
        with pytest.raises(ValueError, match="la_dir"):
            next(loader.iterate([["a"]], kind="aff"))
    finally:
        loader.close()


def test_draws_follow_the_train_batcher_and_mirror_on_a_flip():
    from acr_wsss_amd import data as D
    b = D.AffTrainBatcher(64, "cuda", seed=11)
    py, npr = random.Random(11), np.random.RandomState(11)
    for h, w in ((40, 56), (80, 100), (40, 100), (48, 57), (64, 64)):
        got = b.draw(h, w)
        flip = int(npr.uniform(0, 1) > 0.5)
        assert got == D.aff_record(h, w, 64, *D.random_crop_boxes(h, w, 64, py), flip)
        assert got[3:5] == (h, w) and got[5] == flip
