"""The affinity stage's input on the GPU (csrc/affdata.hip behind ``data.AffTrainBatcher``, ``affinity.aff_label`` and
``ChunkLoader.get_data_from_chunk_aff``): EXACT equality, every cell, with the fixtures the reference's ``VOC12AffDataset.__getitem__``
wrote (tests/golden/make_affdata_golden.py) and with the numpy restatement (tests/affdata_ref.py) on inputs that are 0 or lie in
[2^-20, 1], where a double sum of 64 fp32 values is exact in any order -- so no tolerance and no excluded cell anywhere."""
import ctypes
import os

import numpy as np
import pytest
import torch

import affdata_ref as R
import affinity_ref as AR
from conftest import load_golden
from recipe import recipe_tensor
from test_affdata_cpu import TAGS, gold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 64
T = np.float32(1e-5)


def _records(D, shapes, boxes, flips, size=S):
    rec = np.zeros(len(shapes), D.PRE_IMAGE)
    for i, ((h, w), box, flip) in enumerate(zip(shapes, boxes, flips)):
        rec[i] = D.aff_record(h, w, size, *(int(v) for v in box), int(flip))
    return rec


def test_fixtures_label_masks_and_images():
    from acr_wsss_amd import affinity as A
    from acr_wsss_amd import data as D
    gs = [gold(t) for t in TAGS]                                   # ONE batch: mixed sizes, mixed n, both flips
    images = [g["image"] for g in gs]
    rec = _records(D, [g["image"].shape[:2] for g in gs], [g["box"] for g in gs], [g["flip"] for g in gs])
    batcher = D.AffTrainBatcher(S, DEV, seed=0)
    out, label = batcher(images, [g["la"] for g in gs], [g["ha"] for g in gs], records=rec)
    assert tuple(out.shape) == (len(gs), 3, S, S) and tuple(label.shape) == (len(gs), 8, 8) and label.dtype == torch.uint8
    assert torch.equal(out, D.preprocess_batch(images, rec, S, DEV))
    radius = int(gs[0]["radius"])
    codes, counts = A.pair_codes(label, radius, 1)
    for i, (tag, g) in enumerate(zip(TAGS, gs)):
        assert np.array_equal(label[i].cpu().numpy(), g["label"]), tag
        assert np.array_equal(codes[i].cpu().numpy(), g["bg"] + 2 * g["fg"] + 3 * g["neg"]), tag
        # the image is the reference's cropped and flipped one, normalised: an identity resize samples exactly
        mean, std = (np.asarray(v, np.float32).reshape(3, 1, 1) for v in (D.MEAN, D.STD))
        inside = R.crop_flip(np.ones_like(g["image"]), S, S, g["box"], int(g["flip"])).transpose(2, 0, 1) > 0
        want = np.where(inside, (g["ref_image"].transpose(2, 0, 1).astype(np.float32) / np.float32(255) - mean) / std, np.float32(0))
        assert np.array_equal(out[i].cpu().numpy(), want), tag
    assert counts.tolist() == [sum(int(g[k].sum()) for g in gs) for k in ("bg", "fg", "neg")]


def _exact_scores(rng, n, h, w):
    """(n, h, w) float32 values that are 0 or in [2^-20, 1]"""
    x = rng.rand(n, h, w).astype(np.float32)
    x[x < np.float32(2.0 ** -20)] = 0
    x[rng.rand(n, h, w) < 0.2] = 0
    return x


def _cell(x, k, gy, gx, v):
    x[k, 8 * gy:8 * gy + 8, 8 * gx:8 * gx + 8] = v


def _crafted(rng, flip):
    """A 64 x 64 image taken whole (container = image, mirrored under a flip; a cell keeps its values) with n = 3 and the cells:
    (0,0) la planes 1 < 2 by one ulp of the mean    (0,1) la planes 1 > 2 by one ulp    (0,2) ha planes 0 > 1 by one ulp
    (1,0) la planes 1 = 2 tie                       (1,1) la planes 0 = 1 = 2 tie       (1,2) ha planes 0 = 2 tie
    (2,0) max mean nextafter(1e-5f, -inf)           (2,1) max mean 1e-5f exactly         (2,2) max mean nextafter(1e-5f, +inf)
    (3,0) every plane 0"""
    la, ha = _exact_scores(rng, 3, 64, 64) * np.float32(0.25), _exact_scores(rng, 3, 64, 64) * np.float32(0.25)
    v = np.float32(0.7310791)
    up = np.nextafter(v, np.float32(2))
    _cell(la, 1, 0, 0, v), _cell(la, 2, 0, 0, up)
    _cell(la, 1, 0, 1, up), _cell(la, 2, 0, 1, v)
    _cell(ha, 0, 0, 2, up), _cell(ha, 1, 0, 2, v)
    tie = _exact_scores(rng, 1, 8, 8)[0] * np.float32(0.5) + np.float32(0.5)
    _cell(la, 1, 1, 0, tie), _cell(la, 2, 1, 0, tie)
    for k in range(3):
        _cell(la, k, 1, 1, tie[::-1].copy())
    _cell(ha, 0, 1, 2, tie), _cell(ha, 2, 1, 2, tie)
    for gy, gx in ((0, 0), (0, 1), (1, 0), (1, 1)):               # these cells are decided by la: ha = 1 there
        _cell(ha, 1, gy, gx, np.float32(0.9))
    for gx, t in enumerate((np.nextafter(T, np.float32(0)), T, np.nextafter(T, np.float32(1)))):
        for k in range(3):
            _cell(la, k, 2, gx, 0), _cell(ha, k, 2, gx, 0)
        _cell(la, 1, 2, gx, t)                                     # the maximum of all six planes
        _cell(ha, 2, 2, gx, np.float32(2.0 ** -18))                # ha = 2, la = 1: label 1 with a score, 255 without
    for k in range(3):
        _cell(la, k, 3, 0, 0), _cell(ha, k, 3, 0, 0)
    return la, ha, (0, 0, 0, 0, 64, 64), flip


def _cases():
    rng = np.random.RandomState(20)
    cases = [_crafted(rng, 0), _crafted(rng, 1)]
    for flip in (0, 1):                                            # smaller than S in both axes, odd w, every side of the box cuts a cell
        cases.append((_exact_scores(rng, 4, 37, 43), _exact_scores(rng, 4, 37, 43), (5, 3, 0, 0, 37, 43), flip))
        cases.append((_exact_scores(rng, 2, 33, 57), _exact_scores(rng, 2, 33, 57), (31, 7, 0, 0, 33, 57), flip))
        cases.append((_exact_scores(rng, 3, 80, 101), _exact_scores(rng, 3, 80, 101), (0, 0, 3, 27, 64, 64), flip))     # larger in both
        cases.append((np.ones((2, 1, 1), np.float32), _exact_scores(rng, 2, 1, 1), (13, 27, 0, 0, 1, 1), flip))         # a 1 x 1 box
        cases.append((_exact_scores(rng, 5, 37, 43), _exact_scores(rng, 5, 37, 43), (63, 0, 20, 41, 1, 1), flip))
    cases.append((_exact_scores(rng, 2, 40, 56), _exact_scores(rng, 2, 40, 56), (24, 8, 0, 0, 40, 56), 1))              # n = 2
    cases.append((_exact_scores(rng, 81, 40, 56), _exact_scores(rng, 81, 40, 56), (11, 5, 0, 0, 40, 56), 0))            # n = 81
    return cases


@pytest.fixture(scope="module")
def adversarial():
    """the cases and the restatement's labels, computed once"""
    cases = _cases()
    return cases, [R.aff_label(la, ha, S, S, box, flip) for la, ha, box, flip in cases]


def test_adversarial_cells_equal_the_restatement_exactly(adversarial):
    from acr_wsss_amd import data as D
    cases, want = adversarial
    for i in (0, 1):                                               # the crafted cells decide as they were built to
        w = want[i] if i == 0 else want[i][:, ::-1]
        assert w[0, :3].tolist() == [2, 1, 0] and w[1, :3].tolist() == [1, 255, 0] and w[2, :3].tolist() == [255, 1, 1] and w[3, 0] == 255
    assert {len(c[0]) for c in cases} >= {2, 3, 4, 5, 81}          # one batch mixes the plane counts
    rec = _records(D, [c[0].shape[1:] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    images = [np.zeros(c[0].shape[1:] + (3,), np.uint8) for c in cases]
    first = D.preprocess_aff_batch(images, [c[0] for c in cases], [c[1] for c in cases], rec, S, DEV)[1]
    again = D.preprocess_aff_batch(images, [c[0] for c in cases], [c[1] for c in cases], rec, S, DEV)[1]
    got = first.cpu().numpy()
    for i, (c, w) in enumerate(zip(cases, want)):
        assert np.array_equal(got[i], w), (i, c[2], c[3], np.argwhere(got[i] != w).tolist())
    assert got.tobytes() == again.cpu().numpy().tobytes()          # two calls give identical bytes
    # a sample's label does not depend on its batch
    alone = D.preprocess_aff_batch(images[3:4], [cases[3][0]], [cases[3][1]], rec[3:4], S, DEV)[1]
    assert np.array_equal(alone[0].cpu().numpy(), want[3])


def test_uncropped_form_is_the_zero_padded_container():
    from acr_wsss_amd import affinity as A
    rng = np.random.RandomState(21)
    la, ha = _exact_scores(rng, 4, 37, 61), _exact_scores(rng, 4, 37, 61)
    pad = [np.pad(s, ((0, 0), (0, 3), (0, 3))) for s in (la, ha)]
    want = R.label_of_pooled(R.pool8(R.stack(*pad)))
    got = A.aff_label(torch.from_numpy(la).to(DEV), torch.from_numpy(ha).to(DEV))
    assert tuple(got.shape) == (5, 8) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    keys = [0, 3, 9, 15]
    as_dict = A.aff_label({k: p for k, p in zip(keys, la)}, {k: torch.from_numpy(p).to(DEV) for k, p in zip(keys, ha)})
    assert np.array_equal(as_dict.cpu().numpy(), want)
    boxed = A.aff_label(torch.from_numpy(la).to(DEV), torch.from_numpy(ha).to(DEV), box=(S, 2 * S, 9, 70, 0, 0, 37, 50, 1))
    flipped = [np.ascontiguousarray(s[:, :, ::-1]) for s in (la, ha)]
    assert np.array_equal(boxed.cpu().numpy(), R.aff_label(*flipped, S, 2 * S, (9, 70, 0, 0, 37, 50), 0))


def test_entry_point_only_enqueues_on_the_callers_stream(adversarial):
    """acr_aff_label_batch allocates nothing and does not synchronise: captured once into a graph, replayed on new score values to the
    bytes of the eager launch, and it refuses what its contract excludes without launching"""
    from acr_wsss_amd import _lib as L
    from acr_wsss_amd import data as D
    lib = L.load()
    cases, want = adversarial
    la, ha, box, flip = cases[2]
    n, h, w = la.shape
    rec = _records(D, [(h, w)], [box], [flip])
    table = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV)
    offs = torch.tensor([0, 4 * n * h * w], dtype=torch.int64, device=DEV)
    planes = torch.tensor([n], dtype=torch.int32, device=DEV)
    buf = torch.from_numpy(np.concatenate([la.reshape(-1), ha.reshape(-1)])).to(DEV)
    label = torch.full((1, 8, 8), 7, dtype=torch.uint8, device=DEV)

    def launch():
        return lib.acr_aff_label_batch(L.ptr(buf), L.ptr(table), L.ptr(offs), L.ptr(offs[1:]), L.ptr(planes), 1, S, S, L.ptr(label), L.stream_ptr())
    for bad in ((0, S, S), (1, 60, S), (1, S, 0), (65536, S, S)):
        assert lib.acr_aff_label_batch(L.ptr(buf), L.ptr(table), L.ptr(offs), L.ptr(offs[1:]), L.ptr(planes), *bad, L.ptr(label), L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((label == 7).all())                                # nothing was launched
    L.check(launch(), "acr_aff_label_batch")                       # warm-up outside the capture
    torch.cuda.synchronize()
    assert np.array_equal(label[0].cpu().numpy(), want[2])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(launch(), "acr_aff_label_batch")
    rng = np.random.RandomState(22)
    la2, ha2 = _exact_scores(rng, n, h, w), _exact_scores(rng, n, h, w)
    buf.copy_(torch.from_numpy(np.concatenate([la2.reshape(-1), ha2.reshape(-1)])))
    label.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(label[0].cpu().numpy(), R.aff_label(la2, ha2, S, S, box, flip))


@pytest.fixture(scope="module")
def layers():
    """the small hybrid seg=True model of tests/test_affinity_gpu.py and an AffinityHead on its 16 features"""
    from acr_wsss_amd.affinity import AffinityHead
    from acr_wsss_amd.backbone import set_math
    from acr_wsss_amd.DPT.ACR import ACR
    fx = load_golden("decoder_hybrid_64")
    model = ACR(20, "vitb_hybrid", seg=True, features=16, use_pretrain=False)
    sd = {}
    for k, v in model.state_dict().items():
        if "running_" in k:
            sd[k] = torch.from_numpy(fx["before:" + k])
        elif torch.is_floating_point(v):
            sd[k] = recipe_tensor(k, v.shape, 0)
        else:
            sd[k] = torch.zeros_like(v)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    model.set_math("f32_split").train()
    with torch.random.fork_rng(devices=[]):                      # the head's init draws from the global generator: leave it as found
        torch.manual_seed(5)
        head = AffinityHead(16, dims=(8, 8, 16), out_dim=24)
    head = head.to(DEV).train()
    set_math(head, "f32_split")
    yield model, head
    model.set_math("f32")


def test_train_step_fed_from_the_chunk_loader(layers, tmp_path):
    from PIL import Image
    from acr_wsss_amd import affinity as A
    from acr_wsss_amd import data as D
    from acr_wsss_amd.train import PolyOptimizer
    model, head = layers
    rng = np.random.RandomState(23)
    names, dumps = ["2007_000001", "2007_000002"], {}
    for d in ("img", "crf_1", "crf_12"):
        os.makedirs(tmp_path / d)
    for name, (h, w), keys in zip(names, ((40, 57), (80, 100)), ([0, 2, 15], [0, 7])):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(str(tmp_path / "img" / (name + ".jpg")), quality=90)
        for d in ("crf_1", "crf_12"):                              # scores on the 2^-10 grid: exact block sums
            dumps[d, name] = {k: (rng.randint(0, 1025, (h, w)) * (rng.rand(h, w) < 0.8)).astype(np.float32) / np.float32(1024) for k in keys}
            np.save(str(tmp_path / d / (name + ".npy")), dumps[d, name])
    loader = D.ChunkLoader(str(tmp_path / "img"), {}, S, device=DEV, seed=3, workers=2, la_dir=str(tmp_path / "crf_1"), ha_dir=str(tmp_path / "crf_12"))
    try:
        (images, label, got_names), = list(loader.iterate([names], kind="aff"))
        rec = loader._aff.last_records
    finally:
        loader.close()
    assert got_names == names and tuple(images.shape) == (2, 3, S, S) and tuple(label.shape) == (2, 8, 8)
    want = []
    for i, name in enumerate(names):
        r = rec[i]
        h, w, cw, flip = int(r["h"]), int(r["w"]), int(r["cw"]), int(r["flip"])
        cl, il = (S - int(r["cont_left"]) - cw, w - int(r["img_left"]) - cw) if flip else (int(r["cont_left"]), int(r["img_left"]))
        want.append(R.aff_label(dumps["crf_1", name], dumps["crf_12", name], S, S, (int(r["cont_top"]), cl, int(r["img_top"]), il, int(r["ch"]), cw), flip))
    want = np.stack(want)
    assert np.array_equal(label.cpu().numpy(), want)
    opt = PolyOptimizer(list(head.parameters()), lr=0.01, weight_decay=5e-4, max_step=100)
    terms = A.aff_train_step(model, head, opt, images, label, radius=3)
    terms = [float(t.detach()) for t in terms]
    print("aff_train_step on a chunk-loader batch (loss, bg, fg, neg):", terms)
    assert all(np.isfinite(t) for t in terms) and terms[0] > 0
    _, counts = A.pair_codes(label, 3, 1)
    ref_counts = AR.pair_codes(torch.from_numpy(want), 3, 1)[1]
    assert counts.tolist() == ref_counts.tolist() and min(ref_counts.tolist()) > 0
