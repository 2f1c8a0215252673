"""The segmentation-training input pipeline on the GPU: ``acr_preprocess_seg_batch`` through ``acr_wsss_amd.data`` against fixtures
written by the REFERENCE's own get_data_from_chunk_v4 / _v3 (tests/golden/make_segdata_golden.py), against the existing
``acr_preprocess_batch`` (bit for bit), against the numpy restatement tests/segdata_ref.py on the same pixels and draws, and down the
chain PNG label map -> loader -> ``segloss.joint_loss``.

Tolerances: ``images`` atol 2e-5 with the zero band exact (the bound test_data_gpu.py holds the same arithmetic to); ``ori_images``
+-1 against the reference (fp32 against float64 upstream of a truncation) and EXACT against the truncation rule applied on the CPU
to the kernel's own fp32 ``images``; maps and cropping masks exact."""
import functools
import random
import time

import numpy as np
import pytest
import torch

import segdata_ref as R
from acr_wsss_amd import data
from segdata_ref import FIXTURES, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# S = 32 with sources larger than the crop in both, one and no dimension, odd ones and a narrow one; the same sources at S = 30
# (S % 4 != 0: the one-pixel-per-thread kernel) -- S = 32 takes the 4-pixel vector kernel
SHAPES = [(33, 31), (30, 40), (60, 90), (90, 60), (31, 17)]
SEED = 4


def ori_rule(x_f32):
    """trunc((x * std + mean) * 255), clamped, in float32 multiply / add / multiply: (B,3,S,S) float32 -> uint8."""
    std = np.array(R.STD, np.float32).reshape(1, 3, 1, 1)
    mean = np.array(R.MEAN, np.float32).reshape(1, 3, 1, 1)
    v = (x_f32.astype(np.float32) * std + mean) * np.float32(255.0)
    assert v.dtype == np.float32
    return np.clip(v, 0, 255).astype(np.uint8)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.dtype == torch.bfloat16 else t.dtype)


@functools.lru_cache(maxsize=None)
def case(S, kind):
    """Random sources and maps at SHAPES, the restatement's result for map_fill 0 and the records of its draws; read-only."""
    rng = np.random.default_rng(100 + S)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    maps = [rng.integers(0, 21, (h, w), dtype=np.uint8) for h, w in SHAPES]
    for m in maps:
        m[rng.random(m.shape) < 0.1] = 255
    ref = R.get_data_from_chunk(imgs, maps, S, kind, random.Random(SEED), np.random.RandomState(SEED))
    rec = np.zeros(len(imgs), data.PRE_IMAGE)
    for i, (a, g) in enumerate(zip(imgs, ref["geoms"])):
        rec[i] = (0, a.shape[0], a.shape[1], g["rh"], g["rw"], g["flip"], g["cont_top"], g["cont_left"], g["img_top"], g["img_left"],
                  g["ch"], g["cw"])
    flips = [g["flip"] for g in ref["geoms"]]
    assert 0 < sum(flips) < len(flips), flips                 # a batch with flips both on and off
    return imgs, maps, ref, rec


@pytest.mark.parametrize("name", FIXTURES)
def test_batcher_matches_the_reference_chunk_functions(name):
    fx, decoded, maps, kind = load_fixture(name)
    crop, seed = int(fx["crop"]), int(fx["seed"])
    b = data.SegTrainBatcher(crop, device=DEV, seed=seed, long_range=None if kind == "v4" else R.long_range(crop, "v3"))
    images, ori, labels, croppings, target = b(decoded, maps, torch.from_numpy(fx["labels"]))
    n = len(decoded)
    assert images.shape == (n, 3, crop, crop) and images.dtype == torch.float32 and images.is_cuda
    assert ori.shape == (n, 3, crop, crop) and ori.dtype == torch.uint8 and ori.is_cuda
    assert croppings.shape == (crop, crop, n) and croppings.dtype == torch.float32 and croppings.permute(2, 0, 1).is_contiguous()
    assert target.shape == (n, crop, crop) and target.dtype == torch.uint8 and target.is_cuda
    assert torch.equal(labels.cpu(), torch.from_numpy(fx["labels"]))
    assert np.array_equal(target.cpu().numpy(), fx["target"].astype(np.uint8)) and np.array_equal(target.float().cpu().numpy(), fx["target"])
    assert np.array_equal(croppings.cpu().numpy().astype(np.float64), fx["croppings"])
    got = images.cpu().numpy()
    assert np.array_equal(got == 0, fx["images"] == 0)
    np.testing.assert_allclose(got, fx["images"], rtol=0, atol=2e-5)
    d = np.abs(ori.cpu().numpy().astype(np.int32) - fx["ori_images"].astype(np.int32))
    print("ori_images %s: %d of %d bytes differ from the reference (by 1)" % (name, int((d != 0).sum()), d.size))
    assert d.max() <= 1
    assert np.array_equal(ori.cpu().numpy(), ori_rule(got))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["v3", "v4"])
@pytest.mark.parametrize("S", [32, 30])
def test_images_equal_the_existing_kernel_bit_for_bit_and_ori_is_the_truncation(S, kind, dtype):
    imgs, maps, ref, rec = case(S, kind)
    want = data.preprocess_batch(imgs, rec, S, DEV, dtype)
    images, ori, crop, target = data.preprocess_seg_batch(imgs, maps, rec, S, DEV, dtype)
    assert images.dtype == dtype and torch.equal(bits(images), bits(want))
    # ori_images: a pure function of the fp32 value, whatever the output type rounds it to
    x32 = data.preprocess_batch(imgs, rec, S, DEV, torch.float32).cpu().numpy()
    assert np.array_equal(ori.cpu().numpy(), ori_rule(x32))
    out = crop.cpu().numpy() == 0
    assert out.any() and [set(ori.cpu().numpy()[:, c][out].tolist()) for c in range(3)] == [{123}, {116}, {103}]


@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("kind", ["v3", "v4"])
@pytest.mark.parametrize("S", [32, 30])
def test_against_the_restatement(S, kind, fill):
    imgs, maps, ref, rec = case(S, kind)
    b = data.SegTrainBatcher(S, device=DEV, seed=SEED, long_range=None if kind == "v4" else R.long_range(S, "v3"), map_fill=fill)
    images, ori, _, croppings, target = b(imgs, maps, torch.zeros(len(imgs), 20))
    for k in ("rh", "rw", "flip", "cont_top", "cont_left", "img_top", "img_left", "ch", "cw"):
        assert np.array_equal(b.last_records[k], rec[k]), k
    want_map = ref["target"].astype(np.uint8)
    inside = ref["croppings"].transpose(2, 0, 1) != 0
    if fill:
        want_map = np.where(inside, want_map, fill).astype(np.uint8)
        assert np.array_equal(want_map, np.stack([R.seg_image(a, m, S, g, fill)[3] for a, m, g in zip(imgs, maps, ref["geoms"])]))
    assert np.array_equal(target.cpu().numpy(), want_map)
    assert np.array_equal(croppings.cpu().numpy(), ref["croppings"].astype(np.float32))
    got = images.cpu().numpy()
    assert np.array_equal(got == 0, ref["images"] == 0)
    np.testing.assert_allclose(got, ref["images"], rtol=0, atol=2e-5)
    assert np.abs(ori.cpu().numpy().astype(np.int32) - ref["ori_images"].astype(np.int32)).max() <= 1


@pytest.mark.parametrize("S", [32, 30])
def test_null_outputs_leave_the_others_unchanged(S):
    imgs, maps, ref, rec = case(S, "v3")
    full = data.preprocess_seg_batch(imgs, maps, rec, S, DEV, map_fill=7)
    for skip in range(1, 4):
        kw = dict(with_ori=skip != 1, with_croppings=skip != 2, with_map=skip != 3)
        part = data.preprocess_seg_batch(imgs, maps, rec, S, DEV, map_fill=7, **kw)
        for i, (a, b) in enumerate(zip(full, part)):
            if i == skip:
                assert b is None
            else:
                assert torch.equal(bits(a), bits(b)), (skip, i)
    only = data.preprocess_seg_batch(imgs, maps, rec, S, DEV, with_ori=False, with_croppings=False, with_map=False)
    assert only[1:] == (None, None, None) and torch.equal(bits(only[0]), bits(full[0]))


def _write_pairs(tmp_path, shapes, rng):
    """A JPEG and a palette PNG label map (pseudo.save_label_png) per name, the class vectors, and the PNGs' indices."""
    from PIL import Image
    from acr_wsss_amd import pseudo
    names, labels, maps = [], {}, {}
    for i, (h, w) in enumerate(shapes):
        name = "2007_%06d" % i
        base = rng.integers(0, 256, (h // 4 + 1, w // 4 + 1, 3), dtype=np.uint8)
        arr = np.asarray(Image.fromarray(base).resize((w, h), Image.BICUBIC))
        Image.fromarray(arr).save(tmp_path / (name + ".jpg"), format="JPEG", quality=92)
        m = np.repeat(np.repeat(rng.integers(0, 21, (h // 8 + 1, w // 8 + 1), dtype=np.uint8), 8, 0), 8, 1)[:h, :w].copy()
        m[rng.random(m.shape) < 0.05] = 255
        pseudo.save_label_png(str(tmp_path / (name + ".png")), m)
        names.append(name)
        lab = np.zeros(20, np.float32)
        lab[i % 20] = 1.0
        labels[name], maps[name] = lab, m
    return names, labels, maps


def test_chain_label_png_to_joint_loss(tmp_path):
    """pseudo.save_label_png -> ChunkLoader.get_data_from_chunk_v4 -> segloss.joint_loss: square sources of the crop size make
    every step of the geometry the identity, so the target is the PNG's indices up to the drawn flip; the tuple feeds the loss as
    it is (device tensors, no copy of the croppings) and backward reaches the logits."""
    from acr_wsss_amd import segloss
    S = 64
    names, labels, maps = _write_pairs(tmp_path, [(S, S)] * 3, np.random.default_rng(8))
    loader = data.ChunkLoader(str(tmp_path), labels, S, device=DEV, seed=2, workers=2, map_dir=str(tmp_path))
    images, ori, lab, croppings, name_list, target = loader.get_data_from_chunk_v4(names)
    rec = loader._seg_batcher("v4").last_records
    assert name_list == names and (rec["rh"] == S).all() and (rec["rw"] == S).all() and 0 < rec["flip"].sum() < len(names)
    for i, n in enumerate(names):
        want = maps[n][:, ::-1] if rec["flip"][i] else maps[n]
        assert np.array_equal(target[i].cpu().numpy(), want), n
    assert bool((croppings == 1).all()) and torch.equal(lab.cpu(), torch.from_numpy(np.stack([labels[n] for n in names])))
    assert croppings.shape == (S, S, 3) and croppings.permute(2, 0, 1).is_contiguous() and ori.is_cuda and ori.dtype == torch.uint8
    # the identity resize leaves the decoded pixels: ori_images is the JPEG up to the truncation of a value an ulp below an integer
    dec = np.stack([data.decode_rgb(str(tmp_path / (n + ".jpg"))) for n in names]).transpose(0, 3, 1, 2)
    dec = np.where(rec["flip"].reshape(-1, 1, 1, 1) != 0, dec[..., ::-1], dec)
    assert np.abs(ori.cpu().numpy().astype(np.int32) - dec.astype(np.int32)).max() <= 1
    torch.manual_seed(0)
    logits = torch.randn(3, 21, S // 4, S // 4, device=DEV, requires_grad=True)
    layer = segloss.DenseEnergyLoss(0.5, 15.0, 40.0, 1.0)
    ce, dl = segloss.joint_loss(ori, logits, target, croppings, False, layer)
    loss = ce + dl
    loss.backward()
    assert torch.isfinite(loss) and float(dl) != 0.0
    assert logits.grad is not None and torch.isfinite(logits.grad).all() and float(logits.grad.abs().max()) > 0
    loader.close()


@pytest.mark.parametrize("kind", ["v4", "v3"])
def test_prefetching_iterator_yields_the_synchronous_sequence(tmp_path, kind):
    shapes = [(33, 31), (30, 40), (60, 90), (90, 60), (31, 17), (48, 48), (37, 113), (64, 80)]
    names, labels, maps = _write_pairs(tmp_path, shapes, np.random.default_rng(9))
    S = 32
    chunks = list(data.chunker(names, 3))                    # 3 + 3 + 2
    a = data.ChunkLoader(str(tmp_path), labels, S, device=DEV, seed=3, workers=4, map_dir=str(tmp_path), map_fill=255)
    b = data.ChunkLoader(str(tmp_path), labels, S, device=DEV, seed=3, workers=2, map_dir=str(tmp_path), map_fill=255)
    sync = getattr(a, "get_data_from_chunk_" + kind)
    seq = [sync(c) for c in chunks]
    n = 0
    for got, want in zip(b.iterate(chunks, kind=kind), seq):
        assert got[4] == want[4]
        for i in (0, 1, 2, 3, 5):
            assert torch.equal(bits(got[i]), bits(want[i])), (n, i)
        n += 1
    assert n == len(chunks)
    # and the sequence is the restatement's on the decoded files, one stream of draws across the chunks
    pr, nr = random.Random(3), np.random.RandomState(3)
    for chunk, got in zip(chunks, seq):
        dec = [data.decode_rgb(str(tmp_path / (n_ + ".jpg"))) for n_ in chunk]
        ms = [data.decode_map(str(tmp_path / (n_ + ".png"))) for n_ in chunk]
        assert all(np.array_equal(m, maps[n_]) for m, n_ in zip(ms, chunk))
        ref = R.get_data_from_chunk(dec, ms, S, kind, pr, nr, map_fill=255)
        assert np.array_equal(got[5].cpu().numpy(), ref["target"].astype(np.uint8))
        assert np.array_equal(got[3].cpu().numpy(), ref["croppings"].astype(np.float32))
        np.testing.assert_allclose(got[0].cpu().numpy(), ref["images"], rtol=0, atol=2e-5)
    a.close()
    b.close()


def test_throughput_against_the_previous_composition(tmp_path):
    """For the record (no threshold; DESIGN.md has the measured figures): 16 x 375x500 -> 448^2, the one-launch path against what a
    user had to compose before it existed -- ``TrainBatcher`` + ``ChunkLoader._ori`` (five torch ops and a trip to the host) + the
    mask's nearest resize / flip / crop and the cropping masks in numpy per image + their upload."""
    S, n = 448, 16
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (375, 500, 3), dtype=np.uint8) for _ in range(n)]
    maps = [rng.integers(0, 21, (375, 500), dtype=np.uint8) for _ in range(n)]
    labels = torch.zeros(n, 20)
    new = data.SegTrainBatcher(S, device=DEV, seed=1, long_range=R.long_range(S, "v3"))
    old = data.TrainBatcher(S, device=DEV, seed=1)
    ori_of = data.ChunkLoader(str(tmp_path), {}, S, device=DEV, workers=1, with_ori=True)

    def composed():
        x, y = old(imgs, labels)
        ori = torch.from_numpy(ori_of._ori(x)).to(DEV)
        tg, cr = np.zeros((n, S, S), np.uint8), np.zeros((n, S, S), np.float32)
        for i, (m, r) in enumerate(zip(maps, old.last_records)):
            m = R.cv2_resize_nearest(m, int(r["rw"]), int(r["rh"]))
            if r["flip"]:
                m = m[:, ::-1]
            ct, cl, it, il, ch, cw = (int(r[k]) for k in ("cont_top", "cont_left", "img_top", "img_left", "ch", "cw"))
            tg[i, ct:ct + ch, cl:cl + cw] = m[it:it + ch, il:il + cw]
            cr[i, ct:ct + ch, cl:cl + cw] = 1
        return x, ori, y, torch.from_numpy(cr).to(DEV).permute(1, 2, 0), torch.from_numpy(tg).to(DEV)

    rates = {}
    for what, fn in (("one launch", lambda: new(imgs, maps, labels)), ("previous composition", composed)):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            out = fn()
        torch.cuda.synchronize()
        rates[what] = n * 5 / (time.perf_counter() - t0)
    # the same seed draws the same geometry: both give the same batch
    a, b = new(imgs, maps, labels), composed()
    assert np.array_equal(new.last_records, old.last_records)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[4], b[4]) and torch.equal(a[3], b[3]) and torch.equal(a[1], b[1])
    print("segmentation input pipeline, 16 x 375x500 -> 448^2 (host packing + H2D + kernels): one launch %.0f img/s, previous composition "
          "%.0f img/s (%.2fx)" % (rates["one launch"], rates["previous composition"], rates["one launch"] / rates["previous composition"]))
    ori_of.close()
