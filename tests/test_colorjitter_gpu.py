"""The colour jitter on the GPU (csrc/colorjitter.hip behind ``data.color_jitter_batch``, ``preprocess_batch(jitter=...)`` and
``AffTrainBatcher(color_jitter=...)``): EXACT equality, every byte, with the fixtures Pillow wrote
(tests/golden/make_colorjitter_golden.py) and with the numpy restatement (tests/colorjitter_ref.py), which tests/test_colorjitter_cpu.py
holds against live Pillow.  uint8 in, uint8 out: no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import colorjitter_ref as R
from test_colorjitter_cpu import colour_cube, fixture_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_every_fixture():
    from acr_wsss_amd import data as D
    cases = list(fixture_cases())
    got = D.color_jitter_batch([c[1] for c in cases], [c[2] for c in cases], DEV)      # ONE batch: 100 images, every order
    assert len(got) == len(cases) == 100
    for (what, img, params, want), g in zip(cases, got):
        assert g.dtype == np.uint8 and g.shape == want.shape and np.array_equal(g, want), (what, int((g != want).sum()))


@pytest.fixture(scope="module")
def cube():
    """the colour cube as one 4096 x 4096 image, its HSV form and the HSV -> RGB table (index H 65536 + S 256 + V), computed once"""
    c = colour_cube()
    hsv = R.rgb2hsv(c).astype(np.uint32)
    table = R.hsv2rgb(c).reshape(-1, 3)
    return c, hsv, table


def test_colour_cube_hue_at_several_shifts(cube):
    from acr_wsss_amd import data as D
    c, hsv, table = cube
    hues = (0.0, -0.05, 0.5, 0.1)
    assert [R.hue_shift(v) for v in hues] == [0, 244, 127, 25]
    got = D.color_jitter_batch([c] * len(hues), [((3,), None, None, None, v) for v in hues], DEV)
    for v, g in zip(hues, got):
        idx = (((hsv[..., 0] + R.hue_shift(v)) & 255) << 16) | (hsv[..., 1] << 8) | hsv[..., 2]
        want = table[idx]                                          # each extra shift costs a gather
        assert np.array_equal(g, want), (v, int((g != want).any(-1).sum()))
    assert not np.array_equal(got[0], c)                           # shift 0 is still the lossy round trip


def test_colour_cube_saturation_and_brightness(cube):
    from acr_wsss_amd import data as D
    c = cube[0]
    params = [((2,), None, None, 0.7, None), ((2,), None, None, 1.3, None), ((0,), 1.3, None, None, None)]
    got = D.color_jitter_batch([c] * 3, params, DEV)
    for p, g, want in zip(params, got, (R.saturation(c, 0.7), R.saturation(c, 1.3), R.brightness(c, 1.3))):
        assert np.array_equal(g, want), (p, int((g != want).any(-1).sum()))


MIXED = (((1, 1), ((1, 0, 3, 2), 1.3, 0.74, 0.7, 0.1)),                              # contrast first
         ((1, 3), ((3, 2, 0, 1), 0.8, 1.27, 1.3, -0.05)),                            # contrast last
         ((5, 7), ((2, 0, 3), 1.27, None, 0.74, 0.5)),                               # contrast disabled
         ((33, 65), ((0, 3, 1, 2), 2.5, 0.3, 1.0001, -0.5)),                         # factors that clip
         ((97, 130), ((2, 1), None, 1.3, 0.0, None)))                                # h w % 4 = 2: a tail group; > one workgroup's 1024 pixels


def _mixed_batch():
    rng = np.random.RandomState(31)
    images = [rng.randint(0, 256, hw + (3,)).astype(np.uint8) for hw, _ in MIXED]
    return images, [p for _, p in MIXED]


def test_mixed_batch_padding_and_guards():
    from acr_wsss_amd import data as D
    images, params = _mixed_batch()
    want = [R.color_jitter(a, p) for a, p in zip(images, params)]
    assert all(not np.array_equal(a, w) for a, w in zip(images, want))
    got = D.color_jitter_batch(images, params, DEV)
    for a, g, w, p in zip(images, got, want, params):
        assert np.array_equal(g, w), (a.shape, p, int((g != w).sum()))
    # the same launch on a buffer of this test's own: 0xA5 in front of, between and behind the images
    sizes = [a.size for a in images]
    offs = np.concatenate([[0], np.cumsum([(s + 15) // 16 * 16 for s in sizes])])
    guard, total = 4096, int(offs[-1])
    assert any(s % 16 for s in sizes) and [a.shape[0] * a.shape[1] % 4 for a in images] == [1, 3, 3, 1, 2]
    host = np.full(guard + total + guard, 0xA5, np.uint8)
    for a, o in zip(images, offs[:-1]):
        host[guard + o:guard + o + a.size] = a.reshape(-1)
    buf = torch.from_numpy(host).to(DEV)
    runs = []
    for _ in range(2):
        buf.copy_(torch.from_numpy(host))
        keep = D.color_jitter_launch(buf[guard:guard + total], offs[:-1], [a.shape[:2] for a in images], D.jitter_tables(params, len(images)))
        runs.append(buf.cpu().numpy())
        del keep
    out = runs[0]
    assert out.tobytes() == runs[1].tobytes()                       # two runs with the same parameters: identical bytes
    assert (out[:guard] == 0xA5).all() and (out[guard + total:] == 0xA5).all()
    for a, o, w, nxt in zip(images, offs[:-1], want, offs[1:]):
        assert np.array_equal(out[guard + o:guard + o + a.size].reshape(a.shape), w), a.shape
        assert (out[guard + o + a.size:guard + nxt] == 0xA5).all(), a.shape      # the alignment padding is not touched
    # an image's result does not depend on its batch
    alone = D.color_jitter_batch(images[3:4], params[3:4], DEV)[0]
    assert np.array_equal(alone, want[3])


def test_gray_sum_beyond_32_bits():
    """an all-white 4200 x 4100 image: the gray sum is 255 * 17.22e6 > 2^32, the mean 255, contrast 0.5 leaves the image white; a
    32-bit sum would give a mean of about 6 and a nearly black image"""
    from acr_wsss_amd import data as D
    img = np.full((4200, 4100, 3), 255, np.uint8)
    assert 255 * 4200 * 4100 > 2 ** 32 and (255 * 4200 * 4100 % 2 ** 32) // (4200 * 4100) < 8
    small = np.full((4, 4, 3), 255, np.uint8)
    assert R.contrast_mean(small) == 255 and (R.contrast(small, 0.5) == 255).all()
    got = D.color_jitter_batch([img], [((1,), None, 0.5, None, None)], DEV)[0]
    assert got.min() == 255


def test_entry_point_refuses_what_its_contract_excludes():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    buf = torch.full((64,), 7, dtype=torch.uint8, device=DEV)
    tab = torch.zeros(64, dtype=torch.int64, device=DEV)
    for batch in (0, -1, 65536):
        assert lib.acr_color_jitter_batch(L.ptr(buf), L.ptr(tab), L.ptr(tab), L.ptr(tab), L.ptr(tab), L.ptr(tab), batch, None, L.stream_ptr()) != 0
    assert lib.acr_color_jitter_batch(None, L.ptr(tab), L.ptr(tab), L.ptr(tab), L.ptr(tab), L.ptr(tab), 1, None, L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((buf == 7).all())                                  # nothing was launched


def test_entry_point_only_enqueues_on_the_callers_stream():
    """acr_color_jitter_batch allocates nothing and does not synchronise: both launches captured once into a graph and replayed on
    other pixels give the restatement's bytes"""
    from acr_wsss_amd import _lib as L
    lib = L.load()
    rng = np.random.RandomState(34)
    h, w = 33, 65
    params = ((0, 3, 1, 2), 1.27, 0.74, 1.3, -0.05)
    first, second = (rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2))
    buf = torch.from_numpy(first.reshape(-1).copy()).to(DEV)
    offs = torch.zeros(1, dtype=torch.int64, device=DEV)
    hw = torch.tensor([h, w], dtype=torch.int32, device=DEV)
    order = torch.tensor(params[0], dtype=torch.int32, device=DEV)
    factors = torch.tensor(params[1:4], dtype=torch.float32, device=DEV)
    shift = torch.tensor([R.hue_shift(params[4])], dtype=torch.int32, device=DEV)
    ws, nbytes = L.workspace("acr_color_jitter_ws_bytes", 1, device=DEV)
    assert nbytes > 0

    def launch():
        return lib.acr_color_jitter_batch(L.ptr(buf), L.ptr(offs), L.ptr(hw), L.ptr(order), L.ptr(factors), L.ptr(shift), 1, L.ptr(ws), L.stream_ptr())
    L.check(launch(), "acr_color_jitter_batch")                    # warm-up outside the capture
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(h, w, 3), R.color_jitter(first, params))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(launch(), "acr_color_jitter_batch")
    buf.copy_(torch.from_numpy(second.reshape(-1).copy()))
    ws.fill_(0xFF)                                                 # the workspace's contents are arbitrary
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(h, w, 3), R.color_jitter(second, params))


def _aff_chunk(rng):
    shapes = ((40, 57), (80, 100), (64, 64), (33, 70))
    images = [rng.randint(0, 256, hw + (3,)).astype(np.uint8) for hw in shapes]
    la = [(rng.randint(0, 1025, (3,) + hw) * (rng.rand(3, *hw) < 0.8)).astype(np.float32) / np.float32(1024) for hw in shapes]
    ha = [(rng.randint(0, 1025, (3,) + hw) * (rng.rand(3, *hw) < 0.8)).astype(np.float32) / np.float32(1024) for hw in shapes]
    return images, la, ha


def test_aff_train_batcher_with_and_without_jitter():
    from acr_wsss_amd import data as D
    S = 64
    images, la, ha = _aff_chunk(np.random.RandomState(32))
    b = D.AffTrainBatcher(S, DEV, seed=5, color_jitter=D.ColorJitter(0.3, 0.3, 0.3, 0.1, seed=6))
    out, label = b(images, la, ha)
    ref_draws = D.ColorJitter(0.3, 0.3, 0.3, 0.1, seed=6)
    assert b.last_jitter == [ref_draws.draw() for _ in images] and len(b.last_records) == len(images)
    jittered = [R.color_jitter(a, p) for a, p in zip(images, b.last_jitter)]
    assert all(not np.array_equal(a, j) for a, j in zip(images, jittered))
    assert torch.equal(out, D.preprocess_batch(jittered, b.last_records, S, DEV))
    # the old way, from the same seed: the same records, the un-jittered images, the same label
    old = D.AffTrainBatcher(S, DEV, 5)
    out0, label0 = old(images, la, ha)
    assert old.last_records.tobytes() == b.last_records.tobytes() and old.last_jitter is None
    assert torch.equal(label, label0) and not torch.equal(out, out0)
    none = D.AffTrainBatcher(S, DEV, seed=5, color_jitter=None)
    out1, label1 = none(images, la, ha)
    assert torch.equal(out1, out0) and torch.equal(label1, label0) and none.last_records.tobytes() == old.last_records.tobytes()
    assert torch.equal(out0, D.preprocess_batch(images, old.last_records, S, DEV))
    # records= and jitter= replay both
    again, label2 = D.AffTrainBatcher(S, DEV, seed=99)(images, la, ha, records=b.last_records, jitter=b.last_jitter)
    assert torch.equal(again, out) and torch.equal(label2, label)
    direct, label3 = D.preprocess_aff_batch(images, la, ha, b.last_records, S, DEV, jitter=b.last_jitter)
    assert torch.equal(direct, out) and torch.equal(label3, label)


def test_chunk_loader_applies_the_jitter_to_the_affinity_stage(tmp_path):
    from PIL import Image
    from acr_wsss_amd import data as D
    S, rng = 64, np.random.RandomState(33)
    names = ["2007_000001", "2007_000002"]
    for d in ("img", "crf_1", "crf_12"):
        os.makedirs(tmp_path / d)
    decoded = []
    for name, (h, w) in zip(names, ((40, 57), (80, 100))):
        decoded.append(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        Image.fromarray(decoded[-1]).save(str(tmp_path / "img" / (name + ".png")))
        for d in ("crf_1", "crf_12"):
            np.save(str(tmp_path / d / (name + ".npy")), {k: rng.randint(0, 1025, (h, w)).astype(np.float32) / np.float32(1024) for k in (0, 4)})
    kw = dict(device=DEV, seed=3, workers=2, ext=".png", la_dir=str(tmp_path / "crf_1"), ha_dir=str(tmp_path / "crf_12"))
    loader = D.ChunkLoader(str(tmp_path / "img"), {}, S, color_jitter=D.ColorJitter(0.3, 0.3, 0.3, 0.1, seed=8), **kw)
    plain = D.ChunkLoader(str(tmp_path / "img"), {}, S, **kw)
    try:
        (images, label, got_names), = list(loader.iterate([names], kind="aff"))
        images0, label0, _ = plain.get_data_from_chunk_aff(names)
        rec, params = loader._aff.last_records, loader._aff.last_jitter
        assert plain._aff.last_records.tobytes() == rec.tobytes() and plain._aff.last_jitter is None
    finally:
        loader.close()
        plain.close()
    assert got_names == names and torch.equal(label, label0) and not torch.equal(images, images0)
    assert torch.equal(images, D.preprocess_batch([R.color_jitter(a, p) for a, p in zip(decoded, params)], rec, S, DEV))
