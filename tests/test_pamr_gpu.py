"""Pixel-adaptive mask refinement on the GPU (csrc/pamr.hip through acr_wsss_amd.pamr and the C ABI) against the reference.

Tolerance: for inputs (x, mask) let E = max|fp32 reference - fp64 reference| -- the reference's OWN fp32 error, read from the
fixture (written by the reference module, tests/golden/make_pamr_golden.py) or, at geometries without a fixture, taken at test
time from tests/pamr_ref.py (pinned to those fixtures bit for bit in float64 by tests/test_pamr_cpu.py).  The kernels must stay
within 4 * E of the fp64 reference: a second valid fp32 evaluation order adds an independent error of the reference's own
size (x 2), and another x 2 covers expf / division differences between the CPU's and the GPU's libm.  E is never the kernel's
own error.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

from pamr_ref import neighbours, pamr_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
SIX = (1, 2, 4, 8, 12, 24)
U = 2.0 ** -24                                                # fp32 unit roundoff


def _fixture(tag):
    g = np.load(os.path.join(GOLD, "pamr_%s.npz" % tag))
    return (torch.from_numpy(g["x"]), torch.from_numpy(g["mask"]), int(g["num_iter"]), [int(d) for d in g["dilations"]],
            g["ref32"], g["ref64"])


def _gpu(x, mask, num_iter, dil):
    from acr_wsss_amd.pamr import pamr
    out = pamr(x.to(DEV), mask.to(DEV), num_iter, dil)
    torch.cuda.synchronize()
    return out.cpu()


def _noise_image(g, B, H, W):
    """integers 0..255 as float32, like a decoded image"""
    return torch.randint(0, 256, (B, 3, H, W), generator=g).float()


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_fixtures_of_the_reference_module(tag):
    x, mask, num_iter, dil, ref32, ref64 = _fixture(tag)
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    out = _gpu(x, mask, num_iter, dil)
    err = float(np.abs(out.numpy().astype(np.float64) - ref64).max())
    print("pamr_%s: E_ref = %.3e, max|kernel - ref64| = %.3e (%.2f E_ref)" % (tag, e_ref, err, err / e_ref))
    assert out.dtype == torch.float32 and tuple(out.shape) == ref64.shape
    assert err <= 4 * e_ref
    if x.shape[0] > 1:                                       # a sample's result does not depend on the batch it rides in
        for b in range(x.shape[0]):
            one = _gpu(x[b:b + 1].contiguous(), mask[b:b + 1].contiguous(), num_iter, dil)
            assert torch.equal(one[0], out[b])


@pytest.mark.parametrize("hw", [(375, 500), (500, 333)])
def test_real_geometry_against_the_restatement(hw):
    """B 2, C 8 = two alphas x (background + 3 classes), the list hook's setting"""
    H, W = hw
    g = torch.Generator().manual_seed(H)
    coarse = torch.rand(2, 3, H // 6, W // 6, generator=g)
    x = (255 * torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)).round()
    x = (x + torch.randint(-6, 7, x.shape, generator=g)).clamp(0, 255).float().contiguous()       # smooth + sensor-like noise
    mask = torch.rand(2, 8, H, W, generator=g)
    ref64 = pamr_ref(x.double(), mask.double(), 10, SIX)
    e = float((pamr_ref(x, mask, 10, SIX).double() - ref64).abs().max())
    out = _gpu(x, mask, 10, SIX)
    err = float((out.double() - ref64).abs().max())
    print("%dx%d: E = %.3e, max|kernel - ref64| = %.3e (%.2f E)" % (H, W, e, err, err / e))
    assert err <= 4 * e


def test_flat_image_gives_uniform_weights_and_the_plain_mean():
    from acr_wsss_amd.pamr import affinity
    g = torch.Generator().manual_seed(3)
    H, W = 37, 45
    x = torch.tensor([113.0, 7.25, 0.1]).view(1, 3, 1, 1).expand(1, 3, H, W).contiguous()
    mask = torch.rand(1, 3, H, W, generator=g)
    for dil in ((1,), (1, 2, 4), SIX):
        P = 8 * len(dil)
        w = affinity(x.to(DEV), dil).cpu()
        want = np.float32(1) / np.float32(P)
        assert tuple(w.shape) == (1, P, H, W)
        assert float((w - float(want)).abs().max()) <= float(np.spacing(want))                    # 1 ulp
        out = _gpu(x, mask, 1, dil)
        mean = neighbours(mask.double(), dil, False).mean(2)
        err = float((out.double() - mean).abs().max())
        # rounding of 1 / P, of P products and of P - 1 additions of terms that sum to <= max|mask| <= 1
        print("flat, %d neighbours: max|kernel - neighbour mean| = %.3e, bound %.3e" % (P, err, (P + 2) * U))
        assert err <= (P + 2) * U


def test_constant_mask_stays_constant():
    g = torch.Generator().manual_seed(4)
    x = _noise_image(g, 1, 61, 83)
    n_iter, P = 10, 8 * len(SIX)
    for c in (1.0, 0.37, -5.5):
        mask = torch.full((1, 2, 61, 83), c)
        err = float((_gpu(x, mask, n_iter, SIX).double() - c).abs().max())
        bound = n_iter * (P + 2) * U * abs(c)                 # the rounding of a P-term convex sum, n_iter times
        print("constant %g: max deviation %.3e, bound %.3e" % (c, err, bound))
        assert err <= bound


def test_per_channel_affine_invariance():
    """|difference| and deviation scale alike under x -> a_k x + b_k, a_k > 0 (up to the 1e-8 in the denominator, far below
    fp32 at image contrast); integers keep the mapped image exact in fp32"""
    g = torch.Generator().manual_seed(5)
    x = _noise_image(g, 1, 96, 128)
    mask = torch.rand(1, 4, 96, 128, generator=g)
    a = torch.tensor([2.0, 3.0, 5.0]).view(1, 3, 1, 1)
    b = torch.tensor([7.0, 0.0, 11.0]).view(1, 3, 1, 1)
    assert float((a * x + b).max()) < 2 ** 24
    ref64 = pamr_ref(x.double(), mask.double(), 10, SIX)
    e = float((pamr_ref(x, mask, 10, SIX).double() - ref64).abs().max())
    plain, mapped = _gpu(x, mask, 10, SIX), _gpu((a * x + b).contiguous(), mask, 10, SIX)
    err = float((plain.double() - mapped.double()).abs().max())
    print("affine map: E = %.3e, max|pamr(x) - pamr(a x + b)| = %.3e (%.2f E)" % (e, err, err / e))
    assert err <= 4 * e
    assert float((plain.double() - ref64).abs().max()) <= 4 * e


def test_reproducible_bits_and_loud_errors():
    from acr_wsss_amd.pamr import PAMR, pamr
    g = torch.Generator().manual_seed(6)
    x = _noise_image(g, 2, 50, 70).to(DEV)
    mask = torch.rand(2, 11, 25, 35, generator=g).to(DEV)     # resize path, two channel chunks (8 + 3)
    first = pamr(x, mask, 10, SIX)
    assert torch.equal(first, pamr(x, mask, 10, SIX))
    assert torch.equal(first, PAMR(10, list(SIX))(x, mask))
    ref64 = pamr_ref(x.cpu().double(), mask.cpu().double(), 10, SIX)
    e = float((pamr_ref(x.cpu(), mask.cpu(), 10, SIX).double() - ref64).abs().max())
    err = float((first.cpu().double() - ref64).abs().max())
    print("C = 11 with resize: E = %.3e, max|kernel - ref64| = %.3e" % (e, err))
    assert err <= 4 * e
    with pytest.raises(ValueError):
        pamr(x.transpose(2, 3), mask)                        # not contiguous
    with pytest.raises(ValueError):
        pamr(x, mask.transpose(2, 3))
    with pytest.raises(ValueError):
        pamr(x.double(), mask)
    with pytest.raises(ValueError):
        pamr(x, mask.half())
    with pytest.raises(ValueError):
        pamr(x, mask.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        pamr(x, mask[:1].contiguous())                       # batch sizes differ
    from acr_wsss_amd._lib import AcrHipError
    with pytest.raises(AcrHipError):
        pamr(x, mask, 1, (1, 0))
    with pytest.raises(AcrHipError):
        pamr(x, mask, 1, tuple(range(1, 10)))


def test_c_abi_launches_capture_into_a_hip_graph():
    """acr_pamr_affinity and ten acr_pamr_propagate launches only enqueue work: one chain, captured once, replayed on new input
    values to the bits of the eager launches"""
    import ctypes
    from acr_wsss_amd import _lib as L
    lib = L.load()
    B, K, C, H, W = 1, 3, 8, 120, 160
    dil = (ctypes.c_int32 * len(SIX))(*SIX)
    g = torch.Generator().manual_seed(7)
    x = _noise_image(g, B, H, W).to(DEV)
    mask = torch.rand(B, C, H, W, generator=g).to(DEV)
    w = torch.empty(B, 8 * len(SIX), H, W, device=DEV)
    bufs = [torch.empty_like(mask), torch.empty_like(mask)]

    def launch():
        st = L.stream_ptr()
        L.check(lib.acr_pamr_affinity(L.ptr(x), B, K, H, W, dil, len(SIX), L.ptr(w), st), "affinity")
        src = mask
        for it in range(10):
            L.check(lib.acr_pamr_propagate(L.ptr(w), L.ptr(src), L.ptr(bufs[it % 2]), B, C, H, W, dil, len(SIX), st), "propagate")
            src = bufs[it % 2]
        return src

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        result = launch()
    from acr_wsss_amd.pamr import pamr
    for seed in (11, 12):
        g2 = torch.Generator().manual_seed(seed)
        x.copy_(_noise_image(g2, B, H, W))
        mask.copy_(torch.rand(B, C, H, W, generator=g2))
        eager = launch().clone()
        torch.cuda.synchronize()
        assert torch.equal(eager, pamr(x, mask, 10, SIX))
        result.zero_()
        w.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(result, eager)


def test_infer_cam_list_writes_pamr_outputs(tmp_path):
    """out_pamr: <out_pamr>_<alpha>/<name>.npy holds {0: bg, class + 1: ...} for both alphas, equal to the restatement applied to
    the returned cam_dict; out_cam files do not change; an image without a positive class writes no PAMR file"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from __graft_entry__ import _recipe_model
    from recipe import make_inputs
    from acr_wsss_amd.infer_cam import infer_cam_list
    model, _ = _recipe_model(torch.device(DEV))
    rng = np.random.default_rng(0)
    items = []
    for i, (classes, hw) in enumerate((([2, 9], (40, 52)), ([], (40, 52)), ([0, 5, 17], (50, 70)))):
        img, _ = make_inputs(1, 64, 20, 20 + i)
        label = torch.zeros(1, 20)
        for c in classes:
            label[0, c] = 1
        items.append(("im%d" % i, img, label, hw, rng.integers(0, 256, hw + (3,)).astype(np.uint8)))
    plain = infer_cam_list(model, items, out_cam=str(tmp_path / "cam0"))
    res = infer_cam_list(model, items, out_cam=str(tmp_path / "cam"), out_pamr=str(tmp_path / "pamr"), low_alpha=1, high_alpha=12)
    assert sorted(res) == sorted(plain) == ["im0", "im1", "im2"] and res["im1"] == {}
    for name in res:
        with open(str(tmp_path / "cam0" / (name + ".npy")), "rb") as f0, open(str(tmp_path / "cam" / (name + ".npy")), "rb") as f1:
            assert f0.read() == f1.read()
    for alpha in (1, 12):
        folder = tmp_path / ("pamr_%d" % alpha)
        assert sorted(os.listdir(str(folder))) == ["im0.npy", "im2.npy"]
        for name, orig in (("im0", items[0][4]), ("im2", items[2][4])):
            d = np.load(str(folder / (name + ".npy")), allow_pickle=True).item()
            classes = list(res[name])
            assert sorted(d) == [0] + sorted(c + 1 for c in classes)
            cams = np.stack([res[name][c] for c in classes])
            scores = np.concatenate((np.power(1 - cams.max(0, keepdims=True), alpha), cams), 0).astype(np.float32)
            x = torch.from_numpy(orig).permute(2, 0, 1).float()[None].contiguous()
            m = torch.from_numpy(scores)[None]
            ref64 = pamr_ref(x.double(), m.double(), 10, SIX)[0].numpy()
            e = float(np.abs(pamr_ref(x, m, 10, SIX)[0].numpy().astype(np.float64) - ref64).max())
            got = np.stack([d[0]] + [d[c + 1] for c in classes])
            err = float(np.abs(got.astype(np.float64) - ref64).max())
            print("%s alpha %d: E = %.3e, max|file - ref64| = %.3e (%.2f E)" % (name, alpha, e, err, err / e))
            assert got.dtype == np.float32 and got.shape == ref64.shape
            assert err <= 4 * e
    with pytest.raises(ValueError):
        infer_cam_list(model, [items[0][:4]], out_pamr=str(tmp_path / "x"))
