"""The shared-lattice CRF stage on the GPU: ``crf_with_alphas`` (several background alphas through one pair of lattices) against
the per-alpha functions BIT FOR BIT, the grouped update against ``acr_crf_update``, the device-CAM form's scores against the
float64 power, the label-map CRF (``crf_inference_label``) against the restatement in crf_stage_ref.py, ``segtrain.crf_labels``
against its per-image composition, and a guard on the files ``infer_cam_list`` writes."""
import os

import numpy as np
import pytest
import torch

import crf_stage_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = ((2, 3, 3), (7, 9, 4))                                    # n % 4 != 0: the lattice's phantom pixel


def _cam_dict(h, w, k, seed):
    cams = R.scene_cams(h, w, k, seed)
    return {c: cams[i] for i, c in enumerate((3, 7, 11, 19)[:k])}


def _separate(cam_dict, alpha, img, t):
    """The per-alpha run: crf_with_alpha itself at its fixed t = 10, else its two lines with crf_inference's ``t``."""
    from acr_wsss_amd.crf import crf_inference, crf_with_alpha, score_dict
    if t == 10:
        return crf_with_alpha(cam_dict, alpha, img, device=DEV)
    classes = list(cam_dict.keys())
    cams = np.stack([cam_dict[c] for c in classes], axis=0)
    scores = np.concatenate((np.power(1 - cams.max(axis=0, keepdims=True), alpha), cams), axis=0)
    return score_dict(classes, crf_inference(img, scores, t=t, labels=scores.shape[0], device=DEV))


@pytest.mark.parametrize("scene", R.SCENES + TINY)
def test_shared_lattices_equal_separate_runs_bit_for_bit(scene):
    from acr_wsss_amd.crf import crf_with_alphas
    h, w, seed = scene
    img = R.scene_image(h, w, seed)
    for k in (1, 2, 4):
        cam_dict = _cam_dict(h, w, k, seed)
        for t in (0, 1, 10):
            alone = {a: _separate(cam_dict, a, img, t) for a in (1, 4, 8, 12, 32)}
            for alphas in ((1, 12), (4,), (4, 4), (1, 8, 32)):
                got = crf_with_alphas(cam_dict, alphas, img, t=t, device=DEV)
                assert sorted(got) == sorted(set(alphas))
                for a in alphas:
                    assert sorted(got[a]) == sorted(alone[a]) == [0] + [c + 1 for c in cam_dict]
                    for c in got[a]:
                        assert got[a][c].dtype == np.float32 and got[a][c].shape == (h, w)
                        assert np.array_equal(got[a][c], alone[a][c]), (k, t, alphas, a, c)
        again = crf_with_alphas(cam_dict, (1, 8, 32), img, device=DEV)
        assert all(np.array_equal(again[a][c], got[a][c]) for a in again for c in again[a])          # two runs, equal bits


def test_duplicate_alphas_fill_both_groups():
    from acr_wsss_amd.crf import crf_with_alphas_device
    h, w, seed = R.SCENES[0]
    classes, refined = crf_with_alphas_device(_cam_dict(h, w, 2, seed), (4, 4), R.scene_image(h, w, seed), device=DEV)
    assert classes == [3, 7] and refined.shape == (6, h, w) and torch.equal(refined[:3], refined[3:])


@pytest.mark.parametrize("K", [1, 3, 21])
def test_grouped_update_equals_separate_updates(K):
    from acr_wsss_amd import _lib as L
    lib = L.load()
    gen = torch.Generator().manual_seed(K)
    for G in (1, 2, 5):
        for n in (1, 255, 256, 257, 1000):
            unary, m0, m1 = (torch.randn(G * K, n, generator=gen).mul(3).to(DEV) for _ in range(3))
            for msgs in ((m0, m1), (None, None), (m0, None)):
                q = torch.full((G * K, n), float("nan"), device=DEV)
                L.check(lib.acr_crf_update_groups(L.ptr(unary), L.ptr(msgs[0]), L.ptr(msgs[1]), L.ptr(q), n, K, G, L.stream_ptr()), "groups")
                ref = torch.full((G * K, n), float("nan"), device=DEV)
                for g in range(G):
                    s = slice(g * K, (g + 1) * K)
                    L.check(lib.acr_crf_update(L.ptr(unary[s]), L.ptr(msgs[0][s]) if msgs[0] is not None else None,
                                               L.ptr(msgs[1][s]) if msgs[1] is not None else None, L.ptr(ref[s]), n, K, L.stream_ptr()), "update")
                assert torch.equal(q, ref), (K, G, n)
                assert torch.allclose(q.view(G, K, n).sum(1), torch.ones(G, n, device=DEV), atol=1e-5)


def _ulps(x, ref64):
    """|x - ref| in float32 ulps of the reference value"""
    return np.abs(x.astype(np.float64) - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


DEVICE_ALPHAS = (1, 4, 12, 32, 0.5)


@pytest.mark.parametrize("scene", R.SCENES + TINY[1:])
def test_device_cam_form(scene):
    """CAMs that never leave the device: the score stack holds the CAMs' bits, its backgrounds lie as close to the float64 power
    of the fp32 ``1 - max`` as twice numpy's own float32 ``np.power`` does (floor: 2 ulps of the value), compared after the
    clip to [1e-5, 1] the CRF reads them through; the refined planes are those of crf_inference_device on the very scores."""
    from acr_wsss_amd.crf import crf_inference_device, crf_with_alphas_device
    h, w, seed = scene
    img = R.scene_image(h, w, seed)
    worst_dev = worst_np = 0.0
    for k in (1, 2, 4):
        cams = R.scene_cams(h, w, k, seed)
        cams[:, 0, 0] = 0.0                                      # top = 1 exactly
        cams[0, -1, -1] = 1.0                                    # top = 0 exactly
        cams[-1, h // 2, :] = np.linspace(0, 1, w, dtype=np.float32)
        classes = list(range(2, 2 + k))
        d_cams = torch.from_numpy(cams).to(DEV)
        image = torch.from_numpy(img).to(DEV) if k == 2 else img   # a device image once
        got_classes, refined, scores = crf_with_alphas_device(d_cams, DEVICE_ALPHAS, image, classes=classes, return_scores=True)
        n = 1 + k
        assert got_classes == classes and refined.shape == scores.shape == (len(DEVICE_ALPHAS) * n, h, w)
        assert torch.equal(d_cams, torch.from_numpy(cams).to(DEV))            # the input is left as it was
        top = np.float32(1) - cams.max(axis=0)
        host = scores.cpu().numpy()
        for ai, alpha in enumerate(DEVICE_ALPHAS):
            assert np.array_equal(host[ai * n + 1:(ai + 1) * n], cams)
            exact = np.clip(np.power(top.astype(np.float64), float(np.float32(alpha))), float(np.float32(1e-5)), 1.0)
            dev = np.clip(host[ai * n], np.float32(1e-5), np.float32(1))
            ref32 = np.clip(np.power(top, np.float32(alpha)), np.float32(1e-5), np.float32(1))
            worst_dev, worst_np = max(worst_dev, _ulps(dev, exact).max()), max(worst_np, _ulps(ref32, exact).max())
            alone = crf_inference_device(img, scores[ai * n:(ai + 1) * n].contiguous(), labels=n)
            assert torch.equal(refined[ai * n:(ai + 1) * n], alone), (k, alpha)
    print("\nbackground %dx%d: device powf %.3f ulp, numpy float32 power %.3f ulp from the float64 power" % (h, w, worst_dev, worst_np))
    assert worst_dev <= max(2.0 * worst_np, 2.0), (worst_dev, worst_np)


@pytest.mark.parametrize("scene", R.LABEL_SCENES + ((48, 64, 0, 2),))
def test_label_crf_matches_the_restatement(scene):
    """Q within max(1e-4, 16 x the one-ulp probe) of the restatement (test_crf_gpu.py's rule, the probe recomputed here); every
    pixel's top-2 margin exceeds twice that bound, so the label map must be equal at EVERY pixel."""
    from acr_wsss_amd.crf import crf_inference_label, crf_inference_label_device
    h, w, seed, k = scene
    c = R.label_case(h, w, seed, k)
    img, labels = c["img"], c["labels"]
    fused = crf_inference_label(img, labels, n_labels=k, device=DEV)
    assert fused.shape == (h, w) and fused.dtype == np.int64
    lab, q = crf_inference_label_device(img, labels, n_labels=k, device=DEV, return_q=True)
    assert lab.dtype == torch.uint8 and q.shape == (k, h, w) and q.dtype == torch.float32
    q = q.cpu().numpy()
    err = float(np.abs(q - c["ref_q"]).max())
    print("\nlabel crf %dx%d, %d labels: |dQ| max %.2e (one-ulp probe %.2e, bound %.2e), smallest margin %.2e, labels changed %.3f"
          % (h, w, k, err, c["probe"], c["bound"], c["margin"], float((c["ref_label"] != labels).mean())))
    assert err <= c["bound"], (err, c["bound"])
    assert c["margin"] > 2 * c["bound"]
    assert np.array_equal(fused, c["ref_label"])
    assert np.array_equal(fused, q.argmax(axis=0)) and np.array_equal(lab.cpu().numpy(), fused)
    assert (c["ref_label"] != np.where(labels < k, labels, 0)).mean() > 0.01                           # the CRF does something
    on_dev = crf_inference_label_device(img, torch.from_numpy(labels).to(DEV), n_labels=k, device=DEV)
    assert np.array_equal(on_dev.cpu().numpy(), fused)                                               # numpy and device input
    again = crf_inference_label_device(torch.from_numpy(img).to(DEV), labels.astype(np.int64), n_labels=k, device=DEV)
    assert torch.equal(again, on_dev)


@pytest.mark.parametrize("scene", R.LABEL_SCENES + ((7, 9, 3, 2),))
def test_label_crf_without_iterations_and_its_unary(scene):
    from acr_wsss_amd.crf import crf_inference_label, crf_inference_label_device, label_unary_device
    h, w, seed, k = scene
    img, labels = R.label_scene(h, w, seed, k)
    got = crf_inference_label(img, labels, t=0, n_labels=k, device=DEV)
    assert np.array_equal(got, np.where(labels < k, labels, 0))
    unary, q0 = label_unary_device(labels, k, device=DEV)
    ref = R.label_unary(labels, k, 0.7)
    assert np.array_equal(unary.cpu().numpy().reshape(k, -1), ref)                                   # numpy's bits, no device log
    assert np.abs(q0.cpu().numpy().reshape(k, -1) - R.mean_field(ref, (), 0)).max() <= 1e-6
    _, q = crf_inference_label_device(img, labels, t=0, n_labels=k, device=DEV, return_q=True)
    assert torch.equal(q, q0)
    one = crf_inference_label_device(img, labels, t=1, n_labels=k, device=DEV, return_q=True)
    assert np.array_equal(one[0].cpu().numpy(), one[1].cpu().numpy().argmax(axis=0))


def test_label_crf_errors_are_loud():
    from acr_wsss_amd.crf import crf_inference_label
    img, labels = R.label_scene(8, 8, 0, 3)
    for kw in (dict(n_labels=1), dict(n_labels=256), dict(gt_prob=0.0), dict(gt_prob=1.0), dict(t=-1)):
        with pytest.raises(ValueError):
            crf_inference_label(img, labels, device=DEV, **kw)
    with pytest.raises(ValueError):
        crf_inference_label(img[:7], labels, device=DEV)


def test_crf_labels_is_the_per_image_composition():
    from acr_wsss_amd import pseudo, segtrain
    from acr_wsss_amd.crf import crf_with_alphas_device
    B, C, S = 2, 20, 32
    rng = np.random.default_rng(5)
    cams = rng.random((B, C, S, S)).astype(np.float32) * 0.5
    cams[0, 2, 4:20, 6:22] += 0.5
    cams[0, 9, 18:30, 10:30] += 0.4
    labels = torch.zeros(B, C)
    labels[0, [2, 9]] = 1
    ori = np.stack([R.scene_image(S, S, 0), R.scene_image(S, S, 1)]).transpose(0, 3, 1, 2).copy()
    d_cams, d_ori = torch.from_numpy(cams).to(DEV), torch.from_numpy(ori).to(DEV)
    for kw in ({}, dict(ignore_uncertain=True, bg_alpha=32, fg_quantile=0.6, bg_sure=0.8)):
        got = segtrain.crf_labels(d_cams, labels.to(DEV), d_ori, low_alpha=4, high_alpha=32, **kw)
        assert got.shape == (B, S, S) and got.dtype == torch.uint8 and got.is_cuda
        assert not got[1].any()                                                                      # no class: all background
        mine = d_cams[0, [2, 9]].contiguous()
        _, refined = crf_with_alphas_device(mine, (4, 32), d_ori[0].permute(1, 2, 0).contiguous(), classes=[2, 9])
        want = pseudo.seg_label(mine, [2, 9], refined[:3], refined[3:], num_classes=C, **kw)
        assert torch.equal(got[0], want)
        assert set(np.unique(got[0].cpu().numpy())) <= {0, 3, 10, 255} and (got[0] == 3).any()
    assert torch.equal(segtrain.crf_labels(d_cams, labels.numpy(), d_ori), segtrain.crf_labels(d_cams, labels.to(DEV), d_ori))


def test_infer_cam_list_crf_files_keep_their_bits(tmp_path):
    """A guard that passes before and after infer_cam_list went over to the shared call: the files of out_crf are those of
    crf_with_alpha on the returned CAMs, the PNG of out_pseudo that of pseudo.seg_label on the two stacks."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from PIL import Image
    from __graft_entry__ import _recipe_model
    from recipe import make_inputs
    from acr_wsss_amd import pseudo
    from acr_wsss_amd.crf import crf_with_alpha
    from acr_wsss_amd.infer_cam import infer_cam_list
    model, _ = _recipe_model(torch.device(DEV))
    img, _ = make_inputs(1, 64, 20, 2)
    label = torch.zeros(1, 20)
    label[0, [2, 9]] = 1
    orig = np.random.default_rng(0).integers(0, 256, (40, 52, 3)).astype(np.uint8)
    items = [("im0", img, label, (40, 52), orig)]
    res = infer_cam_list(model, items, out_crf=str(tmp_path / "crf"), low_alpha=1, high_alpha=12, out_pseudo=str(tmp_path / "png"),
                         pseudo_source="crf")
    stacks = {}
    for alpha in (1, 12):
        d = np.load(str(tmp_path / ("crf_%d" % alpha) / "im0.npy"), allow_pickle=True).item()
        ref = crf_with_alpha(res["im0"], alpha, orig, device=DEV)
        assert sorted(d) == sorted(ref) == [0, 3, 10]
        assert all(np.array_equal(d[c], ref[c]) for c in d)
        stacks[alpha] = np.stack([ref[c] for c in sorted(ref)])
    cams = np.stack([res["im0"][c] for c in (2, 9)])
    want = pseudo.seg_label(cams, [2, 9], stacks[1], stacks[12], device=DEV).cpu().numpy()
    assert np.array_equal(np.array(Image.open(str(tmp_path / "png" / "im0.png"))), want)
