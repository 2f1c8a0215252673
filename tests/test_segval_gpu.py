"""Segmentation validation on the device (csrc/segpred.hip behind acr_segpred_f32, acr_wsss_amd/segval.py, crf.crf_inference_inf)
against the float64 restatement tests/segval_ref.py, which test_segval_cpu.py pins to torch's CPU kernels and to the CRF oracle.

Values, the rule of test_segloss_gpu.py: the device's and torch's CPU fp32 probabilities are both compared with the restatement;
the device's largest error may be at most 2x the error torch's own result shows on the same case, with a floor of 4 fp32 ulps
(4 * 2^-23) of the largest reference value.  No absolute number is fixed.  Labels: with tol = max(2 x torch's error on the
interpolated logits, 4 ulps of max|logits|), a pixel is decided when the restatement's top-two margin exceeds 2 tol; on decided
pixels the device label equals the restatement's without exception, and at most 0.5 % of a case's pixels may be undecided.
Accumulation, ties, repeats and guard bytes are exact.  CRF: the tolerance rule of test_crf_gpu.py::_tolerance."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import segval_ref as R
from recipe import recipe_tensor
from acr_wsss_amd import _lib as L
from acr_wsss_amd import segval as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULPS = 4 * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def reference(tag, scale, hflip):
    """(logits, the restatement's result, torch's CPU fp32 interpolation and softmax); treat as read-only"""
    B, K, h, w, H, W = R.SHAPES[tag]
    logits = R.logits_case(tag, scale)
    x = torch.from_numpy(logits)
    tv = F.interpolate(x.flip(-1) if hflip else x, (H, W), mode="bilinear", align_corners=False)
    return logits, R.predict(logits, H, W, hflip), tv.double().numpy(), tv.softmax(1).double().numpy()


def run(logits, hw, hflip=False, probs=False, accumulate=False, want_label=True):
    """one launch -> (label numpy or None, probs numpy or None)"""
    x = torch.from_numpy(logits).to(DEV)
    buf = None
    if probs is not False:
        buf = torch.empty((x.shape[0], x.shape[1]) + tuple(hw), device=DEV) if probs is True else probs
    lab = V.predict(x, hw, hflip=hflip, probs=buf, accumulate=accumulate, want_label=want_label)
    return (None if lab is None else lab.cpu().numpy()), (None if buf is None else buf.cpu().numpy())


@pytest.mark.parametrize("hflip", [False, True])
@pytest.mark.parametrize("scale", [1, 30])
@pytest.mark.parametrize("tag", sorted(R.SHAPES))
def test_probabilities_and_labels(tag, scale, hflip):
    B, K, h, w, H, W = R.SHAPES[tag]
    logits, ref, tv, tp = reference(tag, scale, hflip)
    lab_only, _ = run(logits, (H, W), hflip)
    lab, probs = run(logits, (H, W), hflip, probs=True)
    assert lab_only.shape == (B, H, W) and lab_only.dtype == np.uint8 and probs.shape == (B, K, H, W) and probs.dtype == np.float32
    assert np.array_equal(lab_only, lab)                 # one rule for v in both modes
    if scale == 30:                                      # a naive exp would overflow
        assert np.abs(logits).max() > 88 or tag == "one"
    # probabilities
    terr, derr = np.abs(tp - ref["p"]).max(), np.abs(probs.astype(np.float64) - ref["p"]).max()
    floor = ULPS * np.abs(ref["p"]).max()
    print("%s x%d flip%d probs: device err %.3e, torch fp32 err %.3e, ratio %.2f, floor %.3e" % (tag, scale, hflip, derr, terr, derr / max(terr, 1e-300), floor))
    # labels
    tol = max(2.0 * np.abs(tv - ref["v"]).max(), ULPS * np.abs(logits).max())
    decided = R.top_two_margin(ref["v"]) > 2.0 * tol
    wrong = int((lab[decided] != ref["label"][decided]).sum())
    print("%s x%d flip%d labels: tol %.3e, undecided %.4f %%, wrong among decided %d, differing among undecided %d" % (
        tag, scale, hflip, tol, 100.0 * (1.0 - decided.mean()), wrong, int((lab[~decided] != ref["label"][~decided]).sum())))
    assert np.isfinite(probs).all()
    assert derr <= max(2.0 * terr, floor), (derr, terr, floor)
    assert 1.0 - decided.mean() <= 0.005
    assert wrong == 0


def test_exact_ties_and_constant_logits():
    for tag in ("up", "k81"):
        B, K, h, w, H, W = R.SHAPES[tag]
        logits = R.logits_case(tag).copy()
        logits[:, 3] = np.abs(logits[:, 3]) + 20.0       # two identical dominant planes
        logits[:, 7] = logits[:, 3]
        for hflip in (False, True):
            lab_only, _ = run(logits, (H, W), hflip)
            lab, probs = run(logits, (H, W), hflip, probs=True)
            acc = torch.zeros((B, K, H, W), device=DEV)
            lab_acc, summed = run(logits, (H, W), hflip, probs=acc, accumulate=True)
            lab_acc2, summed = run(logits, (H, W), not hflip, probs=acc, accumulate=True)
            assert (lab_only == 3).all() and (lab == 3).all() and (lab_acc == 3).all() and (lab_acc2 == 3).all()
            assert np.array_equal(probs[:, 3], probs[:, 7]) and np.array_equal(summed[:, 3], summed[:, 7])
        const = np.full((B, K, h, w), np.float32(-7.25))
        lab, probs = run(const, (H, W), probs=True)
        assert (lab == 0).all() and (run(const, (H, W))[0] == 0).all()
        want = np.float32(1.0) / np.float32(K)
        assert np.abs(probs - want).max() <= np.spacing(want)                            # 1 ulp of 1 / K
        acc = torch.zeros((B, K, H, W), device=DEV)
        assert (run(const, (H, W), probs=acc, accumulate=True)[0] == 0).all()


def test_accumulation_is_the_fp32_sum_in_pass_order():
    B, K, H, W = 2, 21, 37, 41
    rng = np.random.default_rng(5)
    passes = [((12, 12), False), ((20, 9), True), ((45, 50), True)]                      # enlarging, mixed, shrinking
    logits = [(2.0 * rng.standard_normal((B, K) + hw)).astype(np.float32) for hw, _ in passes]
    singles = [run(x, (H, W), f, probs=True) for x, (_, f) in zip(logits, passes)]
    acc = torch.zeros((B, K, H, W), device=DEV)
    total = np.zeros((B, K, H, W), np.float32)
    for x, (_, f), (_, p) in zip(logits, passes, singles):
        lab, got = run(x, (H, W), f, probs=acc, accumulate=True)
        total = total + p                                                                # one fp32 add per value, in pass order
        assert got.tobytes() == total.tobytes()
        assert np.array_equal(lab, total.argmax(axis=1))                                 # the first maximum of the updated buffer
    assert not np.array_equal(lab, singles[-1][0])                                       # the sum decides, not the last pass
    # without a label the buffer is the same; without a buffer the call is refused
    again = torch.zeros((B, K, H, W), device=DEV)
    for x, (_, f) in zip(logits, passes):
        assert run(x, (H, W), f, probs=again, accumulate=True, want_label=False)[0] is None
    assert again.cpu().numpy().tobytes() == total.tobytes()
    x = torch.from_numpy(logits[0]).to(DEV)
    with pytest.raises(ValueError):
        V.predict(x, (H, W), accumulate=True)
    lab = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    rc = L.load().acr_segpred_f32(L.ptr(x), B, K, 12, 12, H, W, 0, 1, None, L.ptr(lab), L.stream_ptr())
    assert rc == -1 and "accumulate" in L.load().acr_last_error().decode()


@pytest.mark.parametrize("tag", ["up", "down", "k128", "voc"])
def test_repeats_bit_for_bit_and_leaves_guards_untouched(tag):
    B, K, h, w, H, W = R.SHAPES[tag]
    logits = torch.from_numpy(R.logits_case(tag)).to(DEV)
    G, n = 4096, B * H * W
    outs = []
    for rep in range(2):
        for mode in ("label", "probs", "accumulate"):
            big_p = torch.full((2 * G + K * n,), -12345.0, device=DEV)
            big_l = torch.full((2 * G + n,), 0xA5, dtype=torch.uint8, device=DEV)
            probs = big_p[G:G + K * n].view(B, K, H, W)
            label = big_l[G:G + n].view(B, H, W)
            if mode == "accumulate":
                probs.fill_(0.25)
            rc = L.load().acr_segpred_f32(L.ptr(logits), B, K, h, w, H, W, 1, 1 if mode == "accumulate" else 0,
                                          L.ptr(probs) if mode != "label" else None, L.ptr(label), L.stream_ptr())
            assert rc == 0, L.load().acr_last_error().decode()
            hp, hl = big_p.cpu().numpy(), big_l.cpu().numpy()
            assert (hp[:G] == -12345.0).all() and (hp[G + K * n:] == -12345.0).all(), mode
            assert (hl[:G] == 0xA5).all() and (hl[G + n:] == 0xA5).all(), mode
            if mode == "label":
                assert (hp == -12345.0).all()
            else:
                assert (hp[G:G + K * n] != -12345.0).all()
            assert hl[G:G + n].max() < K
            outs.append((hp.tobytes(), hl.tobytes()))
    assert outs[:3] == outs[3:]
    # the logits were only read
    assert np.array_equal(logits.cpu().numpy(), R.logits_case(tag))


# ------------------------------------------------------------------------------------------------
# CRF with the validation's parameter set
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwk", [(48, 64, 3), (61, 47, 5)])
def test_crf_inference_inf_matches_the_restatement(hwk):
    from acr_wsss_amd.crf import crf_inference_inf, crf_inference_inf_device
    h, w, k = hwk
    img, probs = R.smooth_scene(h, w, k, seed=h)
    ref = R.crf_inference_inf(img, probs, labels=k)
    got = crf_inference_inf(img, probs, labels=k, device=DEV)
    assert got.shape == (k, h, w) and got.dtype == np.float32
    # the rule of test_crf_gpu.py::_tolerance: how far one ulp at the input travels is measured on the instance
    sens = float(np.abs(R.crf_inference_inf(img, probs, labels=k, log_dtype=np.float32) - ref).max())
    tol = max(1e-4, 16.0 * sens)
    err = float(np.abs(got - ref).max())
    print("\ncrf_inference_inf %dx%dx%d: |dQ| max %.2e, mean %.2e (1-ulp sensitivity of the instance %.2e, tolerance %.2e)" % (
        h, w, k, err, float(np.abs(got - ref).mean()), sens, tol))
    assert np.abs(got - ref).mean() <= 1e-5
    assert err <= tol, (err, tol)
    top = np.sort(ref, axis=0)
    decided = (top[-1] - top[-2]) > 2 * tol
    assert decided.mean() > 0.99
    assert np.array_equal(got.argmax(0)[decided], ref.argmax(0)[decided])
    # probabilities that already sit on the device: read in place, the same bits
    on_dev = crf_inference_inf_device(img, torch.from_numpy(probs).to(DEV), labels=k)
    assert on_dev.is_cuda and on_dev.cpu().numpy().tobytes() == got.tobytes()
    with pytest.raises(ValueError):
        crf_inference_inf_device(img, torch.from_numpy(probs).to(DEV)[:, :, :-1], labels=k)
    # the other parameter set gives another answer: the two functions are not one
    from acr_wsss_amd.crf import crf_inference
    assert not np.array_equal(crf_inference(img, probs, labels=k, device=DEV), got)


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
SIZES = [(50, 67), (64, 64), (80, 45), (33, 96), (71, 40)]


@pytest.fixture(scope="module")
def seg_net():
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd.DPT.ACR import ACR
    m = ACR(20, "vitb_hybrid", seg=True, features=16, use_pretrain=False)
    m.load_state_dict({k: (recipe_tensor(k, v.shape, 0) if torch.is_floating_point(v) and "running_" not in k else v)
                       for k, v in m.state_dict().items()}, strict=True)
    torch.manual_seed(11)
    head = D.SegmentationHead(16, 20)
    return m.to(DEV).train(), head.to(DEV).train()


@pytest.fixture(scope="module")
def items():
    rng = np.random.default_rng(17)
    out = []
    for i, (h, w) in enumerate(SIZES):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        img[h // 3:, : w // 2] //= 3                                                    # some structure next to the noise
        gt = rng.integers(0, 21, (h, w)).astype(np.uint8)
        gt[rng.random((h, w)) < 0.1] = 255
        out.append(("im%d" % i, img, gt))
    return out


def own_label_maps(net, items, order, batch_size):
    """forward_seg on val_batch at the given batching and predict per image: what validate is built from"""
    from acr_wsss_amd import data
    model, head = net
    model.eval()
    head.eval()
    maps = {}
    with torch.no_grad():
        for pos in range(0, len(order), batch_size):
            grp = [items[i] for i in order[pos:pos + batch_size]]
            logits = V.forward_seg(model, head, data.val_batch([g[1] for g in grp], 64, DEV))
            assert tuple(logits.shape) == (len(grp), 21, 64, 64)
            for j, (name, img, _) in enumerate(grp):
                maps[name] = V.predict(logits[j:j + 1], img.shape[:2])[0].cpu().numpy()
    model.train()
    head.train()
    return maps


def test_validate_counts_what_forward_seg_and_predict_give(seg_net, items, tmp_path):
    from PIL import Image
    from acr_wsss_amd.evaluation import LabelCounters
    model, head = seg_net
    maps = own_label_maps(seg_net, items, list(range(len(items))), 2)
    want = LabelCounters(21)
    for name, img, gt in items:
        assert maps[name].shape == gt.shape and maps[name].max() < 21
        want.add(maps[name], gt)
    assert want.conf.sum() == sum(int((gt < 21).sum()) for _, _, gt in items) and len(np.unique(np.concatenate([m.ravel() for m in maps.values()]))) > 1
    out = str(tmp_path / "png")
    got = V.validate(model, head, items, batch_size=2, test_size=64, out_png=out)
    assert model.training and head.training                                             # modes restored
    assert isinstance(got, LabelCounters) and np.array_equal(got.conf, want.conf)
    assert got.mean_iou() == want.mean_iou()
    for name, _, _ in items:
        assert np.array_equal(np.array(Image.open(os.path.join(out, name + ".png"))), maps[name])
    # predict_image is the same path, one image at a time
    model.eval()
    head.eval()
    with torch.no_grad():
        one = V.predict_image(model, head, items[1][1], test_size=64)
    model.train()
    head.train()
    assert one.is_cuda and one.dtype == torch.uint8 and tuple(one.shape) == items[1][1].shape[:2]
    assert np.array_equal(one.cpu().numpy(), own_label_maps(seg_net, items, [1], 1)["im1"])
    # two ranks, merged
    parts = [V.validate(model, head, items, rank=r, world=2, batch_size=2, test_size=64) for r in (0, 1)]
    for r, part in enumerate(parts):
        mine = own_label_maps(seg_net, items, list(range(r, len(items), 2)), 2)
        own = LabelCounters(21)
        for name in mine:
            own.add(mine[name], items[int(name[2:])][2])
        assert np.array_equal(part.conf, own.conf)
    merged = parts[0].merge(parts[1])
    print("two ranks merged vs one rank: %d counters differ" % int((merged.conf != want.conf).sum()))
    assert np.array_equal(merged.conf, want.conf)
    # an image without gt is written but not counted; a gt of another shape raises
    nogt = [items[0], ("extra", items[2][1], None)]
    only = V.validate(model, head, nogt, batch_size=2, test_size=64, out_png=out)
    mine = own_label_maps(seg_net, nogt, [0, 1], 2)
    own = LabelCounters(21)
    own.add(mine["im0"], items[0][2])
    assert np.array_equal(only.conf, own.conf)
    assert np.array_equal(np.array(Image.open(os.path.join(out, "extra.png"))), mine["extra"])
    with pytest.raises(ValueError):
        V.validate(model, head, [("bad", items[0][1], items[1][2])], test_size=64)


@pytest.mark.parametrize("kw", [dict(scales=(1.0, 1.5), flip=True), dict(use_crf=True), dict(scales=(1.0, 1.5), flip=True, use_crf=True)],
                         ids=["tta", "crf", "tta+crf"])
def test_augmented_and_crf_validation_runs_and_repeats(seg_net, items, tmp_path, kw):
    from PIL import Image
    model, head = seg_net
    sub = items[:3]
    runs = []
    for rep in range(2):
        out = str(tmp_path / ("png%d" % rep))
        c = V.validate(model, head, sub, batch_size=2, test_size=64, out_png=out, **kw)
        maps = [np.array(Image.open(os.path.join(out, name + ".png"))) for name, _, _ in sub]
        for m, (_, img, gt) in zip(maps, sub):
            assert m.shape == img.shape[:2] and m.dtype == np.uint8 and m.max() <= 20
        assert c.conf.sum() == sum(int((gt < 21).sum()) for _, _, gt in sub) and c.conf[:, 21].sum() == 0
        runs.append((c.conf.tobytes(), [m.tobytes() for m in maps]))
    assert runs[0] == runs[1]
    with pytest.raises(ValueError):
        V.validate(model, head, sub, test_size=64, scales=(1.0, 1.2))
