"""The class-centre feature-distance loss on the device (csrc/featdis.hip through ``featdis.feature_distance_loss``) against the
float64 restatement of tests/featdis_ref.py, and inside ``seg_train_step`` / ``joint_train_step``.

Tolerance, the rule of test_segloss_gpu.py: the device's largest error against the float64 restatement may be at most twice the
error torch's own float32 shows on the same case (the reference's recorded run for the fixtures, the restatement run in float32
otherwise), with a floor of 4 * 2^-23 of the largest reference magnitude.  Labels and counts are exact."""
import functools
import os

import numpy as np
import pytest
import torch

import featdis_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP4 = 4 * 2.0 ** -23
# (B, K, C, h, w); test_featdis_cpu.py ties these to the sizes in csrc/featdis.hip
SHAPES = {
    "c1": (2, 21, 1, 6, 5),
    "c257": (2, 21, 257, 5, 4),                # ragged against every channel chunk
    "k2": (2, 2, 8, 6, 5),
    "k81": (2, 81, 12, 9, 10),                 # more classes than a wave has lanes
    "k128": (1, 128, 9, 8, 9),                 # the narrow class-sum workgroup
    "b1": (1, 21, 8, 7, 6),
    "tiny": (2, 21, 8, 3, 2),                  # fewer pixels than one pixel tile
    "slabs": (2, 21, 40, 70, 33),              # two slabs per image, the last one ragged
    "many": (2, 3, 4, 256, 257),               # enough pixel tiles for the four-group dot-product workgroup
}


def device_run(seg, feat, upstream=None):
    """-> (loss, dis, pixel_dis, d_feat, labels, counts) as numpy / floats, and the raw bytes of loss and gradient"""
    from acr_wsss_amd.featdis import feature_distance_loss
    s = torch.from_numpy(seg).to(DEV)
    f = torch.from_numpy(feat).to(DEV).requires_grad_(True)
    loss, dis, pix, labels, counts = feature_distance_loss(s, f, return_stats=True)
    assert loss.shape == () and loss.dtype == torch.float32 and not dis.requires_grad and not pix.requires_grad
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (seg.shape[0],) + seg.shape[2:]
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (seg.shape[0] + seg.shape[1] - 1,)
    (loss if upstream is None else upstream(loss, f)).backward()
    assert s.grad is None
    return (float(loss.detach()), float(dis), float(pix), f.grad.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy(),
            loss.detach().cpu().numpy().tobytes() + f.grad.cpu().numpy().tobytes())


def bound(ref, fp32):
    """twice the float32 error against the float64 value, at least 4 * 2^-23 of the largest reference magnitude"""
    ref = np.asarray(ref, np.float64)
    return max(2 * float(np.abs(np.asarray(fp32, np.float64) - ref).max()), ULP4 * float(np.abs(ref).max()))


def check(tag, got, ref64, ref32):
    loss, dis, pix, grad, labels, counts, _ = got
    assert np.array_equal(labels, ref64[4]) and np.array_equal(counts, ref64[5])
    for name, g, r, t in (("loss", loss, ref64[0], ref32[0]), ("dis", dis, ref64[1], ref32[1]), ("pixel_dis", pix, ref64[2], ref32[2]),
                          ("d_feat", grad, ref64[3], ref32[3])):
        err, tol = float(np.abs(np.asarray(g, np.float64) - r).max()), bound(r, t)
        print("%s %s: device apart %.3e, allowed %.3e (largest %.3e)" % (tag, name, err, tol, float(np.abs(r).max())))
        assert np.isfinite(np.asarray(g)).all() and err <= tol, (tag, name, err, tol)


@functools.lru_cache(maxsize=None)
def seeded(name):
    B, K, C, h, w = SHAPES[name]
    seg, feat = R.seeded_case(B, K, C, h, w, seed=sum(map(ord, name)))
    return seg, feat, R.loss_and_grad(seg, feat, torch.float64), R.loss_and_grad(seg, feat, torch.float32)


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fixtures_of_the_reference(tag):
    z = np.load(os.path.join(GOLDEN, "featdis_%s.npz" % tag))
    ref64 = R.loss_and_grad(z["seg"], z["feat"], torch.float64)
    dis32, pix32 = R.loss_and_grad(z["seg"], z["feat"], torch.float32)[1:3]
    assert np.array_equal(ref64[4], z["labels"]) and np.array_equal(ref64[5], z["counts"])
    check(tag, device_run(z["seg"], z["feat"]), ref64, (float(z["loss"]), dis32, pix32, z["d_feat"]))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_at_which_the_kernels_can_go_wrong(name):
    seg, feat, ref64, ref32 = seeded(name)
    B, K = seg.shape[:2]
    if name != "k2":
        assert len(np.unique(ref64[4])) > 2
    check(name, device_run(seg, feat), ref64, ref32)


def test_a_class_that_owns_exactly_one_pixel():
    seg, feat = R.seeded_case(2, 21, 8, 6, 7, seed=77)
    seg[:, 7] = -9
    seg[1, 7, 2, 3] = 9
    ref64 = R.loss_and_grad(seg, feat, torch.float64)
    assert ref64[5][2 + 7 - 1] == 1 and ref64[4][1, 2, 3] == 7
    check("one pixel", device_run(seg, feat), ref64, R.loss_and_grad(seg, feat, torch.float32))


def test_ties_go_to_the_first_index_and_a_nan_is_the_maximum():
    seg, feat = R.seeded_case(2, 21, 8, 9, 8, seed=5, integer_logits=True)
    seg[0, 3, 2, 2] = np.nan
    seg[1, 0, 4, 4] = seg[1, 6, 4, 4] = np.nan
    expect = torch.from_numpy(seg).argmax(1).numpy()
    assert expect[0, 2, 2] == 3 and expect[1, 4, 4] == 0 and (np.sort(seg, 1)[:, -1] == np.sort(seg, 1)[:, -2]).mean() > 0.5     # ties nearly everywhere
    ref64 = R.loss_and_grad(seg, feat, torch.float64)
    assert np.array_equal(ref64[4], expect)
    check("ties", device_run(seg, feat), ref64, R.loss_and_grad(seg, feat, torch.float32))


def test_all_zero_feature_vectors():
    """one in a background region, one in a foreground class: their gradient (of order 1 / eps) and the gradient everywhere else are
    compared separately, each against its own largest magnitude; the zero pixel adds nothing to its centre's gradient, so the
    other pixels keep an ordinary one"""
    seg, feat = R.fixture_case("a")
    lab = seg.argmax(1)
    bg, fg = np.argwhere(lab == 0)[0], np.argwhere(lab != 0)[0]
    zero = np.zeros(lab.shape, bool)
    for b, y, x in (bg, fg):
        feat[b, :, y, x] = 0
        zero[b, y, x] = True
    ref64, ref32 = R.loss_and_grad(seg, feat, torch.float64), R.loss_and_grad(seg, feat, torch.float32)
    got = device_run(seg, feat)
    check("zero vectors (loss)", got[:3] + (np.zeros(1),) + got[4:], ref64[:3] + (np.zeros(1),) + ref64[4:], ref32[:3] + (np.zeros(1),) + ref32[4:])
    m = np.broadcast_to(zero[:, None], feat.shape)
    for what, sel in (("the zero pixels", m), ("every other pixel", ~m)):
        err, tol = float(np.abs(got[3][sel] - ref64[3][sel]).max()), bound(ref64[3][sel], ref32[3][sel])
        print("%s: device apart %.3e, allowed %.3e (largest %.3e)" % (what, err, tol, float(np.abs(ref64[3][sel]).max())))
        assert np.isfinite(got[3]).all() and err <= tol, what
    assert np.abs(ref64[3][m]).max() > 1e3 > np.abs(ref64[3][~m]).max() and np.abs(got[3][~m]).max() < 1e3


def test_an_upstream_factor_and_a_larger_graph():
    seg, feat, ref64, ref32 = seeded("b1")
    got = device_run(seg, feat, upstream=lambda loss, f: 2.5 * loss + f.sum())
    want, want32 = 2.5 * ref64[3] + 1.0, (2.5 * ref32[3].astype(np.float64) + 1.0).astype(np.float32)
    err, tol = float(np.abs(got[3] - want).max()), bound(want, want32)
    print("upstream 2.5, + feat.sum(): device apart %.3e, allowed %.3e" % (err, tol))
    assert err <= tol
    plain = device_run(seg, feat)
    assert got[0] == plain[0] and not np.array_equal(got[3], plain[3])


@pytest.mark.parametrize("name", ["slabs", "k81"])
def test_forward_and_backward_are_bit_identical_run_to_run(name):
    seg, feat, _, _ = seeded(name)
    assert device_run(seg, feat)[6] == device_run(seg, feat)[6]


def test_contiguity_and_the_drop_in_name():
    """a channels-last feature tensor gives what its contiguous copy gives, and seg takes no gradient even when it asks for one"""
    from acr_wsss_amd.featdis import compute_dis_no_batch
    seg, feat, _, _ = seeded("b1")
    s = torch.from_numpy(seg).to(DEV).requires_grad_(True)
    f = torch.from_numpy(feat).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    loss = compute_dis_no_batch(s, f)
    loss.backward()
    plain = device_run(seg, feat)
    assert s.grad is None and float(loss.detach()) == plain[0] and np.array_equal(f.grad.cpu().numpy(), plain[3])


# ---- the head and the two steps ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    """model, head and batch of test_jointtrain_gpu.py (their builders), with a label map for ``seg_train_step``"""
    import test_jointtrain_gpu as TJ
    model, head = TJ.build("vitb_hybrid", "decoder_hybrid_64")
    state = ({k: v.detach().clone() for k, v in model.state_dict().items()}, {k: v.detach().clone() for k, v in head.state_dict().items()})
    images, ori, crop, labels, sal = TJ.make_batch(43)
    rng = np.random.default_rng(44)
    seg_label = rng.integers(0, 21, (2, 64, 64)).astype(np.uint8)
    seg_label[rng.random(seg_label.shape) < 0.1] = 255
    yield model, head, state, dict(seg=(images, ori, crop, torch.from_numpy(seg_label).to(DEV)), joint=(images, ori, crop, labels, sal))
    model.set_math("f32")


WATCHED = ("head.0.weight", "head.4.weight", "model.scratch.layer1_rn.weight")


def run_step(rig, kind, **kw):
    """one step from the recorded state under torch.manual_seed(6) (the head's Dropout) -> (loss bytes, terms, watched gradients)"""
    import test_jointtrain_gpu as TJ
    from acr_wsss_amd import segtrain
    from acr_wsss_amd.train import PolyOptimizer
    model, head, state, batches = rig
    model.load_state_dict(state[0])
    head.load_state_dict(state[1])
    params = list(model.parameters()) + list(head.parameters())
    for p in params:
        p.grad = None
    opt = PolyOptimizer(params, lr=TJ.LR, weight_decay=5e-4, max_step=100)
    torch.manual_seed(6)
    if kind == "seg":
        loss, terms = segtrain.seg_train_step(model, head, opt, *batches["seg"], None, **kw)
    else:
        loss, terms = segtrain.joint_train_step(model, head, opt, *batches["joint"], None, alpha=TJ.ALPHA, **kw)
    named = dict([("model." + k, p) for k, p in model.named_parameters()] + [("head." + k, p) for k, p in head.named_parameters()])
    return TJ.raw(loss), terms, {k: TJ.raw(named[k].grad) for k in WATCHED}


def head_tensors(rig, kind):
    """(logits, feat, logits_half) of the head in the step's own pass, from the recorded state under the step's seed"""
    import test_jointtrain_gpu as TJ
    from acr_wsss_amd import decoder
    model, head, state, batches = rig
    model.load_state_dict(state[0])
    head.load_state_dict(state[1])
    model.invalidate_caches()
    images = batches[kind][0]
    torch.manual_seed(6)
    if kind == "seg":
        decoded = decoder.decode(model, images)
    else:
        model.forward_mirror(images, images.flip(-1))
        TJ.hand_targets(model, batches["joint"][3], batches["joint"][4], 64)
        decoded = decoder.decode_taps(model, model.pretrained.activations, (64, 64), rows=images.shape[0])
    rng = torch.cuda.get_rng_state()
    out = tuple(t.detach() for t in head.forward_features(decoded))
    torch.cuda.set_rng_state(rng)
    return out, head(decoded).detach()


def test_forward_features_returns_the_logits_of_forward(rig):
    import test_jointtrain_gpu as TJ
    (logits, feat, half), plain = head_tensors(rig, "seg")
    assert TJ.raw(logits) == TJ.raw(plain)
    assert tuple(feat.shape) == (2, 16, 32, 32) and tuple(half.shape) == (2, 21, 32, 32) and tuple(logits.shape) == (2, 21, 64, 64)
    head = rig[1]
    from acr_wsss_amd.decoder import conv, upsample2x
    assert TJ.raw(conv(head[4], feat, head.acr_math)) == TJ.raw(half) and TJ.raw(upsample2x(half)) == TJ.raw(logits)


@pytest.mark.parametrize("kind", ["seg", "joint"])
def test_the_steps_with_the_weight_off_and_on(rig, kind):
    import test_jointtrain_gpu as TJ
    from acr_wsss_amd.featdis import feature_distance_loss
    base, off, on = run_step(rig, kind), run_step(rig, kind, dis_weight=0), run_step(rig, kind, dis_weight=0.1)
    assert base[0] == off[0] and base[2] == off[2] and set(base[1]) == set(off[1]) and "disloss" not in off[1]
    assert set(on[1]) == set(base[1]) | {"disloss"}
    (_, feat, half), _ = head_tensors(rig, kind)
    expect = feature_distance_loss(half, feat)
    assert TJ.raw(on[1]["disloss"]) == TJ.raw(expect) and np.isfinite(float(expect)) and float(expect) > 0
    assert TJ.raw(on[1]["celoss"]) == TJ.raw(base[1]["celoss"])
    assert on[0] != base[0] and on[2]["head.0.weight"] != base[2]["head.0.weight"]
    rest = float(on[1]["loss"].detach()) - 0.1 * float(expect)
    assert abs(rest - float(base[1]["loss"].detach())) <= 1e-5 * abs(rest)
