"""The affinity stage on the GPU (csrc/affinity.hip through acr_wsss_amd.affinity) against the restatement tests/affinity_ref.py,
which tests/test_affinity_cpu.py pins to fixtures written by the reference's own classes.

Pair codes and counts are integers: exact equality.  For floating-point results the rule of tests/test_pamr_gpu.py: with
E = max|fp32 restatement - fp64 restatement| -- the restatement's OWN fp32 error, taken separately for every quantity (each of
the four loss values, aff, d feat; the walk's output) -- the kernel must lie within 4 * E of the fp64 restatement: x 2 for a second
valid fp32 evaluation order, x 2 for libm differences.  E is never the kernel's own error; every figure is printed before it is
asserted.

One check of the issue is stated differently here because the property as worded does not hold: a plane's plain sum is NOT
invariant under a column-stochastic T (that needs unit ROW sums); what new = old . T conserves is the sum weighted by the column
sums, sum_j colsum[j] new[j] = sum_i colsum[i] old[i] (A symmetric).  test_walk_conserves_the_weighted_plane_sum checks that,
within the same 4 * E per pixel."""
import os

import numpy as np
import pytest
import torch

import affinity_ref as R
from conftest import load_golden
from recipe import recipe_tensor

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
LABELS = torch.tensor([0, 0, 1, 2, 255], dtype=torch.uint8)
GRIDS = [(5, 9, 9), (5, 12, 17), (3, 6, 7), (5, 5, 75)]          # (radius, h, w); 5 x 75: one from-row wider than a wave


def _label_grid(g, B, h, w):
    return LABELS[torch.randint(0, 5, (B, h, w), generator=g)]


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


# ---- pair codes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["r5_9", "r5_28", "r3_6", "r2_3"])
def test_pair_codes_equal_the_reference_masks(tag):
    from acr_wsss_amd.affinity import pair_codes
    g = np.load(os.path.join(GOLD, "affinity_%s.npz" % tag))
    radius = int(g["radius"])
    codes, counts = pair_codes(torch.from_numpy(g["label"]).to(DEV), radius, 1)
    codes = codes.cpu().numpy()[0]
    for k, name in ((1, "bg"), (2, "fg"), (3, "neg")):
        assert np.array_equal((codes == k).astype(np.uint8), g[name]), name
    assert counts.dtype == torch.int64 and counts.tolist() == [int(g["bg"].sum()), int(g["fg"].sum()), int(g["neg"].sum())]


@pytest.mark.parametrize("radius,h,w", GRIDS)
@pytest.mark.parametrize("stride", [8, 1])
def test_pair_codes_equal_the_restatement(radius, h, w, stride):
    from acr_wsss_amd.affinity import pair_codes
    g = torch.Generator().manual_seed(1000 * h + w + stride)
    grid = _label_grid(g, 3, h, w)
    if stride == 1:
        full = grid
    else:                                                    # every pixel off the sampling lattice holds another random label
        full = _label_grid(g, 3, h * stride, w * stride)
        full[:, ::stride, ::stride] = grid
    want, want_counts = R.pair_codes(full, radius, stride)
    assert torch.equal(want, R.pair_codes(grid, radius, 1)[0])
    codes, counts = pair_codes(full.to(DEV), radius, stride)
    assert codes.dtype == torch.uint8 and torch.equal(codes.cpu(), want)
    assert counts.cpu().tolist() == want_counts.tolist()
    for b in range(3):                                       # B = 1: each sample is independent of its batch
        one, n1 = pair_codes(full[b:b + 1].to(DEV), radius, stride)
        assert torch.equal(one[0], codes[b])
        assert n1.cpu().tolist() == [int((want[b] == k).sum()) for k in (1, 2, 3)]
    none, n0 = pair_codes(torch.full_like(full, 255).to(DEV), radius, stride)
    assert not none.any() and n0.cpu().tolist() == [0, 0, 0]


def test_pair_codes_refuse_bad_arguments():
    from acr_wsss_amd.affinity import pair_codes
    m = torch.zeros(1, 64, 64, dtype=torch.uint8, device=DEV)
    for args in ((m, 5, 7), (m[:, :32], 5, 8), (m[:, :, :64], 6, 8), (m, 1, 8)):      # 64 / 7; 4 x 8 grid; radius not built
        with pytest.raises(ValueError):
            pair_codes(*args)
    with pytest.raises(ValueError):
        pair_codes(m.cpu().float(), 5, 8)


# ---- loss and gradient --------------------------------------------------------------------------------------------------------
def _features(seed, B, C, h, w):
    """class-dependent means plus noise: pairs inside a class are near, pairs across classes far"""
    g = torch.Generator().manual_seed(seed)
    label = _label_grid(g, B, h, w)
    means = torch.randn(256, C, generator=g)
    feat = means[label.long()].permute(0, 3, 1, 2) + 0.3 * torch.randn(B, C, h, w, generator=g)
    return label, feat.contiguous()


def _restated(feat, codes, counts, radius, upstream):
    out = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        f = feat.detach().to(dt).clone().requires_grad_(True)
        loss, bg, fg, neg, aff = R.aff_loss(f, codes, counts, radius)
        (loss * upstream).backward()
        out[name] = dict(loss=loss.detach().double(), bg=bg.detach().double(), fg=fg.detach().double(), neg=neg.detach().double(),
                         aff=aff.detach().double(), dfeat=f.grad.double())
    return out


def _kernel(feat, codes, counts, radius, upstream):
    from acr_wsss_amd.affinity import _aff_loss
    f = feat.detach().to(DEV).requires_grad_(True)
    loss, terms, aff = _aff_loss(f, codes.to(DEV), counts.to(DEV), radius)
    (loss * upstream).backward()
    torch.cuda.synchronize()
    return dict(loss=loss.detach().cpu(), bg=terms[0].cpu(), fg=terms[1].cpu(), neg=terms[2].cpu(), aff=aff.cpu(), dfeat=f.grad.cpu())


def _check(tag, got, ref):
    for key in ("loss", "bg", "fg", "neg", "aff", "dfeat"):
        e = float((ref["32"][key] - ref["64"][key]).abs().max())
        err = float((got[key].double() - ref["64"][key]).abs().max())
        print("%s %s: E = %.3e, max|kernel - ref64| = %.3e (%.2f E)" % (tag, key, e, err, err / e if e else float("inf") if err else 0.0))
        assert got[key].dtype == torch.float32 and tuple(got[key].shape) == tuple(ref["64"][key].shape), key
        assert err <= 4 * e, key


@pytest.mark.parametrize("shape", [(2, 5, 9, 9), (2, 70, 12, 17), (1, 448, 28, 28), (2, 3, 5, 75)])
def test_loss_and_gradient_against_the_restatement(shape):
    label, feat = _features(sum(shape), *shape)
    codes, counts = R.pair_codes(label, 5, 1)
    assert all(int(c) > 0 for c in counts)
    _check("x".join(map(str, shape)), _kernel(feat, codes, counts, 5, 1.0), _restated(feat, codes, counts, 5, 1.0))


def test_loss_upstream_gradient_radius_3_and_repeatability():
    from acr_wsss_amd.affinity import aff_loss, pair_affinity, pair_codes
    label, feat = _features(7, 2, 9, 6, 7)
    codes, counts = R.pair_codes(label, 3, 1)
    got = _kernel(feat, codes, counts, 3, -2.5)
    _check("R 3, upstream -2.5", got, _restated(feat, codes, counts, 3, -2.5))
    again = _kernel(feat, codes, counts, 3, -2.5)
    for key in got:
        assert _bytes(got[key]) == _bytes(again[key]), key      # two runs: identical bits
    assert _bytes(pair_affinity(feat.to(DEV), 3)) == _bytes(got["aff"])         # the inference forward is the same arithmetic
    dcodes, dcounts = pair_codes(label.to(DEV), 3, 1)
    loss, bg, fg, neg = aff_loss(feat.to(DEV), dcodes, dcounts)                  # radius from the codes' shape
    assert _bytes(loss) == _bytes(got["loss"]) and _bytes(neg) == _bytes(got["neg"])
    one = _kernel(feat[1:], codes[1:], counts, 3, -2.5)                          # same batch counts: the sample's own aff and gradient
    assert _bytes(one["aff"][0]) == _bytes(got["aff"][1]) and _bytes(one["dfeat"][0]) == _bytes(got["dfeat"][1])


def test_loss_edge_cases_are_exact():
    label, feat = _features(11, 2, 6, 9, 12)
    codes, counts = R.pair_codes(label, 5, 1)
    flat = torch.full_like(feat, 0.375)
    got = _kernel(flat, codes, counts, 5, 1.0)                  # constant features: d = 0, aff = 1, sign(0) = 0
    assert torch.equal(got["aff"], torch.ones_like(got["aff"]))
    assert torch.equal(got["dfeat"], torch.zeros_like(got["dfeat"]))
    ref = R.aff_loss(flat.double(), codes, counts, 5)
    for key, want in zip(("loss", "bg", "fg", "neg"), ref):
        assert abs(float(got[key]) - float(want)) <= 2.0 ** -23 * abs(float(want)), key
    none = torch.full_like(label, 255)
    c0, n0 = R.pair_codes(none, 5, 1)
    got = _kernel(feat, c0, n0, 5, 1.0)                         # no labelled pair: every term and the gradient exactly 0, no NaN
    for key in ("loss", "bg", "fg", "neg"):
        assert float(got[key]) == 0.0, key
    assert torch.equal(got["dfeat"], torch.zeros_like(got["dfeat"]))
    assert torch.isfinite(got["aff"]).all()


def test_loss_refuses_bad_arguments():
    from acr_wsss_amd.affinity import aff_loss, pair_affinity
    label, feat = _features(3, 1, 4, 9, 9)
    codes, counts = (t.to(DEV) for t in R.pair_codes(label, 5, 1))
    f = feat.to(DEV)
    for args in ((f.double(), codes, counts), (f, codes.float(), counts), (f, codes, counts.int()), (f, codes[:, :5], counts),
                 (f, codes.cpu(), counts), (f[:, :, :4], codes, counts)):
        with pytest.raises(ValueError):
            aff_loss(*args)
    with pytest.raises(ValueError):
        pair_affinity(f[:, :, :, :8], 5)                       # w <= 2 r


# ---- random walk --------------------------------------------------------------------------------------------------------------
WALKS = [(2, 1, 9, 9), (2, 21, 12, 17), (1, 8, 56, 56)]         # (B, K, h, w)
_WALK_CACHE = {}


def _walk_case(B, K, h, w):
    """inputs and both restatements per step count, computed once per geometry and shared (treat as read-only)"""
    key = (B, K, h, w)
    if key not in _WALK_CACHE:
        g = torch.Generator().manual_seed(h * w + K)
        P, N = len(R.search_dist(5)), (h - 4) * (w - 8)
        aff = (torch.rand(B, P, N, generator=g) * 0.7 + 0.3).to(DEV)
        scores = torch.rand(B, K, h, w, generator=g).to(DEV)
        refs = {}
        for steps in (0, 1, 2, 256):
            r64 = torch.stack([R.walk_dense(aff[b].double(), scores[b].double(), 5, 8, 8 if steps == 256 else None, steps) for b in range(B)])
            r32 = torch.stack([R.walk_steps(aff[b], scores[b], 5, 8, steps) for b in range(B)])
            refs[steps] = (r64, float((r32.double() - r64).abs().max()))
        _WALK_CACHE[key] = (aff, scores, refs)
    return _WALK_CACHE[key]


@pytest.mark.parametrize("B,K,h,w", WALKS)
def test_walk_against_the_dense_power(B, K, h, w):
    from acr_wsss_amd.affinity import random_walk
    aff, scores, refs = _walk_case(B, K, h, w)
    for steps in (0, 1, 2, 256):
        r64, e = refs[steps]
        kw = dict(logt=8) if steps == 256 else dict(logt=None, steps=steps)
        out = random_walk(aff, scores, **kw)
        res, stp = random_walk(aff, scores, resident=True, **kw), random_walk(aff, scores, resident=False, **kw)
        err = float((out.double() - r64).abs().max())
        print("%d x %d x %d x %d, %d steps: E = %.3e, max|kernel - dense fp64| = %.3e (%.2f E)" % (B, K, h, w, steps, e, err, err / e if e else 0.0))
        assert out.dtype == torch.float32 and out.shape == scores.shape
        assert torch.equal(res, stp) and torch.equal(out, res)           # resident and stepwise forms: bit for bit
        if steps == 0:
            assert torch.equal(out, scores) and out.data_ptr() != scores.data_ptr()
        else:
            assert err <= 4 * e
        if B > 1:                                                        # a sample does not depend on its batch
            assert torch.equal(random_walk(aff[1:], scores[1:], **kw)[0], out[1])


def test_walk_uniform_affinity_keeps_a_constant():
    from acr_wsss_amd.affinity import random_walk
    h, w, P, N = 12, 17, 34, 8 * 9
    aff = torch.full((1, P, N), 0.8, device=DEV)
    for c in (1.0, 0.37):
        scores = torch.full((1, 3, h, w), c, device=DEV)
        r64 = R.walk_dense(aff[0].double(), scores[0].double(), 5, 8, 8)
        e = float((R.walk_steps(aff[0], scores[0], 5, 8, 256).double() - r64).abs().max())
        e = max(e, 2.0 ** -24 * c)                                       # the restatement may hit c exactly; one rounding of c is the floor
        c = float(np.float32(c))                                         # the constant the fp32 tensor holds
        assert float((r64 - c).abs().max()) <= 1e-13
        for resident in (True, False):
            dev = float((random_walk(aff, scores, resident=resident).double() - c).abs().max())
            print("constant %g, resident %s: max deviation %.3e, E = %.3e" % (c, resident, dev, e))
            assert dev <= 4 * e


def test_walk_conserves_the_weighted_plane_sum():
    """sum_j colsum[j] new[j] = sum_i colsum[i] old[i] for symmetric A (module docstring)"""
    from acr_wsss_amd.affinity import random_walk
    B, K, h, w = 2, 21, 12, 17
    aff, scores, refs = _walk_case(B, K, h, w)
    e = refs[256][1]
    out = random_walk(aff, scores)
    for b in range(B):
        frm, to = R.pair_indices(5, h, w)
        A = torch.eye(h * w, dtype=torch.float64, device=DEV)
        a = aff[b].double().reshape(-1) ** 8
        f, t = frm[None].expand_as(to).reshape(-1).to(DEV), to.reshape(-1).to(DEV)
        A[f, t] = a
        A[t, f] = a
        colsum = A.sum(0)
        before = (scores[b].double().reshape(K, -1) * colsum).sum(1)
        after = (out[b].double().reshape(K, -1) * colsum).sum(1)
        bound = 4 * e * float(colsum.sum())
        print("image %d: max|weighted sum after - before| = %.3e, bound %.3e" % (b, float((after - before).abs().max()), bound))
        assert float((after - before).abs().max()) <= bound


def test_walk_refuses_bad_arguments():
    from acr_wsss_amd._lib import AcrHipError
    from acr_wsss_amd.affinity import random_walk
    aff = torch.rand(1, 34, 92 * 88, device=DEV)
    scores = torch.rand(1, 2, 96, 96, device=DEV)
    with pytest.raises(AcrHipError):
        random_walk(aff, scores, resident=True)                  # two padded 96 x 96 planes exceed the LDS budget
    out = random_walk(aff, scores, logt=None, steps=3)           # the stepwise form is chosen
    assert torch.equal(out, random_walk(aff, scores, logt=None, steps=3, resident=False))
    r64 = R.walk_steps(aff[0].double(), scores[0].double(), 5, 8, 3)          # the sparse form, pinned to the dense power on the CPU
    e = float((R.walk_steps(aff[0], scores[0], 5, 8, 3).double() - r64).abs().max())
    err = float((out[0].double() - r64).abs().max())
    print("96 x 96, 3 steps, stepwise: E = %.3e, err = %.3e" % (e, err))
    assert err <= 4 * e
    for kw in (dict(logt=8, steps=2), dict(logt=None), dict(logt=None, steps=-1)):
        with pytest.raises(ValueError):
            random_walk(aff, scores, **kw)
    with pytest.raises(ValueError):
        random_walk(aff[:, :, :100], scores)
    with pytest.raises(ValueError):
        random_walk(aff, scores.double())
    with pytest.raises(AcrHipError):
        random_walk(aff, scores, beta=0)


# ---- layers -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layers():
    """the small hybrid seg=True model of tests/test_segtrain_gpu.py and an AffinityHead on its 16 features"""
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
    torch.manual_seed(5)
    head = AffinityHead(16, dims=(8, 8, 16), out_dim=24).to(DEV).train()
    set_math(head, "f32_split")
    g = torch.Generator().manual_seed(9)
    images = torch.randn(2, 3, 64, 96, generator=g).to(DEV)
    label = _label_grid(g, 2, 8, 12).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous().to(DEV)
    yield model, head, {k: v.detach().clone() for k, v in head.state_dict().items()}, images, label
    model.set_math("f32")


def test_aff_train_step_equals_the_hand_composition(layers):
    from acr_wsss_amd import affinity as A
    from acr_wsss_amd import decoder
    from acr_wsss_amd.train import PolyOptimizer
    model, head, state, images, label = layers
    with torch.no_grad():
        before = decoder.decode(model, images).clone()

    def run(how):
        head.load_state_dict(state)
        for p in list(model.parameters()) + list(head.parameters()):
            p.grad = None
        opt = PolyOptimizer(list(head.parameters()), lr=0.01, weight_decay=5e-4, max_step=100)
        if how == "step":
            terms = A.aff_train_step(model, head, opt, images, label)
        else:
            opt.zero_grad(set_to_none=True)
            feat = head(decoder.layers_rn(model, images))
            assert tuple(feat.shape) == (2, 24, 8, 12)
            codes, counts = A.pair_codes(label, 5, 8)
            assert tuple(codes.shape) == (2, 34, 16)
            terms = A.aff_loss(feat, codes, counts, 5)
            terms[0].backward()
            opt.step()
        return [_bytes(t) for t in terms], {k: _bytes(v) for k, v in head.state_dict().items()}, [float(t) for t in terms]

    a, hand = run("step"), run("hand")
    print("aff_train_step terms (loss, bg, fg, neg):", a[2])
    assert all(np.isfinite(v) for v in a[2]) and a[2][0] > 0
    assert a[0] == hand[0] and a[1] == hand[1]
    assert all(a[1][k] != _bytes(state[k]) for k in a[1])        # every convolution of the head moved
    with torch.no_grad():
        assert torch.equal(decoder.decode(model, images), before)   # the decoder's own path is untouched


def test_aff_with_alpha_device_equals_its_parts(layers):
    from acr_wsss_amd import _lib as L
    from acr_wsss_amd import affinity as A
    from acr_wsss_amd import decoder
    from acr_wsss_amd.pamr import pamr_with_alpha_device
    model, head, state, _, _ = layers
    head.load_state_dict(state)
    rng = np.random.default_rng(4)
    h, w, alphas = 50, 70, [4, 24]
    cam_dict = {3: rng.random((h, w), dtype=np.float32), 11: rng.random((h, w), dtype=np.float32)}
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    classes, refined = A.aff_with_alpha_device(model, head, cam_dict, alphas, img, logt=3, device=DEV)
    pc, pr = pamr_with_alpha_device(cam_dict, alphas, img, device=DEV)
    assert classes == pc == [3, 11] and refined.shape == pr.shape == (6, h, w) and refined.dtype == pr.dtype and refined.is_contiguous()
    assert torch.isfinite(refined).all()
    _, scores = A.score_stack(cam_dict, alphas)
    with torch.no_grad():
        x, s = A.aff_inputs(scores, img, torch.device(DEV))
        assert tuple(x.shape) == (1, 3, 64, 96) and tuple(s.shape) == (1, 6, 8, 12)
        assert float(x[0, :, 50:].abs().max()) == 0.0 and float(x[0, :, :, 70:].abs().max()) == 0.0
        walked = A.random_walk(A.pair_affinity(head(decoder.layers_rn(model, x)), 5), s, 8, 3)
        full = torch.empty(6, 64, 96, device=DEV)
        L.check(L.load().acr_bilinear_resize(L.ptr(walked), 96, 1, 6, 8, 12, L.ptr(full), 64, 96, 0, None, 0, 0, L.stream_ptr()), "resize")
    assert torch.equal(refined, full[:, :h, :w])
    assert _bytes(refined) == _bytes(A.aff_with_alpha_device(model, head, cam_dict, alphas, img, logt=3, device=DEV)[1])
