"""Every HIP launch of the model, at the shapes the product runs, against float64.

Each case runs the real model once under the launch census (tests/launch_census.py): a training step (forward, ACR loss with
consistency and MLSM, backward) or CAM generation over the four scales.  The recorder keeps the distinct launches of the public
``ops`` entries; each then runs through its checker -- seeded inputs at exactly the recorded shapes, the same path, output and
every gradient against float64 at the tolerance of that kernel's own test.  The hand-written kernel tests pick their shapes; this
file takes them from the shipped geometries (448^2 -> T = 785, COCO 512^2 -> T = 1025, CAM 384^2 x {0.5, 1, 1.5, 2} ->
T = 145 / 577 / 1297 / 2305) -- and from geometries that are no multiple of 32 (80^2, 112^2, CAM generation at 160^2 x the four
scales), where the stage maps are 20 / 10 / 5, 28 / 14 / 7, 30 / 15: every stage mixes hand-written kernels and library calls, and
the kernels run at the edges of their dispatch predicates (tests/test_dispatch_gpu.py has those edges one by one).

The same runs audit the library fallbacks: stock F.conv2d / F.linear / F.layer_norm / F.group_norm calls made on behalf of the
model are pinned per case with their reason, so that a dispatch change has to be deliberate.
"""
import time

import pytest
import torch

import launch_census as LC
from conftest import recipe_sd
from recipe import make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(kind, math):
    from acr_wsss_amd.DPT.ACR import ACR
    m = ACR(num_classes=80 if kind == "coco" else 20, backbone_name="vit_tiny" if kind == "tiny" else "vitb_hybrid", use_pretrain=False)
    m.load_state_dict(recipe_sd(kind), strict=(kind != "tiny"))
    return m.to(DEV).set_math(math)


def _census(run):
    census, audit = LC.Census(), LC.FallbackAudit()
    with pytest.MonkeyPatch.context() as mp:
        census.install(mp)
        audit.install(mp)
        run()
        torch.cuda.synchronize()
    return census, audit


def _check(case, census):
    t0 = time.time()
    cmp = LC.Cmp()
    LC.check_all(census.records, cmp)
    print("\n[census] %s: %s" % (case, census.summary()))
    for rec in sorted(census.records, key=LC.fmt):
        print("[census]   %4d x %s" % (census.counts[rec], LC.fmt(rec)))
    print("[census] %s: %d comparisons in %.1f s, %d failures" % (case, cmp.compared, time.time() - t0, len(cmp.failures)))
    assert census.launches > 0 and cmp.compared > 0
    return ["%s: %d failing launches:\n%s" % (case, len(cmp.failures), "\n".join(cmp.failures))] if cmp.failures else []


def _audit(case, audit, pinned):
    found = audit.sites()
    print("[fallbacks] %s: %s" % (case, ["%s from %s.%s" % s for s in found]))
    return [] if set(found) == set(pinned) else ["%s: library fallbacks %s, pinned %s" % (case, found, sorted(pinned))]


# Library calls of a training step that are not a missing kernel.  The final LayerNorm (VisionTransformer.norm) runs once on the
# (2B, T, 768) tokens; ACR reads the taps, not its output (DPT/ACR.py:100-105), so it is the reference's unused tail, left on the
# stock op.  cls_head: the 768 -> C classifier on the class token and the mean patch token, two (2B, 768) rows.
TRAIN_FALLBACKS = {
    ("layer_norm", "backbone", "VisionTransformer.forward_flex"): "the final LayerNorm: computed, never read by ACR",
    ("linear", "ACR", "ACR.forward_cls"): "cls_head on 2B class / mean-patch tokens (a (2B, 768) x (768, C) product)",
}
# exact fp32 has no HIP 3x3 or strided convolution: those kernels exist for split products only (ops.conv3x3_fusable,
# ops.conv_s2_fusable), so the stem's 3x3, 7x7/2 and 3x3/2 convolutions run on MIOpen under "f32"
EXACT_CONVS = {("conv2d", "backbone", "StdConv2dSame.forward"): "3x3 and strided (7x7/2, 3x3/2) stem convolutions: split-product kernels only"}
# vit_tiny's rows are 192 wide: the HIP LayerNorm covers C % 256 == 0 (ops.layer_norm_fusable), and its patch embedding is an
# nn.Conv2d 16x16/16 on the image (PatchEmbed) -- the hybrid stem's kernels do not apply
TINY_FALLBACKS = {**TRAIN_FALLBACKS, **{
    ("layer_norm", "ops", "layer_norm_skip"): "192-wide rows: the HIP LayerNorm takes C % 256 == 0",
    ("conv2d", "backbone", "VisionTransformer.embed_tokens"): "PatchEmbed's 16x16/16 convolution of the image (vit_tiny)",
}}
# CAM generation: the backward stops at the GETAM start layer, so the final LayerNorm never runs
CAM_FALLBACKS = {
    "f32": {
        **EXACT_CONVS,
        ("linear", "ACR", "ACR.forward_cam"): "cls_head on B class / mean-patch tokens",
    },
    "f32_split": {
        ("linear", "ACR", "ACR.forward_cam"): "cls_head on B class / mean-patch tokens",
    },
}
# nothing of the stem, the norms or the block Linears may reach the library in an f32_split step at the shipped geometries
NO_FALLBACK_CALLERS = ("StdConv2dSame", "GroupNormAct", "MaxPool2dSame", "Block", "Mlp", "Attention", "linear_or_hip", "layer_norm_skip",
                       "ResNetV2", "Bottleneck")


def _audit_shapes(case, audit, sites, shapes):
    """The awkward geometries pin every stem fallback WITH the shape of its first input (``shapes``: {(function, module, caller,
    shape): the predicate clause that sends it there}); ``sites`` are the calls that are no missing kernel, pinned as before."""
    found = sorted(k for k in audit.calls if k[:3] not in sites)
    print("[fallbacks] %s:" % case)
    for k in found:
        print("[fallbacks]   %4d x %s from %s.%s on %s  (%s)" % ((audit.calls[k],) + k + (shapes.get(k, "NOT PINNED"),)))
    problems = _audit(case, audit, set(sites) | set(k[:3] for k in shapes))
    if set(found) != set(shapes):
        problems.append("%s: stem fallbacks by shape:\n  not pinned: %s\n  pinned but not seen: %s"
                        % (case, sorted(set(found) - set(shapes)), sorted(set(shapes) - set(found))))
    return problems


def _stem(shape, kind="conv"):
    return {"conv": ("conv2d", "backbone", "StdConv2dSame.forward"), "gn": ("group_norm", "backbone", "GroupNormAct.forward"),
            "proj": ("conv2d", "backbone", "VisionTransformer.embed_tokens")}[kind] + (shape,)


def _awkward_train_fallbacks(n, s, math):
    """A training step on ``n`` samples whose stage maps are s x s (stage 0), s/2 (stage 1, H*W % 8 == 4) and s/4 (stage 2, odd):
    s = 20 at 80^2, 28 at 112^2.  Shapes are those of the call's input: a strided convolution's is the map it reads, SAME-padded
    for a 3x3.  The transformer blocks and the stage-0 maps stay on the kernels."""
    h, q = s // 2, s // 4
    t = {
        _stem((n, 256, s, s)): "1x1/2 shortcut of stage 1, subsampled to %dx%d: H*W %% 8 (conv1x1_fusable)" % (h, h),
        _stem((n, 128, s + 1, s + 1)): "3x3/2 of stage 1 on %dx%d with gradients: W %% 8 (conv_s2_fusable)" % (s, s),
        _stem((n, 128, h, h)): "1x1 (conv3) and 3x3 (conv2) at %dx%d: H*W %% 8 (conv1x1_fusable), W %% 4 (conv3x3_fusable)" % (h, h),
        _stem((n, 512, h, h)): "1x1 (conv1) at %dx%d: H*W %% 8; the 1x1/2 shortcut of stage 2, subsampled to %dx%d" % (h, h, q, q),
        _stem((n, 256, h + 1, h + 1)): "3x3/2 of stage 2 on %dx%d: output %dx%d, H2*W2 %% 4 (conv_s2_fusable)" % (h, h, q, q),
        _stem((n, 256, q, q)): "1x1 (conv3) and 3x3 (conv2) at %dx%d: H*W %% 8, W %% 4" % (q, q),
        _stem((n, 1024, q, q)): "1x1 (conv1) at %dx%d: H*W %% 8" % (q, q),
        _stem((n, 256, q, q), "gn"): "GroupNorm at %dx%d: H*W %% 4 (groupnorm_fusable)" % (q, q),
        _stem((n, 1024, q, q), "gn"): "GroupNorm at %dx%d: H*W %% 4" % (q, q),
        _stem((n, 1024, q, q), "proj"): "patch projection (1x1) at %dx%d: H*W %% 8; the torch token chain follows it" % (q, q),
    }
    if math == "f32":                                       # EXACT_CONVS: no exact-fp32 3x3 / strided kernels
        t[_stem((n, 3, 4 * s + 5, 4 * s + 5))] = "7x7/2 stem convolution (SAME-padded image): split-product kernels only"
        t[_stem((n, 64, s, s))] = "3x3 of stage 0 at %dx%d: split-product kernels only" % (s, s)
    return t


AWKWARD_TRAIN_CASES = [(80, "f32"), (80, "f32_split"), (112, "f32_split")]


@pytest.mark.parametrize("size,math", AWKWARD_TRAIN_CASES, ids=["hybrid%d-%s" % c for c in AWKWARD_TRAIN_CASES])
def test_training_step_launches_at_awkward_geometries(size, math):
    """train.train_step on one image (two views) whose size is no multiple of 32: the launches at the predicates' edges against
    float64, the library calls of the other stages pinned by shape and reason."""
    from acr_wsss_amd.train import train_step
    model = _model("hybrid", math).train()
    img, label = make_inputs(1, size, 20, 0)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)

    def run():
        loss, _ = train_step(model, opt, img.to(DEV), label.to(DEV), 125)
        assert torch.isfinite(loss)

    census, audit = _census(run)
    del model, opt
    torch.cuda.empty_cache()
    case = "train hybrid %d^2 %s" % (size, math)
    s = size // 4
    problems = _check(case, census) + _audit_shapes(case, audit, TRAIN_FALLBACKS, _awkward_train_fallbacks(2, s, math))
    recs = [(r.name, dict(r.args)) for r in census.records]
    hw = lambda a: a["x"].shape[2] * a["x"].shape[3]
    # the edge launches these sizes exist for: GroupNorm at H*W % 8 == 4, a 1x1 at the stage-0 map, the token count
    assert any(n == "groupnorm_act" and a["x"].shape[2:] == (s // 2, s // 2) and hw(a) % 8 == 4 for n, a in recs)
    assert any(n.startswith("conv1x1") and hw(a) == s * s for n, a in recs)
    assert any(n.startswith("attention_core") and a["qkv"].shape[1] == (size // 16) ** 2 + 1 for n, a in recs)
    if math == "f32_split":
        assert any(n == "conv3x3" and a["x"].shape[3] == s for n, a in recs)
    assert not any(n == "tokens" for n, a in recs)           # an odd token grid: the projection and the chain behind it are torch's
    assert not problems, "\n".join(problems)


TRAIN_CASES = [("hybrid", 448, "f32"), ("hybrid", 448, "f32_split"), ("hybrid", 448, "f32_fp16x2"), ("coco", 512, "f32_split"),
               ("tiny", 224, "f32_split")]


@pytest.mark.parametrize("kind,size,math", TRAIN_CASES, ids=["%s%d-%s" % c for c in TRAIN_CASES])
def test_training_step_launches_against_fp64(kind, size, math):
    """train.train_step on one image (two views: batch 2) at the shipped geometry."""
    from acr_wsss_amd.train import train_step
    model = _model(kind, math).train()
    img, label = make_inputs(1, size, 80 if kind == "coco" else 20, 0)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)

    def run():
        loss, _ = train_step(model, opt, img.to(DEV), label.to(DEV), 125)
        assert torch.isfinite(loss)

    census, audit = _census(run)
    del model, opt
    torch.cuda.empty_cache()
    case = "train %s %d^2 %s" % (kind, size, math)
    pinned = TINY_FALLBACKS if kind == "tiny" else {**TRAIN_FALLBACKS, **EXACT_CONVS} if math == "f32" else TRAIN_FALLBACKS
    problems = _check(case, census) + _audit(case, audit, pinned)
    if math == "f32_split" and kind != "tiny":
        bad = [s for s in audit.sites() if s[2].split(".")[0] in NO_FALLBACK_CALLERS]
        problems += ["%s: stem / norm / block Linear on the library: %s" % (case, bad)] if bad else []
    p = size // 16
    Tn = p * p + 1
    names = set(r.name for r in census.records)
    # split products: o leaves the attention forward as proj's operand image (fp16x2 changes the Linears, the core stays split)
    assert {"attention_core_oimg" if math == "f32_split" else "attention_core", "consistency", "mlsm_loss"} <= names, names
    assert any(r.name.startswith("attention_core") and dict(r.args)["qkv"].shape[1] == Tn for r in census.records)
    if math == "f32_fp16x2":                                # the fp16x2 Linears at the 448^2 token count
        assert any(r.name in ("linear_or_hip", "mlp_f32") and dict(r.args)["math"] == 2 and dict(r.args)["x"].shape[1] == Tn
                   for r in census.records)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("math", ["f32", "f32_split"])
def test_cam_generation_launches_against_fp64(math):
    """infer_cam_images on two 384^2 images at scales (0.5, 1, 1.5, 2), eager launches (no captured graphs, one stream)."""
    from acr_wsss_amd.infer_cam import infer_cam_images
    model = _model("hybrid", math).eval()
    vit = model.pretrained.model
    vit.graph_prefix = vit.graph_pass = False
    imgs, labels = make_inputs(2, 384, 20, 3)

    def run():
        out = infer_cam_images(model, imgs.to(DEV), labels, [(384, 384)] * 2, scales=(0.5, 1.0, 1.5, 2.0), concurrent_scales=False)
        assert len(out) == 2

    census, audit = _census(run)
    del model
    torch.cuda.empty_cache()
    case = "CAM 384^2 x (0.5, 1, 1.5, 2) %s" % math
    problems = _check(case, census) + _audit(case, audit, CAM_FALLBACKS[math])
    att = set(dict(r.args)["qkv"].shape[1] for r in census.records if r.name.startswith("attention_core"))
    assert att == {145, 577, 1297, 2305}, att
    if math == "f32_split":                                 # 3x3 convolutions at the 72 / 144 / 192 maps of the larger scales
        c3 = set(dict(r.args)["x"].shape[2] for r in census.records if r.name == "conv3x3")
        assert {72, 144, 192} <= c3, c3
    assert not problems, "\n".join(problems)


def _awkward_cam_fallbacks(n):
    """CAM generation on ``n`` samples per pass (two images x the flip pair) at 160^2 x (0.5, 1, 1.5, 2): inputs 80 / 160 / 240 / 320,
    stage maps 20-10-5 / 40-20-10 / 60-30-15 / 80-40-20.  No gradients in the stem: the 3x3/2 convolutions take every map whose
    OUTPUT has H2*W2 % 4 == 0.  The 320^2 pass stays on the kernels throughout."""
    t = {}
    for s in (20, 60):                                      # scales 0.5 and 1.5
        h, q = s // 2, s // 4
        t.update({
            _stem((n, 256, s, s)): "1x1/2 shortcut of stage 1, subsampled to %dx%d: H*W %% 8 (conv1x1_fusable)" % (h, h),
            _stem((n, 128, h, h)): "1x1 (conv3) and 3x3 (conv2) at %dx%d: H*W %% 8 (conv1x1_fusable), W %% 4 (conv3x3_fusable)" % (h, h),
            _stem((n, 512, h, h)): "1x1 (conv1) at %dx%d: H*W %% 8; the 1x1/2 shortcut of stage 2, subsampled to %dx%d" % (h, h, q, q),
            _stem((n, 256, h + 1, h + 1)): "3x3/2 of stage 2 on %dx%d: output %dx%d, H2*W2 %% 4 (conv_s2_fusable)" % (h, h, q, q),
            _stem((n, 256, q, q)): "1x1 (conv3) and 3x3 (conv2) at %dx%d: H*W %% 8, W %% 4" % (q, q),
            _stem((n, 1024, q, q)): "1x1 (conv1) at %dx%d: H*W %% 8" % (q, q),
            _stem((n, 256, q, q), "gn"): "GroupNorm at %dx%d: H*W %% 4 (groupnorm_fusable)" % (q, q),
            _stem((n, 1024, q, q), "gn"): "GroupNorm at %dx%d: H*W %% 4" % (q, q),
            _stem((n, 1024, q, q), "proj"): "patch projection (1x1) at %dx%d: H*W %% 8; the torch token chain follows it" % (q, q),
        })
    t.update({                                              # scale 1: only the last stage's 10x10 maps
        _stem((n, 512, 20, 20)): "1x1/2 shortcut of stage 2, subsampled to 10x10: H*W % 8 (conv1x1_fusable)",
        _stem((n, 256, 10, 10)): "1x1 (conv3) and 3x3 (conv2) at 10x10: H*W % 8, W % 4",
        _stem((n, 1024, 10, 10)): "1x1 (conv1) at 10x10: H*W % 8",
        _stem((n, 1024, 10, 10), "proj"): "patch projection (1x1) at 10x10: H*W % 8; the torch token chain follows it",
    })
    return t


def test_cam_generation_launches_at_awkward_geometries():
    """infer_cam_images on two 160^2 images at scales (0.5, 1, 1.5, 2) under split products, eager launches: token grids 5, 10, 15, 20."""
    from acr_wsss_amd.infer_cam import infer_cam_images
    model = _model("hybrid", "f32_split").eval()
    vit = model.pretrained.model
    vit.graph_prefix = vit.graph_pass = False
    imgs, labels = make_inputs(2, 160, 20, 3)

    def run():
        out = infer_cam_images(model, imgs.to(DEV), labels, [(160, 160)] * 2, scales=(0.5, 1.0, 1.5, 2.0), concurrent_scales=False)
        assert len(out) == 2

    census, audit = _census(run)
    del model
    torch.cuda.empty_cache()
    case = "CAM 160^2 x (0.5, 1, 1.5, 2) f32_split"
    problems = _check(case, census) + _audit_shapes(case, audit, CAM_FALLBACKS["f32_split"], _awkward_cam_fallbacks(4))
    recs = [(r.name, dict(r.args)) for r in census.records]
    att = set(a["qkv"].shape[1] for n, a in recs if n.startswith("attention_core"))
    assert att == {26, 101, 226, 401}, att
    assert any(n == "groupnorm_act" and a["x"].shape[2:] == (10, 10) for n, a in recs)          # H*W a multiple of 4, not of 8
    assert any(n == "conv3x3" and a["x"].shape[3] == 20 for n, a in recs)
    assert any(n.startswith("conv1x1") and a["x"].shape[2] * a["x"].shape[3] == 400 for n, a in recs)
    assert set(a["pos"].shape[1] for n, a in recs if n == "tokens") == {401}                   # only the 20 x 20 grid is assembled by the kernel
    assert not problems, "\n".join(problems)
