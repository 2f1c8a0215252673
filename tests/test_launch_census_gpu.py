"""Every HIP launch of the model, at the shapes the product runs, against float64.

Each case runs the real model once under the launch census (tests/launch_census.py): a training step (forward, ACR loss with
consistency and MLSM, backward) or CAM generation over the four scales.  The recorder keeps the distinct launches of the public
``ops`` entries; each then runs through its checker -- seeded inputs at exactly the recorded shapes, the same path, output and
every gradient against float64 at the tolerance of that kernel's own test.  The hand-written kernel tests pick their shapes; this
file takes them from the shipped geometries (448^2 -> T = 785, COCO 512^2 -> T = 1025, CAM 384^2 x {0.5, 1, 1.5, 2} ->
T = 145 / 577 / 1297 / 2305).

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
