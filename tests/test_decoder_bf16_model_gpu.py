"""The bf16 mode of the segmentation stage above the C ABI: ``decoder.batch_norm_act`` / ``relu`` / ``upsample2x`` through autograd,
``decode`` + ``SegmentationHead`` of the hybrid model, ``segtrain.seg_train_step`` / ``joint_train_step`` under
``train.MasterWeights`` and ``segval.predict_image`` on ``model.bfloat16()``, all at the size of tests/golden/decoder_hybrid_64.npz
(64 x 64, batch 2, features 16).

Rules, none of them new:
  functions   tests/decoder_bf16_checks.py against the fp32 functions on the upcast inputs (the rule of test_decoder_bf16_gpu.py).
  decode      tests/test_model_gpu.py::test_bf16_train_step_448's shape: the HIP bf16 result may be at most twice as far from the
              fp32 result as a kernel-free bf16-storage emulation of the same module graph (F.conv2d, F.batch_norm, F.relu,
              F.interpolate on bf16 tensors on the device) is; distances by test_decoder_gpu.py's ``_rel``.
  steps       tests/test_model_gpu.py::test_bf16_and_fp32_loss_trajectories_agree's bound, 2e-2 relative, on the first step's
              celoss and acr_loss against the fp32 step on the same (bf16-representable) weights and batch.
  prediction  test_crf_stage_gpu.py's margin rule: labels agree wherever the fp32 top-2 probability margin exceeds twice the largest
              bf16-vs-fp32 probability difference observed; at least half of the pixels must be compared."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import decoder_bf16_checks as K
from conftest import load_golden
from recipe import make_inputs, recipe_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHA = 125
LOSS_BOUND = 2e-2               # test_bf16_and_fp32_loss_trajectories_agree
FACTOR = 2.0                    # test_bf16_train_step_448's margin over the emulation


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def bf16_exact(t):
    """fp32 values that bf16 holds exactly"""
    return t.to(torch.bfloat16).float()


def held(what, got_bf16, ref_f32):
    res = K.accept_bf16(bits(got_bf16), ref_f32.detach().float().cpu().numpy(), what)
    print("%s: %d/%d exact, %d in the window" % (what, res["exact"], res["size"], res["exempt"]))
    assert res["ok"], (what, res)


# ------------------------------------------------------------------------------------------------
# the functions through autograd
# ------------------------------------------------------------------------------------------------
def make_bn(c, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(c).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(bf16_exact(1 + 0.1 * torch.randn(c, generator=g)))
        bn.bias.copy_(bf16_exact(0.1 * torch.randn(c, generator=g)))
        bn.running_mean.copy_(0.2 * torch.randn(c, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(c, generator=g))
    bn.weight.data, bn.bias.data = bn.weight.data.to(dtype), bn.bias.data.to(dtype)
    return bn


@pytest.mark.parametrize("relu,nres,training", [(False, 0, True), (True, 2, True), (True, 1, False)])
def test_batch_norm_act_bf16_through_autograd(relu, nres, training):
    from acr_wsss_amd import decoder as D
    g = torch.Generator().manual_seed(11)
    shape = (2, 5, 5, 7)
    x, dy = bf16_exact(torch.randn(shape, generator=g) + 0.5), bf16_exact(torch.randn(shape, generator=g))
    res = [bf16_exact(torch.randn(shape, generator=g)) for _ in range(nres)]
    out = {}
    for dtype in (torch.float32, torch.bfloat16):
        bn = make_bn(5, dtype, 3).train(training)
        xs = [t.to(DEV).to(dtype).requires_grad_(True) for t in [x] + res]
        y = D.batch_norm_act(xs[0], bn, "relu" if relu else "none", *xs[1:])
        y.backward(dy.to(DEV).to(dtype))
        out[dtype] = dict(y=y, dx=xs[0].grad, dres=[t.grad for t in xs[1:]], dgamma=bn.weight.grad, dbeta=bn.bias.grad,
                          rm=bn.running_mean, rv=bn.running_var, tracked=int(bn.num_batches_tracked))
    ref, got = out[torch.float32], out[torch.bfloat16]
    assert got["y"].dtype == got["dx"].dtype == torch.bfloat16 and all(d.dtype == torch.bfloat16 for d in got["dres"])
    assert got["dgamma"].dtype == got["dbeta"].dtype == torch.bfloat16                      # the parameter's dtype: MasterWeights' fused step
    assert got["rm"].dtype == got["rv"].dtype == torch.float32 and got["tracked"] == ref["tracked"] == int(training)
    for name in ("y", "dx", "dgamma", "dbeta"):
        held("batch_norm_act %s" % name, got[name], ref[name])
    for a, b in zip(got["dres"], ref["dres"]):
        held("batch_norm_act dres", a, b)
    for name in ("rm", "rv"):
        assert K.close_f32(got[name].cpu().numpy(), ref[name].cpu().numpy())["ok"], name


def test_relu_and_upsample2x_bf16_through_autograd():
    from acr_wsss_amd import decoder as D
    g = torch.Generator().manual_seed(12)
    x = bf16_exact(torch.randn(2, 3, 5, 7, generator=g))
    for fn, dshape in ((D.relu, (2, 3, 5, 7)), (D.upsample2x, (2, 3, 10, 14))):
        dy = bf16_exact(torch.randn(dshape, generator=g))
        out = {}
        for dtype in (torch.float32, torch.bfloat16):
            xd = x.to(DEV).to(dtype).requires_grad_(True)
            y = fn(xd)
            y.backward(dy.to(DEV).to(dtype))
            out[dtype] = (y, xd.grad)
        assert out[torch.bfloat16][0].dtype == out[torch.bfloat16][1].dtype == torch.bfloat16
        held("%s y" % fn.__name__, out[torch.bfloat16][0], out[torch.float32][0])
        held("%s dx" % fn.__name__, out[torch.bfloat16][1], out[torch.float32][1])


def test_mixed_dtypes_and_bf16_running_statistics():
    from acr_wsss_amd import decoder as D
    x16 = torch.randn(2, 5, 4, 4, device=DEV).bfloat16()
    with pytest.raises(ValueError):
        D.batch_norm_act(x16, make_bn(5, torch.float32, 1))                                 # bf16 x, fp32 parameters
    with pytest.raises(ValueError):
        D.batch_norm_act(x16.float(), make_bn(5, torch.bfloat16, 1))                        # the reverse
    with pytest.raises(ValueError):
        D.batch_norm_act(x16, make_bn(5, torch.bfloat16, 1), "none", x16.float())           # an fp32 addend
    bn = make_bn(5, torch.bfloat16, 1)
    bn.weight.data = bn.weight.data.float()                                                 # weight and bias disagree
    with pytest.raises(ValueError):
        D.batch_norm_act(x16, bn)
    # bf16 running statistics: refused while training, upcast (exactly) in eval mode
    bn = make_bn(5, torch.bfloat16, 2)
    bn.running_mean, bn.running_var = bn.running_mean.bfloat16(), bn.running_var.bfloat16()
    with pytest.raises(ValueError, match="float32"):
        D.batch_norm_act(x16, bn.train())
    assert int(bn.num_batches_tracked) == 0
    y = D.batch_norm_act(x16, bn.eval())
    up = make_bn(5, torch.bfloat16, 2).eval()
    up.running_mean, up.running_var = bn.running_mean.float(), bn.running_var.float()
    assert bits(y).tobytes() == bits(D.batch_norm_act(x16, up)).tobytes()
    assert bn.running_mean.dtype == torch.bfloat16                                          # read only: the module keeps its buffers


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def to_bf16_keep_stats(module):
    """module.bfloat16() with the BatchNorm buffers left fp32: what train.MasterWeights does to a module"""
    keep = {k: v.clone() for k, v in module.state_dict().items() if "running_" in k}
    module.bfloat16()
    for name, m in module.named_modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.running_mean, m.running_var = keep[name + ".running_mean"], keep[name + ".running_var"]
    return module


@pytest.fixture(scope="module")
def pair():
    """(model, head) in fp32 on the device with bf16-representable weights: the recipe's, and the fixture's running statistics"""
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd.DPT.ACR import ACR
    fx = load_golden("decoder_hybrid_64")
    model = ACR(20, "vitb_hybrid", seg=True, features=16, use_pretrain=False)
    sd = {}
    for k, v in model.state_dict().items():
        if "running_" in k:
            sd[k] = torch.from_numpy(fx["before:" + k])
        elif torch.is_floating_point(v):
            sd[k] = bf16_exact(recipe_tensor(k, v.shape, 0))
        else:
            sd[k] = torch.zeros_like(v)
    model.load_state_dict(sd, strict=True)
    torch.manual_seed(5)
    head = D.SegmentationHead(16, 20)
    with torch.no_grad():
        for p in head.parameters():
            p.copy_(bf16_exact(p))
    return model.to(DEV).train(), head.to(DEV).train()


def fresh(pair, dtype):
    model, head = copy.deepcopy(pair[0]), copy.deepcopy(pair[1])
    if dtype == torch.bfloat16:
        to_bf16_keep_stats(model), to_bf16_keep_stats(head)
    return model, head


def emu_bn(bn, x, act=None):
    y = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight.float(), bn.bias.float(), bn.training, bn.momentum, bn.eps)
    return F.relu(y) if act else y


def emu_conv(m, x):
    return F.conv2d(x, m.weight, m.bias, m.stride, m.padding)


def emu_rcu(u, x):
    out = emu_conv(u.conv1, F.relu(x))
    out = emu_conv(u.conv2, emu_bn(u.bn1, out, "relu"))
    return emu_bn(u.bn2, out) + x


def emu_fusion(blk, *xs):
    output = xs[0]
    if len(xs) == 2:
        output = output + emu_rcu(blk.resConfUnit1, xs[1])
    output = emu_rcu(blk.resConfUnit2, output)
    return emu_conv(blk.out_conv, F.interpolate(output, scale_factor=2, mode="bilinear", align_corners=True))


def emu_decode_head(scratch, pp3, pp4, head, taps, skip, gh, gw):
    """decoder.layers_rn_taps (hybrid) + fuse + SegmentationHead as torch calls on bf16 tensors"""
    b = taps["4"].shape[0]

    def grid(tok):
        return tok[:, skip:].transpose(1, 2).reshape(b, tok.shape[2], gh, gw).contiguous()
    l3 = emu_conv(pp3[3], grid(taps["3"]))
    l4 = emu_conv(pp4[4], emu_conv(pp4[3], grid(taps["4"])))
    l1, l2, l3, l4 = emu_conv(scratch.layer1_rn, taps["1"]), emu_conv(scratch.layer2_rn, taps["2"]), emu_conv(scratch.layer3_rn, l3), \
        emu_conv(scratch.layer4_rn, l4)
    p4 = emu_fusion(scratch.refinenet4, l4)
    p3 = emu_fusion(scratch.refinenet3, p4, l3)
    p2 = emu_fusion(scratch.refinenet2, p3, l2)
    path_1 = emu_fusion(scratch.refinenet1, p2, l1)
    feat = emu_bn(head[1], emu_conv(head[0], path_1), "relu")
    half = emu_conv(head[4], feat).float()
    return path_1, F.interpolate(half, scale_factor=2, mode="bilinear", align_corners=True)


def running(model, head):
    out = {"mean": [], "var": []}
    for mod in (model.scratch, head):
        for k, v in mod.state_dict().items():
            if k.endswith("running_mean") and "refinenet4.resConfUnit1" not in k:
                out["mean"].append(v.detach().float().cpu().numpy().reshape(-1))
            elif k.endswith("running_var") and "refinenet4.resConfUnit1" not in k:
                out["var"].append(v.detach().float().cpu().numpy().reshape(-1))
    return {k: np.concatenate(v) for k, v in out.items()}


def test_decode_and_head_bf16_against_the_emulation(pair):
    from acr_wsss_amd import decoder as D
    img = bf16_exact(make_inputs(2, 64, 20, 43)[0]).to(DEV)
    m32, h32 = fresh(pair, torch.float32)
    m16, h16 = fresh(pair, torch.bfloat16)
    for h in (h32, h16):
        h[3].eval()                                          # the Dropout draws another mask per dtype: out of this comparison
    before = running(m16, h16)
    with torch.no_grad():
        path16 = D.decode(m16, img.bfloat16())
        logits16 = h16(path16)
        taps = {k: m16.pretrained.activations[k].detach().clone() for k in ("1", "2", "3", "4")}
        # the fp32 pass and the emulation decode the SAME taps: what is compared is the decoder and the head
        path32 = D.decode_taps(m32, {k: v.float() for k, v in taps.items()}, (64, 64))
        logits32 = h32(path32)
    assert path16.dtype == torch.bfloat16 and tuple(path16.shape) == (2, 16, 32, 32)
    assert logits16.dtype == torch.float32 and tuple(logits16.shape) == (2, 21, 64, 64)
    assert all(v.dtype == torch.float32 for mod in (m16, h16) for k, v in mod.state_dict().items() if "running_" in k)
    # the emulation: the modules of a second bf16 copy through torch's own operators, on the device -- its convolutions are then
    # the library calls the HIP pass makes too, and what differs is the norm, the ReLU and the upsampling
    e16, eh16 = fresh(pair, torch.bfloat16)
    eh16[3].eval()
    vit = e16.pretrained.model
    with torch.no_grad():
        epath, elogits = emu_decode_head(e16.scratch, e16.pretrained.act_postprocess3, e16.pretrained.act_postprocess4, eh16, taps,
                                         vit.num_tokens, 4, 4)
    assert epath.dtype == torch.bfloat16
    for what, hip, emu, ref in (("path_1", path16, epath, path32), ("logits", logits16, elogits, logits32)):
        d_hip, d_emu = _rel(hip.float().cpu().numpy(), ref.cpu().numpy()), _rel(emu.float().cpu().numpy(), ref.cpu().numpy())
        print("bf16 %s vs fp32: HIP %.3e, emulation %.3e" % (what, d_hip, d_emu))
        assert d_hip <= FACTOR * d_emu, (what, d_hip, d_emu)
    # the running statistics moved, are fp32 and stay as close to the fp32 pass's as the emulation's do
    r16, r32, remu = running(m16, h16), running(m32, h32), running(e16, eh16)
    for k in ("mean", "var"):
        assert np.abs(r16[k] - before[k]).max() > 0
        d_hip, d_emu = _rel(r16[k], r32[k]), _rel(remu[k], r32[k])
        print("running %s after one pass vs fp32: HIP %.3e, emulation %.3e" % (k, d_hip, d_emu))
        assert d_hip <= FACTOR * d_emu, (k, d_hip, d_emu)


def test_refusals(pair):
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd.DPT.ACR import ACR
    m32, _ = pair
    x = torch.zeros(1, 3, 64, 64, device=DEV)
    with pytest.raises(NotImplementedError):
        D.decode(m32, x.bfloat16())                           # bf16 input, fp32 weights
    m16, _ = fresh(pair, torch.bfloat16)
    with pytest.raises(NotImplementedError):
        D.decode(m16, x)                                      # fp32 input, bf16 weights
    with pytest.raises(NotImplementedError):
        D.decode_taps(m16, {k: torch.zeros(1, 17, 768, device=DEV) for k in ("1", "2", "3", "4")}, (64, 64))
    plain = to_bf16_keep_stats(ACR(20, "vitb", seg=True, features=16, use_pretrain=False).to(DEV))
    with pytest.raises(NotImplementedError, match="hybrid"):
        D.decode(plain, x.bfloat16())
    with pytest.raises(NotImplementedError):
        D.readout(torch.zeros(1, 17, 768, device=DEV, dtype=torch.bfloat16), 1, 4, 4, plain.pretrained.act_postprocess3[3], None)
    with pytest.raises(NotImplementedError):
        D.reassemble(torch.zeros(17, 16, device=DEV, dtype=torch.bfloat16), None, 1, 17, 1, 4, 4, 16, 1)


# ------------------------------------------------------------------------------------------------
# the steps
# ------------------------------------------------------------------------------------------------
def make_batch(seed):
    rng = np.random.default_rng(seed)
    images, labels = make_inputs(2, 64, 20, seed)
    ori = torch.from_numpy(rng.integers(0, 256, (2, 3, 64, 64), dtype=np.uint8)).to(DEV)
    crop = torch.zeros(2, 64, 64, device=DEV)
    crop[0, 5:60, :] = 1
    crop[1, :, 8:64] = 1
    sal = rng.integers(1, 256, (2, 64, 64)).astype(np.uint8)
    sal[0, 20:44, 10:50] = 0
    sal[1, :, :24] = 0
    seg = rng.integers(0, 21, (2, 64, 64)).astype(np.uint8)
    seg[rng.random(seg.shape) < 0.1] = 255
    return dict(images=bf16_exact(images).to(DEV), ori=ori, crop=crop.permute(1, 2, 0), labels=labels.to(DEV), sal=torch.from_numpy(sal).to(DEV),
                seg=torch.from_numpy(seg).to(DEV))


def one_step(pair, dtype, which, dis_weight, dense, drop):
    """one step from the fixture's weights -> everything the checks look at"""
    from acr_wsss_amd import segloss as S
    from acr_wsss_amd.segtrain import joint_train_step, seg_train_step
    from acr_wsss_amd.train import MasterWeights, PolyOptimizer
    model, head = copy.deepcopy(pair[0]), copy.deepcopy(pair[1])
    if not drop:
        head[3].p = 0.0
    both = nn.ModuleList([model, head])
    if dtype == torch.bfloat16:
        opt = MasterWeights(both, lambda ps: PolyOptimizer(ps, lr=0.01, weight_decay=0, max_step=100))
    else:
        opt = PolyOptimizer(list(both.parameters()), lr=0.01, weight_decay=0, max_step=100)
    named = dict(both.named_parameters())
    start = {k: p.detach().clone() for k, p in named.items()}
    stats0 = running(model, head)
    b = make_batch(43)
    layer = S.DenseEnergyLoss(1e-3, 15.0, 40.0, 1.0) if dense else None
    images = b["images"].to(dtype)
    torch.manual_seed(6)
    if which == "seg":
        loss, terms = seg_train_step(model, head, opt, images, b["ori"], b["crop"], b["seg"], layer, dis_weight=dis_weight)
    else:
        loss, terms = joint_train_step(model, head, opt, images, b["ori"], b["crop"], b["labels"], b["sal"], layer, alpha=ALPHA,
                                       dis_weight=dis_weight)
    return dict(loss=loss, terms=terms, named=named, start=start, stats0=stats0, stats1=running(model, head), opt=opt, model=model, head=head)


@pytest.mark.parametrize("dis_weight,dense", [(0.0, True), (0.5, True), (0.0, False)])
@pytest.mark.parametrize("which", ["seg", "joint"])
def test_steps_run_in_bf16_under_master_weights(pair, which, dis_weight, dense):
    ref = one_step(pair, torch.float32, which, dis_weight, dense, drop=True)
    got = one_step(pair, torch.bfloat16, which, dis_weight, dense, drop=True)
    terms = got["terms"]
    names = ["celoss", "dloss", "loss"] + (["disloss"] if dis_weight > 0 else []) + (["acr_loss", "cls_align", "aff_align"] if which == "joint" else [])
    for k in names:
        assert torch.isfinite(terms[k]).all(), k
    assert terms["celoss"].dtype == torch.float32                     # the head's logits, and with them the seg losses, are fp32
    print("%s step dis_weight=%g dense=%d: bf16 %s | fp32 %s" % (which, dis_weight, dense, {k: "%.5f" % float(terms[k]) for k in names},
                                                                  {k: "%.5f" % float(ref["terms"][k]) for k in names}))
    if which == "joint":
        assert terms["seg_label"].dtype == torch.uint8 and tuple(terms["seg_label"].shape) == (2, 64, 64)
    # every parameter with a gradient in the fp32 step has a bf16 one here; the fused optimizer took all of them
    opt = got["opt"]
    assert len(opt.masters) == len(got["named"]) and opt._fused_ok()
    for k, p in ref["named"].items():
        q = got["named"][k]
        assert q.dtype == torch.bfloat16
        if p.grad is not None:
            assert q.grad is not None and q.grad.dtype == torch.bfloat16 and torch.isfinite(q.grad).all(), k
    moved = [k for k, p in got["named"].items() if p.grad is not None and not torch.equal(p.detach().float(), got["start"][k].float())]
    with_grad = [k for k, p in got["named"].items() if p.grad is not None and float(p.grad.float().abs().max()) > 0]
    masters = dict(zip(got["named"], opt.masters))
    assert all(m.dtype == torch.float32 for m in opt.masters)
    for k in with_grad:
        assert not torch.equal(masters[k], got["start"][k].float()), k       # the fp32 master moved
    dec = [k for k in with_grad if k.startswith(("0.scratch.", "1."))]
    assert dec and len(moved) > 0 and any(k in moved for k in dec)
    # BatchNorm running statistics: fp32, and moved
    for mod in (got["model"], got["head"]):
        assert all(v.dtype == torch.float32 for k, v in mod.state_dict().items() if "running_" in k)
    for k in ("mean", "var"):
        assert np.abs(got["stats1"][k] - got["stats0"][k]).max() > 0


@pytest.mark.parametrize("which", ["seg", "joint"])
def test_first_step_losses_agree_with_the_fp32_step(pair, which):
    """celoss and acr_loss of the first step, bf16 against fp32 on the same weights and batch, within 2e-2 relative (the bound of
    test_bf16_and_fp32_loss_trajectories_agree).  The head's Dropout is switched off in both: torch draws another mask per dtype,
    which is no property of the arithmetic."""
    ref = one_step(pair, torch.float32, which, 0.0, True, drop=False)
    got = one_step(pair, torch.bfloat16, which, 0.0, True, drop=False)
    names = ["celoss"] + (["acr_loss"] if which == "joint" else [])
    rel = {k: abs(float(got["terms"][k]) - float(ref["terms"][k])) / abs(float(ref["terms"][k])) for k in names}
    print("%s first step: bf16 %s, fp32 %s, rel %s" % (which, {k: float(got["terms"][k]) for k in names},
                                                      {k: float(ref["terms"][k]) for k in names}, {k: "%.3e" % v for k, v in rel.items()}))
    if which == "joint":
        agree = float((got["terms"]["seg_label"] == ref["terms"]["seg_label"]).float().mean())
        print("   pseudo-labels of the two modes agree on %.4f of the pixels" % agree)
    for k in names:
        assert rel[k] <= LOSS_BOUND, (k, rel)


# ------------------------------------------------------------------------------------------------
# validation
# ------------------------------------------------------------------------------------------------
def test_predict_image_on_a_bfloat16_model(pair):
    from acr_wsss_amd import data, segval
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)
    from acr_wsss_amd import decoder as D
    m32 = fresh(pair, torch.float32)[0]
    torch.manual_seed(5)
    h32 = D.SegmentationHead(16, 1)
    with torch.no_grad():
        for q in h32.parameters():
            q.copy_(bf16_exact(q))
    h32 = h32.to(DEV)
    # Inputs with margins: on the recipe's weights with the fixture's running statistics the eval-mode maps are not normalised, the
    # softmax saturates and single pixels flip between classes (largest probability difference 0.44: no margin decides anything).
    # So the instance is made well-conditioned, the same for both modes: the encoder as test_model_gpu.py's `_tame` makes it
    # (residual branches / 4, the logit sharpening undone), and running statistics that ARE those of this image -- one training-mode
    # pass with momentum 1 -- rounded to bf16 so that model.bfloat16() changes no value.  An untrained head's probabilities are
    # near uniform (logit std 0.37), and the gap between the top two of 21 such classes is small against the bf16 noise of the whole
    # network: measured on this image, the share of pixels the margin decides is 0.31 with 21 classes (largest probability
    # difference 1.1e-2), 0.52 with 5 and 0.86 with 2 (2.4e-2); labels agreed on every decided pixel in all three, and on 0.95 /
    # 0.95 / 0.98 of all pixels.  The head here has two classes (background + 1): the largest margins, not a smaller cap.
    norms = [m for mod in (m32, h32) for m in mod.modules() if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        for k, q in m32.named_parameters():
            if k.endswith(("attn.proj.weight", "mlp.fc2.weight")) or (k.endswith("norm3.weight") and "stages" in k):
                q.mul_(0.25)
            elif k.endswith("attn.qkv.weight"):
                q.copy_(bf16_exact(q / 1.4))
        for bn in norms:
            bn.momentum = 1.0
        m32.train(), h32.train()
        h32[3].eval()
        h32(D.decode(m32, data.val_batch([img], 64, next(m32.parameters()).device)))
        for bn in norms:
            bn.momentum = 0.1
            bn.running_mean.copy_(bf16_exact(bn.running_mean))
            bn.running_var.copy_(bf16_exact(bn.running_var))
    m16, h16 = copy.deepcopy(m32).bfloat16(), copy.deepcopy(h32).bfloat16()                  # model.bfloat16(): the buffers too
    assert m16.scratch.refinenet1.resConfUnit1.bn1.running_var.dtype == torch.bfloat16
    probs, labels = {}, {}
    for tag, m, h in (("f32", m32, h32), ("bf16", m16, h16)):
        m.eval(), h.eval()
        with torch.no_grad():
            labels[tag] = segval.predict_image(m, h, img, test_size=64).cpu().numpy()
            x = data.val_batch([img], 64, next(m.parameters()).device)
            logits = segval.forward_seg(m, h, x.to(next(m.parameters()).dtype))
            assert logits.dtype == torch.float32
            p = torch.empty((1, 2, 50, 70), dtype=torch.float32, device=DEV)
            segval.predict(logits, (50, 70), probs=p)
            probs[tag] = p[0].cpu().numpy().astype(np.float64)
    assert labels["bf16"].dtype == np.uint8 and labels["bf16"].shape == (50, 70)
    diff = float(np.abs(probs["bf16"] - probs["f32"]).max())
    top2 = np.sort(probs["f32"], axis=0)[-2:]
    margin = top2[1] - top2[0]
    decided = margin > 2 * diff
    share = float(decided.mean())
    print("predict_image bf16 vs fp32: largest probability difference %.3e, %.4f of the pixels decided by the margin, %.4f of all agree"
          % (diff, share, float((labels["bf16"] == labels["f32"]).mean())))
    assert share >= 0.5, share
    assert np.array_equal(labels["bf16"][decided], labels["f32"][decided])
