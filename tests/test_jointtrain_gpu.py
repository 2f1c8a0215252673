"""``segtrain.joint_train_step`` on the device, set up as test_segtrain_gpu.py: the hybrid ``ACR(..., seg=True)`` +
``SegmentationHead`` at 64 x 64, B = 2, split-product math, ``PolyOptimizer`` over every parameter of both.  The step has no
arithmetic of its own, so every check is bit for bit: against itself, against the hand-written sequence of the calls it is made
of, against ``train.train_step``'s terms of the same 2B pass, and over two consecutive steps."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from recipe import make_inputs, recipe_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 0.01
ALPHA = 125
ACR_TERMS = ("cls_loss_1", "cls_loss_2", "cls_align", "aff_align")


def build(backbone, fixture):
    """model and head as test_decoder_gpu.py / test_readout_gpu.py build them: weights by the recipe, running statistics from the fixture"""
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd.backbone import set_math
    from acr_wsss_amd.DPT.ACR import ACR
    fx = load_golden(fixture)
    model = ACR(20, backbone, seg=True, features=16, use_pretrain=False)
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
    head = D.SegmentationHead(16, 20).to(DEV).train()
    set_math(head, "f32_split")
    return model, head


def make_batch(seed):
    rng = np.random.default_rng(seed)
    images, labels = make_inputs(2, 64, 20, seed)
    ori = torch.from_numpy(rng.integers(0, 256, (2, 3, 64, 64), dtype=np.uint8)).to(DEV)
    crop = torch.zeros(2, 64, 64, device=DEV)
    crop[0, 5:60, :] = 1
    crop[1, :, 8:64] = 1
    sal = rng.integers(1, 256, (2, 64, 64)).astype(np.uint8)
    sal[0, 20:44, 10:50] = 0                                   # a zero region: the grab rule's pixels
    sal[1, :, :24] = 0
    return images.to(DEV), ori, crop.permute(1, 2, 0), labels.to(DEV), torch.from_numpy(sal).to(DEV)


@pytest.fixture(scope="module")
def setup():
    from acr_wsss_amd import segloss as S
    model, head = build("vitb_hybrid", "decoder_hybrid_64")
    state = ({k: v.detach().clone() for k, v in model.state_dict().items()}, {k: v.detach().clone() for k, v in head.state_dict().items()})
    yield model, head, state, make_batch(43), S.DenseEnergyLoss(1e-3, 15.0, 40.0, 1.0)
    model.set_math("f32")


def hand_targets(model, labels, saliency, S):
    """the targets of the pass that has just run, view by view from the taps: contiguous (B, N, C) CAMs per view"""
    from acr_wsss_amd import ops
    from acr_wsss_amd.segtrain import saliency_labels
    from acr_wsss_amd.traincam import training_cams
    with torch.no_grad():
        tok = model.pretrained.activations["4"].detach()
        B, skip = tok.shape[0] // 2, model.pretrained.model.num_tokens
        W, b = model.cls_head.weight.detach(), model.cls_head.bias.detach()
        views = []
        for v in range(2):
            x = tok[v * B:(v + 1) * B, skip:].contiguous()
            views.append(ops.patch_cam(x.reshape(-1, x.shape[2]), W, b).reshape(B, x.shape[1], -1))
        norm_cam = training_cams(views[0], labels, (S, S), patch_cam_flipped=views[1])
        return saliency_labels(norm_cam, labels, saliency) + (norm_cam,)


def hand_step(model, head, opt, images, ori, croppings, labels, saliency, layer, seg_weight):
    """The sequence joint_train_step stands for, written out; no cache is renewed by hand -- the fused optimizer moves the version
    counters, which is what every cache is keyed on."""
    from acr_wsss_amd import decoder, segloss
    from acr_wsss_amd.train import acr_loss
    S = images.shape[2]
    opt.zero_grad(set_to_none=True)
    cls_list, attn_list = model.forward_mirror(images, images.flip(-1))
    acr, _ = acr_loss(cls_list, attn_list, labels, S // 16, ALPHA)
    seg_label = hand_targets(model, labels, saliency, S)[0]
    logits = head(decoder.decode_taps(model, model.pretrained.activations, (S, S), rows=images.shape[0]))
    if layer is None:
        seg = segloss.split_cross_entropy(logits, seg_label, False)[0]
    else:
        ce, dl = segloss.joint_loss(ori, logits, seg_label, croppings, False, layer)
        seg = ce + dl
    loss = acr + seg_weight * seg
    loss.backward()
    opt.step()
    return loss


def run(setup, steps, how, layer="dense", seg_weight=1.0):
    """`steps` steps from the recorded state under torch.manual_seed(6) (the head's Dropout) -> (loss bytes per step, terms of the
    last step, parameters after, gradients after)."""
    from acr_wsss_amd.segtrain import joint_train_step
    from acr_wsss_amd.train import PolyOptimizer
    model, head, state, batch, dense = setup
    layer = dense if layer == "dense" else None
    model.load_state_dict(state[0])
    head.load_state_dict(state[1])
    params = list(model.parameters()) + list(head.parameters())
    for p in params:
        p.grad = None
    opt = PolyOptimizer(params, lr=LR, weight_decay=5e-4, max_step=100)
    torch.manual_seed(6)
    losses, terms = [], None
    for _ in range(steps):
        if how == "step":
            loss, terms = joint_train_step(model, head, opt, *batch, layer, alpha=ALPHA, seg_weight=seg_weight)
            assert set(terms) == set(ACR_TERMS) | {"acr_loss", "celoss", "dloss", "loss", "seg_label", "saliency_out"} and terms["loss"] is loss
        else:
            loss = hand_step(model, head, opt, *batch, layer, seg_weight)
        losses.append(loss.detach().cpu().numpy().tobytes())
    named = [("model." + k, p) for k, p in model.named_parameters()] + [("head." + k, p) for k, p in head.named_parameters()]
    after = {k: p.detach().cpu().clone() for k, p in named}
    grads = {k: None if p.grad is None else p.grad.detach().cpu().clone() for k, p in named}
    assert opt.global_step == steps
    return losses, terms, after, grads


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), k


def raw(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def one_step(setup):
    return run(setup, 1, "step")


def test_one_step_repeats_and_equals_the_hand_written_sequence(setup, one_step):
    a, b, hand = one_step, run(setup, 1, "step"), run(setup, 1, "hand")
    assert np.isfinite(np.frombuffer(a[0][0], np.float32)).all()
    assert a[0] == b[0] == hand[0]
    same(a[2], b[2])
    same(a[3], b[3])
    same(a[2], hand[2])
    same(a[3], hand[3])
    terms = a[1]
    assert float(terms["dloss"].detach()) != 0.0
    assert raw(terms["loss"]) == raw(terms["acr_loss"] + 1.0 * (terms["celoss"] + terms["dloss"]))
    assert raw(terms["seg_label"]) == raw(b[1]["seg_label"]) and raw(terms["saliency_out"]) == raw(b[1]["saliency_out"])


def test_acr_terms_are_those_of_train_step_and_the_targets_those_of_the_taps(setup, one_step):
    """the same 2B pass from the same state: ``train.train_step`` reports the same four terms, bit for bit; and the label the step
    reports is ``saliency_labels(training_cams(...))`` of the taps that pass leaves, computed view by view"""
    from acr_wsss_amd.train import PolyOptimizer, train_step
    model, head, state, batch, _ = setup
    images, _, _, labels, saliency = batch
    terms = one_step[1]
    model.load_state_dict(state[0])
    for p in model.parameters():
        p.grad = None
    opt = PolyOptimizer(list(model.parameters()), lr=LR, weight_decay=5e-4, max_step=100)
    loss, ref = train_step(model, opt, images, labels, ALPHA)
    for k in ACR_TERMS:
        assert raw(terms[k]) == raw(ref[k]), k
    assert raw(terms["acr_loss"]) == raw(loss)
    model.load_state_dict(state[0])                           # the pass again, from the recorded state: its taps
    model.invalidate_caches()
    model.forward_mirror(images, images.flip(-1))
    seg_label, sal_out, norm_cam = hand_targets(model, labels, saliency, 64)
    assert raw(terms["seg_label"]) == raw(seg_label) and raw(terms["saliency_out"]) == raw(sal_out)
    lab = seg_label.cpu().numpy()
    present = labels.cpu().numpy() > 0
    assert norm_cam.shape == (2, 20, 64, 64) and float(norm_cam.min()) == 0 and 0 < float(norm_cam.max()) <= 1
    assert (norm_cam.cpu().numpy()[~present] == 0).all()
    for b in range(2):                                        # labels of present classes only, and not one value everywhere
        vals = set(np.unique(lab[b]).tolist())
        assert vals <= {0, 255} | {c + 1 for c in np.flatnonzero(present[b])} and len(vals) > 1, vals
    for p in model.parameters():
        p.grad = None


def test_decode_taps_equals_decode_on_the_taps_of_its_own_pass(setup):
    from acr_wsss_amd import decoder as D
    model, _, state, batch, _ = setup
    model.load_state_dict(state[0])
    model.invalidate_caches()
    with torch.no_grad():
        ref = D.decode(model, batch[0])
        taps = model.pretrained.activations
        got = D.decode_taps(model, taps, (64, 64))
        rows = D.decode_taps(model, taps, (64, 64), rows=2)
        one = D.decode_taps(model, taps, (64, 64), rows=1)
    assert raw(got) == raw(ref) and raw(rows) == raw(ref) and tuple(one.shape) == (1,) + tuple(ref.shape[1:])
    with pytest.raises(ValueError):
        D.decode_taps(model, taps, (64, 64), rows=3)
    with pytest.raises(ValueError):
        D.decode_taps(model, {}, (64, 64))


def test_seg_weight_zero_leaves_head_and_fusion_blocks_without_gradient(setup, one_step):
    off = run(setup, 1, "step", seg_weight=0.0)
    seg_only = [k for k in one_step[3] if k.startswith("head.") or k.startswith("model.scratch.")]
    assert len(seg_only) > 40
    for k in seg_only:
        g0, g1 = off[3][k], one_step[3][k]
        assert g0 is None or float(g0.abs().max()) == 0, k
        if "refinenet4.resConfUnit1." in k:
            assert g1 is None, k                             # refinenet4 takes one input: this unit never runs
        else:
            assert g1 is not None and float(g1.abs().max()) > 0, k
    assert raw(off[1]["acr_loss"]) == raw(one_step[1]["acr_loss"]) and raw(off[1]["loss"]) == raw(off[1]["acr_loss"] + 0.0 * (off[1]["celoss"] + off[1]["dloss"]))
    assert float(off[3]["model.cls_head.weight"].abs().max()) > 0               # the classification loss still trains the encoder


def test_second_step_uses_the_updated_weights(setup, one_step):
    two = run(setup, 2, "step")
    hand = run(setup, 2, "hand")
    assert two[0][0] == one_step[0][0] and two[0][1] != two[0][0]
    assert two[0] == hand[0]
    same(two[2], hand[2])
    same(two[3], hand[3])
    assert any(not torch.equal(two[2][k], one_step[2][k]) for k in two[2])


def test_without_the_energy_layer_the_segmentation_term_is_cross_entropy_only(setup, one_step):
    a, hand = run(setup, 1, "step", None), run(setup, 1, "hand", None)
    terms = a[1]
    assert float(terms["dloss"]) == 0.0 and raw(terms["celoss"]) == raw(one_step[1]["celoss"])
    assert a[0] == hand[0]
    same(a[2], hand[2])
    same(a[3], hand[3])


def test_bf16_is_refused(setup):
    from acr_wsss_amd.segtrain import joint_train_step
    model, head, _, batch, _ = setup
    with pytest.raises(NotImplementedError):
        joint_train_step(model, head, None, batch[0].bfloat16(), *batch[1:], None, alpha=ALPHA)


def test_a_plain_backbone_runs_a_step():
    """vitb: every tap is a block's tokens and goes through the read-outs; a finite loss and finite parameters after the update"""
    from acr_wsss_amd.segtrain import joint_train_step
    from acr_wsss_amd.train import PolyOptimizer
    model, head = build("vitb", "decoder_vitb_64x96")
    batch = make_batch(44)
    opt = PolyOptimizer(list(model.parameters()) + list(head.parameters()), lr=LR, weight_decay=5e-4, max_step=100)
    torch.manual_seed(6)
    loss, terms = joint_train_step(model, head, opt, *batch, None, alpha=ALPHA)
    assert torch.isfinite(loss) and all(torch.isfinite(terms[k]) for k in ACR_TERMS + ("celoss",))
    assert tuple(terms["seg_label"].shape) == (2, 64, 64) and terms["seg_label"].dtype == torch.uint8
    assert all(torch.isfinite(v).all() for v in model.state_dict().values())
    moved = [k for k, p in model.named_parameters() if k.startswith("pretrained.act_postprocess") and p.grad is not None and float(p.grad.abs().max()) > 0]
    assert len(moved) == 14, moved
