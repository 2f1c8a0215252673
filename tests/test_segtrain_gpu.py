"""``segtrain.seg_train_step`` on the device: the hybrid ``ACR(..., seg=True)`` + ``SegmentationHead`` at 64 x 64, B = 2, split-product
math, ``PolyOptimizer`` over every parameter of both (the setup test_decoder_gpu.py runs).  The step has no arithmetic of its own,
so every check is bit for bit: against itself, against the hand-written sequence of the calls it is made of, and over two
consecutive steps (a weight image that survived the in-place update would show in the second)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from recipe import make_inputs, recipe_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDLE = "scratch.refinenet4.resConfUnit1."                    # refinenet4 takes one input (DPT/DPT.py:283): this unit never runs
LR = 0.01


@pytest.fixture(scope="module")
def setup():
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd import segloss as S
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
    head = D.SegmentationHead(16, 20).to(DEV).train()
    set_math(head, "f32_split")
    state = ({k: v.detach().clone() for k, v in model.state_dict().items()}, {k: v.detach().clone() for k, v in head.state_dict().items()})
    rng = np.random.default_rng(43)
    images = make_inputs(2, 64, 20, 43)[0].to(DEV)
    ori = torch.from_numpy(rng.integers(0, 256, (2, 3, 64, 64), dtype=np.uint8)).to(DEV)
    crop = torch.zeros(2, 64, 64, device=DEV)
    crop[0, 5:60, :] = 1
    crop[1, :, 8:64] = 1
    label = rng.integers(0, 21, (2, 64, 64)).astype(np.uint8)
    label[rng.random(label.shape) < 0.1] = 255
    batch = (images, ori, crop.permute(1, 2, 0), torch.from_numpy(label).to(DEV))     # croppings as the loader hands them: (S, S, B)
    yield model, head, state, batch, S.DenseEnergyLoss(1e-3, 15.0, 40.0, 1.0)
    model.set_math("f32")


def hand_step(model, head, opt, images, ori, croppings, label, layer):
    """The sequence seg_train_step stands for, written out; no cache is renewed by hand -- the fused optimizer moves the version
    counters, which is what every cache is keyed on."""
    from acr_wsss_amd import segloss, segval
    opt.zero_grad(set_to_none=True)
    logits = segval.forward_seg(model, head, images)
    if layer is None:
        loss = segloss.split_cross_entropy(logits, label, False)[0]
    else:
        ce, dl = segloss.joint_loss(ori, logits, label, croppings, False, layer)
        loss = ce + dl
    loss.backward()
    opt.step()
    return loss


def run(setup, steps, how, layer="dense"):
    """`steps` steps from the recorded state under torch.manual_seed(6) (the head's Dropout) -> (loss bytes per step, terms of
    the last step, parameters after, gradients after)."""
    from acr_wsss_amd.segtrain import seg_train_step
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
            loss, terms = seg_train_step(model, head, opt, *batch, layer)
            assert set(terms) == {"celoss", "dloss", "loss"} and terms["loss"] is loss
        else:
            loss = hand_step(model, head, opt, *batch, layer)
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


@pytest.fixture(scope="module")
def two_steps(setup):
    return run(setup, 2, "step")


def test_one_step_repeats_and_equals_the_hand_written_sequence(setup):
    a, b, hand = run(setup, 1, "step"), run(setup, 1, "step"), run(setup, 1, "hand")
    assert np.isfinite(np.frombuffer(a[0][0], np.float32)).all()
    assert a[0] == b[0] == hand[0]
    same(a[2], b[2])
    same(a[2], hand[2])
    same(a[3], hand[3])
    terms = a[1]
    assert float(terms["dloss"]) != 0.0 and float(terms["loss"]) == float(terms["celoss"] + terms["dloss"])


def test_parameters_with_gradients_moved_and_the_idle_unit_has_none(setup):
    model, head, state, _, _ = setup
    _, _, after, grads = run(setup, 1, "step")
    before = {"model." + k: v.cpu() for k, v in state[0].items()}
    before.update({"head." + k: v.cpu() for k, v in state[1].items()})
    idle = [k for k in grads if k.startswith("model." + IDLE)]
    assert len(idle) == 6 and all(grads[k] is None for k in idle)             # two convolutions, two BatchNorms: 2 + 4 tensors
    moved = 0
    for k, g in grads.items():
        assert torch.isfinite(after[k]).all(), k
        if g is None:
            assert torch.equal(after[k], before[k]), k                          # no gradient: the optimizer leaves it alone
            continue
        assert torch.isfinite(g).all(), k
        if float(g.abs().max()) > 0:
            assert not torch.equal(after[k], before[k]), k
            moved += 1
    heads = [k for k in grads if k.startswith("head.")]
    assert all(grads[k] is not None and float(grads[k].abs().max()) > 0 for k in heads)
    assert moved >= len(heads) + 4 + 4 * 14 - 6 + 6                             # head, layerN_rn, fusion blocks, read-outs (test_decoder_gpu.py)


def test_second_step_uses_the_updated_weights(setup, two_steps):
    losses, _, after, grads = two_steps
    hand = run(setup, 2, "hand")
    first = run(setup, 1, "step")
    assert losses[0] == first[0][0] and losses[1] != losses[0]
    assert losses == hand[0]
    same(after, hand[2])
    same(grads, hand[3])
    again = run(setup, 2, "step")
    assert again[0] == losses
    same(again[2], after)


def test_without_the_energy_layer_the_step_is_cross_entropy_only(setup):
    a, hand, dense = run(setup, 1, "step", None), run(setup, 1, "hand", None), run(setup, 1, "step")
    terms = a[1]
    assert float(terms["dloss"]) == 0.0 and terms["loss"].detach().cpu().numpy().tobytes() == terms["celoss"].detach().cpu().numpy().tobytes()
    assert a[0] == hand[0]
    same(a[2], hand[2])
    same(a[3], hand[3])                                                         # the cross-entropy's gradient, nothing else
    assert terms["celoss"].detach().cpu().numpy().tobytes() == dense[1]["celoss"].detach().cpu().numpy().tobytes()
    assert any(a[3][k] is not None and not torch.equal(a[3][k], dense[3][k]) for k in a[3])    # the energy term does reach the gradients
