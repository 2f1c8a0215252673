#!/usr/bin/env python3
"""Generate the DPT decoder fixtures by running the *reference itself* on the CPU (``ACR_REFERENCE``, default /root/reference):

    python tests/golden/make_decoder_golden.py [layouts] [blocks] [hybrid]

``DPT.blocks.FeatureFusionBlock_custom``, ``DPT.ACR.ACR(seg=True)`` and ``DPT.vit.forward_vit`` are imported UNMODIFIED (behind the
constants-only ``timm`` stub of make_golden.py); nothing of them is restated here.  Written, data only:
  state_dict_layout_seg_{hybrid,vitb,deit,distil}.json   keys and shapes of the reference's ACR(seg=True)
  decoder_block_a.npz   a fusion block, features 64, two inputs (2, 64, 16, 16), training mode, in fp32 and as .double()
  decoder_block_b.npz   features 16, one input (2, 16, 5, 7) (the refinenet4 form), training and eval mode
  decoder_hybrid_64.npz the whole decoder path of the hybrid model, features 16, 64 x 64, batch 2, training mode
Weights are tests/golden/recipe.py's function of (key, shape); the recipe has no rule for BatchNorm's running statistics, so those
follow ``running_rule`` below and are STORED (before and after the pass).  Inputs are rounded to 8 significand bits and the output
gradient takes four values so that the files stay small; tensors above 4096 values are stored as every ``stride``-th value
(tests/decoder_ref.py ``sample``).  A block fixture's seed is the first one for which every ReLU input of the float64 run lies
further from 0 than 8x the fp32 run's deviation on that tensor (recorded as relu_min64 / relu_dev32)."""
import copy
import json
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _install_timm_stub  # noqa: E402
from recipe import make_inputs, recipe_tensor, weights_checksum  # noqa: E402
from decoder_ref import sample  # noqa: E402

MARGIN = 8.0


def running_rule(key, shape, seed=0):
    rng = np.random.default_rng((zlib.crc32(key.encode()) ^ (seed * 0x9E3779B1)) & 0x7FFFFFFF)
    if key.endswith("running_mean"):
        return torch.from_numpy((0.2 * rng.standard_normal(shape)).astype(np.float32))
    return torch.from_numpy((0.5 + rng.random(shape)).astype(np.float32))


@torch.no_grad()
def fill(module, seed=0):
    for key, t in module.state_dict().items():
        if not torch.is_floating_point(t):
            continue
        t.copy_(running_rule(key, tuple(t.shape), seed) if "running_" in key else recipe_tensor(key, t.shape, seed))


def buffers(module):
    return {k: v.detach().clone().numpy() for k, v in module.state_dict().items() if "running_" in k}


def coarse(t):
    """fp32 values with 8 significand bits (the low 16 bits zero: compresses to half)"""
    return t.to(torch.bfloat16).to(torch.float32)


def run_block(blk, xs, dy, dtype):
    """(out, input grads, parameter grads, ReLU inputs, running statistics after) of one pass of ``blk`` (a fresh copy)"""
    blk = copy.deepcopy(blk).to(dtype)
    relu_in = []
    acts = {id(m): m for m in blk.modules() if isinstance(m, nn.ReLU)}
    hooks = [m.register_forward_pre_hook(lambda mod, inp: relu_in.append(inp[0].detach().clone())) for m in acts.values()]
    xs = [x.to(dtype).clone().requires_grad_(True) for x in xs]
    # FeatureFusionBlock_custom.forward adds out of place (skip_add.add), so the leaves stay untouched
    out = blk(*xs)
    out.backward(dy.to(dtype))
    for h in hooks:
        h.remove()
    grads = {k: p.grad.detach().numpy() for k, p in blk.named_parameters() if p.grad is not None}     # one input: unit 1 idle
    return out.detach().numpy(), [x.grad.numpy() for x in xs], grads, [r.numpy() for r in relu_in], buffers(blk)


def block_case(tag, features, shapes, stride, modes):
    from DPT.blocks import FeatureFusionBlock_custom
    blk = FeatureFusionBlock_custom(features, nn.ReLU(False), deconv=False, bn=True, expand=False, align_corners=True)
    fill(blk, 0)
    for seed in range(64):
        g = torch.Generator().manual_seed(7000 + seed)
        xs = [coarse(torch.randn(s, generator=g)) for s in shapes]
        n, c, h, w = shapes[0]
        dy = torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, (n, c, 2 * h, 2 * w), generator=g)]
        fx = {"seed": np.array(seed), "features": np.array(features), "stride": np.array(stride), "dy": dy.numpy()}
        for i, x in enumerate(xs):
            fx["x%d" % i] = x.numpy()
        for k, v in buffers(blk).items():
            fx["before:" + k] = v
        ok = True
        for mode in modes:
            blk.train(mode == "train")
            pre = "" if mode == "train" else "eval_"
            r32, r64 = run_block(blk, xs, dy, torch.float32), run_block(blk, xs, dy, torch.float64)
            dev = np.array([np.abs(a.astype(np.float64) - b).max() for a, b in zip(r32[3], r64[3])])
            mn = np.array([np.abs(b).min() for b in r64[3]])
            ok = ok and bool((mn > MARGIN * dev).all())
            fx[pre + "relu_dev32"], fx[pre + "relu_min64"] = dev, mn
            for name, r in (("32", r32), ("64", r64)):
                fx[pre + "out" + name] = sample(r[0], stride)
                for i, gx in enumerate(r[1]):
                    fx[pre + "dx%d_%s" % (i, name)] = sample(gx, stride)
                for k, v in r[2].items():
                    fx[pre + "grad%s:%s" % (name, k)] = sample(v, stride)
                for k, v in r[4].items():
                    fx[pre + "after%s:%s" % (name, k)] = v
        if ok:
            break
        print("  %s: seed %d has an indecisive ReLU input (min %s, 8 x dev %s)" % (tag, seed, mn, MARGIN * dev))
    else:
        raise SystemExit("no decisive seed for " + tag)
    fx["weights_checksum"] = np.array(weights_checksum(blk.state_dict()))
    path = os.path.join(HERE, "decoder_block_%s.npz" % tag)
    np.savez_compressed(path, **fx)
    print("decoder_block_%s: seed %d, %d ReLU inputs, min|pre| / dev32 >= %.1f, %d bytes"
          % (tag, seed, len(fx["relu_dev32"]), float((fx["relu_min64"] / np.maximum(fx["relu_dev32"], 1e-300)).min()), os.path.getsize(path)))


def hybrid_case():
    from DPT.ACR import ACR
    from DPT.vit import forward_vit
    model = ACR(20, "vitb_hybrid", seg=True, features=16, use_pretrain=False)
    fill(model, 0)
    model.train()
    img, _ = make_inputs(2, 64, 20, 41)
    fx = {"meta": np.array([64, 2, 20, 41, 16])}
    for k, v in buffers(model).items():
        fx["before:" + k] = v
    with torch.no_grad():
        l1, l2, l3, l4, _, _ = forward_vit(model.pretrained, img)
        sc = model.scratch
        rn = [sc.layer1_rn(l1), sc.layer2_rn(l2), sc.layer3_rn(l3), sc.layer4_rn(l4)]
        p4 = sc.refinenet4(rn[3])
        p3 = sc.refinenet3(p4, rn[2])
        p2 = sc.refinenet2(p3, rn[1])
        p1 = sc.refinenet1(p2, rn[0])
    for i, t in enumerate(rn):
        fx["layer_%d_rn" % (i + 1)] = t.numpy()
    fx["path_1"] = p1.numpy()
    for k, v in buffers(model).items():
        fx["after:" + k] = v
    fx["weights_checksum"] = np.array(weights_checksum({k: v for k, v in model.state_dict().items() if "running_" not in k
                                                        and torch.is_floating_point(v)}))
    path = os.path.join(HERE, "decoder_hybrid_64.npz")
    np.savez_compressed(path, **fx)
    print("decoder_hybrid_64: path_1 %s max %.4f, %d bytes" % (p1.shape, float(p1.abs().max()), os.path.getsize(path)))


def main():
    _install_timm_stub()
    torch.set_num_threads(8)
    torch.manual_seed(0)
    which = set(sys.argv[1:]) or {"layouts", "blocks", "hybrid"}
    if "layouts" in which:
        from DPT.ACR import ACR
        for tag, name in (("hybrid", "vitb_hybrid"), ("vitb", "vitb"), ("deit", "deit"), ("distil", "deit_distilled")):
            mdl = ACR(20, name, seg=True, use_pretrain=False)
            layout = {k: list(v.shape) for k, v in mdl.state_dict().items()}
            with open(os.path.join(HERE, "state_dict_layout_seg_%s.json" % tag), "w") as f:
                json.dump(layout, f, indent=0)
            print("layout seg %s: %d tensors" % (tag, len(layout)))
            del mdl
    if "blocks" in which:
        block_case("a", 64, [(2, 64, 16, 16), (2, 64, 16, 16)], 13, ["train"])
        block_case("b", 16, [(2, 16, 5, 7)], 1, ["train", "eval"])
    if "hybrid" in which:
        hybrid_case()


if __name__ == "__main__":
    main()
