#!/usr/bin/env python3
"""Generate the decoder fixtures of the plain ViT backbones by running the *reference itself* on the CPU (``ACR_REFERENCE``,
default /root/reference):

    python tests/golden/make_decoder_vit_golden.py [layouts] [vitb] [distil]

``DPT.ACR.ACR(seg=True)``, ``DPT.vit.forward_vit`` and the fusion blocks are imported UNMODIFIED (behind the constants-only ``timm``
stub of make_golden.py); nothing of them is restated here.  Written, data only:
  state_dict_layout_seg_vitl.json   keys and shapes of the reference's ACR(20, "vitl", seg=True)
  decoder_vitb_64x96.npz     ACR(20, "vitb", seg=True, features=16), batch 2, 64 x 96 (a 4 x 6 token grid), training mode
  decoder_distil_96x64.npz   the same for "deit_distilled" at 96 x 64 (start_index 2, a 6 x 4 grid; tap 4 is 3 x 2)
Each .npz holds ``forward_vit``'s four maps (``layer_1`` .. ``layer_4``), the four ``layer_N_rn``, ``path_1`` and the BatchNorm
running statistics before and after the pass.  Weights are tests/golden/recipe.py's function of (key, shape), the running
statistics make_decoder_golden.py's ``running_rule``; the image is ``make_inputs(batch, max(h, w), ...)`` cut to (h, w) from the
top-left corner.  Tensors above 4096 values are stored as every ``stride``-th value (tests/decoder_ref.py ``sample``); the stride, 7,
shares no factor with any extent of these tensors, so the samples walk through every row, column and channel position."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _install_timm_stub  # noqa: E402
from make_decoder_golden import buffers, fill  # noqa: E402
from recipe import make_inputs, weights_checksum  # noqa: E402
from decoder_ref import sample  # noqa: E402

STRIDE = 7
FEATURES = 16
CASES = {"vitb": ("decoder_vitb_64x96", "vitb", 64, 96, 51), "distil": ("decoder_distil_96x64", "deit_distilled", 96, 64, 52)}


def image(batch, h, w, ncls, seed):
    img, _ = make_inputs(batch, max(h, w), ncls, seed)
    return img[:, :, :h, :w].contiguous()


def vit_case(fname, name, h, w, seed):
    from DPT.ACR import ACR
    from DPT.vit import forward_vit
    model = ACR(20, name, seg=True, features=FEATURES, use_pretrain=False)
    fill(model, 0)
    model.train()
    img = image(2, h, w, 20, seed)
    fx = {"meta": np.array([h, w, 2, 20, seed, FEATURES, STRIDE])}
    for k, v in buffers(model).items():
        fx["before:" + k] = v
    with torch.no_grad():
        maps = forward_vit(model.pretrained, img)[:4]
        sc = model.scratch
        rn = [sc.layer1_rn(maps[0]), sc.layer2_rn(maps[1]), sc.layer3_rn(maps[2]), sc.layer4_rn(maps[3])]
        p4 = sc.refinenet4(rn[3])
        p3 = sc.refinenet3(p4, rn[2])
        p2 = sc.refinenet2(p3, rn[1])
        p1 = sc.refinenet1(p2, rn[0])
    for i, (m, t) in enumerate(zip(maps, rn)):
        fx["layer_%d" % (i + 1)] = sample(m.numpy(), STRIDE)
        fx["layer_%d_shape" % (i + 1)] = np.array(m.shape)
        fx["layer_%d_rn" % (i + 1)] = sample(t.numpy(), STRIDE)
        fx["layer_%d_rn_shape" % (i + 1)] = np.array(t.shape)
    fx["path_1"] = sample(p1.numpy(), STRIDE)
    fx["path_1_shape"] = np.array(p1.shape)
    for k, v in buffers(model).items():
        fx["after:" + k] = v
    fx["weights_checksum"] = np.array(weights_checksum({k: v for k, v in model.state_dict().items() if "running_" not in k
                                                        and torch.is_floating_point(v)}))
    path = os.path.join(HERE, fname + ".npz")
    np.savez_compressed(path, **fx)
    print("%s: maps %s, path_1 %s max %.4f, %d bytes" % (fname, [tuple(m.shape) for m in maps], tuple(p1.shape), float(p1.abs().max()),
                                                          os.path.getsize(path)))


def main():
    _install_timm_stub()
    torch.set_num_threads(8)
    torch.manual_seed(0)
    which = set(sys.argv[1:]) or {"layouts", "vitb", "distil"}
    if "layouts" in which:
        from DPT.ACR import ACR
        mdl = ACR(20, "vitl", seg=True, use_pretrain=False)
        layout = {k: list(v.shape) for k, v in mdl.state_dict().items()}
        with open(os.path.join(HERE, "state_dict_layout_seg_vitl.json"), "w") as f:
            json.dump(layout, f, indent=0)
        print("layout seg vitl: %d tensors" % len(layout))
        del mdl
    for tag in ("vitb", "distil"):
        if tag in which:
            vit_case(*CASES[tag])


if __name__ == "__main__":
    main()
