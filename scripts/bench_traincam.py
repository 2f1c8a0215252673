#!/usr/bin/env python3
"""Micro-benchmark of the training-time CAM targets (csrc/traincam.hip, ``traincam.training_cams``) and of the joint step that
uses them (``segtrain.joint_train_step``).

    python scripts/bench_traincam.py [--repeats 9] [--iters 20] [--sizes 256 448] [--step] [--dense]

Kernel timing, B = 16 images, C = 20 classes, three present classes per image, two views, 16 x 16 -> 256 x 256 (the reference's
--crop_size) and 28 x 28 -> 448 x 448:
    fused        training_cams(view 1, labels, (S, S), patch_cam_flipped=view 2): one launch for the extremes, one that writes
    torch        the operator sequence the caller would otherwise write: F.interpolate, multiply, flip, add, amin, amax,
                 subtract, divide
    resize loop  the existing per-image ops.bilinear_resize(..., channels_last=True, chan_mul=, hflip=, out=) calls (two per
                 image), torch.stack and torch's normalisation (amin, amax, subtract, divide)
Every entry is timed with device events around ``iters`` calls, the entries alternated inside each of ``repeats`` rounds in one
process; the median and the [min, max] range over the rounds are printed, with the bytes the entry's operators move (computed
from the shapes below: reads and writes of (B, C, S, S) fp32 tensors, the sources being negligible) and the rate that makes
against the HBM peak.  The output (21 MB / 64 MB) fits the 256 MiB Infinity Cache: warm-cache figures, as in training, where the
next kernel reads the result at once.  The three results are compared before anything is timed.

--step: ``joint_train_step`` against ``train.train_step`` + ``segtrain.seg_train_step`` back to back (two encoder passes) on the
hybrid model, features = 256, 256 x 256, B = 4, split-product math; --dense adds the dense-energy layer to both.
Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acr_wsss_amd import ops  # noqa: E402
from acr_wsss_amd import traincam as T  # noqa: E402

DEV = "cuda:0"
B, C, PRESENT, EPS = 16, 20, 3, 1e-5
HBM_PEAK = 8.0e12          # bytes/s, the HBM3E datasheet figure (a float4 copy reaches 6.3e12)
# passes over a (B, C, S, S) fp32 tensor (reads + writes) of each entry
PASSES = {
    "fused": 1,                                              # every element stored once
    "torch": 2 * 1 + 2 * 2 + 2 + 3 + 1 + 1 + 2 + 2,         # interpolate x2, multiply x2, flip, add, amin, amax, subtract, divide
    "resize loop": 1 + 2 + 2 + 1 + 1 + 2 + 2,               # resize, resize accumulating, stack, amin, amax, subtract, divide
}


def torch_sequence(c1, c2, labels, g, S):
    def up(c):
        x = c.permute(0, 2, 1).reshape(B, C, g, g)
        return F.interpolate(x, (S, S), mode="bilinear", align_corners=False) * labels.view(B, C, 1, 1)
    s = up(c1) + up(c2).flip(-1)
    mn, mx = s.amin((2, 3), keepdim=True), s.amax((2, 3), keepdim=True)
    return (s - mn) / (mx - mn + EPS)


def resize_loop(c1, c2, labels, g, S):
    planes = []
    for b in range(B):
        r = ops.bilinear_resize(c1[b].view(g, g, C), (S, S), False, chan_mul=labels[b], channels_last=True)
        planes.append(ops.bilinear_resize(c2[b].view(g, g, C), (S, S), False, chan_mul=labels[b], hflip=True, out=r, channels_last=True))
    s = torch.stack(planes)
    mn, mx = s.amin((2, 3), keepdim=True), s.amax((2, 3), keepdim=True)
    return (s - mn) / (mx - mn + EPS)


def timed(fns, iters, repeats):
    """fns: name -> callable().  Alternates the entries inside every round; returns name -> list of us per call"""
    out = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(3):                                   # warm-up: code objects, the allocator's blocks
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return out


def bench_kernel(S, iters, repeats):
    g = S // 16
    rng = np.random.default_rng(S)
    lab = np.zeros((B, C), np.float32)
    for i in range(B):
        lab[i, rng.choice(C, PRESENT, replace=False)] = 1
    c1 = torch.from_numpy((rng.random((B, g * g, C), dtype=np.float32) * 4).astype(np.float32)).to(DEV)
    c2 = torch.from_numpy((rng.random((B, g * g, C), dtype=np.float32) * 4).astype(np.float32)).to(DEV)
    labels = torch.from_numpy(lab).to(DEV)
    out = torch.empty((B, C, S, S), dtype=torch.float32, device=DEV)
    fns = {
        "fused": lambda: T.training_cams(c1, labels, (S, S), patch_cam_flipped=c2, eps=EPS, out=out),
        "torch": lambda: torch_sequence(c1, c2, labels, g, S),
        "resize loop": lambda: resize_loop(c1, c2, labels, g, S),
    }
    fused, seq, loop = fns["fused"]().clone(), fns["torch"](), fns["resize loop"]()
    print("%d x %d -> %d x %d: fused vs torch max |diff| %.2e, fused vs resize loop max |diff| %.2e (values in [0, 1])" % (
        g, g, S, S, float((fused - seq).abs().max()), float((fused - loop).abs().max())))
    tensor_bytes = B * C * S * S * 4
    for k, v in timed(fns, iters, repeats).items():
        med = statistics.median(v)
        nbytes = PASSES[k] * tensor_bytes
        print("  %-12s median %9.2f us  [%9.2f, %9.2f]   %7.1f MB moved   %6.3f TB/s = %4.1f %% of the HBM peak" % (
            k, med, min(v), max(v), nbytes / 1e6, nbytes / med / 1e6, 100.0 * nbytes / (med * 1e-6) / HBM_PEAK))


def bench_step(iters, repeats, dense):
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd import segloss
    from acr_wsss_amd.backbone import set_math
    from acr_wsss_amd.DPT.ACR import ACR
    from acr_wsss_amd.segtrain import joint_train_step, seg_train_step
    from acr_wsss_amd.train import PolyOptimizer, train_step
    S, Bs, alpha = 256, 4, 125
    torch.manual_seed(0)
    model = ACR(20, "vitb_hybrid", seg=True, features=256, use_pretrain=False).to(DEV)
    model.set_math("f32_split").train()
    head = D.SegmentationHead(256, 20).to(DEV).train()
    set_math(head, "f32_split")
    layer = segloss.DenseEnergyLoss(1e-3, 15.0, 40.0, 1.0) if dense else None
    rng = np.random.default_rng(1)
    images = torch.randn(Bs, 3, S, S, device=DEV)
    ori = torch.from_numpy(rng.integers(0, 256, (Bs, 3, S, S), dtype=np.uint8)).to(DEV)
    crop = torch.ones(S, S, Bs, device=DEV)
    labels = torch.zeros(Bs, 20, device=DEV)
    for i in range(Bs):
        labels[i, rng.choice(20, PRESENT, replace=False)] = 1
    sal = rng.integers(1, 256, (Bs, S, S)).astype(np.uint8)
    sal[:, :, : S // 4] = 0
    sal = torch.from_numpy(sal).to(DEV)
    seg_label = torch.from_numpy(rng.integers(0, 21, (Bs, S, S)).astype(np.uint8)).to(DEV)
    opt = PolyOptimizer(list(model.parameters()) + list(head.parameters()), lr=1e-4, weight_decay=5e-4, max_step=10 ** 6)

    def joint():
        joint_train_step(model, head, opt, images, ori, crop, labels, sal, layer, alpha=alpha)

    def two_programmes():
        train_step(model, opt, images, labels, alpha)
        seg_train_step(model, head, opt, images, ori, crop, seg_label, layer)
    print("step, hybrid, features 256, %d x %d, B = %d, f32_split%s:" % (S, S, Bs, ", dense energy" if dense else ""))
    for k, v in timed({"joint_train_step": joint, "train_step + seg_train_step": two_programmes}, iters, repeats).items():
        print("  %-28s median %9.2f ms  [%9.2f, %9.2f]" % (k, statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 448], help="crop sizes of the kernel timing (multiples of 16)")
    ap.add_argument("--step", action="store_true", help="time joint_train_step against train_step + seg_train_step instead")
    ap.add_argument("--dense", action="store_true", help="--step with the dense-energy layer")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_traincam.py needs a GPU"
    print("device: %s   repeats %d x iters %d" % (torch.cuda.get_device_name(0), args.repeats, args.iters))
    if args.step:
        bench_step(args.iters, args.repeats, args.dense)
        return
    print("B = %d, C = %d, %d present classes per image, two views" % (B, C, PRESENT))
    for S in args.sizes:
        bench_kernel(S, args.iters, args.repeats)


if __name__ == "__main__":
    main()
