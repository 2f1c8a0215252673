#!/usr/bin/env python3
"""Micro-benchmark of the class-centre feature-distance loss (csrc/featdis.hip, ``acr_wsss_amd.featdis``) against the float32 torch
composition of the same definition on the device (tests/featdis_ref.feature_distance: index_add centres, gathered centres, autograd
backward -- not the reference's clone-and-mask text, which no longer runs on the installed torch).

    python scripts/bench_featdis.py [--repeats 7] [--iters 3] [--shapes 16,21,256,224,224 4,21,1024,56,56]

Forward + backward per call.  Both entries are timed with device events around ``iters`` calls, alternated inside each of
``repeats`` rounds in one process after a warm-up; the median and the [min, max] range over the rounds are printed, with the rate
the median stands for over 3 reads + 1 write of ``feat`` (the traffic the arithmetic needs; the kernels as built read it four
times: three in the forward, one in the backward) and the peak device memory of one call of each.  The results are compared before
anything is timed.  Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import featdis_ref as R  # noqa: E402
from acr_wsss_amd.featdis import feature_distance_loss  # noqa: E402

DEV = "cuda:0"


def composition(seg, feat):
    """featdis_ref.feature_distance on the device: its index tensors are built on the CPU there, so the labels' device is used here"""
    B, K, h, w = seg.shape
    C, N = feat.shape[1], h * w
    lab = seg.argmax(1).reshape(B * N)
    f = feat.reshape(B, C, N).permute(0, 2, 1).reshape(B * N, C)
    img = torch.arange(B, device=seg.device).repeat_interleave(N)
    cid = torch.where(lab == 0, img, B + lab - 1)
    NC = B + K - 1
    counts = torch.bincount(cid, minlength=NC)
    div = (counts.double() + R.EPS).float()
    cen = torch.zeros(NC, C, device=seg.device).index_add(0, cid, f) / div[:, None]
    valid = counts >= 1
    mine = cen[cid]
    per_pixel = 1 - (f * mine).sum(1) / (f.norm(dim=1) * mine.norm(dim=1) + R.EPS)
    per_centre = torch.zeros(NC, device=seg.device).index_add(0, cid, per_pixel) / div
    Fn = valid[B:].sum()
    pixel_dis = (torch.where(valid, per_centre, torch.zeros_like(per_centre)).sum() + 2.0 * (~valid[:B]).sum()) / (Fn + B)
    # the centre term with every class kept and the absent ones masked: no host read of F (bench inputs have F > 1 and background)
    g, cb = cen[B:], cen[:B]
    vf = valid[B:].float()
    m = (1 + R.cos(g, g)) * vf[:, None] * vf[None, :]
    ff = (m.sum() - m.diagonal().sum()) / (Fn * (Fn - 1))
    fb = ((1 + R.cos(g, cb)) * vf[:, None]).sum() / (Fn * B)
    return 0.5 * ff + 0.5 * fb + pixel_dis


def timed(fns, iters, repeats):
    out = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(2):
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
            out[k].append(e0.elapsed_time(e1) / iters)
    return out


def peak_mib(fn, resident):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - resident) / 2 ** 20


def bench(shape, iters, repeats):
    B, K, C, h, w = shape
    g = torch.Generator().manual_seed(0)
    # blocky labels as a head predicts them: 8 x 8 patches of one class, background favoured; features = class mean + noise, relu
    coarse = torch.randint(0, K, (B, (h + 7) // 8, (w + 7) // 8), generator=g)
    coarse[torch.rand(coarse.shape, generator=g) < 0.5] = 0
    lab = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :h, :w]
    seg = (torch.nn.functional.one_hot(lab, K).permute(0, 3, 1, 2).float() * 4 + torch.randn(B, K, h, w, generator=g)).contiguous().to(DEV)
    means = torch.randn(K, C, generator=g)
    feat = torch.empty(B, C, h, w, device=DEV)
    for b in range(B):                                           # image by image: the host never holds the whole tensor twice
        feat[b] = torch.relu(means[lab[b]].permute(2, 0, 1) + 0.5 * torch.randn(C, h, w, generator=g)).to(DEV)
    resident = torch.cuda.memory_allocated()
    nbytes = feat.numel() * 4

    def fused():
        f = feat.detach().requires_grad_(True)
        feature_distance_loss(seg, f).backward()
        return f.grad

    def torch32():
        f = feat.detach().requires_grad_(True)
        composition(seg, f).backward()
        return f.grad
    ga, gb = fused(), torch32()
    la, lb = float(feature_distance_loss(seg, feat)), float(composition(seg, feat))
    print("B = %d, K = %d, C = %d, %d x %d (feat %.0f MB): loss fused %.7f torch %.7f; d feat max |diff| %.2e (max |d feat| %.2e)"
          % (B, K, C, h, w, nbytes / 1e6, la, lb, float((ga - gb).abs().max()), float(gb.abs().max())))
    del ga, gb
    fns = {"fused (HIP)": fused, "torch fp32 composition": torch32}
    peaks = {k: peak_mib(fn, resident) for k, fn in fns.items()}
    for k, v in timed(fns, iters, repeats).items():
        med = statistics.median(v)
        print("  %-24s median %9.3f ms  [%9.3f, %9.3f]   %7.1f GB/s over 3 reads + 1 write of feat   peak %8.0f MiB above the inputs"
              % (k, med, min(v), max(v), 4 * nbytes / med / 1e6, peaks[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["16,21,256,224,224", "4,21,1024,56,56"], help="B,K,C,h,w")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_featdis.py needs a GPU"
    print("device: %s   repeats %d x iters %d" % (torch.cuda.get_device_name(0), args.repeats, args.iters))
    for s in args.shapes:
        bench(tuple(int(v) for v in s.split(",")), args.iters, args.repeats)


if __name__ == "__main__":
    main()
