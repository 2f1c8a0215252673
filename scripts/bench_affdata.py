#!/usr/bin/env python3
"""Micro-benchmark of the affinity stage's label kernel (csrc/affdata.hip, ``acr_aff_label_batch``) against a torch composition of
the same rule on the device.

    python scripts/bench_affdata.py [--repeats 7] [--iters 20] [--batch 16] [--size 448] [--height 375] [--width 500]

  kernel  ONE ``acr_aff_label_batch`` launch on scores that already lie on the device (the table and the offsets too: the entry point
          alone, not the H2D copy in front of it);
  torch   per image flip, crop and ``F.pad`` of both stacks into the (2n, S, S) zero container, then over the batch ``avg_pool2d(8)``,
          the maximum, two argmaxes and three ``where`` -- every image with n planes, so that the containers stack.
at n = 3 and n = 21 planes per dump, images of height x width cropped to size x size with boxes and flips drawn by
``AffTrainBatcher(seed=0)``.  Scores lie on a 2^-10 grid, so both sides sum exactly and the labels are compared for equality before
anything is timed.  Every entry is timed with device events around ``iters`` calls, the entries alternated inside each of ``repeats``
rounds in one process; the median and the [min, max] range over the rounds are printed, and the kernel's GB/s over the bytes the rule
needs (2 n ch cw 4 per image).  Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acr_wsss_amd import _lib as L  # noqa: E402
from acr_wsss_amd import data as D  # noqa: E402

DEV = "cuda:0"


def torch_labels(la, ha, rec, S):
    conts = []
    for a, b, r in zip(la, ha, rec):
        x = torch.cat((a, b))
        if r["flip"]:
            x = x.flip(-1)
        ct, cl, it, il, ch, cw = (int(r[k]) for k in ("cont_top", "cont_left", "img_top", "img_left", "ch", "cw"))
        conts.append(F.pad(x[:, it:it + ch, il:il + cw], (cl, S - cl - cw, ct, S - ct - ch)))
    pooled = F.avg_pool2d(torch.stack(conts), 8)
    n = pooled.shape[1] // 2
    lo, hi = pooled[:, :n].argmax(1), pooled[:, n:].argmax(1)
    label = torch.where(lo == 0, 255, lo)
    label = torch.where(hi == 0, 0, label)
    return torch.where(pooled.amax(1) < 1e-5, 255, label).to(torch.uint8)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=500)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_affdata.py needs a GPU"
    B, S, h, w = args.batch, args.size, args.height, args.width
    lib = L.load()
    print("device: %s   repeats %d x iters %d" % (torch.cuda.get_device_name(0), args.repeats, args.iters))
    batcher = D.AffTrainBatcher(S, DEV, seed=0)
    rec = np.zeros(B, D.PRE_IMAGE)
    for i in range(B):
        rec[i] = batcher.draw(h, w)
    D._check_aff_records(rec, [(h, w)] * B, S, S)
    table = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV)
    label = torch.empty((B, S // 8, S // 8), dtype=torch.uint8, device=DEV)
    g = torch.Generator().manual_seed(0)
    for n in (3, 21):
        buf = (torch.randint(0, 1025, (B, 2, n, h, w), generator=g).to(torch.float32) / 1024).to(DEV)
        offs = (torch.arange(2 * B, dtype=torch.int64) * (4 * n * h * w)).view(B, 2).t().contiguous().to(DEV)      # row 0: la, row 1: ha
        planes = torch.full((B,), n, dtype=torch.int32, device=DEV)
        la, ha = [buf[i, 0] for i in range(B)], [buf[i, 1] for i in range(B)]

        def kernel():
            L.check(lib.acr_aff_label_batch(L.ptr(buf), L.ptr(table), L.ptr(offs[0]), L.ptr(offs[1]), L.ptr(planes), B, S, S, L.ptr(label),
                                            L.stream_ptr()), "acr_aff_label_batch")
            return label

        def composition():
            return torch_labels(la, ha, rec, S)
        same = torch.equal(kernel(), composition())
        nbytes = sum(2 * n * int(r["ch"]) * int(r["cw"]) * 4 for r in rec)
        print("B = %d, %d x %d -> %d x %d, n = %d: labels equal: %s; %.1f MB of scores inside the boxes" % (B, h, w, S, S, n, same, nbytes / 1e6))
        assert same
        times = timed({"acr_aff_label_batch (HIP)": kernel, "torch composition": composition}, args.iters, args.repeats)
        for k, v in times.items():
            print("  %-28s median %9.4f ms  [%9.4f, %9.4f]" % (k, statistics.median(v), min(v), max(v)))
        med = statistics.median(times["acr_aff_label_batch (HIP)"])
        print("  kernel: %.1f GB/s at the median" % (nbytes / (med * 1e-3) / 1e9))


if __name__ == "__main__":
    main()
