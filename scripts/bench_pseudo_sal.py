#!/usr/bin/env python3
"""Micro-benchmark of the saliency-guided pseudo-labels (csrc/pseudo_sal.hip, ``pseudo.seg_label_saliency``) at the training shape:
B = 16 images, C = 20 classes, 448 x 448, three present classes per image.

    python scripts/bench_pseudo_sal.py [--repeats 9] [--iters 20]

    compose      seg_label_saliency (clear | 4 x (histogram, pick) | per-pixel | opening), device tensors in, device tensors out
    opening      morph_open alone on the (B, 448, 448) byte map, next to a plain device copy of the same bytes
    host         the numpy restatement of the rule (tests/pseudo_sal_ref.py: np.sort per present class, a brute-force opening) on
                 the same batch, timed once with time.perf_counter -- what the step would cost per batch on the CPU, before the
                 device -> host -> device trip it would also need
Device entries are timed with device events around ``iters`` calls, repeated ``repeats`` times: the median and the [min, max]
range are printed, once for eager calls (the enqueue of each call included) and once for the same calls replayed from a captured
graph (device time alone).  The batch (103 MB of CAMs, of which the 48 present planes are read) stays in the 256 MiB Infinity
Cache between calls: the figures are warm-cache ones, as they are in training, where forward_cam has just written the CAMs.
The device's result is compared with the restatement's before anything is timed.  The inputs and the host baseline come from
tests/pseudo_sal_ref.py (as scripts/pseudo_micro.py takes tests/pseudo_ref.py): the script runs inside a checkout, next to the
test tree.  Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pseudo_sal_ref as R  # noqa: E402
from acr_wsss_amd import pseudo as P  # noqa: E402

DEV = "cuda:0"
B, C, S, PRESENT = 16, 20, 448, 3


def timed(fns, iters, repeats, graph):
    """fns: name -> callable().  Alternates the entries inside every repeat; returns name -> list of us per call"""
    out = {k: [] for k in fns}
    run = {}
    for k, fn in fns.items():
        for _ in range(3):                                   # warm-up: code objects
            fn()
        torch.cuda.synchronize()
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(iters):
                    fn()
            g.replay()
            run[k] = g.replay
        else:
            run[k] = lambda fn=fn: [fn() for _ in range(iters)]
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run[k]()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pseudo_sal.py needs a GPU"
    rng = np.random.default_rng(0)
    present = np.zeros((B, C), np.uint8)
    for i in range(B):
        present[i, rng.choice(C, PRESENT, replace=False)] = 1
    cams = np.zeros((B, C, S, S), np.float32)
    sal = np.zeros((B, S, S), np.uint8)
    for i in range(B):                                       # absent planes stay zero: they are never read
        cams[i, np.flatnonzero(present[i])] = R.bumps(rng, PRESENT, S, S)
        sal[i] = R.saliency_map(rng, S, S)
    print("device: %s   cams %d x %d x %d x %d fp32, %d present classes per image, repeats %d x iters %d" % (
        torch.cuda.get_device_name(0), B, C, S, S, PRESENT, args.repeats, args.iters))
    t0 = time.perf_counter()
    want, want_sal = R.seg_label(cams, present, sal)
    host_s = time.perf_counter() - t0
    d_cams, d_present, d_sal = (torch.from_numpy(x).to(DEV) for x in (cams, present, sal))
    got, got_sal = P.seg_label_saliency(d_cams, d_present, d_sal)
    pre = P.seg_label_saliency(d_cams, d_present, d_sal, open_size=0)[0]
    margin = min(R.margin(cams[i], present[i]) for i in range(B))
    print("device == restatement: label %s, saliency %s (margin of the batch %.2e; decisive above 1e-5)" % (
        bool((got.cpu().numpy() == want).all()), bool((got_sal.cpu().numpy() == want_sal).all()), margin))
    print("host   numpy restatement, whole batch, once: %.1f ms" % (host_s * 1e3))
    dst = torch.empty_like(pre)
    fns = {
        "compose": lambda: P.seg_label_saliency(d_cams, d_present, d_sal),
        "compose open_size=0": lambda: P.seg_label_saliency(d_cams, d_present, d_sal, open_size=0),
        "opening": lambda: P.morph_open(pre, 10),
        "byte copy": lambda: dst.copy_(pre),
    }
    for graph in (False, True):
        for k, v in timed(fns, args.iters, args.repeats, graph).items():
            print("%-6s %-20s median %8.2f us  [%8.2f, %8.2f]" % ("graph" if graph else "eager", k, statistics.median(v), min(v), max(v)))


if __name__ == "__main__":
    main()
