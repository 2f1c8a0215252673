#!/usr/bin/env python3
"""Micro-benchmark of the fused segmentation prediction kernel (csrc/segpred.hip, ``segval.predict``) at the validation shape:
1 x 21 x 384 x 384 fp32 logits -> 375 x 500 and -> 500 x 375.

    python scripts/bench_segval.py [--repeats 9] [--iters 20]

Every entry runs next to torch's own operator sequence on the same tensors, alternating inside every repeat:
    label        F.interpolate(align_corners=False) -> argmax                   vs  predict(logits, hw)
    probs+label  F.interpolate -> softmax -> argmax                             vs  predict(logits, hw, probs=buffer)
    accumulate   buffer += softmax(F.interpolate); argmax(buffer)               vs  predict(..., probs=buffer, accumulate=True)
Timed with device events around ``iters`` calls that ROTATE over enough logits (and probability) buffers to exceed the 256 MiB
Infinity Cache, repeated ``repeats`` times: the median and the [min, max] range are printed, once for eager calls (the enqueue of
each call included: a kernel of a few microseconds is bounded by it) and once for the same calls replayed from a captured graph
(device time alone).  GB/s are ALGORITHMIC bytes over the median: the source once, every output once (the accumulating buffer is
read and written).  torch's intermediate (K, H, W) tensors come from its caching allocator and are not rotated.  Needs a GPU:
there is no fallback."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acr_wsss_amd import segval as V  # noqa: E402

DEV = "cuda:0"
B, K, S = 1, 21, 384
CACHE_BYTES = 256 << 20
HBM_BYTES_PER_S = 6.3e12                  # achievable streaming rate of the MI355X (8.0 TB/s peak by specification)


def timed(fns, iters, repeats, graph):
    """fns: name -> callable(i) (i = rotation index).  Alternates the entries inside every repeat; returns name -> list of us"""
    out = {k: [] for k in fns}
    run = {}
    for k, fn in fns.items():                                # warm-up: code objects
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for i in range(iters):
                    fn(i)
            g.replay()
            run[k] = g.replay
        else:
            run[k] = lambda fn=fn: [fn(i) for i in range(iters)]
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


def report(title, times, nbytes):
    for k, v in times.items():
        med = statistics.median(v)
        print("%-30s %-6s median %8.2f us  [%8.2f, %8.2f]  %7.1f GB/s algorithmic = %4.1f %% of %.1f TB/s" % (
            title, k, med, min(v), max(v), nbytes / med / 1e3, 100.0 * nbytes / (med * 1e-6) / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_segval.py needs a GPU"
    src = 4 * B * K * S * S
    R = -(-2 * CACHE_BYTES // src)                           # logits buffers: twice the Infinity Cache
    print("device: %s   logits %d x %d x %d x %d fp32 (%.1f MB), %d rotating sets, repeats %d x iters %d" % (
        torch.cuda.get_device_name(0), B, K, S, S, src / 1e6, R, args.repeats, args.iters))
    torch.manual_seed(0)
    xs = [2.0 * torch.randn(B, K, S, S, device=DEV) for _ in range(R)]
    with torch.no_grad():
        for hw in ((375, 500), (500, 375)):
            H, W = hw
            lab, prb = B * H * W, 4 * B * K * H * W
            ps = [torch.zeros(B, K, H, W, device=DEV) for _ in range(R)]
            # the two paths agree on what they compute (labels may differ on fp32 ties only)
            want = F.interpolate(xs[0], hw, mode="bilinear", align_corners=False)
            got = V.predict(xs[0], hw, probs=ps[0])
            print("\n== -> %d x %d: labels differing from torch %d of %d, max |probs - torch| %.2e ==" % (
                H, W, int((got.long() != want.argmax(1)).sum()), lab, float((ps[0] - want.softmax(1)).abs().max())))

            def t_acc(i):
                p = ps[i % R]
                p += F.interpolate(xs[i % R], hw, mode="bilinear", align_corners=False).softmax(1)
                return p.argmax(1)
            entries = (
                ("label", src + lab, {"hip": lambda i: V.predict(xs[i % R], hw),
                                      "torch": lambda i: F.interpolate(xs[i % R], hw, mode="bilinear", align_corners=False).argmax(1)}),
                ("probs+label", src + prb + lab, {"hip": lambda i: V.predict(xs[i % R], hw, probs=ps[i % R]),
                                                  "torch": lambda i: F.interpolate(xs[i % R], hw, mode="bilinear", align_corners=False).softmax(1).argmax(1)}),
                ("accumulate+label", src + 2 * prb + lab, {"hip": lambda i: V.predict(xs[i % R], hw, probs=ps[i % R], accumulate=True),
                                                           "torch": t_acc}),
            )
            for graph in (False, True):
                for name, nbytes, fns in entries:
                    title = "%s %s" % ("graph" if graph else "eager", name)
                    report(title, timed(fns, args.iters, args.repeats, graph), nbytes)
            del ps
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
