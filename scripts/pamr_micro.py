"""PAMR at VOC size (375 x 500, C = 8 mask planes = two alphas x (background + 3 classes), dilations (1, 2, 4, 8, 12, 24),
10 iterations) for timing and rocprofv3:  python scripts/pamr_micro.py [--reps N] [--out FILE]

Times, at B = 1 and B = 8, with device events around ``--reps`` back-to-back calls after a warm-up of the same shape, repeated
5 times (median, and min..max as the spread): the affinity kernel, one propagate launch, the whole pamr() call, the stock-ops
restatement tests/pamr_ref.py on the same GPU, and crf_with_alpha at two alphas on the same image (host to host, for context).
Achieved GB/s are over the bytes the algorithm needs: affinity K*H*W*4 read + P*H*W*4 written, propagate (P + 2 C)*H*W*4."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from acr_wsss_amd import pamr as P  # noqa: E402
from acr_wsss_amd.crf import crf_with_alpha  # noqa: E402
from pamr_ref import pamr_ref  # noqa: E402

H, W, K, C, N_ITER = 375, 500, 3, 8, 10
DIL = (1, 2, 4, 8, 12, 24)
NP = 8 * len(DIL)


def timed(fn, reps, rounds=5):
    """ms per call: median and (min, max) over `rounds` windows of `reps` calls each, device events, one warm-up window first"""
    for _ in range(max(2, reps // 4)):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def image(B, seed):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, K, H // 6, W // 6, generator=g)
    x = (255 * torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)).round()
    return (x + torch.randint(-6, 7, x.shape, generator=g)).clamp(0, 255).float().contiguous(), torch.rand(B, C, H, W, generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pamr_micro needs a GPU: a CPU run says nothing about these kernels")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("PAMR micro-benchmark: %d x %d, K %d, C %d, dilations %s (P = %d), %d iterations; %s; %d calls per window, 5 windows"
        % (H, W, K, C, DIL, NP, N_ITER, torch.cuda.get_device_name(0), args.reps))
    for B in (1, 8):
        x, mask = image(B, B)
        x, mask = x.cuda(), mask.cuda()
        w = P.affinity(x, DIL)
        aff_bytes = B * (K + NP) * H * W * 4
        prop_bytes = B * (NP + 2 * C) * H * W * 4
        t = timed(lambda: P.affinity(x, DIL), args.reps)
        say("B %d  affinity kernel        %8.4f ms (%.4f .. %.4f)  %7.1f GB/s of %.1f MB algorithmic" % (B, *t, aff_bytes / t[0] / 1e6, aff_bytes / 1e6))
        t = timed(lambda: P.propagate(w, mask, 1, DIL), args.reps)
        say("B %d  one propagate launch   %8.4f ms (%.4f .. %.4f)  %7.1f GB/s of %.1f MB algorithmic" % (B, *t, prop_bytes / t[0] / 1e6, prop_bytes / 1e6))
        t = timed(lambda: P.pamr(x, mask, N_ITER, DIL), args.reps)
        say("B %d  pamr() whole call      %8.4f ms (%.4f .. %.4f)  affinity + %d propagate launches + allocations" % (B, *t, N_ITER))
        t = timed(lambda: pamr_ref(x, mask, N_ITER, DIL), max(2, args.reps // 10))
        say("B %d  stock torch ops (pamr_ref, same GPU) %8.4f ms (%.4f .. %.4f)" % (B, *t))
        err = float((P.pamr(x, mask, N_ITER, DIL) - pamr_ref(x, mask, N_ITER, DIL)).abs().max())
        say("B %d  max|kernels - stock torch ops| = %.3e" % (B, err))
    # the CRF on the same image at two alphas, host dict in, host dict out -- and its PAMR twin, same interface
    x, _ = image(1, 1)
    orig = x[0].permute(1, 2, 0).to(torch.uint8).numpy()
    rng = np.random.default_rng(0)
    cams = {c: rng.random((H, W)).astype(np.float32) for c in (2, 9, 14)}
    for name, fn in (("crf_with_alpha, alphas 1 and 12 (two calls)", lambda: [crf_with_alpha(cams, a, orig) for a in (1, 12)]),
                     ("pamr_with_alpha, alphas 1 and 12 (one call)", lambda: P.pamr_with_alpha(cams, (1, 12), orig, N_ITER, DIL))):
        for _ in range(5):                                   # the first calls of a new shape pay for allocations
            fn()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        say("%s, 3 classes, host to host: %.2f ms / image" % (name, 1e3 * (time.time() - t0) / 20))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
