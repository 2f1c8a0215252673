#!/usr/bin/env python3
"""Call-time benchmark of the dense CRF at two background alphas: two ``crf.crf_with_alpha_device`` calls (what
``infer_cam_list`` made per image) against one ``crf.crf_with_alphas_device`` call over shared lattices, in both input forms.

    python scripts/bench_crf.py [--repeats 9] [--iters 5] [--planes 2 4 21] [--size 375 500] [--alphas 1 12]

Per plane count n (1 background + n - 1 classes per alpha), on one seeded 375 x 500 scene, t = 10 iterations:
    separate      crf_with_alpha_device(cam_dict, low) + crf_with_alpha_device(cam_dict, high): four lattices, two uploads
    shared dict   crf_with_alphas_device(cam_dict, (low, high)): two lattices, numpy backgrounds, one upload (bit-equal planes)
    shared device crf_with_alphas_device(device CAMs, (low, high), device image): two lattices, nothing uploaded
A call holds host work and synchronisations of its own (``acr_lattice_info`` once per lattice), so each entry is timed with a
host clock around ``iters`` calls that ends in a device synchronise; the entries are alternated inside each of ``repeats``
rounds in one process after a warm-up of every entry, and the median and [min, max] over the rounds are printed in ms per
call.  The shared dict planes are compared with the separate ones bit for bit before anything is timed.
Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acr_wsss_amd import crf  # noqa: E402

DEV = "cuda:0"


def scene(h, w, k, seed=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 3) % 256, (yy * 2) % 256, (xx * yy) % 256], -1).astype(np.uint8)
    img[h // 4: 3 * h // 4, w // 3: 2 * w // 3] = (230, 40, 40)
    cams = rng.random((k, h, w)).astype(np.float32) * 0.4
    cams[0, h // 4: 3 * h // 4, w // 3: 2 * w // 3] += 0.55
    return img, cams


def timed(fns, iters, repeats):
    """fns: name -> callable().  Alternates the entries inside every round; returns name -> list of ms per call"""
    out = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / iters * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--planes", type=int, nargs="+", default=[2, 4, 21], help="planes per alpha (background + classes)")
    ap.add_argument("--size", type=int, nargs=2, default=[375, 500])
    ap.add_argument("--alphas", type=float, nargs=2, default=[1, 12])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crf.py needs a GPU"
    h, w = args.size
    low, high = args.alphas
    print("device: %s   %d x %d, alphas %g / %g, t = 10, repeats %d x iters %d" % (torch.cuda.get_device_name(0), h, w, low, high,
                                                                                 args.repeats, args.iters))
    for n in args.planes:
        img, cams = scene(h, w, n - 1)
        classes = list(range(n - 1))
        cam_dict = {c: cams[c] for c in classes}
        d_cams, d_img = torch.from_numpy(cams).to(DEV), torch.from_numpy(img).to(DEV)
        fns = {
            "separate": lambda: [crf.crf_with_alpha_device(cam_dict, a, img, device=DEV)[1] for a in (low, high)],
            "shared dict": lambda: crf.crf_with_alphas_device(cam_dict, (low, high), img, device=DEV)[1],
            "shared device": lambda: crf.crf_with_alphas_device(d_cams, (low, high), d_img, classes=classes)[1],
        }
        sep, both, dev = fns["separate"](), fns["shared dict"](), fns["shared device"]()
        assert torch.equal(torch.cat(sep), both), "shared planes differ from the separate ones"
        print("%d planes per alpha: shared dict == separate bit for bit; shared device vs separate max |dQ| %.2e" % (
            n, float((dev - both).abs().max())))
        res = timed(fns, args.iters, args.repeats)
        base = statistics.median(res["separate"])
        for k, v in res.items():
            med = statistics.median(v)
            print("  %-14s median %8.3f ms  [%8.3f, %8.3f]   %.2f x separate" % (k, med, min(v), max(v), med / base))


if __name__ == "__main__":
    main()
