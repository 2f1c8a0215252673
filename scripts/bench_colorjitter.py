#!/usr/bin/env python3
"""Micro-benchmark of the colour jitter (csrc/colorjitter.hip, ``acr_color_jitter_batch``) against Pillow, the only other
implementation of it a user of this machine has.

    python scripts/bench_colorjitter.py [--repeats 7] [--iters 20] [--batch 16] [--height 375] [--width 500] [--size 448]

  device   the launches of ``acr_color_jitter_batch`` alone, on pixels and tables that already lie on the device: all four operations
           (a mean pass and an apply pass) and brightness only (no workspace: the apply pass alone).  The jitter works in place, so the
           pixels are restored from a pristine copy before every call, outside the timed interval: device events around each single
           call, summed over ``iters`` calls.  The interval holds both launches and whatever gap the host leaves between them.
  pillow   the same parameters through ``ImageEnhance.Brightness / Contrast / Color`` and the HSV round trip on PIL images that are
           already decoded, the batch on 1 and on 8 host threads (Pillow releases the GIL in these operations); host clock.
  batch    ``preprocess_aff_batch`` (H2D copies, jitter, ``acr_preprocess_batch``, ``acr_aff_label_batch``; n = 3 planes per dump,
           crop ``size``) with and without jitter, host clock around the call and a device synchronise.
Parameters are drawn by ``ColorJitter(0.3, 0.3, 0.3, 0.1, seed=0)``, PSA's setting; the device result is compared with Pillow's for
equality before anything is timed.  The entries are alternated inside each of ``repeats`` rounds in one process; the median and the
[min, max] range over the rounds are printed.  Needs a GPU: there is no fallback."""
import argparse
import concurrent.futures
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acr_wsss_amd import data as D  # noqa: E402

DEV = "cuda:0"


def pil_jitter(im, params):
    from PIL import Image, ImageEnhance
    order, factors = params[0], params[1:]
    for op in order:
        f = factors[op]
        if f is None:
            continue
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(f)
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(f)
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(f)
        else:
            h, s, v = im.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.uint8(int(f * 255) % 256)
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return im


def report(times):
    for k, v in times.items():
        print("  %-44s median %9.4f ms  [%9.4f, %9.4f]" % (k, statistics.median(v), min(v), max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--size", type=int, default=448)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_colorjitter.py needs a GPU"
    from PIL import Image
    import PIL
    B, h, w, S = args.batch, args.height, args.width, args.size
    print("device: %s   Pillow %s   host CPUs %s   repeats %d x iters %d   B = %d images of %d x %d"
          % (torch.cuda.get_device_name(0), PIL.__version__, len(os.sched_getaffinity(0)), args.repeats, args.iters, B, h, w))
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(B)]
    drawer = D.ColorJitter(0.3, 0.3, 0.3, 0.1, seed=0)
    sets = {"all four operations": [drawer.draw() for _ in range(B)]}
    sets["brightness only"] = [((0,), p[1], None, None, None) for p in sets["all four operations"]]
    pil_images = [Image.fromarray(a, "RGB") for a in images]
    shapes = [a.shape[:2] for a in images]
    offs, stage, pristine = D._upload_packed(images, torch.device(DEV))
    packed = pristine.clone()
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=8)

    # ---- the two launches against Pillow ----
    fns, host_fns = {}, {}
    for name, params in sets.items():
        want = [np.asarray(pil_jitter(im, p)) for im, p in zip(pil_images, params)]
        got = D.color_jitter_batch(images, params, DEV)
        same = all(np.array_equal(g, x) for g, x in zip(got, want))
        print("%s: device result equals Pillow's: %s" % (name, same))
        assert same
        tables = D.jitter_tables(params, B)

        def device(tables=tables):
            packed.copy_(pristine)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keep = D.color_jitter_launch(packed, offs, shapes, tables)
            e1.record()
            return e0, e1, keep
        fns["acr_color_jitter_batch, " + name] = device
        host_fns["Pillow, 1 thread, " + name] = lambda params=params: [pil_jitter(im, p) for im, p in zip(pil_images, params)]
        host_fns["Pillow, 8 threads, " + name] = lambda params=params: list(pool.map(pil_jitter, pil_images, params))
    times = {k: [] for k in list(fns) + list(host_fns)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, fn in fns.items():
            pairs = [fn() for _ in range(args.iters)]
            torch.cuda.synchronize()
            times[k].append(sum(e0.elapsed_time(e1) for e0, e1, _ in pairs) / args.iters)
        for k, fn in host_fns.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    print("one batch (the device entries hold the H2D copy of the 5 small tables, not that of the pixels):")
    report(times)
    nbytes = 2 * B * h * w * 3
    for k in fns:
        med = statistics.median(times[k])
        print("  %s: %.1f GB/s of pixel traffic (read + write) at the median -- ALU-bound, not a bandwidth figure" % (k, nbytes / (med * 1e-3) / 1e9))

    # ---- the affinity stage's batch with and without jitter ----
    batcher = D.AffTrainBatcher(S, DEV, seed=0)
    rec = np.zeros(B, D.PRE_IMAGE)
    for i in range(B):
        rec[i] = batcher.draw(h, w)
    la = [(rng.randint(0, 1025, (3, h, w)).astype(np.float32) / np.float32(1024)) for _ in range(B)]
    ha = [(rng.randint(0, 1025, (3, h, w)).astype(np.float32) / np.float32(1024)) for _ in range(B)]
    params = sets["all four operations"]
    plain = D.preprocess_aff_batch(images, la, ha, rec, S, DEV)
    jit = D.preprocess_aff_batch(images, la, ha, rec, S, DEV, jitter=params)
    assert torch.equal(plain[1], jit[1]) and not torch.equal(plain[0], jit[0])
    batch_fns = {"preprocess_aff_batch": lambda: D.preprocess_aff_batch(images, la, ha, rec, S, DEV),
                 "preprocess_aff_batch, jitter": lambda: D.preprocess_aff_batch(images, la, ha, rec, S, DEV, jitter=params)}
    times = {k: [] for k in batch_fns}
    for fn in batch_fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, fn in batch_fns.items():
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / args.iters)
    print("the affinity stage's batch, host clock (n = 3 planes per dump, crop %d):" % S)
    report(times)
    pool.shutdown()


if __name__ == "__main__":
    main()
