"""Pseudo-label composition at VOC size (375 x 500) for timing:
    python scripts/pseudo_micro.py [--reps N] [--out FILE]

``pseudo.seg_label`` on device tensors, K in {3, 20} present classes, ignore_uncertain off and on, in two cache states: "warm", the
same buffers call after call (they stay in the caches), and "rotating", each call on the next of enough copies to exceed the
256 MiB Infinity Cache.  Device events around windows of ``--reps`` calls after a warm-up window, 21 windows: median and min..max per
call; a call is every launch of the composition (1 without the confidence rule, a clear + 9 with it) plus the Python wrapper and its
two allocations.  GB/s are algorithmic: the (3 K + 2) input planes read once plus the label map written once.
For comparison, same arrays: the numpy restatement tests/pseudo_ref.py on the host (host clock, 3 calls).
The device result is compared with the restatement's before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 375, 500
CLASSES = {3: [1, 8, 14], 20: list(range(20))}


def windows(launch, reps, rounds=21):
    for _ in range(reps):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            launch()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / reps)
    us.sort()
    return us[len(us) // 2], us[0], us[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pseudo_micro needs a GPU: a CPU run says nothing about these kernels")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pseudo_ref as R
    from acr_wsss_amd import pseudo as P
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("pseudo-label composition micro-benchmark: %d x %d; %s; %d calls per window, 21 windows (median, min .. max)"
        % (W, H, torch.cuda.get_device_name(0), args.reps))
    for k, classes in CLASSES.items():
        cams_np, _, la_np, ha_np, mg = R.decisive_case(seed=100 + k, k=k, w=W, h=H, classes=classes)
        nbytes = (3 * k + 2) * W * H * 4 + W * H
        copies = min(200, -(-320 * 2 ** 20 // nbytes))
        sets = [[torch.from_numpy(a).to(dev) for a in (cams_np, la_np, ha_np)] for _ in range(copies)]
        pos = [0]
        for unc in (False, True):
            def launch(rotate, unc=unc):
                i = pos[0] = (pos[0] + 1) % copies if rotate else 0
                return P.seg_label(sets[i][0], classes, sets[i][1], sets[i][2], ignore_uncertain=unc)

            want = R.seg_label(cams_np, classes, la_np, ha_np, ignore_uncertain=unc)
            assert np.array_equal(launch(False).cpu().numpy(), want) and np.array_equal(launch(True).cpu().numpy(), want)
            for state, rotate in (("warm", False), ("rotating over %d copies" % copies, True)):
                t = windows(lambda: launch(rotate), args.reps)
                say("K %2d ignore_uncertain=%d seg_label %-26s %8.2f us (%.2f .. %.2f)  %7.1f GB/s of %.2f MB algorithmic"
                    % (k, unc, state, *t, nbytes / t[0] / 1e3, nbytes / 1e6))
            R.seg_label(cams_np, classes, la_np, ha_np, ignore_uncertain=unc)
            t0 = time.perf_counter()
            for _ in range(3):
                R.seg_label(cams_np, classes, la_np, ha_np, ignore_uncertain=unc)
            say("K %2d ignore_uncertain=%d numpy restatement on the host      %8.2f ms" % (k, unc, 1e3 * (time.perf_counter() - t0) / 3))
        del sets
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
