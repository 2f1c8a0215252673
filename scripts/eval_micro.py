"""Device CAM evaluation at VOC size (375 x 500, 100 thresholds, 21 classes) for timing:
    python scripts/eval_micro.py [--reps N] [--list-images M] [--out FILE]

1. acr_eval_sweep_f32 with n in {1, 3, 20} planes on two inputs -- uniform noise with a random ground truth (every pixel its own
   bin: the worst case for the counting) and a CAM-like one (exact zeros, a few smooth bumps per class, a blocky ground truth: most
   lanes of a wave share a bin) -- in two cache states: "warm", the same buffers launch after launch (they stay in the caches), and
   "rotating", each launch on the next of enough copies to exceed the 256 MiB Infinity Cache.  Device events around windows of
   ``--reps`` launches after a warm-up window, 21 windows: median and min..max per launch.  GB/s are algorithmic:
   (n h w 4 + h w) bytes over the time.
2. For comparison, same arrays: host ``SweepCounters.add`` (host clock), and the device-to-host copy of the CAMs into pinned memory
   (device events) that scoring on the device makes unnecessary FOR SCORING.
3. ``infer_cam_list`` over one fixed list (384^2 inputs, 375 x 500 outputs, 2 positive classes, batch 8) with ``evaluate`` unset
   and set, alternated, ``--rounds`` each, host clock around the whole call (it ends with every result on the host).

``--list-rate TAG [--tree DIR]`` instead times only the walk with ``evaluate`` unset, importing the package from DIR (default:
this tree), and prints / appends to ``--out`` one line ``TAG: <img/s per round>``.  That is how the hook's cost when it is off is
compared with the parent commit (profiles/eval_list_parent_cmp.txt): export the parent into a directory
(``git archive HEAD~1 | tar -x -C DIR``), build its library there, and alternate fresh processes:
    for r in 1 2 3; do python scripts/eval_micro.py --list-rate parent --tree DIR --out F; python scripts/eval_micro.py --list-rate this --out F; done"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W, NT, NC = 375, 500, 100, 21
CLASSES = {1: [14], 3: [1, 8, 14], 20: list(range(20))}


def noise_case(rng, classes):
    cams = rng.random((len(classes), H, W)).astype(np.float32)
    gt = rng.integers(0, NC, (H, W)).astype(np.uint8)
    gt[rng.random((H, W)) < 0.05] = 255
    return cams, gt


def cam_like_case(rng, classes):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    cams = np.zeros((len(classes), H, W), np.float32)
    gt = np.zeros((H, W), np.uint8)
    for j, c in enumerate(classes):
        for _ in range(2):
            cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(20, 70)
            bump = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)
            cams[j] = np.maximum(cams[j], bump)
            if j < 3:
                gt[bump > 0.5] = c + 1
        cams[j][cams[j] < 0.1] = 0.0                          # min-max normalised CAMs: the background is exactly 0
        cams[j] /= cams[j].max()
    gt[:3] = 255
    return cams, gt


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


def list_items(n_images, rng, with_gt=True):
    g = torch.Generator().manual_seed(0)
    items, gts = [], {}
    for i in range(n_images):
        lab = torch.zeros(1, 20)
        lab[0, i % 20] = 1
        lab[0, (i + 7) % 20] = 1
        items.append(("im%d" % i, torch.randn(1, 3, 384, 384, generator=g), lab, (H, W)))
        if with_gt:
            gts["im%d" % i] = cam_like_case(rng, sorted({i % 20, (i + 7) % 20}))[1]
    return items, gts


def list_rate(args):
    """evaluate unset only, package imported from args.tree: works on a tree that has no evaluate keyword yet"""
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import acr_wsss_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(acr_wsss_amd.__file__))) == tree, acr_wsss_amd.__file__
    from acr_wsss_amd.DPT.ACR import ACR
    from acr_wsss_amd.infer_cam import infer_cam_list
    torch.manual_seed(0)
    model = ACR(20, "vitb_hybrid", use_pretrain=False).to("cuda:0").eval()
    items, _ = list_items(args.list_images, None, with_gt=False)
    for _ in range(2):
        infer_cam_list(model, items)
    rates = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        infer_cam_list(model, items)
        rates.append(len(items) / (time.perf_counter() - t0))
    line = "%s: %s img/s" % (args.list_rate, " ".join("%.2f" % r for r in rates))
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--list-images", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--list-rate", default=None, metavar="TAG")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_micro needs a GPU: a CPU run says nothing about these kernels")
    if args.list_rate:
        return list_rate(args)
    sys.path.insert(0, ROOT)
    from acr_wsss_amd import _lib as L
    from acr_wsss_amd import evaluation as E
    lib = L.load()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("CAM evaluation micro-benchmark: %d x %d, %d thresholds, %d classes; %s; %d launches per window, 21 windows (median, min .. max)"
        % (H, W, NT, NC, torch.cuda.get_device_name(0), args.reps))
    th = torch.from_numpy(np.arange(NT, dtype=np.float32) / NT).to(dev)
    raw = torch.zeros(2 * (NT + 1) * NC + NT + 1 + NC + 1, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(0)
    for n, classes in CLASSES.items():
        arr = (ctypes.c_int32 * n)(*classes)
        nbytes = n * H * W * 4 + H * W
        for kind, make in (("noise   ", noise_case), ("cam-like", cam_like_case)):
            cams_np, gt_np = make(rng, classes)
            copies = min(400, -(-320 * 2 ** 20 // nbytes))
            cams = [torch.from_numpy(cams_np).to(dev) for _ in range(copies)]
            gts = [torch.from_numpy(gt_np).to(dev) for _ in range(copies)]
            st = L.stream_ptr()
            pos = [0]

            def launch(rotate):
                i = pos[0] = (pos[0] + 1) % copies if rotate else 0
                L.check(lib.acr_eval_sweep_f32(L.ptr(cams[i]), arr, n, L.ptr(gts[i]), H, W, L.ptr(th), NT, NC, L.ptr(raw), st), "sweep")

            # the counters must be the host's before anything is timed
            raw.zero_()
            launch(False)
            dc = E.DeviceSweepCounters(device=dev)
            dc._raw.copy_(raw)
            want = E.SweepCounters(dc.t)
            want.add({c: cams_np[j] for j, c in enumerate(classes)}, gt_np)
            got = dc.to_host()
            assert np.array_equal(got.TP, want.TP) and np.array_equal(got.P, want.P) and np.array_equal(got.T, want.T)
            for state, rotate in (("warm", False), ("rotating over %d copies" % copies, True)):
                t = windows(lambda: launch(rotate), args.reps)
                say("n %2d %s acr_eval_sweep_f32 %-26s %7.2f us (%.2f .. %.2f)  %7.1f GB/s of %.2f MB algorithmic"
                    % (n, kind, state, *t, nbytes / t[0] / 1e3, nbytes / 1e6))
            cam_dict = {c: cams_np[j] for j, c in enumerate(classes)}
            sc = E.SweepCounters(dc.t)
            sc.add(cam_dict, gt_np)
            t0 = time.perf_counter()
            for _ in range(5):
                sc.add(cam_dict, gt_np)
            say("n %2d %s host SweepCounters.add              %7.2f ms" % (n, kind, 1e3 * (time.perf_counter() - t0) / 5))
            pinned = torch.empty(cams_np.shape, dtype=torch.float32, pin_memory=True)
            t = windows(lambda: pinned.copy_(cams[0], non_blocking=True), max(10, args.reps // 10))
            say("n %2d %s device-to-host copy of the CAMs (pinned) %7.2f us (%.2f .. %.2f)" % (n, kind, *t))
            del cams, gts
    t = windows(lambda: L.check(lib.acr_eval_sweep_finish(L.ptr(raw), NT, NC, L.ptr(raw.new_empty(NT * NC)), L.ptr(raw.new_empty(NT * NC)),
                                                            L.stream_ptr()), "finish"), args.reps)
    say("acr_eval_sweep_finish (once per list)            %7.2f us (%.2f .. %.2f), allocations included" % t)

    # infer_cam_list with and without evaluate, alternated
    from acr_wsss_amd.DPT.ACR import ACR
    from acr_wsss_amd.infer_cam import infer_cam_list
    torch.manual_seed(0)
    model = ACR(20, "vitb_hybrid", use_pretrain=False).to(dev).eval()
    items, gts = list_items(args.list_images, rng)
    infer_cam_list(model, items)                                              # warm-up: graphs, allocator, pinned buffers
    infer_cam_list(model, items, evaluate=E.CamEvaluation(gts.__getitem__))
    rates = {"unset": [], "set": []}
    for _ in range(args.rounds):
        for mode in ("unset", "set"):
            ev = E.CamEvaluation(gts.__getitem__) if mode == "set" else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            infer_cam_list(model, items, evaluate=ev)
            if ev is not None:
                ev.cam.to_host()
            rates[mode].append(len(items) / (time.perf_counter() - t0))
    for mode in ("unset", "set"):
        r = rates[mode]
        say("infer_cam_list, %d images, batch 8, evaluate %-5s: %s img/s (min %.2f, max %.2f)%s"
            % (len(items), mode, " ".join("%.2f" % x for x in r), min(r), max(r), ", to_host() included" if mode == "set" else ""))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
