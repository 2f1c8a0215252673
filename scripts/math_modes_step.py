"""Step time of the BASELINE training step (448^2, batch 16, fp32 tensors) under math="f32_split" and math="f32_fp16x2",
alternating in one process on one model (outside bench.py: fp16x2 is opt-in and never the headline).

    python scripts/math_modes_step.py [--steps 6] [--warmup 2] [--rounds 3] [--modes f32_split,f32_fp16x2] [--out FILE]

Per mode and round: ms per step (host clock around K steps that end in a device synchronise), img/s and
torch.cuda.max_memory_allocated over those steps.  One JSON line per (round, mode), then a summary line with the medians."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--modes", default="f32_split,f32_fp16x2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from acr_wsss_amd.DPT.ACR import ACR
    from acr_wsss_amd.train import PolyOptimizer, train_step

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = ACR(num_classes=20, backbone_name="vitb_hybrid", use_pretrain=False, math="f32_split").to(dev).train()
    opt = PolyOptimizer(model.parameters(), lr=0.05, weight_decay=5e-4, max_step=100000)
    g = torch.Generator(device="cpu").manual_seed(0)
    img = torch.randn(args.batch, 3, args.size, args.size, generator=g).to(dev)
    label = (torch.rand(args.batch, 20, generator=g) < 0.15).float().to(dev)
    label[:, 0] = 1.0
    modes = args.modes.split(",")
    recs = []
    for rnd in range(args.rounds):
        for mode in modes:
            model.set_math(mode)
            for _ in range(args.warmup):
                train_step(model, opt, img, label, 125)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss, _ = train_step(model, opt, img, label, 125)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            rec = {"round": rnd, "mode": mode, "ms_per_step": round(dt * 1e3, 3), "img_per_s": round(args.batch / dt, 2),
                   "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), "loss": round(float(loss.detach()), 5)}
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    summary = {"summary": {m: {"ms_per_step_median": statistics.median(r["ms_per_step"] for r in recs if r["mode"] == m),
                                "img_per_s_median": statistics.median(r["img_per_s"] for r in recs if r["mode"] == m),
                                "max_memory_allocated_gb": max(r["max_memory_allocated_gb"] for r in recs if r["mode"] == m)} for m in modes},
               "config": {"batch": args.batch, "size": args.size, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                          "device": torch.cuda.get_device_name(0)}}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in recs + [summary]:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
