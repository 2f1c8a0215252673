#!/usr/bin/env python3
"""Micro-benchmark of the affinity stage (csrc/affinity.hip, ``acr_wsss_amd.affinity``) against the stock-operator compositions.

    python scripts/bench_affinity.py [--repeats 7] [--iters 5] [--batch 16] [--channels 448] [--size 56] [--planes 21]

  loss   fused ``aff_loss`` forward + backward against the torch gather composition (index the (B, C, hw) map into (B, C, N) and
         (B, C, P, N), abs, mean, exp, log, masked sums, autograd backward) at B = 16, C = 448, 56 x 56, radius 5;
  walk   ``random_walk`` (weight table + 2^8 gather steps), resident and stepwise form, against torch's dense squaring of the
         (hw x hw) transition matrix (build, eight matmuls, one product with the scores) at 56 x 56, K = 21, one image.
Every entry is timed with device events around ``iters`` calls, the entries alternated inside each of ``repeats`` rounds in one
process; the median and the [min, max] range over the rounds are printed.  The results are compared before anything is timed.
Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acr_wsss_amd import affinity as A  # noqa: E402

DEV = "cuda:0"
EPS = 1e-5


def pair_indices(radius, h, w):
    r = radius - 1
    full = torch.arange(h * w, device=DEV).view(h, w)
    frm = full[:h - r, r:w - r].reshape(-1)
    return frm, torch.stack([frm + dy * w + dx for dy, dx in A.search_dist(radius)])


def torch_loss(feat, codes, counts, frm, to):
    B, C, h, w = feat.shape
    flat = feat.reshape(B, C, h * w)
    aff = torch.exp(-(flat[:, :, frm].unsqueeze(2) - flat[:, :, to]).abs().mean(1))
    cnt = counts.to(aff.dtype)
    zero = torch.zeros((), dtype=aff.dtype, device=aff.device)
    bg = torch.where(codes == 1, -torch.log(aff + EPS), zero).sum() / (cnt[0] + EPS)
    fg = torch.where(codes == 2, -torch.log(aff + EPS), zero).sum() / (cnt[1] + EPS)
    neg = torch.where(codes == 3, -torch.log(1 + EPS - aff), zero).sum() / (cnt[2] + EPS)
    return bg / 4 + fg / 4 + neg / 2


def torch_walk(aff, scores, frm, to, beta, logt):
    K, h, w = scores.shape
    T = torch.eye(h * w, device=DEV)
    f, t, a = frm[None].expand_as(to).reshape(-1), to.reshape(-1), aff.reshape(-1) ** beta
    T[f, t] = a
    T[t, f] = a
    T = T / T.sum(0, keepdim=True)
    for _ in range(logt):
        T = T @ T
    return (scores.reshape(K, h * w) @ T).view(K, h, w)


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


def report(title, times):
    print(title)
    for k, v in times.items():
        print("  %-28s median %9.3f ms  [%9.3f, %9.3f]" % (k, statistics.median(v), min(v), max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--channels", type=int, default=448)
    ap.add_argument("--size", type=int, default=56)
    ap.add_argument("--planes", type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_affinity.py needs a GPU"
    B, C, S, K, radius = args.batch, args.channels, args.size, args.planes, 5
    print("device: %s   repeats %d x iters %d" % (torch.cuda.get_device_name(0), args.repeats, args.iters))
    g = torch.Generator().manual_seed(0)
    label = torch.tensor([0, 0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 5, (B, S, S), generator=g)].to(DEV)
    means = torch.randn(256, C, generator=g)
    feat = (means[label.cpu().long()].permute(0, 3, 1, 2) + 0.3 * torch.randn(B, C, S, S, generator=g)).contiguous().to(DEV)
    codes, counts = A.pair_codes(label, radius, 1)
    frm, to = pair_indices(radius, S, S)

    def fused():
        f = feat.detach().requires_grad_(True)
        A.aff_loss(f, codes, counts, radius)[0].backward()
        return f.grad

    def gather():
        f = feat.detach().requires_grad_(True)
        torch_loss(f, codes, counts, frm, to).backward()
        return f.grad
    ga, gb = fused(), gather()
    print("loss, B = %d, C = %d, %d x %d: d feat fused vs torch max |diff| %.2e (max |d feat| %.2e)" % (
        B, C, S, S, float((ga - gb).abs().max()), float(gb.abs().max())))
    del ga, gb
    report("aff_loss forward + backward:", timed({"fused (HIP)": fused, "torch gather composition": gather}, args.iters, args.repeats))

    aff = A.pair_affinity(feat[:1], radius)
    scores = torch.rand(1, K, S, S, generator=g).to(DEV)
    fns = {"random_walk, resident": lambda: A.random_walk(aff, scores, resident=True),
           "random_walk, stepwise": lambda: A.random_walk(aff, scores, resident=False),
           "torch dense squaring": lambda: torch_walk(aff[0], scores[0], frm, to, 8, 8)}
    ref = fns["torch dense squaring"]()
    print("walk, %d x %d, K = %d, logt 8: resident vs torch max |diff| %.2e, resident vs stepwise equal bits: %s" % (
        S, S, K, float((fns["random_walk, resident"]()[0] - ref).abs().max()),
        torch.equal(fns["random_walk, resident"](), fns["random_walk, stepwise"]())))
    report("random_walk (weight table + 256 steps) against the dense power:", timed(fns, args.iters, args.repeats))


if __name__ == "__main__":
    main()
