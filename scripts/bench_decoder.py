#!/usr/bin/env python3
"""Micro-benchmark of the DPT decoder kernels (csrc/decoder.hip) and of one fusion block, forward and backward, at the decoder's
production width: 16 x 256 x {28^2, 112^2} fp32.

    python scripts/bench_decoder.py [--sizes 28 112] [--repeats 7] [--iters 10] [--sync W | --readout | --bf16]

Each entry is timed with device events around ``iters`` calls that ROTATE over enough buffer sets to exceed the 256 MiB Infinity
Cache (so a 13 MB tensor at 28^2 is not served from cache), repeated ``repeats`` times: the median and the [min, max] range are
printed.  GB/s are ALGORITHMIC bytes -- what the operation has to move, each tensor once -- over the median; the two-pass
norm kernels read more than that (x twice in the forward, x and dy twice in the backward) and the table says so.  Every
hand-written entry runs next to torch's own operator on the same machine, alternating; the fusion block runs next to a plain torch
composition (nn.BatchNorm2d, F.conv2d, F.relu, F.interpolate) built here.  Needs a GPU: there is no fallback.

``--sync W`` times the cross-rank norm's two halves instead, on ONE device: moments -> W device copies of the (C, 3) rows into the
(W, C, 3) buffer, standing in for the gather -> merged forward, next to the fused ``acr_bn2d_fwd``; and sums -> W copies ->
merged backward next to the fused ``acr_bn2d_bwd``, all through the C ABI on preallocated buffers.  What it shows is the cost of
splitting the per-channel finish in two (launches, the extra round trip of the rows); the collective itself is not in it and
cannot be measured on one GPU.

``--readout [--math f32|f32_split]`` times the read-out heads of the plain ViT backbones instead (``readout_mode``): the two
csrc/reassemble.hip kernels next to a ``copy_`` of the same size, and ``decoder.readout`` forward + backward next to torch's
operators, per tap shape of vitb and vitl at 384^2, batch 16.

``--bf16`` times each of the ten bf16-storage entry points (``acr_bn2d_*_bf16``, ``acr_relu_*_bf16``, ``acr_upsample2x_*_bf16``) next
to its fp32 twin at the same shapes (``bf16_mode``)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acr_wsss_amd import decoder as D  # noqa: E402
from acr_wsss_amd.backbone import set_math  # noqa: E402

DEV = "cuda:0"
N, C = 16, 256
CACHE_BYTES = 256 << 20


def timed(fns, iters, repeats):
    """fns: name -> callable(i) (i = rotation index).  Alternates the entries inside every repeat; returns name -> list of us"""
    out = {k: [] for k in fns}
    for k, fn in fns.items():                                # warm-up: code objects, library algorithm choice
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                fn(i)
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return out


def report(title, times, nbytes):
    for k, v in times.items():
        med = statistics.median(v)
        print("%-34s %-6s median %9.1f us  [%9.1f, %9.1f]  %8.1f GB/s algorithmic" % (title, k, med, min(v), max(v), nbytes / med / 1e3))


def rotation(elem_bytes_per_set):
    return max(2, min(24, -(-2 * CACHE_BYTES // elem_bytes_per_set)))


class TorchRCU(nn.Module):
    def __init__(self, f):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(f, f, 3, 1, 1, bias=False), nn.Conv2d(f, f, 3, 1, 1, bias=False)
        self.bn1, self.bn2 = nn.BatchNorm2d(f), nn.BatchNorm2d(f)

    def forward(self, x):
        return self.bn2(self.conv2(F.relu(self.bn1(self.conv1(F.relu(x)))))) + x


class TorchFusion(nn.Module):
    def __init__(self, f):
        super().__init__()
        self.out_conv = nn.Conv2d(f, f, 1)
        self.resConfUnit1, self.resConfUnit2 = TorchRCU(f), TorchRCU(f)

    def forward(self, a, b):
        out = self.resConfUnit2(a + self.resConfUnit1(b))
        return self.out_conv(F.interpolate(out, scale_factor=2, mode="bilinear", align_corners=True))


def sync_mode(args):
    from acr_wsss_amd import _lib as L
    lib, W = L.load(), args.sync
    st = L.stream_ptr()
    for s in args.sizes:
        tb, hw = 4 * N * C * s * s, s * s
        R = rotation(3 * tb)
        print("\n== %d x %d x %d x %d (%.1f MB per tensor, %d rotating buffer sets), W = %d ==" % (N, C, s, s, tb / 1e6, R, W))
        xs, gs = ([torch.randn(N, C, s, s, device=DEV) for _ in range(R)] for _ in range(2))
        y, dx = torch.empty_like(xs[0]), torch.empty_like(xs[0])
        gamma, beta, rm, rv = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ws = torch.empty(lib.acr_bn2d_ws_bytes(N, C, hw), dtype=torch.uint8, device=DEV)
        f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=DEV)
        stats2, stats3, moments, gathered, sums, gsums = f64(C, 2), f64(3 * C), f64(C, 3), f64(W, C, 3), f64(C, 2), f64(W, C, 2)
        p, nb = L.ptr, ws.numel()

        def fwd_fused(i):
            L.check(lib.acr_bn2d_fwd(p(xs[i % R]), p(gamma), p(beta), p(rm), p(rv), None, None, N, C, hw, 1, 1e-5, 0.1, 0, p(ws), nb, p(stats2),
                                     p(y), st), "acr_bn2d_fwd")

        def fwd_split(i):
            L.check(lib.acr_bn2d_moments(p(xs[i % R]), N, C, hw, p(ws), nb, p(moments), st), "acr_bn2d_moments")
            for r in range(W):
                gathered[r].copy_(moments)
            L.check(lib.acr_bn2d_fwd_merged(p(xs[i % R]), p(gamma), p(beta), p(rm), p(rv), None, None, N, C, hw, p(gathered), W, 1e-5, 0.1, 0,
                                            p(ws), nb, p(stats3), p(y), st), "acr_bn2d_fwd_merged")

        def bwd_fused(i):
            L.check(lib.acr_bn2d_bwd(p(xs[i % R]), None, p(gs[i % R]), p(gamma), p(stats2), N, C, hw, 1, 0, p(ws), nb, p(dx), p(dgamma),
                                     p(dbeta), None, st), "acr_bn2d_bwd")

        def bwd_split(i):
            L.check(lib.acr_bn2d_bwd_sums(p(xs[i % R]), None, p(gs[i % R]), p(stats3), N, C, hw, 0, p(ws), nb, p(sums), p(dgamma), p(dbeta),
                                          st), "acr_bn2d_bwd_sums")
            for r in range(W):
                gsums[r].copy_(sums)
            L.check(lib.acr_bn2d_bwd_merged(p(xs[i % R]), None, p(gs[i % R]), p(gamma), p(stats3), p(gsums), W, N, C, hw, 0, p(ws), nb, p(dx),
                                            None, st), "acr_bn2d_bwd_merged")
        report("bn fwd (train)", timed({"fused": fwd_fused, "split": fwd_split}, args.iters, args.repeats), 2 * tb)
        report("bn bwd (train)", timed({"fused": bwd_fused, "split": bwd_split}, args.iters, args.repeats), 3 * tb)
        del xs, gs
        torch.cuda.empty_cache()


def bf16_mode(args):
    """Each of the ten ``*_bf16`` entry points next to its fp32 twin, through the C ABI on preallocated buffers, alternating inside
    every repeat.  Both walk the same number of values with the same lane assignment; the bf16 one moves half the bytes.  The two
    storage types rotate over the same number of buffer sets, sized so that the bf16 sets alone exceed the Infinity Cache."""
    from acr_wsss_amd import _lib as L
    lib, st, p = L.load(), L.stream_ptr(), L.ptr
    print("%-22s %12s %12s %8s" % ("entry point", "fp32 us", "bf16 us", "bf16/fp32"))
    for s in args.sizes:
        hw, n = s * s, N * C * s * s
        R = rotation(3 * 2 * n)
        print("\n== %d x %d x %d x %d (%.1f MB fp32, %.1f MB bf16 per tensor, %d rotating buffer sets) ==" % (N, C, s, s, 4 * n / 1e6, 2 * n / 1e6, R))
        ws = torch.empty(lib.acr_bn2d_ws_bytes(N, C, hw), dtype=torch.uint8, device=DEV)
        nb = ws.numel()
        f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=DEV)
        stats, stats3, moments, sums = f64(C, 2), f64(3 * C), f64(C, 3), f64(1, C, 2)
        rm, rv, dgamma, dbeta = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        R4 = max(2, R // 4)
        sets = {}
        for tag, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            mk = lambda k, *shape: [torch.randn(*shape, device=DEV).to(dt) for _ in range(k)]
            sets[tag] = dict(x=mk(R, N, C, s, s), g=mk(R, N, C, s, s), y=torch.empty(N, C, s, s, device=DEV, dtype=dt),
                             dx=torch.empty(N, C, s, s, device=DEV, dtype=dt), big=mk(R4, N, C, 2 * s, 2 * s),
                             gamma=torch.ones(C, device=DEV, dtype=dt), beta=torch.zeros(C, device=DEV, dtype=dt))

        def entries(tag):
            b, sfx = sets[tag], "" if tag == "f32" else "_bf16"
            f = lambda name: getattr(lib, (name[:-4] if sfx and name.endswith("_f32") else name) + sfx)
            x, g, big = (lambda i: p(b["x"][i % R])), (lambda i: p(b["g"][i % R])), (lambda i: p(b["big"][i % R4]))
            y, dx, ga, be = p(b["y"]), p(b["dx"]), p(b["gamma"]), p(b["beta"])
            return {
                "bn2d_fwd": lambda i: f("acr_bn2d_fwd")(x(i), ga, be, p(rm), p(rv), None, None, N, C, hw, 1, 1e-5, 0.1, 0, p(ws), nb, p(stats), y, st),
                "bn2d_bwd": lambda i: f("acr_bn2d_bwd")(x(i), None, g(i), ga, p(stats), N, C, hw, 1, 0, p(ws), nb, dx, p(dgamma), p(dbeta), None, st),
                "bn2d_moments": lambda i: f("acr_bn2d_moments")(x(i), N, C, hw, p(ws), nb, p(moments), st),
                "bn2d_fwd_merged": lambda i: f("acr_bn2d_fwd_merged")(x(i), ga, be, p(rm), p(rv), None, None, N, C, hw, p(moments), 1, 1e-5, 0.1, 0,
                                                                      p(ws), nb, p(stats3), y, st),
                "bn2d_bwd_sums": lambda i: f("acr_bn2d_bwd_sums")(x(i), None, g(i), p(stats3), N, C, hw, 0, p(ws), nb, p(sums), p(dgamma), p(dbeta), st),
                "bn2d_bwd_merged": lambda i: f("acr_bn2d_bwd_merged")(x(i), None, g(i), ga, p(stats3), p(sums), 1, N, C, hw, 0, p(ws), nb, dx, None, st),
                "relu_fwd": lambda i: f("acr_relu_fwd_f32")(x(i), n, y, st),
                "relu_bwd": lambda i: f("acr_relu_bwd_f32")(x(i), g(i), n, dx, st),
                "upsample2x_fwd": lambda i: f("acr_upsample2x_fwd")(x(i), N * C, s, s, 2 * s, 2 * s, big(i + 1), st),
                "upsample2x_bwd": lambda i: f("acr_upsample2x_bwd")(big(i), N * C, s, s, 2 * s, 2 * s, dx, st)}
        e32, e16 = entries("f32"), entries("bf16")
        for name in e32:                                         # in this order: moments and sums are filled before the merged halves read them
            def checked(fn, name=name):
                def run(i):
                    L.check(fn(i), name)
                return run
            times = timed({"f32": checked(e32[name]), "bf16": checked(e16[name])}, args.iters, args.repeats)
            m32, m16 = statistics.median(times["f32"]), statistics.median(times["bf16"])
            print("%-22s %12.1f %12.1f %8.2f   [fp32 %.1f .. %.1f, bf16 %.1f .. %.1f]" % (name, m32, m16, m16 / m32, min(times["f32"]),
                                                                                         max(times["f32"]), min(times["bf16"]), max(times["bf16"])))
        del sets
        torch.cuda.empty_cache()


READOUT_SHAPES = {"vitb": (768, [(96, 4), (192, 2), (384, 1), (768, 1)]), "vitl": (1024, [(256, 4), (512, 2), (1024, 1), (1024, 1)])}


def readout_mode(args):
    """Per tap shape of vitb and vitl at 384^2, batch 16 (a 24 x 24 grid, 577 tokens): the two reassemble kernels through the C ABI
    on preallocated buffers, a plain ``copy_`` of the output's size from the same run (the bandwidth yardstick: it reads and writes
    what the shuffle has to), the whole ``decoder.readout`` forward + backward, and torch's operator sequence for the same work
    (slice / transpose / contiguous, ``F.conv2d``, ``F.conv_transpose2d``).  Tap 4's stride-2 3x3 is torch's on both sides and is
    left out."""
    from acr_wsss_amd import _lib as L
    lib, st, p = L.load(), L.stream_ptr(), L.ptr
    B, gh, gw, start = N, 24, 24, 1
    T = start + gh * gw
    math = L.MATH[args.math]
    for name, (Dm, taps) in READOUT_SHAPES.items():
        for tap, (f, s) in enumerate(taps, 1):
            ob = 4 * B * f * gh * s * gw * s                   # bytes of the output map (the token side holds the skipped rows on top)
            R = rotation(2 * ob)
            print("\n== %s tap %d: D %d -> f %d, s %d, out %d x %d x %d x %d (%.1f MB, %d rotating buffer sets), math %s =="
                  % (name, tap, Dm, f, s, B, f, gh * s, gw * s, ob / 1e6, R, args.math))
            y2 = [torch.randn(B * T, f * s * s, device=DEV) for _ in range(R)]
            outs = [torch.randn(B, f, gh * s, gw * s, device=DEV) for _ in range(R)]
            bias, dbias = torch.randn(f, device=DEV), torch.empty(f, device=DEV)
            nws = lib.acr_reassemble_ws_bytes(B, gh, gw, f, s)
            ws = torch.empty(nws, dtype=torch.uint8, device=DEV)

            def k_fwd(i):
                L.check(lib.acr_reassemble_fwd(p(y2[i % R]), f * s * s, p(bias), B, T, start, gh, gw, f, s, p(outs[(i + 1) % R]), st),
                        "acr_reassemble_fwd")

            def k_bwd(i):
                L.check(lib.acr_reassemble_bwd(p(outs[i % R]), B, T, start, gh, gw, f, s, p(y2[(i + 1) % R]), f * s * s, p(dbias), p(ws), nws,
                                               st), "acr_reassemble_bwd")

            def k_copy(i):
                outs[(i + 1) % R].copy_(outs[i % R])
            times = timed({"fwd": k_fwd, "bwd": k_bwd, "copy_": k_copy}, args.iters, args.repeats)
            report("reassemble kernels", times, 2 * ob)
            med = {k: statistics.median(v) for k, v in times.items()}
            print("%-34s fwd %.2f, bwd %.2f of the copy_ rate" % ("reassemble / copy_", med["copy_"] / med["fwd"], med["copy_"] / med["bwd"]))
            del y2
            conv1 = nn.Conv2d(Dm, f, 1).to(DEV)
            deconv = nn.ConvTranspose2d(f, f, s, stride=s).to(DEV) if s > 1 else None
            Rt = max(2, min(R, 4))
            toks = [torch.randn(B, T, Dm, device=DEV) for _ in range(Rt)]
            params = list(conv1.parameters()) + (list(deconv.parameters()) if deconv is not None else [])

            def torch_ops(tok):
                x = tok[:, start:].transpose(1, 2).reshape(B, Dm, gh, gw).contiguous()
                x = F.conv2d(x, conv1.weight, conv1.bias)
                return x if deconv is None else F.conv_transpose2d(x, deconv.weight, deconv.bias, stride=s)

            def whole(fn):
                def run(i):
                    tok = toks[i % Rt].requires_grad_(True)
                    fn(tok).backward(outs[i % R])
                    tok.grad = None
                    for q in params:
                        q.grad = None
                return run
            with torch.no_grad():
                a, b = D.readout(toks[0], start, gh, gw, conv1, deconv, math), torch_ops(toks[0])
                print("readout output, hand-written vs torch's operators: max |diff| %.3e of max %.3e" % (float((a - b).abs().max()), float(b.abs().max())))
                del a, b
            times = timed({"hip": whole(lambda tok: D.readout(tok, start, gh, gw, conv1, deconv, math)), "torch": whole(torch_ops)},
                          max(2, args.iters // 2), args.repeats)
            for k, v in times.items():
                print("%-34s %-6s median %9.1f us  [%9.1f, %9.1f]" % ("readout fwd+bwd", k, statistics.median(v), min(v), max(v)))
            del toks, outs
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--readout", action="store_true", help="time the plain-ViT read-outs (reassemble kernels, readout, torch's operators) instead")
    ap.add_argument("--math", default="f32_split", choices=["f32", "f32_split"], help="arithmetic of --readout's products")
    ap.add_argument("--sizes", type=int, nargs="+", default=[28, 112])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sync", type=int, default=0, metavar="W", help="time the cross-rank norm's halves for W ranks instead")
    ap.add_argument("--bf16", action="store_true", help="time each *_bf16 entry point next to its fp32 twin instead")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decoder.py needs a GPU"
    print("device: %s   N x C = %d x %d fp32   repeats %d x iters %d" % (torch.cuda.get_device_name(0), N, C, args.repeats, args.iters))
    if args.bf16:
        return bf16_mode(args)
    if args.sync:
        return sync_mode(args)
    if args.readout:
        return readout_mode(args)
    for s in args.sizes:
        n = N * C * s * s
        tb = 4 * n                                          # bytes of one (N, C, s, s) tensor
        R = rotation(3 * tb)
        print("\n== %d x %d x %d x %d (%.1f MB per tensor, %d rotating buffer sets) ==" % (N, C, s, s, tb / 1e6, R))
        xs = [torch.randn(N, C, s, s, device=DEV) for _ in range(R)]
        rs = [torch.randn(N, C, s, s, device=DEV) for _ in range(R)]
        gs = [torch.randn(N, C, s, s, device=DEV) for _ in range(R)]
        bn = nn.BatchNorm2d(C).to(DEV).train()
        with torch.no_grad():
            # ---- forward entries
            report("bn fwd (train)", timed({"hip": lambda i: D.batch_norm_act(xs[i % R], bn),
                                            "torch": lambda i: F.batch_norm(xs[i % R], bn.running_mean, bn.running_var, bn.weight, bn.bias, True, 0.1, 1e-5)},
                                           args.iters, args.repeats), 2 * tb)
            report("bn+relu+2 addends fwd (train)",
                   timed({"hip": lambda i: D.batch_norm_act(xs[i % R], bn, "relu", rs[i % R], gs[i % R]),
                          "torch": lambda i: F.relu(F.batch_norm(xs[i % R], bn.running_mean, bn.running_var, bn.weight, bn.bias, True, 0.1, 1e-5)
                                                    + rs[i % R] + gs[i % R])}, args.iters, args.repeats), 4 * tb)
            bn.eval()
            report("bn fwd (eval)", timed({"hip": lambda i: D.batch_norm_act(xs[i % R], bn),
                                           "torch": lambda i: F.batch_norm(xs[i % R], bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.1, 1e-5)},
                                          args.iters, args.repeats), 2 * tb)
            bn.train()
            report("relu fwd", timed({"hip": lambda i: D.relu(xs[i % R]), "torch": lambda i: F.relu(xs[i % R])}, args.iters, args.repeats), 2 * tb)
            report("upsample x2 fwd", timed({"hip": lambda i: D.upsample2x(xs[i % R]),
                                             "torch": lambda i: F.interpolate(xs[i % R], scale_factor=2, mode="bilinear", align_corners=True)},
                                            args.iters, args.repeats), 5 * tb)
        # ---- backward entries: the graph is built once per buffer set, the timed call is the backward alone
        def graphs(fn):
            leaves = [x.detach().clone().requires_grad_(True) for x in xs]
            return leaves, [fn(x) for x in leaves]

        def bwd(leaves, outs, seeds):
            params = [bn.weight, bn.bias]

            def run(i):
                torch.autograd.grad(outs[i % R], [leaves[i % R]] + params, seeds[i % len(seeds)], retain_graph=True, allow_unused=True)
            return run
        h = graphs(lambda x: D.batch_norm_act(x, bn))
        t = graphs(lambda x: F.batch_norm(x, None, None, bn.weight, bn.bias, True, 0.1, 1e-5))
        report("bn bwd (train)", timed({"hip": bwd(*h, gs), "torch": bwd(*t, gs)}, args.iters, args.repeats), 3 * tb)
        del h, t
        h = graphs(lambda x: D.batch_norm_act(x, bn, "relu"))
        t = graphs(lambda x: F.relu(F.batch_norm(x, None, None, bn.weight, bn.bias, True, 0.1, 1e-5)))
        report("bn+relu bwd (train)", timed({"hip": bwd(*h, gs), "torch": bwd(*t, gs)}, args.iters, args.repeats), 4 * tb)
        del h, t
        R4 = max(2, R // 4)
        g4 = [torch.randn(N, C, 2 * s, 2 * s, device=DEV) for _ in range(R4)]
        h = graphs(D.upsample2x)
        t = graphs(lambda x: F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True))

        def ubwd(leaves, outs):
            def run(i):
                torch.autograd.grad(outs[i % R], [leaves[i % R]], g4[i % R4], retain_graph=True)
            return run
        report("upsample x2 bwd", timed({"hip": ubwd(*h), "torch": ubwd(*t)}, args.iters, args.repeats), 5 * tb)
        del h, t, g4
        # ---- one fusion block, two inputs, forward + backward, split-product convolutions against torch's own composition
        torch.manual_seed(0)
        ours = set_math(D.FeatureFusionBlock_custom(C, nn.ReLU(False), bn=True).to(DEV).train(), "f32_split")
        ref = TorchFusion(C).to(DEV).train()
        ref.load_state_dict(ours.state_dict())
        ga = torch.randn(N, C, 2 * s, 2 * s, device=DEV)

        def block(m):
            def run(i):
                a, b = xs[i % R].requires_grad_(True), rs[i % R].requires_grad_(True)
                m(a, b).backward(ga)
                a.grad = b.grad = None
                m.zero_grad(set_to_none=True)
            return run
        with torch.no_grad():
            a, b = ours(xs[0], rs[0]), ref(xs[0], rs[0])
            print("fusion block output, hand-written vs torch composition: max |diff| %.3e of max %.3e" % (float((a - b).abs().max()), float(b.abs().max())))
        times = timed({"hip": block(ours), "torch": block(ref)}, max(2, args.iters // 2), args.repeats)
        for k, v in times.items():
            print("%-34s %-6s median %9.1f us  [%9.1f, %9.1f]" % ("fusion block fwd+bwd (2 inputs)", k, statistics.median(v), min(v), max(v)))
        del xs, rs, gs, ours, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
