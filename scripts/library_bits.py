#!/usr/bin/env python3
"""library_bits.py LIB.so: the bits a build of the library computes, one line per output, to be diffed against another build's.

Runs once, in this one process, the entry points whose kernels share acr_resample.h / acr_reduce.h (and preprocess.hip's sample)
and the three generations of fp32 attention (attn_f32_scores.h) on seeded inputs at the smallest shapes that reach every branch, and prints `entry  case  shape  dtype  sha256` per output.  All of
these kernels are bit-identical run to run, so two builds agree exactly when the two outputs are equal line for line:
    library_bits.py old/libacr_hip.so > a; library_bits.py new/libacr_hip.so > b; diff a b
The library is picked through ACR_LIB_PATH (acr_wsss_amd/_lib.py).  Needs a GPU; takes seconds."""
import hashlib
import os
import sys

if len(sys.argv) != 2:
    sys.exit(__doc__)
os.environ["ACR_LIB_PATH"] = os.path.abspath(sys.argv[1])          # read when the package is imported
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from acr_wsss_amd import _lib as L, data, decoder, ops, segloss, segval  # noqa: E402

DEV = torch.device("cuda:0")
GEN = torch.Generator(device="cpu").manual_seed(20)


def emit(entry, case, t):
    t = t.detach().contiguous().cpu()
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    print("%-22s %-34s %-18s %-9s %s" % (entry, case, tuple(t.shape), str(t.dtype)[6:], hashlib.sha256(raw.numpy().tobytes()).hexdigest()))


def rnd(*shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(shape, generator=GEN) * scale).to(DEV).to(dtype)


def grads(entry, case, outs, ins, names, show=False):
    """the gradients of sum(out * seeded weights) over `outs` with respect to `ins`; with `show` the single output first"""
    if show:
        emit(entry, case, outs[0])
    for n, g in zip(names, torch.autograd.grad(outs, ins, [rnd(*o.shape, dtype=o.dtype) for o in outs], allow_unused=True)):
        if g is not None:
            emit(entry, case + " d" + n, g)


def segpred():
    for (b, k, h, w, H, W) in ((2, 21, 12, 20, 37, 53), (2, 3, 40, 24, 17, 11)):       # enlarging; shrinking with K below the unroll
        lg = rnd(b, k, h, w, scale=3.0)
        for flip in (False, True):
            case = "%dx%d>%dx%d K%d flip%d" % (h, w, H, W, k, flip)
            emit("segval.predict", case + " label", segval.predict(lg, (H, W), hflip=flip))
            probs = torch.empty((b, k, H, W), device=DEV)
            emit("segval.predict", case + " probs.label", segval.predict(lg, (H, W), hflip=flip, probs=probs))
            emit("segval.predict", case + " probs", probs)
            emit("segval.predict", case + " accum.label", segval.predict(lg, (H, W), hflip=flip, probs=probs, accumulate=True))
            emit("segval.predict", case + " accum", probs)


def seglosses():
    for (b, k, h, w, W, H) in ((2, 21, 9, 13, 33, 50), (1, 2, 8, 8, 8, 8)):
        lab = torch.randint(0, k, (b, W, H), generator=GEN).to(torch.uint8)
        lab[torch.rand(b, W, H, generator=GEN) < 0.1] = 255
        lab = lab.to(DEV)
        for want_probs in (False, True):
            lg = rnd(b, k, h, w, scale=2.0).requires_grad_(True)
            case = "%dx%d>%dx%d K%d probs%d" % (h, w, W, H, k, want_probs)
            loss, probs, sums, counts = segloss._split_ce(lg, lab, True, want_probs)
            for n, t in (("loss", loss), ("sums", sums), ("counts", counts)) + ((("probs", probs),) if want_probs else ()):
                emit("segloss", case + " " + n, t)
            grads("segloss", case, [loss, probs] if want_probs else [loss], [lg], ["logits"])
    lib = L.load()
    for count in (1000, 256 * 256 + 17):                                               # the latter: the cap of 256 workgroups
        s, a = rnd(count), rnd(count)
        grad, out = torch.empty(count, device=DEV), torch.empty(1, device=DEV)
        ws = torch.empty(segloss._ENERGY_WS_BYTES, dtype=torch.uint8, device=DEV)
        L.check(lib.acr_dense_energy_dot(L.ptr(s), L.ptr(a), count, -0.25, L.ptr(grad), L.ptr(ws), ws.numel(), L.ptr(out), L.stream_ptr()),
                "acr_dense_energy_dot")
        emit("acr_dense_energy_dot", "count %d dot" % count, out)
        emit("acr_dense_energy_dot", "count %d grad" % count, grad)


def resize():
    src = rnd(3, 7, 5)
    for hw in ((16, 11), (3, 2)):
        for ac in (False, True):
            out = ops.bilinear_resize(src, hw, ac, chan_mul=torch.tensor([1.0, 0.5, 2.0]))
            emit("ops.bilinear_resize", "7x5>%dx%d corners%d" % (hw + (ac,)), out)
            emit("ops.bilinear_resize", "7x5>%dx%d corners%d +flip" % (hw + (ac,)), ops.bilinear_resize(src, hw, ac, hflip=True, out=out))


def decoders():
    for (n, c, h, w) in ((2, 5, 7, 9), (2, 16, 8, 8)):                                 # unaligned rows (scalar walk); 16-byte vectors
        for act in ("none", "relu"):
            bn = torch.nn.BatchNorm2d(c).to(DEV).train()
            with torch.no_grad():
                bn.weight.copy_(1 + 0.2 * rnd(c))
                bn.bias.copy_(0.3 * rnd(c))
            x, r = rnd(n, c, h, w, scale=1.5).requires_grad_(True), rnd(n, c, h, w).requires_grad_(True)
            case = "%dx%dx%dx%d %s" % (n, c, h, w, act)
            y = decoder.batch_norm_act(x, bn, act, r if act == "relu" else None)
            for nm, t in (("y", y), ("running_mean", bn.running_mean), ("running_var", bn.running_var)):
                emit("decoder.batch_norm_act", case + " " + nm, t)
            grads("decoder.batch_norm_act", case, [y], [x, bn.weight, bn.bias, r], ["x", "gamma", "beta", "resid"])
    x = rnd(1, 3, 5, 7).requires_grad_(True)
    grads("decoder.upsample2x", "3 planes 5x7", [decoder.upsample2x(x)], [x], ["x"], show=True)


def loaders():
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), rng.integers(0, 256, (64, 40, 3), dtype=np.uint8)]
    maps = [rng.integers(0, 21, a.shape[:2], dtype=np.uint8) for a in imgs]
    for S in (32, 30):                                                                 # 4 pixels per thread; one
        draw = data.TrainBatcher(S, device=DEV, seed=S).draw                           # resize-long to about S, crop box smaller than S
        rec = np.zeros(2, data.PRE_IMAGE)
        for i, a in enumerate(imgs):
            rec[i] = draw(a.shape[0], a.shape[1])
        rec["flip"] = (1, 0)
        for dtype in (torch.float32, torch.bfloat16):
            case = "S%d %s" % (S, str(dtype)[6:])
            emit("data.preprocess_batch", case, data.preprocess_batch(imgs, rec, S, DEV, dtype))
            for n, t in zip(("images", "ori", "croppings", "map"), data.preprocess_seg_batch(imgs, maps, rec, S, DEV, dtype, map_fill=255)):
                emit("data.preprocess_seg", case + " " + n, t)


def step_kernels():
    for n in (3, 300):
        x, y = rnd(n, 20).requires_grad_(True), (torch.rand(n, 20, generator=GEN) < 0.2).float().to(DEV)
        grads("ops.mlsm_loss", "N%d C20" % n, [ops.mlsm_loss(x, y)], [x], ["x"], show=True)
    for dtype in (torch.bfloat16, torch.float32):
        dn = str(dtype)[6:]
        for act in ("none", "relu", "add_relu"):
            x = rnd(2, 64, 8, 8, scale=1.7, dtype=dtype).requires_grad_(True)
            w, b = (1 + 0.2 * rnd(64)).to(dtype).requires_grad_(True), rnd(64, scale=0.3, dtype=dtype).requires_grad_(True)
            r = rnd(2, 64, 8, 8, dtype=dtype).requires_grad_(True) if act == "add_relu" else None
            grads("ops.groupnorm_act", "2x64x8x8 %s %s" % (dn, act), [ops.groupnorm_act(x, w, b, act, r)], [x, w, b] + ([r] if r is not None else []),
                  ["x", "gamma", "beta", "resid"], show=True)
        for (m, c) in ((1, 256), (37, 768)):
            ln = torch.nn.LayerNorm(c, eps=1e-6).to(DEV).to(dtype)
            with torch.no_grad():
                ln.weight.copy_(1 + 0.2 * rnd(c))
                ln.bias.copy_(0.3 * rnd(c))
            x = rnd(m, c, scale=2.0, dtype=dtype).requires_grad_(True)
            grads("ops.layer_norm", "%dx%d %s" % (m, c, dn), [ops.layer_norm(x, ln)], [x, ln.weight, ln.bias], ["x", "gamma", "beta"], show=True)
    ws = [rnd(*s, scale=0.3, dtype=torch.bfloat16).requires_grad_(True) for s in ((64, 3, 7, 7), (64, 64, 1, 1), (256, 64, 3, 3), (33, 5, 1, 1))]
    outs = ops.weight_std_all(ws)
    for i, o in enumerate(outs):
        emit("ops.weight_std_all", "weight %d" % i, o)
    grads("ops.weight_std_all", "weights", list(outs), ws, [str(i) for i in range(len(ws))])
    for (b, l, p) in ((1, 1, 1), (2, 3, 4)):                                           # the lane-per-element kernel; the p % 4 == 0 one
        a = torch.rand(2 * b, l, p * p + 1, p * p + 1, generator=GEN).to(DEV).requires_grad_(True)
        cls, aff = ops.consistency(a, p)
        emit("ops.consistency", "B%d L%d p%d cls" % (b, l, p), cls)
        emit("ops.consistency", "B%d L%d p%d aff" % (b, l, p), aff)
        grads("ops.consistency", "B%d L%d p%d" % (b, l, p), [cls + 2 * aff], [a], ["a"])


class _Owner:
    """stands in for the attention module: AttnCoreFn leaves (qkv, lse2, heads) on it"""
    training, keep_state_in_training = True, True


def attention():
    # T = 33: two blocks, the second with one key; 145 / 273: the smallest split tails of four- and eight-wave workgroups; 785: the bench's
    for gen, scores, math in (("recompute", False, 0), ("scores", True, 0), ("split", True, 1)):
        ops.ATTN_F32_SCORES = scores
        for (T, H) in ((33, 1), (145, 4), (273, 2), (785, 12)):
            for with_g in (True, False):
                qkv = rnd(1, T, 3 * H * 64, scale=1.5).requires_grad_(True)
                d_o, gpm = rnd(1, T, H * 64), rnd(1, T, T)
                stack, own = ops.MeanStack(1, 1, T, DEV), _Owner()
                o, pm = ops.attention_core(qkv, H, stack, 0, own, math)
                case = "%s T%d H%d g%d" % (gen, T, H, with_g)
                for n, t in (("o", o), ("lse2", own._saved[1]), ("pmean", pm)):
                    emit("ops.attention_core", case + " " + n, t)
                (dqkv,) = torch.autograd.grad([o, pm] if with_g else [o], [qkv], [d_o, gpm] if with_g else [d_o])
                emit("ops.attention_core", case + " dqkv", dqkv)
    ops.ATTN_F32_SCORES = True
    qkv = rnd(1, 785, 3 * 12 * 64, scale=1.5).requires_grad_(True)
    stack, own = ops.MeanStack(1, 1, 785, DEV), _Owner()
    o, pm, img = ops.attention_core_oimg(qkv, 12, stack, 0, own, 1)
    for n, t in (("o", o), ("lse2", own._saved[1]), ("pmean", pm), ("o_image", img)):
        emit("ops.attention_core_oimg", "split T785 H12 " + n, t)
    (dqkv,) = torch.autograd.grad([o, pm], [qkv], [rnd(1, 785, 12 * 64), rnd(1, 785, 785)])
    emit("ops.attention_core_oimg", "split T785 H12 dqkv", dqkv)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "library_bits.py needs a GPU"
    assert os.path.samefile(L.LIB_PATH, sys.argv[1]), (L.LIB_PATH, sys.argv[1])
    for part in (segpred, seglosses, resize, decoders, loaders, step_kernels, attention):
        part()
    torch.cuda.synchronize()
