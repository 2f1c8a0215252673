#!/usr/bin/env python3
"""Generate tests/golden/segloss_{a,b,c}.npz: what torch's CPU kernels and the *reference's own* ``SegmentationLosses`` give for
the split cross-entropy of ``compute_joint_loss`` (myTool.py:825-857).

Run where the reference tree exists (``ACR_REFERENCE``, default /root/reference):   python tests/golden/make_segloss_golden.py
``tool/loss.py`` (it imports only torch) is imported UNMODIFIED from where it lies; nothing of it is restated here.  Per case the
seeded logits (B, K, h, w) are upsampled with ``F.interpolate(..., mode="bilinear", align_corners=False)`` (:831), the label is
edited into its background-only and foreground-only copies as :845-848 do, and both meet
  * ``nn.CrossEntropyLoss(ignore_index=255)`` -- the ``critersion`` of :851-853 -- recorded as ``*_ba0``, and
  * ``SegmentationLosses(batch_average=True).CrossEntropyLoss`` (tool/loss.py:21-33) -- recorded as ``*_ba1``;
  ``SegmentationLosses(batch_average=False)`` is asserted to give the first one's bits.
``celoss.backward()`` gives ``d_logits_ba{0,1}``.  Everything is fp32 on the CPU.  The files hold data only."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("ACR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import segloss_ref as R  # noqa: E402  (the seeded labels only; the expectations come from torch and the reference)

CASES = {
    # tag: (B, K, h, w, W, H, seed)
    "a": (2, 21, 5, 7, 37, 41, 21),
    "b": (1, 2, 1, 1, 3, 2, 22),
    "c": (3, 21, 9, 4, 70, 33, 23),
}


def torch_split_ce(logits, label, criterion):
    """(celoss, bg, fg, d_logits) of :831,845-855 with ``criterion(pred, target)``; fp32 CPU tensors in, numpy out"""
    x = torch.from_numpy(logits).clone().requires_grad_(True)
    seg_label = torch.from_numpy(label.astype(np.int64))
    pred = F.interpolate(x, tuple(label.shape[1:]), mode="bilinear", align_corners=False)
    bg_label, fg_label = seg_label.clone(), seg_label.clone()
    bg_label[seg_label != 0] = 255
    fg_label[seg_label == 0] = 255
    # a label in K..254 is ignored like 255 (the product's rule; torch would raise on it)
    bg_label[(seg_label >= logits.shape[1]) & (seg_label != 255)] = 255
    fg_label[(seg_label >= logits.shape[1]) & (seg_label != 255)] = 255
    bg, fg = criterion(pred, bg_label), criterion(pred, fg_label)
    ce = bg + fg
    ce.backward()
    return tuple(t.detach().numpy().astype(np.float32) for t in (ce, bg, fg)) + (x.grad.numpy().copy(),)


def main():
    sys.path.insert(0, REF)
    from tool.loss import SegmentationLosses                       # the reference, unmodified
    plain = torch.nn.CrossEntropyLoss(ignore_index=255)
    for tag, (B, K, h, w, W, H, seed) in CASES.items():
        rng = np.random.default_rng(seed)
        logits = (2.0 * rng.standard_normal((B, K, h, w))).astype(np.float32)
        label = R.labels_case(rng, B, K, W, H)
        if tag == "b":
            label = np.array([[[0, 1], [255, 1], [0, 0]]], np.uint8)
        out = dict(logits=logits, label=label)
        for ba in (0, 1):
            crit = SegmentationLosses(batch_average=bool(ba), ignore_index=255).build_loss("ce")
            got = torch_split_ce(logits, label, crit)
            if not ba:
                want = torch_split_ce(logits, label, plain)
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), tag
            for name, v in zip(("celoss", "bg", "fg", "d_logits"), got):
                out["%s_ba%d" % (name, ba)] = v
        lab = label.astype(np.int64)
        out["counts"] = np.array([(lab == 0).sum(), ((lab >= 1) & (lab < K)).sum()], np.int64)
        path = os.path.join(HERE, "segloss_%s.npz" % tag)
        np.savez_compressed(path, **out)
        print("segloss_%s: %s -> %s  celoss %.6f / %.6f  n_bg %d n_fg %d  ignored %d (K..254: %d)  (%d bytes)"
              % (tag, logits.shape, label.shape[1:], out["celoss_ba0"], out["celoss_ba1"], out["counts"][0], out["counts"][1],
                 (lab >= K).sum(), ((lab >= K) & (lab < 255)).sum(), os.path.getsize(path)))


if __name__ == "__main__":
    main()
