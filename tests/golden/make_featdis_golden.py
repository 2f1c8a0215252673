#!/usr/bin/env python3
"""Generate tests/golden/featdis_{a..f}.npz by running the *reference's own* ``compute_dis_no_batch`` (myTool.py:1624-1710) in
float32 on the CPU, with autograd's gradient in the features.

Run where the reference tree exists (``ACR_REFERENCE``, default /root/reference):   python tests/golden/make_featdis_golden.py
``myTool`` is imported UNMODIFIED from where it lies, under the throw-away stubs make_data_golden.py installs; nothing of it is
restated here.  Two throw-away torch shims stand around the calls:
  * ``torch.Tensor.cuda`` returns the tensor itself: the function calls ``.cuda()`` unconditionally;
  * ``torch.Tensor.clone`` passes ``memory_format=torch.contiguous_format``, which is what ``clone`` did when the reference was
    written: ``permute(...).clone()`` preserves strides now, and ``.view(-1, C)`` at :1636 then raises for B > 1.
The inputs come from tests/featdis_ref.fixture_case (seeded; no pixel's feature vector is all zero).  Each file holds data only:
seg, feat, loss, d_feat, labels (B, h, w) uint8, counts (B + 20) int64 -- the labels and counts are ``argmax`` and its histogram,
which the reference forms inside and does not return."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("ACR_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_data_golden import install_stubs  # noqa: E402
import featdis_ref as R  # noqa: E402  (the seeded inputs; the expectations come from the reference)


def main():
    install_stubs()
    sys.path.insert(0, REF)
    import myTool                                                  # the reference, unmodified
    clone = torch.Tensor.clone
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.Tensor.clone = lambda self, *a, **k: clone(self, memory_format=torch.contiguous_format)
    for tag, (B, K, C, h, w) in R.CASES.items():
        seg, feat = R.fixture_case(tag)
        f = torch.from_numpy(feat).requires_grad_(True)
        loss = myTool.compute_dis_no_batch(torch.from_numpy(seg), f)
        loss.sum().backward()
        lab = torch.from_numpy(seg).argmax(1)
        counts = np.concatenate([(lab == 0).reshape(B, -1).sum(1).numpy(), np.bincount(lab.reshape(-1).numpy(), minlength=K)[1:]])
        path = os.path.join(HERE, "featdis_%s.npz" % tag)
        np.savez_compressed(path, seg=seg, feat=feat, loss=np.float32(loss.detach().reshape(-1)[0].item()), d_feat=f.grad.numpy(),
                            labels=lab.numpy().astype(np.uint8), counts=counts.astype(np.int64))
        print("featdis_%s: %s loss %.7f  |d_feat| max %.3e  labels %s  (%d bytes)"
              % (tag, (B, K, C, h, w), float(loss.detach().sum()), float(f.grad.abs().max()), sorted(set(lab.reshape(-1).tolist())), os.path.getsize(path)))


if __name__ == "__main__":
    main()
