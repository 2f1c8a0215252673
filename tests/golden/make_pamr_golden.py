#!/usr/bin/env python
"""Generate tests/golden/pamr_{a,b,c,d}.npz by running the *reference's own* ``PAMR`` module (pamr.py) on the CPU.

Run where the reference tree exists (``ACR_REFERENCE``, default /root/reference); the module is imported from where it lies,
nothing of it is restated here.  Each file holds the seeded inputs (x, mask), the parameters (num_iter, dilations), the
module's float32 output ``ref32`` and the output of the same module under ``.double()`` on the same values, ``ref64``.
``E_ref = max|ref32 - ref64|`` -- the reference's own fp32 error -- is what the kernel tests scale their bound by; it is printed.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("ACR_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
from pamr import PAMR  # noqa: E402

SIX = (1, 2, 4, 8, 12, 24)


def smooth_image(g, B, K, H, W):
    """a smooth random field on the 0..255 grey scale: coarse noise, bicubic up"""
    coarse = torch.rand(B, K, max(H // 8, 2), max(W // 8, 2), generator=g)
    img = F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True)
    img = (img - img.amin()) / (img.amax() - img.amin())
    return (255 * img).float().contiguous()


def case_a(g):
    x = smooth_image(g, 1, 3, 48, 64)
    x[:, :, 6:22, 8:30] = torch.tensor([37.0, 120.0, 201.0]).view(1, 3, 1, 1)                      # exactly flat
    noise = torch.randint(-1, 2, (1, 3, 16, 24), generator=g).float()                               # +-1 grey level
    x[:, :, 28:44, 34:58] = torch.tensor([90.0, 64.0, 143.0]).view(1, 3, 1, 1) + noise
    return x, torch.rand(1, 4, 48, 64, generator=g), 10, SIX


def case_b(g):
    return smooth_image(g, 2, 3, 40, 52), torch.rand(2, 3, 10, 13, generator=g), 10, SIX


def case_c(g):
    return smooth_image(g, 1, 3, 20, 30), torch.rand(1, 5, 20, 30, generator=g), 10, SIX


def case_d(g):
    return smooth_image(g, 1, 3, 32, 40), torch.rand(1, 1, 32, 40, generator=g), 1, (1,)


def main():
    for i, (tag, fn) in enumerate((("a", case_a), ("b", case_b), ("c", case_c), ("d", case_d))):
        g = torch.Generator().manual_seed(1000 + i)
        x, mask, num_iter, dilations = fn(g)
        with torch.no_grad():
            ref32 = PAMR(num_iter, list(dilations))(x, mask)
            ref64 = PAMR(num_iter, list(dilations)).double()(x.double(), mask.double())
        assert ref32.dtype == torch.float32 and ref64.dtype == torch.float64
        path = os.path.join(HERE, "pamr_%s.npz" % tag)
        np.savez_compressed(path, x=x.numpy(), mask=mask.numpy(), num_iter=np.int32(num_iter),
                            dilations=np.asarray(dilations, np.int32), ref32=ref32.numpy(), ref64=ref64.numpy())
        print("pamr_%s: x %s mask %s iter %d dilations %s  E_ref = max|ref32 - ref64| = %.3e  (%d bytes)"
              % (tag, tuple(x.shape), tuple(mask.shape), num_iter, dilations, float((ref32.double() - ref64).abs().max()),
                 os.path.getsize(path)))


if __name__ == "__main__":
    main()
