"""CPU restatement of pixel-adaptive mask refinement (the reference's pamr.py:115-144) in gather form: the neighbours of every
pixel are shifted views of the replicate-padded tensor, stacked.  Plain torch, any float dtype -- the checker of
acr_wsss_amd.pamr, itself pinned to the reference module's outputs by tests/golden/pamr_*.npz (tests/test_pamr_cpu.py)."""
import torch
import torch.nn.functional as F

_OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def neighbours(t, dilations, centre):
    """(B, C, H, W) -> (B, C, P, H, W): per dilation d the samples at (y + dy * d, x + dx * d), (dy, dx) row-major, clamped
    to the image; with the centre 9 per dilation, without it 8."""
    H, W = t.shape[-2:]
    views = []
    for d in dilations:
        p = F.pad(t, [d] * 4, mode="replicate")
        for dy, dx in _OFFSETS:
            if (dy, dx) != (0, 0) or centre:
                views.append(p[:, :, d + dy * d: d + dy * d + H, d + dx * d: d + dx * d + W])
    return torch.stack(views, 2)


def pamr_weights(x, dilations):
    """(B, K, H, W) image -> (B, 1, P, H, W) softmax weights of the P = 8 * len(dilations) neighbours."""
    std = neighbours(x, dilations, True).std(2, keepdim=True)
    diff = (x.unsqueeze(2) - neighbours(x, dilations, False)).abs()
    a = -diff / (1e-8 + 0.1 * std)
    return F.softmax(a.mean(1, keepdim=True), 2)


def pamr_ref(x, mask, num_iter=1, dilations=(1,)):
    mask = F.interpolate(mask, size=x.shape[-2:], mode="bilinear", align_corners=True)
    w = pamr_weights(x, dilations)
    for _ in range(num_iter):
        mask = (neighbours(mask, dilations, False) * w).sum(2)
    return mask
