"""Float64 numpy restatement of BatchNorm2d with cross-rank statistics (nn.SyncBatchNorm) as csrc/decoder.hip splits it: the
moments of a rank's tensor, the merge of the gathered moments by the pairwise update in ascending rank order, the forward under the
merged statistics, and the backward with the ranks' gradient sums added.  tests/test_syncbn_cpu.py pins it to
``decoder_ref.bn_fwd`` / ``bn_bwd`` on the concatenated batch: the split formulation is the full batch's.  The kernels themselves
are held against ``decoder_ref`` on the full batch (tests/test_syncbn_gpu.py), not against this file."""
import numpy as np

F64 = np.float64


def _b(v):
    return v[None, :, None, None]


def moments(x):
    """(C, 3): count, mean, M2 = sum (x - mean)^2 of one rank's (N, C, H, W) tensor.  One value per channel gives M2 = 0."""
    x = np.asarray(x, F64)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.mean(axis=(0, 2, 3))
    m2 = ((x - _b(mean)) ** 2).sum(axis=(0, 2, 3))
    return np.stack([np.full_like(mean, n), mean, m2], axis=1)


def merge(rows):
    """rows (W, C, 3) -> (n, mean, M2), each (C,): rank 0's moments take in rank 1's, then rank 2's, ... by
    n = n_a + n_b, delta = mean_b - mean_a, mean = mean_a + delta n_b / n, M2 = M2_a + M2_b + delta^2 n_a n_b / n"""
    rows = np.asarray(rows, F64)
    n, mean, m2 = rows[0, :, 0].copy(), rows[0, :, 1].copy(), rows[0, :, 2].copy()
    for r in range(1, rows.shape[0]):
        nb, mb, m2b = rows[r, :, 0], rows[r, :, 1], rows[r, :, 2]
        na, delta = n, mb - mean
        n = na + nb
        mean = mean + delta * nb / n
        m2 = m2 + m2b + delta * delta * na * nb / n
    return n, mean, m2


def fwd(shards, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu=False, resids=None, resids2=None):
    """``shards``: the ranks' tensors in rank order (N may differ, C, H, W agree).  dict: y / pre (lists, one per rank), n, mean,
    invstd (merged), running_mean / running_var after the call -- the same on every rank."""
    gamma, beta = np.asarray(gamma, F64), np.asarray(beta, F64)
    n, mean, m2 = merge(np.stack([moments(x) for x in shards]))
    if (n < 2).any():
        raise ValueError("Expected more than 1 value per channel when training")
    invstd = 1.0 / np.sqrt(m2 / n + eps)
    rm = None if running_mean is None else (1 - momentum) * np.asarray(running_mean, F64) + momentum * mean
    rv = None if running_var is None else (1 - momentum) * np.asarray(running_var, F64) + momentum * m2 / (n - 1)
    pres = []
    for r, x in enumerate(shards):
        pre = (np.asarray(x, F64) - _b(mean)) * _b(invstd * gamma) + _b(beta)
        for rs in (resids, resids2):
            if rs is not None:
                pre = pre + np.asarray(rs[r], F64)
        pres.append(pre)
    return dict(y=[np.maximum(p, 0) if relu else p for p in pres], pre=pres, n=n, mean=mean, invstd=invstd, running_mean=rm,
                running_var=rv)


def sums(x, mean, invstd, dy, mask=None):
    """(C, 2): sum g, sum g * xhat of one rank under the merged statistics; ``mask`` the ReLU's pass mask (None: no ReLU)"""
    g = np.asarray(dy, F64) if mask is None else np.asarray(dy, F64) * mask
    xhat = (np.asarray(x, F64) - _b(mean)) * _b(invstd)
    return np.stack([g.sum(axis=(0, 2, 3)), (g * xhat).sum(axis=(0, 2, 3))], axis=1)


def bwd(shards, gamma, n, mean, invstd, dys, masks=None):
    """list per rank of (dx, dgamma, dbeta, dres): dx with the ranks' sums added in rank order and divided by the merged count,
    dgamma / dbeta the rank's LOCAL sums (their sum over the ranks is the full batch's gradient)"""
    gamma = np.asarray(gamma, F64)
    masks = masks if masks is not None else [None] * len(shards)
    rows = [sums(x, mean, invstd, dy, m) for x, dy, m in zip(shards, dys, masks)]
    total = rows[0].copy()
    for r in rows[1:]:
        total = total + r
    mg, mgx = total[:, 0] / n, total[:, 1] / n
    out = []
    for x, dy, m, row in zip(shards, dys, masks, rows):
        g = np.asarray(dy, F64) if m is None else np.asarray(dy, F64) * m
        xhat = (np.asarray(x, F64) - _b(mean)) * _b(invstd)
        out.append((_b(gamma * invstd) * (g - _b(mg) - xhat * _b(mgx)), row[:, 1], row[:, 0], g))
    return out
