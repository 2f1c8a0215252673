"""The affinity stage restated in plain torch, dtype-generic (float32 for the reference's own error, float64 for the truth):
the pair geometry and the pair labels of the reference (tool/pyutils.py:125-159, tool/torchutils.py:107-157; pinned to fixtures
written by those functions in tests/test_affinity_cpu.py), and this project's statement of the PSA affinity, its loss and the random
walk (include/acr_hip.h, "affinity stage").  Everything gathers through the index lists: no shortcut shared with the kernels."""
import torch

EPS = 1e-5


def search_dist(radius):
    out = [(0, x) for x in range(1, radius)]
    for y in range(1, radius):
        for x in range(-radius + 1, radius):
            if x * x + y * y < radius * radius:
                out.append((y, x))
    return out


def pair_indices(radius, h, w):
    """(from (N,), to (P, N)) int64 flat pixel indices: from-pixels are rows [0, h - r), columns [r, w - r); to = from + dy w + dx"""
    r = radius - 1
    if h <= r or w <= 2 * r:
        raise ValueError("no pair on a %d x %d grid at radius %d" % (h, w, radius))
    full = torch.arange(h * w, dtype=torch.int64).view(h, w)
    frm = full[:h - r, r:w - r].reshape(-1)
    to = torch.stack([frm + dy * w + dx for dy, dx in search_dist(radius)])
    return frm, to


def subsample(label_map, stride):
    """THE rule for the reference's RescaleNearest(0.125): g[y, x] = map[stride y, stride x]"""
    if label_map.shape[-2] % stride or label_map.shape[-1] % stride:
        raise ValueError("map is no multiple of the stride")
    return label_map[..., ::stride, ::stride]


def pair_masks(grid, radius):
    """grid (h, w) integer labels -> (bg_pos, fg_pos, neg) bool (P, N), the three masks of ExtractAffinityLabelInRadius"""
    h, w = grid.shape
    frm, to = pair_indices(radius, h, w)
    flat = grid.reshape(-1).to(torch.int64)
    lf, lt = flat[frm][None], flat[to]
    valid = (lf < 255) & (lt < 255)
    pos = lf == lt
    return pos & (lf == 0), pos & (lf != 0) & valid, ~pos & valid


def pair_codes(label_map, radius=5, stride=8):
    """(B, S, S') -> (codes (B, P, N) uint8, counts int64[3])"""
    codes = []
    for m in subsample(label_map, stride):
        bg, fg, neg = pair_masks(m, radius)
        codes.append((bg.to(torch.uint8) + 2 * fg.to(torch.uint8) + 3 * neg.to(torch.uint8)))
    codes = torch.stack(codes)
    return codes, torch.stack([(codes == k).sum() for k in (1, 2, 3)]).to(torch.int64)


def pair_dist(feat, radius=5):
    """feat (B, C, h, w) -> d (B, P, N) = mean_c |feat[from] - feat[to]|"""
    B, C, h, w = feat.shape
    frm, to = pair_indices(radius, h, w)
    flat = feat.reshape(B, C, h * w)
    return (flat[:, :, frm].unsqueeze(2) - flat[:, :, to]).abs().mean(1)


def pair_affinity(feat, radius=5):
    return torch.exp(-pair_dist(feat, radius))


def aff_loss(feat, codes, counts, radius=5):
    """-> (loss, bg, fg, neg, aff); counts over the whole batch"""
    aff = pair_affinity(feat, radius)
    cnt = counts.to(aff.dtype)
    zero = torch.zeros((), dtype=aff.dtype)
    bg = torch.where(codes == 1, -torch.log(aff + EPS), zero).sum() / (cnt[0] + EPS)
    fg = torch.where(codes == 2, -torch.log(aff + EPS), zero).sum() / (cnt[1] + EPS)
    neg = torch.where(codes == 3, -torch.log(1 + EPS - aff), zero).sum() / (cnt[2] + EPS)
    return bg / 4 + fg / 4 + neg / 2, bg, fg, neg, aff


def transition(aff, h, w, radius=5, beta=8):
    """aff (P, N) of one image -> dense T (h w, h w): A symmetric with aff^beta on the listed pairs and 1 on the diagonal,
    T[i, j] = A[i, j] / sum_k A[k, j]"""
    frm, to = pair_indices(radius, h, w)
    A = torch.eye(h * w, dtype=aff.dtype, device=aff.device)
    f = frm[None].expand_as(to).reshape(-1).to(aff.device)
    t = to.reshape(-1).to(aff.device)
    a = aff.reshape(-1) ** beta
    A[f, t] = a
    A[t, f] = a
    return A / A.sum(0, keepdim=True)


def walk_dense(aff, scores, radius=5, beta=8, logt=8, steps=None):
    """scores (K, h, w) of one image -> scores . T^(2^logt) by squaring (or T^steps with logt=None)"""
    K, h, w = scores.shape
    T = transition(aff, h, w, radius, beta)
    if logt is None:
        T = torch.linalg.matrix_power(T, steps)
    else:
        for _ in range(logt):
            T = T @ T
    return (scores.reshape(K, h * w) @ T).view(K, h, w)


def walk_steps(aff, scores, radius=5, beta=8, steps=256):
    """The same product as `steps` sparse gathers new[j] = (sum_{i in nbr(j) + {j}} A[i, j] old[i]) / colsum[j]: per pixel the
    2 P + 1 taps (itself, +offset, -offset), absent pairs with weight 0"""
    K, h, w = scores.shape
    hw = h * w
    frm, to = pair_indices(radius, h, w)
    frm, to = frm.to(aff.device), to.to(aff.device)
    P = to.shape[0]
    a = aff ** beta
    idx = torch.arange(hw, device=aff.device).repeat(2 * P + 1, 1)
    wt = torch.zeros(2 * P + 1, hw, dtype=aff.dtype, device=aff.device)
    wt[0] = 1
    for p in range(P):
        idx[1 + 2 * p, frm], wt[1 + 2 * p, frm] = to[p], a[p]         # the pair j starts: neighbour `to`
        idx[2 + 2 * p, to[p]], wt[2 + 2 * p, to[p]] = frm, a[p]       # the pair that ends in j: neighbour `from`
    colsum = wt.sum(0)
    cur = scores.reshape(K, hw)
    for _ in range(steps):
        cur = (cur[:, idx] * wt).sum(1) / colsum
    return cur.view(K, h, w)
