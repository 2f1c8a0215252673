"""float64 numpy restatement of the pseudo-label segmentation loss (include/acr_hip.h "pseudo-label segmentation loss"): the
bilinear rule, the split cross-entropy with its gradient, and the dense energy with its DEFINED gradient.  Independent of the
package; tests/test_segloss_cpu.py pins it to torch's own CPU results recorded in tests/golden/segloss_{a..c}.npz.

The bilinear rule is torch's ``align_corners=False`` one as torch evaluates it for fp32 tensors: the scale in / out, the source
coordinate max(scale * (dst + 0.5) - 0.5, 0) and the two weights are fp32 numbers (they define which combination of texels a
pixel is); everything after them -- the interpolation, the softmax, the sums, the gradient -- is float64."""
import numpy as np

F32 = np.float32


def bilinear_matrix(n_in, n_out):
    """(n_out, n_in) float64: row d holds the two weights of destination d (torch's fp32 source index and lambdas)."""
    scale = F32(n_in) / F32(n_out)
    dst = np.arange(n_out, dtype=F32)
    src = np.maximum(scale * (dst + F32(0.5)) - F32(0.5), F32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    m = np.zeros((n_out, n_in), np.float64)
    np.add.at(m, (np.arange(n_out), i0), l0.astype(np.float64))
    np.add.at(m, (np.arange(n_out), i1), l1.astype(np.float64))
    return m


def nearest_index(n_in, n_out):
    """torch's 'nearest' source index: min(floor(dst * scale), n_in - 1), scale = in / out in fp32."""
    scale = F32(n_in) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F32) * scale).astype(np.int64), n_in - 1)


def upsample(x, W, H):
    """(B, K, h, w) -> (B, K, W, H) float64."""
    ry, rx = bilinear_matrix(x.shape[2], W), bilinear_matrix(x.shape[3], H)
    return np.einsum("Yy,bkyx,Xx->bkYX", ry, x.astype(np.float64), rx)


def upsample_transposed(d, h, w):
    """the adjoint of ``upsample``: (B, K, W, H) -> (B, K, h, w) float64."""
    ry, rx = bilinear_matrix(h, d.shape[2]), bilinear_matrix(w, d.shape[3])
    return np.einsum("Yy,bkYX,Xx->bkyx", ry, d.astype(np.float64), rx)


def split_ce(logits, label, batch_average=False, g=(1.0, 0.0, 0.0), d_probs=None):
    """logits (B, K, h, w), label (B, W, H) uint8 -> dict: celoss, bg, fg, sums (B, 2), counts (B + 1, 2) int64, probs
    (B, K, W, H), d_logits (B, K, h, w) under the output gradients ``g`` = (d celoss, d bg, d fg) and the gradient ``d_probs`` of
    the probabilities (None: none).  A term without a pixel is NaN; its pixels (there are none) add nothing to d_logits."""
    B, K, h, w = logits.shape
    _, W, H = label.shape
    pred = upsample(logits, W, H)
    z = pred - pred.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    lab = label.astype(np.int64)
    is_bg, is_fg = lab == 0, (lab >= 1) & (lab < K)
    nll = -np.take_along_axis(logp, np.where(lab < K, lab, 0)[:, None], axis=1)[:, 0]
    sums = np.stack([(nll * is_bg).sum(axis=(1, 2)), (nll * is_fg).sum(axis=(1, 2))], axis=1)
    counts = np.stack([is_bg.sum(axis=(1, 2)), is_fg.sum(axis=(1, 2))], axis=1).astype(np.int64)
    counts = np.concatenate([counts, counts.sum(axis=0, keepdims=True)])
    div = float(B) if batch_average else 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        bg = sums[:, 0].sum() / np.float64(counts[B, 0]) / div
        fg = sums[:, 1].sum() / np.float64(counts[B, 1]) / div
    coef = np.zeros(lab.shape, np.float64)
    if counts[B, 0]:
        coef[is_bg] = (g[0] + g[1]) / div / counts[B, 0]
    if counts[B, 1]:
        coef[is_fg] = (g[0] + g[2]) / div / counts[B, 1]
    onehot = (np.arange(K)[None, :, None, None] == lab[:, None]).astype(np.float64)
    dpred = coef[:, None] * (p - onehot)
    if d_probs is not None:
        dp = d_probs.astype(np.float64)
        dpred = dpred + p * (dp - (p * dp).sum(axis=1, keepdims=True))
    return dict(celoss=bg + fg, bg=bg, fg=fg, sums=sums, counts=counts, probs=p, d_logits=upsample_transposed(dpred, h, w))


def energy(S, AS, weight):
    """S, AS (B, K, W, H) -> (E, dE/dS as DEFINED): E = -(weight / B) sum S * AS, dE/dS = -(2 weight / B) AS; float64."""
    B = S.shape[0]
    return -(weight / B) * (S.astype(np.float64) * AS.astype(np.float64)).sum(), -(2.0 * weight / B) * AS.astype(np.float64)


def energy_inputs(img, probs, roi, scale_factor):
    """the ``scale_factor`` plumbing: img (B, 3, W, H), probs (B, K, W, H), roi (B, W, H) -> (img (B, W', H', 3) uint8, probs
    float64, roi) at (floor(W f), floor(H f)): nearest for image and roi, the bilinear rule above for the probabilities."""
    W, H = probs.shape[2:]
    if scale_factor != 1:
        w2, h2 = max(1, int(W * scale_factor)), max(1, int(H * scale_factor))
        iy, ix = nearest_index(W, w2), nearest_index(H, h2)
        img, roi, probs = img[:, :, iy][:, :, :, ix], roi[:, iy][:, :, ix], upsample(probs, w2, h2)
    return np.ascontiguousarray(img.astype(np.uint8).transpose(0, 2, 3, 1)), probs.astype(np.float64), np.ascontiguousarray(roi)


def labels_case(rng, B, K, W, H, kind="random"):
    """seeded (B, W, H) uint8 labels: 'random' ~30 % ignore (255 and a few values in K..254), 'bg' only background and ignore,
    'ignore' all 255"""
    if kind == "ignore":
        return np.full((B, W, H), 255, np.uint8)
    if kind == "bg":
        lab = np.zeros((B, W, H), np.uint8)
        lab[rng.random((B, W, H)) < 0.3] = 255
        return lab
    lab = rng.integers(0, K, (B, W, H)).astype(np.uint8)
    lab[rng.random((B, W, H)) < 0.3] = 0                                   # background is a common label
    r = rng.random((B, W, H))
    lab[r < 0.3] = 255
    if K < 254:
        lab[r < 0.03] = rng.integers(K, 255, int((r < 0.03).sum())).astype(np.uint8)
    return lab
