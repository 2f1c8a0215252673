"""The affinity stage of PSA (Ahn & Kwak, CVPR 2018) on the GPU: the branch of the reference tree that reads what this project
already writes -- the ``<out_crf>_<alpha>/<name>.npy`` dumps (``VOC12AffDataset``, voc12/data.py:222-278) and the pseudo-label
PNGs (``AffinityFromMaskDataset``, tool/torchutils.py:159-173) -- into pair labels (``ExtractAffinityLabelInRadius``,
tool/torchutils.py:107-157, pair geometry ``get_indices_of_pairs``, tool/pyutils.py:125-159).  The reference ships the labels and
the indices and expects PSA's loss and random walk around them; their statement here is this project's own
(include/acr_hip.h, "affinity stage", has every rule in full).

  ``aff_label``      the two score stacks of an image -> the label grid of ``VOC12AffDataset`` (csrc/affdata.hip; the batched, cropped
                     and flipped form is ``data.AffTrainBatcher`` / ``ChunkLoader.get_data_from_chunk_aff``)
  ``pair_codes``     label map -> one code per pixel pair (1 bg-pos, 2 fg-pos, 3 neg, 0 none) and the batch counts
  ``pair_affinity``  feat (B, C, h, w) -> aff = exp(-mean_c |f_from - f_to|), (B, P, N); no grad
  ``aff_loss``       the three-term loss on aff, differentiable in feat
  ``random_walk``    scores . T^(2^logt) under T = column-normalised aff^beta, as 2^logt sparse gather steps
  ``AffinityHead``, ``aff_train_step``, ``aff_with_alpha_device``: the thin layers above

All arithmetic runs in csrc/affinity.hip behind the C ABI (``acr_aff_*``); there is no CPU path -- without the HIP library and a
GPU these raise.  Every result is bit-identical run to run."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _args as A
from . import _lib as L

MIN_RADIUS, MAX_RADIUS = 2, 5
_BCHW = ("B", "C", "h", "w")


def search_dist(radius):
    """The (dy, dx) offsets in the reference's order (tool/pyutils.py:127-135)"""
    out = [(0, x) for x in range(1, radius)]
    for y in range(1, radius):
        for x in range(-radius + 1, radius):
            if x * x + y * y < radius * radius:
                out.append((y, x))
    return out


def _geometry(h, w, radius):
    """(P, N) of an h x w grid; raises where the grid has no pair or the radius is not built"""
    radius = int(radius)
    if not MIN_RADIUS <= radius <= MAX_RADIUS:
        raise ValueError("radius %d outside %d..%d" % (radius, MIN_RADIUS, MAX_RADIUS))
    r = radius - 1
    if h <= r or w <= 2 * r:
        raise ValueError("a %d x %d grid has no pair at radius %d (needs h > %d and w > %d)" % (h, w, radius, r, 2 * r))
    return len(search_dist(radius)), (h - r) * (w - 2 * r)


def pair_codes(label_map, radius=5, stride=8):
    """label_map (B, S, S') uint8 on the device, class ids with 255 = ignore (what ``ChunkLoader.get_data_from_chunk_v4`` returns
    with ``map_fill=255``; a single (S, S') map is a batch of one) -> (codes (B, P, N) uint8, counts int64[3] on the device: the
    batch totals of codes 1, 2, 3).  The grid is the map subsampled by ``stride`` -- g[y, x] = map[stride y, stride x], the
    reference's ``RescaleNearest(0.125)`` -- in the same kernel; ``stride=1`` takes a grid-sized map."""
    lib = L.load()
    label_map = A.tensor_arg(label_map, "label_map", torch.uint8, contiguous=False, on_gpu=False)
    if label_map.dim() == 2:
        label_map = label_map.unsqueeze(0)
    if label_map.dim() != 3:
        raise ValueError("label_map %s must be (B, S, S')" % (tuple(label_map.shape),))
    L.require_gpu(label_map)
    stride = int(stride)
    B, S0, S1 = label_map.shape
    if stride < 1 or S0 % stride or S1 % stride:
        raise ValueError("label_map %d x %d is no multiple of stride %d" % (S0, S1, stride))
    P, N = _geometry(S0 // stride, S1 // stride, radius)
    label_map = label_map.contiguous()
    dev = label_map.device
    codes = torch.empty((B, P, N), dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.acr_aff_pair_codes(L.ptr(label_map), B, S0, S1, stride, int(radius), L.ptr(codes), L.ptr(counts), L.stream_ptr()),
                "acr_aff_pair_codes")
    return codes, counts


def aff_label(la, ha, *, box=None):
    """The label grid of ONE image out of its two CRF score stacks (``VOC12AffDataset.__getitem__``, voc12/data.py:251-275;
    include/acr_hip.h, "affinity-stage input"): ``la`` / ``ha`` the low- / high-alpha scores, each an (n, h, w) float32 device tensor
    (what ``crf.crf_with_alpha_device`` returns) or a {key: (h, w)} dict of device tensors or arrays (what the dumps hold; both dicts
    with the same keys in the same order; host planes go to the current GPU).  With ``box=None`` the image is taken whole: the result
    is the (ceil(h / 8), ceil(w / 8)) uint8 label of the image zero-padded to multiples of 8, as ``block_reduce`` pads.  ``box`` =
    (SH, SW, cont_top, cont_left, img_top, img_left, ch, cw, flip) is an ``acr_pre_image`` geometry in a SH x SW container (flip, then
    crop) -> (SH / 8, SW / 8).  A stride-1 grid for ``pair_codes``; plane indices, 0 and 255, not class ids."""
    from . import data as D

    def stack(s, who):
        if isinstance(s, dict):
            keys, planes = list(s.keys()), [v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v)) for v in s.values()]
            if len(planes) < D.AFF_MIN_PLANES:
                raise ValueError("%s: %d planes, need at least %d" % (who, len(planes), D.AFF_MIN_PLANES))
            if any(p.dim() != 2 or p.shape != planes[0].shape or p.device != planes[0].device for p in planes):
                raise ValueError("%s: every plane must be (h, w) like the first, on one device" % who)
            return keys, torch.stack(planes)
        if not torch.is_tensor(s) or s.dim() != 3:
            raise ValueError("%s must be an (n, h, w) tensor or a {key: (h, w)} dict" % who)
        return None, s
    (kl, la), (kh, ha) = stack(la, "la"), stack(ha, "ha")
    if (kl is not None and kh is not None and kl != kh) or la.shape != ha.shape:
        raise ValueError("la (keys %s, %s) and ha (keys %s, %s) differ" % (kl, tuple(la.shape), kh, tuple(ha.shape)))
    if la.dtype != torch.float32 or ha.dtype != torch.float32:
        raise ValueError("scores must be float32, got %s and %s" % (la.dtype, ha.dtype))
    n, h, w = la.shape
    if not D.AFF_MIN_PLANES <= n <= D.AFF_MAX_PLANES or h == 0 or w == 0:
        raise ValueError("%d planes of %d x %d outside %d..%d non-empty planes" % (n, h, w, D.AFF_MIN_PLANES, D.AFF_MAX_PLANES))
    if box is None:
        box = ((h + 7) // 8 * 8, (w + 7) // 8 * 8, 0, 0, 0, 0, h, w, 0)
    SH, SW, ct, cl, it, il, ch, cw, flip = (int(v) for v in box)
    rec = np.zeros(1, D.PRE_IMAGE)
    rec[0] = (0, h, w, h, w, flip, ct, cl, it, il, ch, cw)
    D._check_aff_records(rec, [(h, w)], SH, SW)
    if (kl is not None and not la.is_cuda) or (kh is not None and not ha.is_cuda):      # host planes of a dump: to the GPU
        dev = la.device if la.is_cuda else ha.device if ha.is_cuda else A.gpu_device("cuda", "aff_label")
        la, ha = (la.to(dev) if kl is not None else la), (ha.to(dev) if kh is not None else ha)
    L.require_gpu(la, ha)
    if la.device != ha.device:
        raise ValueError("la on %s and ha on %s do not belong together" % (la.device, ha.device))
    buf = torch.cat((la.reshape(-1), ha.reshape(-1)))
    label = D.aff_label_launch(buf, rec, [0], [4 * n * h * w], [n], SH, SW)
    out = label[0]
    out._acr_keep = label._acr_keep
    return out


def pair_affinity(feat, radius=5):
    """feat (B, C, h, w) float32 on the GPU -> aff (B, P, N) = exp(-(1 / C) sum_c |feat[from] - feat[to]|).  The inference
    forward: no grad (the result is detached whatever feat requires)."""
    lib = L.load()
    feat = A.tensor_arg(feat, "feat", torch.float32, shape=_BCHW, contiguous=False).detach().contiguous()
    B, C, h, w = feat.shape
    P, N = _geometry(h, w, radius)
    aff = torch.empty((B, P, N), dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device):
        L.check(lib.acr_aff_loss_fwd(L.ptr(feat), B, C, h, w, int(radius), None, None, L.ptr(aff), None, None, 0, None, L.stream_ptr()),
                "acr_aff_loss_fwd")
    return aff


class _AffLoss(torch.autograd.Function):
    """(loss4 = loss, bg, fg, neg; aff (B, P, N)) of acr_aff_loss_fwd; the gradient flows through loss4[0] alone"""

    @staticmethod
    def forward(ctx, feat, codes, counts, radius):
        lib = L.load()
        feat = feat.contiguous()
        B, C, h, w = feat.shape
        dev = feat.device
        with torch.cuda.device(dev):
            ws, nbytes = L.workspace("acr_aff_loss_ws_bytes", B, h, w, radius, device=dev, dtype=torch.float64)
            aff = torch.empty(codes.shape, dtype=torch.float32, device=dev)
            g = torch.empty(codes.shape, dtype=torch.float32, device=dev)
            loss4 = torch.empty(4, dtype=torch.float32, device=dev)
            L.check(lib.acr_aff_loss_fwd(L.ptr(feat), B, C, h, w, radius, L.ptr(codes), L.ptr(counts), L.ptr(aff), L.ptr(g), L.ptr(ws),
                                         nbytes, L.ptr(loss4), L.stream_ptr()), "acr_aff_loss_fwd")
        ctx.save_for_backward(feat, g)
        ctx.radius = radius
        terms = loss4[1:].clone()
        ctx.mark_non_differentiable(terms, aff)
        return loss4[0].clone(), terms, aff

    @staticmethod
    def backward(ctx, g_loss, _g_terms, _g_aff):
        lib = L.load()
        feat, g = ctx.saved_tensors
        B, C, h, w = feat.shape
        with torch.cuda.device(feat.device):
            scale = g_loss.to(torch.float32).reshape(1).contiguous()
            dfeat = torch.empty_like(feat)
            L.check(lib.acr_aff_loss_bwd(L.ptr(feat), L.ptr(g), L.ptr(scale), B, C, h, w, ctx.radius, L.ptr(dfeat), L.stream_ptr()),
                    "acr_aff_loss_bwd")
        return dfeat, None, None, None


def _aff_loss(feat, codes, counts, radius=None):
    feat = A.tensor_arg(feat, "feat", torch.float32, shape=_BCHW, contiguous=False)
    B, C, h, w = feat.shape
    codes = A.tensor_arg(codes, "codes", torch.uint8, shape=("B", "P", "N"), contiguous=False, on_gpu=False)
    counts = A.tensor_arg(counts, "counts", torch.int64, contiguous=False, on_gpu=False)
    if codes.device != feat.device:
        raise ValueError("codes must be the (B, P, N) uint8 tensor pair_codes returned, on the device of feat")
    if counts.numel() != 3 or counts.device != feat.device:
        raise ValueError("counts must be the int64[3] tensor pair_codes returned, on the device of feat")
    if radius is None:
        fits = [R for R in range(MIN_RADIUS, MAX_RADIUS + 1) if h > R - 1 and w > 2 * (R - 1) and tuple(codes.shape[1:]) == _geometry(h, w, R)]
        if len(fits) != 1:
            raise ValueError("codes %s belong to no radius on a %d x %d grid" % (tuple(codes.shape), h, w))
        radius = fits[0]
    if tuple(codes.shape) != (B,) + _geometry(h, w, radius):
        raise ValueError("codes %s do not fit feat %s at radius %d" % (tuple(codes.shape), tuple(feat.shape), radius))
    return _AffLoss.apply(feat, codes.contiguous(), counts.contiguous(), int(radius))


def aff_loss(feat, codes, counts, radius=None):
    """feat (B, C, h, w) float32 on the GPU, (codes, counts) from ``pair_codes`` -> (loss, bg, fg, neg) with
    ``loss = bg / 4 + fg / 4 + neg / 2``; bg / fg the mean of -log(aff + 1e-5) over the pairs of code 1 / 2, neg the mean of
    -log(1 + 1e-5 - aff) over those of code 3, each over the whole batch (a term without a pair is 0).  ``loss`` is differentiable
    in feat; bg, fg, neg are reported values and carry no gradient.  ``radius``: taken from the shape of ``codes`` when None."""
    loss, terms, _ = _aff_loss(feat, codes, counts, radius)
    return loss, terms[0], terms[1], terms[2]


def walk_weights(aff, hw, radius=5, beta=8):
    """aff (B, P, N) -> the normalised (B, 2 P + 1, h w) tap table of the transition matrix T (include/acr_hip.h)"""
    lib = L.load()
    h, w = hw
    aff = A.tensor_arg(aff, "aff", torch.float32, shape=("B", "P", "N"), contiguous=False).detach().contiguous()
    P, N = _geometry(h, w, radius)
    if tuple(aff.shape[1:]) != (P, N):
        raise ValueError("aff %s does not fit a %d x %d grid at radius %d" % (tuple(aff.shape), h, w, radius))
    wt = torch.empty((aff.shape[0], 2 * P + 1, h * w), dtype=torch.float32, device=aff.device)
    with torch.cuda.device(aff.device):
        L.check(lib.acr_aff_walk_weights(L.ptr(aff), aff.shape[0], h, w, int(radius), float(beta), L.ptr(wt), L.stream_ptr()),
                "acr_aff_walk_weights")
    return wt


def random_walk(aff, scores, beta=8, logt=8, resident=None, steps=None, radius=5):
    """scores (B, K, h, w) float32 on the GPU -> scores . T^(2^logt), T[i, j] = A[i, j] / sum_k A[k, j] with the symmetric
    A = aff^beta on the listed pairs, 1 on the diagonal, 0 elsewhere (aff (B, P, N) from ``pair_affinity``).  ``resident``: True:
    one launch, a workgroup per plane with the plane in LDS (two padded planes must fit); False: one launch per step with every
    plane spread over the chip; bit-identical.  None chooses, and chooses the stepwise form: the faster one at every plane count
    measured.  ``logt=None`` with ``steps=t`` runs t steps.  No grad."""
    lib = L.load()
    scores = A.tensor_arg(scores, "scores", torch.float32, shape=_BCHW, contiguous=False).detach().contiguous()
    B, K, h, w = scores.shape
    if (logt is None) == (steps is None):
        raise ValueError("give logt, or logt=None with steps")
    steps = int(steps) if logt is None else 1 << int(logt)
    if steps < 0:
        raise ValueError("steps=%d is negative" % steps)
    if aff.shape[0] != B or aff.device != scores.device:
        raise ValueError("aff %s on %s and scores %s on %s do not belong together" % (tuple(aff.shape), aff.device, tuple(scores.shape),
                                                                                      scores.device))
    wt = walk_weights(aff, (h, w), radius, beta)
    mode = -1 if resident is None else (1 if resident else 0)
    dev = scores.device
    out = torch.empty_like(scores)
    with torch.cuda.device(dev):
        ws, nbytes = None, 0
        if steps > 0 and mode != 1:
            ws, nbytes = L.workspace("acr_aff_walk_ws_bytes", B, K, h, w, int(radius), device=dev, dtype=torch.float32)
        L.check(lib.acr_aff_walk(L.ptr(wt), L.ptr(scores), L.ptr(out), B, K, h, w, int(radius), steps, mode, L.ptr(ws), nbytes,
                                 L.stream_ptr()), "acr_aff_walk")
    return out


class AffinityHead(nn.Module):
    """The affinity branch on the decoder's ``layers_rn`` maps: 1x1 convolutions of l2, l3, l4 (h / 8, h / 16, h / 32) to ``dims``,
    l3 upsampled x2 once and l4 twice, concatenated at stride 8, ELU, a 1x1 convolution to ``out_dim``, ELU ->
    (B, out_dim, h / 8, w / 8), the ``feat`` of ``aff_loss`` / ``pair_affinity``."""
    acr_math = 0

    def __init__(self, features=256, dims=(64, 128, 256), out_dim=448):
        super().__init__()
        self.f8_2 = nn.Conv2d(features, dims[0], 1, bias=False)
        self.f8_3 = nn.Conv2d(features, dims[1], 1, bias=False)
        self.f8_4 = nn.Conv2d(features, dims[2], 1, bias=False)
        self.f9 = nn.Conv2d(sum(dims), out_dim, 1, bias=False)
        for m in (self.f8_2, self.f8_3, self.f8_4, self.f9):
            nn.init.xavier_uniform_(m.weight, gain=4)

    def forward(self, layers):
        from .decoder import conv, upsample2x
        _, l2, l3, l4 = layers
        f2 = conv(self.f8_2, l2, self.acr_math)
        f3 = upsample2x(conv(self.f8_3, l3, self.acr_math))
        f4 = upsample2x(upsample2x(conv(self.f8_4, l4, self.acr_math)))
        x = F.elu(torch.cat((f2, f3, f4), dim=1))
        return F.elu(conv(self.f9, x, self.acr_math))


def aff_train_step(model, head, optimizer, images, label_map, radius=5):
    """``optimizer.zero_grad`` -> ``decoder.layers_rn(model, images)`` -> ``head`` -> ``pair_codes(label_map, radius, stride)`` ->
    ``aff_loss`` -> backward -> ``optimizer.step`` -> the cached weight images of model and head renewed, as in
    ``segtrain.seg_train_step``.  images (B, 3, S, S') float32 on the GPU (multiples of 32), label_map (B, S, S') uint8 at image
    size (stride 8) or at the head's grid (stride 1).  The label of ``ChunkLoader.get_data_from_chunk_aff`` is a stride-1 grid.
    Returns (loss, bg, fg, neg)."""
    from . import decoder
    from .train import refresh_weight_transposes
    optimizer.zero_grad(set_to_none=True)
    feat = head(decoder.layers_rn(model, images))
    if label_map.dim() == 2:
        label_map = label_map.unsqueeze(0)
    if label_map.shape[1] % feat.shape[2] or label_map.shape[1] // feat.shape[2] * feat.shape[3] != label_map.shape[2]:
        raise ValueError("label_map %s is no whole multiple of the %d x %d grid" % (tuple(label_map.shape), feat.shape[2], feat.shape[3]))
    codes, counts = pair_codes(label_map, radius, label_map.shape[1] // feat.shape[2])
    loss, bg, fg, neg = aff_loss(feat, codes, counts, radius)
    loss.backward()
    optimizer.step()
    refresh_weight_transposes(model, head)
    return loss, bg, fg, neg


def score_stack(cam_dict, alphas):
    """({class: cam (h, w)}, alphas) -> (classes, (len(alphas) * n, h, w) float32 numpy): per alpha the background
    (1 - max_c cam)^alpha and the classes, ``pamr_with_alpha_device``'s layout"""
    classes = list(cam_dict.keys())
    cams = np.stack([cam_dict[c] for c in classes], axis=0).astype(np.float32, copy=False)
    top = 1 - cams.max(axis=0, keepdims=True)
    return classes, np.concatenate([np.concatenate((np.power(top, a), cams), axis=0) for a in alphas], axis=0).astype(np.float32, copy=False)


def aff_inputs(scores, orig_img, device):
    """What ``aff_with_alpha_device`` hands to model and walk: (x (1, 3, H, W) the image normalised with ``data.MEAN`` / ``STD`` and
    zero-padded bottom / right to multiples of 32, s (1, n, H / 8, W / 8) the score stack padded alike and average-pooled 8 x 8)"""
    from .data import MEAN, STD
    img = torch.as_tensor(np.ascontiguousarray(orig_img))
    if img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8 or tuple(img.shape[:2]) != tuple(scores.shape[1:]):
        raise ValueError("orig_img must be (h, w, 3) uint8 matching the cams %s, got %s %s" % (tuple(scores.shape[1:]), tuple(img.shape), img.dtype))
    h, w = img.shape[:2]
    H, W = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    x = img.to(device).permute(2, 0, 1).to(torch.float32) / 255.0
    mean = torch.tensor(MEAN, dtype=torch.float32, device=device).view(3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32, device=device).view(3, 1, 1)
    x = F.pad((x - mean) / std, (0, W - w, 0, H - h))[None].contiguous()
    s = F.pad(torch.as_tensor(scores).to(device), (0, W - w, 0, H - h))[None]
    return x, F.avg_pool2d(s, 8).contiguous()


def aff_with_alpha_device(model, head, cam_dict, alphas, orig_img, beta=8, logt=8, radius=5, device="cuda"):
    """The twin of ``pamr.pamr_with_alpha_device`` with the learned affinity as the refinement: {class: cam (h, w)} -> (classes in
    the dict's order, (len(alphas) * n, h, w) float32 device tensor, n = 1 + len(classes): planes [ai * n, (ai + 1) * n) the
    background and the classes at alphas[ai]) -- what ``pseudo.seg_label`` / ``pseudo.label_map`` take.  The image is normalised
    and zero-padded to a multiple of 32, the score stack of ALL alphas padded alike and average-pooled 8 x 8; one
    ``pair_affinity`` on ``head(layers_rn(model, image))``, one ``random_walk`` with every plane, ``acr_bilinear_resize`` x 8
    (align_corners=False) and the crop back to (h, w).  No grad; ``model`` and ``head`` are used as they are (call ``eval()``)."""
    lib = L.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.AcrHipError("aff_with_alpha needs a GPU (no CPU path in the product)")
    from . import decoder
    alphas = list(alphas)
    classes, scores = score_stack(cam_dict, alphas)
    h, w = scores.shape[1:]
    with torch.cuda.device(dev), torch.no_grad():
        x, s = aff_inputs(scores, orig_img, dev)
        aff = pair_affinity(head(decoder.layers_rn(model, x)), radius)
        walked = random_walk(aff, s, beta, logt, radius=radius)
        n, gh, gw = walked.shape[1:]
        full = torch.empty((n, 8 * gh, 8 * gw), dtype=torch.float32, device=dev)
        L.check(lib.acr_bilinear_resize(L.ptr(walked), gh * gw, 1, n, gh, gw, L.ptr(full), 8 * gh, 8 * gw, 0, None, 0, 0, L.stream_ptr()),
                "acr_bilinear_resize")
        return classes, full[:, :h, :w].contiguous()
