"""One training step of the segmentation head on the pseudo-labels, on the HIP path.

The reference tree has the loss (``compute_joint_loss``, myTool.py:825-857), the loaders that feed it
(``get_data_from_chunk_v4`` / ``_v3``, :1257-1310 / :1202-1253) and ``forward_seg`` (:1869), but no script that calls them
together: the composition below is this project's.  It ties ``segval.forward_seg`` (decoder + ``SegmentationHead``),
``segloss.joint_loss`` and the optimizer together in the order ``train.train_step`` uses for the classification step, and takes the
tensors ``data.ChunkLoader.get_data_from_chunk_v4`` returns as they are -- nothing leaves the device.  With ``_v3``, which brings a
saliency map instead of a label, ``saliency_labels`` makes the label on the way (``compute_seg_label_3``, :188-264, the call the
reference's ``_v3`` loader is written for), and ``crf_labels`` from the CAMs through the dense CRF (``compute_seg_label`` /
``compute_seg_label_2``, :57-185)."""
import numpy as np
import torch

from . import featdis, ops, pseudo, segloss, segval
from .train import refresh_weight_transposes


def seg_train_step(model, head, optimizer, images, ori_images, croppings, seg_label, dense_energy_layer, *, batch_average=False,
                   grad_sync=None, dis_weight=0.0):
    """``optimizer.zero_grad`` -> ``forward_seg(model, head, images)`` -> ``joint_loss`` -> ``loss = celoss + dloss`` -> backward ->
    ``optimizer.step``.  images (B,3,S,S) float32 on the GPU (S a multiple of 32; or bfloat16 with a bf16 model and head under
    ``train.MasterWeights(nn.ModuleList([model, head]), ...)``, whose BatchNorm buffers stay fp32), ori_images (B,3,S,S) values
    0..255, croppings (S,S,B), seg_label (B,S,S) uint8 (255 = ignore) -- the loader's tuple; ``optimizer`` holds the parameters of ``model`` and
    ``head`` that are to train.  ``dense_energy_layer``: a ``segloss.DenseEnergyLoss``, or None for the cross-entropy alone (dloss
    is then 0).  ``batch_average`` is ``joint_loss``'s ``criterion_batch_average``.  ``grad_sync`` (``dp.GradSync``) all-reduces the
    gradients while backward runs, as in ``train.train_step``.  After the update the cached split-product weight images and weight
    transposes of model and head are renewed: the fused optimizer writes the weights in place.  ``dis_weight`` > 0 adds
    ``dis_weight * featdis.feature_distance_loss(logits_half, feat)`` on the head's own tensors (``head.forward_features``: the
    features its classifier reads and the logits before the x2 upsampling); at 0 the step makes the calls it made without the
    argument.  Returns (loss, terms) with terms = dict(celoss, dloss, loss), and disloss when ``dis_weight`` > 0."""
    optimizer.zero_grad(set_to_none=True)
    if dis_weight > 0:
        from . import decoder
        logits, feat, logits_half = head.forward_features(decoder.decode(model, images))
    else:
        logits = segval.forward_seg(model, head, images)
    if dense_energy_layer is None:
        celoss = segloss.split_cross_entropy(logits, seg_label, batch_average)[0]
        dloss = torch.zeros((), dtype=celoss.dtype, device=celoss.device)
    else:
        celoss, dloss = segloss.joint_loss(ori_images, logits, seg_label, croppings, batch_average, dense_energy_layer)
    loss = celoss + dloss
    terms = dict(celoss=celoss, dloss=dloss)
    if dis_weight > 0:
        terms["disloss"] = featdis.feature_distance_loss(logits_half, feat)
        loss = loss + dis_weight * terms["disloss"]
    if grad_sync is not None:
        grad_sync.prepare()
    loss.backward()
    if grad_sync is not None:
        grad_sync.finish()
    optimizer.step()
    refresh_weight_transposes(model, head)
    return loss, dict(terms, loss=loss)


def joint_targets(model, labels, saliency, hw, *, cam_kw=None, label_kw=None):
    """The segmentation targets of a ``forward_mirror`` pass that has just run (its 2B batch: view 1, then the h-flipped view 2),
    without grad: the tap-4 tokens of both views -- ``vit.num_tokens`` leading tokens skipped, so the distilled DeiT yields a grid
    too -- through ``ops.patch_cam`` (DPT/ACR.py:133-134), ``traincam.training_cams`` (view 2 mirrored back and added, min-max
    normalised) and ``saliency_labels``.  Returns (seg_label, saliency_out)."""
    from . import traincam
    vit = model.pretrained.model
    with torch.no_grad():
        tok = model.pretrained.activations["4"].detach()           # (2B, T, D), contiguous
        n2, T, D = tok.shape
        B = n2 // 2
        w, b = model.cls_head.weight.detach(), model.cls_head.bias.detach()
        if tok.dtype != torch.float32:                              # bf16 mode: the targets are computed in fp32 whatever the mode
            tok, w, b = tok.float(), w.float(), b.float()           # (exact upcasts; 2B x T x D values once per step)
        cams = ops.patch_cam(tok.reshape(n2 * T, D), w, b).view(n2, T, -1)
        skip = vit.num_tokens
        norm_cam = traincam.training_cams(cams[:B, skip:], labels, hw, patch_cam_flipped=cams[B:, skip:],
                                          grid=(hw[0] // vit.patch_size[1], hw[1] // vit.patch_size[0]), **(cam_kw or {}))
        return saliency_labels(norm_cam, labels, saliency, **(label_kw or {}))


def joint_train_step(model, head, optimizer, images, ori_images, croppings, labels, saliency, dense_energy_layer, *, alpha,
                     seg_weight=1.0, batch_average=False, grad_sync=None, cam_kw=None, label_kw=None, dis_weight=0.0):
    """One single-stage iteration on a ``get_data_from_chunk_v3`` batch: the classifier's own CAMs become the segmentation head's
    targets in the same step, over ONE 2B encoder pass (the loop ``_v3`` and ``compute_seg_label_3`` are written for; the
    reference tree holds no script that runs it, the composition is this project's).
      ``optimizer.zero_grad`` -> ``model.forward_mirror(images, images.flip(-1))`` (``train.train_step``'s pass) ->
      ``train.acr_loss`` -> targets without grad (``joint_targets``: tap-4 tokens of both views -> ``ops.patch_cam`` ->
      ``traincam.training_cams`` -> ``saliency_labels``) -> ``head(decoder.decode_taps(first B rows))`` -> ``segloss.joint_loss``
      (``split_cross_entropy`` alone when ``dense_energy_layer`` is None) -> ``loss = acr + seg_weight * (celoss + dloss)`` ->
      one backward (``grad_sync.prepare`` / ``finish`` around it as in the other steps) -> ``optimizer.step`` ->
      ``refresh_weight_transposes(model, head)``.
    images (B,3,S,S) float32 on the GPU (S a multiple of 32), ori_images, croppings as in ``seg_train_step``; labels (B,C) the
    image-level labels; saliency (B,S,S) uint8.  ``cam_kw`` goes to ``training_cams`` (eps), ``label_kw`` to ``saliency_labels``
    (bg_alpha, cut, open_size).  bf16 images with a bf16 model and head (vitb_hybrid; ``train.MasterWeights`` over
    ``nn.ModuleList([model, head])`` as the optimizer, which keeps the BatchNorm buffers fp32) run the whole step in bf16 storage
    with fp32 targets, logits and losses; a mixed pair raises NotImplementedError as ``decode`` does.  ``dis_weight`` > 0 adds
    ``dis_weight * featdis.feature_distance_loss(logits_half, feat)`` (``head.forward_features``) to the loss, beside the
    ``seg_weight`` term; at 0 the step makes the calls it made without the argument.  Returns (loss, terms): the four ACR terms
    (cls_loss_1, cls_loss_2, cls_align, aff_align), acr_loss, celoss, dloss, loss, disloss when ``dis_weight`` > 0, and seg_label /
    saliency_out for inspection."""
    from . import decoder
    from .train import acr_loss
    if not hasattr(model.scratch, "refinenet1"):
        raise ValueError("joint_train_step needs a model built with seg=True")
    from .backbone import HybridEmbed
    decoder.check_precision(model, images.dtype, "input", isinstance(model.pretrained.model.patch_embed, HybridEmbed))
    hw = tuple(images.shape[2:])
    optimizer.zero_grad(set_to_none=True)
    cls_list, attn_list = model.forward_mirror(images, images.flip(-1))
    acr, terms = acr_loss(cls_list, attn_list, labels, hw[0] // 16, alpha)
    seg_label, saliency_out = joint_targets(model, labels, saliency, hw, cam_kw=cam_kw, label_kw=label_kw)
    decoded = decoder.decode_taps(model, model.pretrained.activations, hw, rows=images.shape[0])
    if dis_weight > 0:
        logits, feat, logits_half = head.forward_features(decoded)
    else:
        logits = head(decoded)
    if dense_energy_layer is None:
        celoss = segloss.split_cross_entropy(logits, seg_label, batch_average)[0]
        dloss = torch.zeros((), dtype=celoss.dtype, device=celoss.device)
    else:
        celoss, dloss = segloss.joint_loss(ori_images, logits, seg_label, croppings, batch_average, dense_energy_layer)
    loss = acr + seg_weight * (celoss + dloss)
    if dis_weight > 0:
        terms = dict(terms, disloss=featdis.feature_distance_loss(logits_half, feat))
        loss = loss + dis_weight * terms["disloss"]
    if grad_sync is not None:
        grad_sync.prepare()
    loss.backward()
    if grad_sync is not None:
        grad_sync.finish()
    optimizer.step()
    refresh_weight_transposes(model, head)
    terms = dict(terms, acr_loss=acr, celoss=celoss, dloss=dloss, loss=loss, seg_label=seg_label, saliency_out=saliency_out)
    return loss, terms


def crf_labels(norm_cam, labels, ori_images, *, low_alpha=4, high_alpha=32, t=10, **seg_label_kw):
    """The CRF-based pseudo-labels of a training batch, the label source of ``compute_seg_label`` / ``compute_seg_label_2``
    (myTool.py:57-185) without their saliency line (``crf_label[saliency == 0] = 0``): norm_cam (B, C, S, S) float32 normalised
    CAMs on the GPU (``traincam.training_cams``), labels (B, C) the image-level labels (any real dtype; the reference's
    ``cam_label.astype(np.uint8) > 1e-5`` decides which classes are present), ori_images (B, 3, S, S) uint8 on the GPU.  Per image
    the CAMs of the present classes go through ``crf.crf_with_alphas_device`` in its device form -- both alphas in one mean field
    of ``t`` iterations, nothing leaves the device -- and ``pseudo.seg_label`` composes the label.  Returns the (B, S, S) uint8
    label on the GPU that ``segloss.joint_loss`` / ``seg_train_step`` take as ``seg_label``; an image with no present class is 0
    everywhere.  The CAMs are targets, not part of the graph: they are detached.
    ``seg_label_kw`` goes to ``pseudo.seg_label``.  The reference's constants are ``low_alpha=8`` (``compute_seg_label``) or 4
    (``compute_seg_label_2``, the default here), ``high_alpha=32``, and, for its confidence rule, ``ignore_uncertain=True,
    bg_alpha=32, cam_floor=0.1, fg_quantile=0.6, bg_sure=0.8, crf_sure=0.8``; ``seg_label``'s own defaults are those of
    ``compute_seg_label_rrm``.  ``compute_seg_label`` itself does not run (``for class_i in 20``), so no fixture pins this
    composition.  Reading which classes are present costs one host copy of ``labels`` per call (a synchronisation when they
    sit on the GPU); each image's two lattices synchronise once each (``acr_lattice_info``)."""
    from . import _args as A
    from . import crf
    norm_cam = A.tensor_arg(norm_cam.detach() if torch.is_tensor(norm_cam) else norm_cam, "norm_cam", torch.float32,
                            shape=("B", "C", "S", "S2"), on_gpu=False)
    b, c, h, w = norm_cam.shape
    ori_images = A.tensor_arg(ori_images, "ori_images", torch.uint8, shape=(b, 3, h, w), on_gpu=False)
    present = torch.as_tensor(labels).detach().to("cpu").numpy()
    if present.shape != (b, c):
        raise ValueError("labels must be (%d, %d) like the CAMs, got %s" % (b, c, present.shape))
    present = present.astype(np.uint8) > 1e-5
    norm_cam = A.on_device(norm_cam, "norm_cam")
    ori_images = A.on_device(ori_images, "ori_images", norm_cam.device)
    seg_label_kw.setdefault("num_classes", c)
    with torch.cuda.device(norm_cam.device):
        out = torch.zeros((b, h, w), dtype=torch.uint8, device=norm_cam.device)
        for i in range(b):
            classes = [int(j) for j in np.flatnonzero(present[i])]
            if not classes:
                continue
            cams = norm_cam[i, classes].contiguous()
            img = ori_images[i].permute(1, 2, 0).contiguous()
            _, refined = crf.crf_with_alphas_device(cams, (low_alpha, high_alpha), img, classes=classes, t=t)
            out[i] = pseudo.seg_label(cams, classes, refined[:len(classes) + 1], refined[len(classes) + 1:], **seg_label_kw)
    return out


def saliency_labels(norm_cam, labels, saliency, **kw):
    """The pseudo-labels of a ``get_data_from_chunk_v3`` batch while training runs: norm_cam (B, C, S, S) float32 normalised CAMs
    (``forward_cam``), labels (B, C) the image-level labels of the batch (any real dtype; the reference's
    ``cam_label.astype(np.uint8) > 1e-5`` decides which classes are present), saliency (B, S, S) uint8 -- all on the GPU.  Returns
    ``pseudo.seg_label_saliency``'s (label, saliency_out); label goes into ``segloss.joint_loss`` / ``seg_train_step`` as
    ``seg_label``.  The CAMs are targets, not part of the graph: they are detached.  With device inputs nothing synchronises
    (``labels`` given on the host are uploaded first).  ``kw``: bg_alpha, cut, open_size."""
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(labels)
    present = labels.to(device=norm_cam.device, dtype=torch.uint8) if labels.dtype != torch.bool else labels.to(norm_cam.device)
    return pseudo.seg_label_saliency(norm_cam.detach().contiguous(), present.contiguous(), saliency, **kw)
