"""One training step of the segmentation head on the pseudo-labels, on the HIP path.

The reference tree has the loss (``compute_joint_loss``, myTool.py:825-857), the loaders that feed it
(``get_data_from_chunk_v4`` / ``_v3``, :1257-1310 / :1202-1253) and ``forward_seg`` (:1869), but no script that calls them
together: the composition below is this project's.  It ties ``segval.forward_seg`` (decoder + ``SegmentationHead``),
``segloss.joint_loss`` and the optimizer together in the order ``train.train_step`` uses for the classification step, and takes the
tensors ``data.ChunkLoader.get_data_from_chunk_v4`` returns as they are -- nothing leaves the device.  With ``_v3``, which brings a
saliency map instead of a label, ``saliency_labels`` makes the label on the way (``compute_seg_label_3``, :188-264, the call the
reference's ``_v3`` loader is written for)."""
import torch

from . import ops, pseudo, segloss, segval
from .train import refresh_weight_transposes


def seg_train_step(model, head, optimizer, images, ori_images, croppings, seg_label, dense_energy_layer, *, batch_average=False,
                   grad_sync=None):
    """``optimizer.zero_grad`` -> ``forward_seg(model, head, images)`` -> ``joint_loss`` -> ``loss = celoss + dloss`` -> backward ->
    ``optimizer.step``.  images (B,3,S,S) float32 on the GPU (S a multiple of 32), ori_images (B,3,S,S) values 0..255, croppings
    (S,S,B), seg_label (B,S,S) uint8 (255 = ignore) -- the loader's tuple; ``optimizer`` holds the parameters of ``model`` and
    ``head`` that are to train.  ``dense_energy_layer``: a ``segloss.DenseEnergyLoss``, or None for the cross-entropy alone (dloss
    is then 0).  ``batch_average`` is ``joint_loss``'s ``criterion_batch_average``.  ``grad_sync`` (``dp.GradSync``) all-reduces the
    gradients while backward runs, as in ``train.train_step``.  After the update the cached split-product weight images and weight
    transposes of model and head are renewed: the fused optimizer writes the weights in place.  Returns (loss, terms) with terms =
    dict(celoss, dloss, loss)."""
    optimizer.zero_grad(set_to_none=True)
    logits = segval.forward_seg(model, head, images)
    if dense_energy_layer is None:
        celoss = segloss.split_cross_entropy(logits, seg_label, batch_average)[0]
        dloss = torch.zeros((), dtype=celoss.dtype, device=celoss.device)
    else:
        celoss, dloss = segloss.joint_loss(ori_images, logits, seg_label, croppings, batch_average, dense_energy_layer)
    loss = celoss + dloss
    if grad_sync is not None:
        grad_sync.prepare()
    loss.backward()
    if grad_sync is not None:
        grad_sync.finish()
    optimizer.step()
    refresh_weight_transposes(model)
    ops.invalidate_weight_images(head)
    return loss, dict(celoss=celoss, dloss=dloss, loss=loss)


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
