"""The DPT decoder, ``ACR(..., seg=True)`` (DPT/ACR.py:51,78-85): the segmentation head's feature path that turns the encoder's
four taps into ``path_1`` -- ``forward_vit`` (DPT/vit.py:103-148), ``layerN_rn`` and ``refinenet4 .. 1`` (DPT/DPT.py:274-286) --
and the head itself (DPT/DPT.py:376-383), whose logits ``segloss.joint_loss`` takes.

BatchNorm2d (training and eval; optional fused ReLU and up to two residual addends), the x2 ``align_corners=True`` bilinear
upsampling and the leading ReLU of a residual unit run in csrc/decoder.hip behind ``acr_bn2d_*``, ``acr_upsample2x_*`` and
``acr_relu_*`` (include/acr_hip.h states the rules in full); the 3x3 and 1x1 convolutions go through ``ops.conv3x3`` /
``ops.conv1x1`` where ``ops.conv3x3_fusable`` / ``ops.conv1x1_fusable`` accept the shape and through ``F.conv2d`` otherwise.
The read-out heads of the plain ViT backbones (1x1 convolution, then a ``ConvTranspose2d`` whose kernel equals its stride) run as
two products on the fp32 GEMMs and the token-major -> NCHW depth-to-space shuffle of csrc/reassemble.hip (``readout``,
``reassemble``; ``acr_reassemble_*``).
There is no CPU path: a CPU tensor raises ``AcrHipError``.  Forward and backward are bit-identical run to run.

Precision: fp32 tensors under ``math="f32"`` and ``math="f32_split"``; under ``math="bf16"`` (bf16 input or taps AND bf16 weights,
``vitb_hybrid`` only) every map of the decoder is stored in bf16 and the norm, ReLU and upsampling run on the ``*_bf16`` entry
points, each defined as its fp32 twin's result rounded to bf16 (all sums stay double; the statistics equal the fp32 kernels' bit
for bit).  The 3x3 convolutions are torch's (MIOpen) in bf16, the 1x1 ones ``acr_conv1x1_bf16`` where the channel counts are on
its tile.  The running statistics stay fp32 (``train.MasterWeights`` keeps a norm's buffers fp32); the head casts its classifier
output to fp32 once, so logits, losses and predictions are fp32 in every mode.  A mixed pair (bf16 input with fp32 weights or the
reverse) and bf16 with a plain ViT backbone raise NotImplementedError.
Multi-GPU: ``torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)`` (train_acr.py:95), verbatim, is the switch.  A converted norm
in training mode, inside an initialised process group of more than one rank, normalises with the statistics of ALL ranks' values
and its backward uses all ranks' gradient sums.  Per layer and direction one fixed-size double tensor is exchanged -- forward
(C, 3): count, mean, sum of squared deviations; backward (C, 2): sum g, sum g * xhat -- by a ``torch.distributed.all_gather`` into
W rows in rank order; the kernels merge the rows in ascending rank order, so every rank computes the same bits whatever algorithm
the backend picks.  Ranks may hold different batch sizes (the count travels), but every rank must bring at least one image --
an empty shard, which torch's module accepts, is refused here on that rank before the gather, and the other ranks then wait in
it until the group's timeout; H * W must agree.  Parameter gradients stay local
sums: ``dp.GradSync`` averages them like every other parameter's, as ``nn.SyncBatchNorm`` relies on DDP to.  The gathers go to the
norm's ``process_group`` (None: the default group) from forward and from autograd's backward, in the same order on every rank
(DESIGN.md says why).  ``nn.BatchNorm2d`` modules never exchange anything.  The gather has run over gloo only (CPU tensors, and
two ranks sharing one GPU); no RCCL run of it exists yet, and no multi-GPU timing of this path has been measured."""
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import _lib as L
from . import ops


def _dev32(t, what):
    """a non-empty (N, C, H, W) float32 or bfloat16 tensor on the GPU (the name is older than the bf16 entry points)"""
    if not torch.is_tensor(t):
        raise ValueError("%s must be a torch tensor on the GPU, got %s" % (what, type(t).__name__))
    L.require_gpu(t)
    if t.dtype not in (torch.float32, torch.bfloat16) or t.dim() != 4 or t.numel() == 0:
        raise ValueError("%s must be a non-empty (N, C, H, W) float32 or bfloat16 tensor, got %s %s" % (what, t.dtype, tuple(t.shape)))
    return t


def _entry(name, dtype):
    """the entry point ``name`` for tensors stored as ``dtype``: (function, its name).  The bf16 twin of acr_X is acr_X_bf16
    (acr_relu_*_f32: acr_relu_*_bf16); include/acr_hip.h defines it as the fp32 result rounded to bf16."""
    if dtype == torch.bfloat16:
        name = (name[:-4] if name.endswith("_f32") else name) + "_bf16"
    return getattr(L.load(), name), name


def _param_grad(g, like):
    """a parameter gradient the kernels wrote in fp32, in the parameter's dtype (bf16: one rounding)"""
    return g if g is None or g.dtype == like.dtype else g.to(like.dtype)


def _c16(t):
    """contiguous with a 16-byte aligned base (a view into a larger buffer may start anywhere)"""
    if t is None:
        return None
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


# ------------------------------------------------------------------------------------------------
# autograd functions over the C ABI
# ------------------------------------------------------------------------------------------------
class _BatchNormAct(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, relu, resid, resid2):
        x, resid, resid2 = _c16(x), _c16(resid), _c16(resid2)
        n, c, h, w = x.shape
        dev = x.device
        with torch.cuda.device(dev):
            ws, nbytes = L.workspace("acr_bn2d_ws_bytes", n, c, h * w, device=dev)
            stats = torch.empty((c, 2), dtype=torch.float64, device=dev)
            y = torch.empty_like(x)
            fwd, name = _entry("acr_bn2d_fwd", x.dtype)
            L.check(fwd(L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(running_mean), L.ptr(running_var), L.ptr(resid),
                        L.ptr(resid2), n, c, h * w, 1 if training else 0, float(eps), float(momentum), 1 if relu else 0,
                        L.ptr(ws), nbytes, L.ptr(stats), L.ptr(y), L.stream_ptr()), name)
        ctx.save_for_backward(x, weight, stats, y if relu else None)
        ctx.training, ctx.relu, ctx.ws = bool(training), bool(relu), ws
        ctx.nres = (resid is not None) + (resid2 is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, stats, y = ctx.saved_tensors
        n, c, h, w = x.shape
        dev = x.device
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_r = ctx.nres and (ctx.needs_input_grad[9] or ctx.needs_input_grad[10])
        with torch.cuda.device(dev):
            dy = _c16(dy.to(x.dtype))
            dx = torch.empty_like(x) if need_x else None
            dgamma = torch.empty(c, dtype=torch.float32, device=dev) if need_w else None
            dbeta = torch.empty(c, dtype=torch.float32, device=dev) if need_b else None
            dres = torch.empty_like(x) if (need_r and ctx.relu) else None
            if need_x or need_w or need_b or dres is not None:
                bwd, name = _entry("acr_bn2d_bwd", x.dtype)
                L.check(bwd(L.ptr(x), L.ptr(y), L.ptr(dy), L.ptr(weight), L.ptr(stats), n, c, h * w, 1 if ctx.training else 0,
                            1 if ctx.relu else 0, L.ptr(ctx.ws), ctx.ws.numel(), L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta),
                            L.ptr(dres), L.stream_ptr()), name)
        if need_r and not ctx.relu:
            dres = dy                                       # without a ReLU the addends' gradient is dy itself
        d1 = dres if (ctx.nres >= 1 and ctx.needs_input_grad[9]) else None
        d2 = dres if (ctx.nres >= 2 and ctx.needs_input_grad[10]) else None
        return dx, _param_grad(dgamma, weight), _param_grad(dbeta, weight), None, None, None, None, None, None, d1, d2


def gather_rows(t, group=None):
    """The exchange of the cross-rank norm: ``t`` (C, k) float64, the same shape on every rank -> (W, C, k), row r rank r's ``t``,
    the same on every rank.  One ``all_gather`` on ``group`` (None: the default group) straight into the rows of the result (the
    output list is views of one buffer: exercised over gloo; not yet run over RCCL)."""
    t = t.contiguous()
    buf = torch.empty((dist.get_world_size(group),) + tuple(t.shape), dtype=t.dtype, device=t.device)
    dist.all_gather(list(buf.unbind(0)), t, group=group)
    return buf


class _SyncBatchNormAct(Function):
    """``_BatchNormAct`` in training mode with the statistics of every rank of ``group``: moments -> gather -> merged forward, and
    sums -> gather -> merged backward"""
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu, resid, resid2, group):
        x, resid, resid2 = _c16(x), _c16(resid), _c16(resid2)
        n, c, h, w = x.shape
        dev = x.device
        with torch.cuda.device(dev):
            ws = L.workspace("acr_bn2d_ws_bytes", n, c, h * w, device=dev)[0]
            moments = torch.empty((c, 3), dtype=torch.float64, device=dev)
            mom, name = _entry("acr_bn2d_moments", x.dtype)
            L.check(mom(L.ptr(x), n, c, h * w, L.ptr(ws), ws.numel(), L.ptr(moments), L.stream_ptr()), name)
            gathered = gather_rows(moments, group)
            stats = torch.empty(3 * c, dtype=torch.float64, device=dev)          # (C, 2) mean / invstd, then the C merged counts
            y = torch.empty_like(x)
            fwd, name = _entry("acr_bn2d_fwd_merged", x.dtype)
            L.check(fwd(L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(running_mean), L.ptr(running_var), L.ptr(resid),
                        L.ptr(resid2), n, c, h * w, L.ptr(gathered), gathered.shape[0], float(eps), float(momentum),
                        1 if relu else 0, L.ptr(ws), ws.numel(), L.ptr(stats), L.ptr(y), L.stream_ptr()), name)
        ctx.save_for_backward(x, weight, stats, y if relu else None)
        ctx.relu, ctx.ws, ctx.group = bool(relu), ws, group
        ctx.nres = (resid is not None) + (resid2 is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, stats, y = ctx.saved_tensors
        n, c, h, w = x.shape
        dev = x.device
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_r = ctx.nres and (ctx.needs_input_grad[8] or ctx.needs_input_grad[9])
        relu = 1 if ctx.relu else 0
        with torch.cuda.device(dev):
            dy = _c16(dy.to(x.dtype))
            dx = torch.empty_like(x) if need_x else None
            dgamma = torch.empty(c, dtype=torch.float32, device=dev) if need_w else None
            dbeta = torch.empty(c, dtype=torch.float32, device=dev) if need_b else None
            dres = torch.empty_like(x) if (need_r and ctx.relu) else None
            if need_x or need_w or need_b or dres is not None:
                sums = torch.empty((c, 2), dtype=torch.float64, device=dev)
                bsum, name = _entry("acr_bn2d_bwd_sums", x.dtype)
                L.check(bsum(L.ptr(x), L.ptr(y), L.ptr(dy), L.ptr(stats), n, c, h * w, relu, L.ptr(ctx.ws), ctx.ws.numel(),
                             L.ptr(sums), L.ptr(dgamma), L.ptr(dbeta), L.stream_ptr()), name)
                if need_x or dres is not None:
                    # the exchange happens exactly when x needs a gradient, as in torch; dres alone is the masked dy, no sums in it
                    rows = gather_rows(sums, ctx.group) if need_x else sums.unsqueeze(0)
                    bmer, name = _entry("acr_bn2d_bwd_merged", x.dtype)
                    L.check(bmer(L.ptr(x), L.ptr(y), L.ptr(dy), L.ptr(weight), L.ptr(stats), L.ptr(rows), rows.shape[0],
                                 n, c, h * w, relu, L.ptr(ctx.ws), ctx.ws.numel(), L.ptr(dx), L.ptr(dres), L.stream_ptr()), name)
        if need_r and not ctx.relu:
            dres = dy                                       # without a ReLU the addends' gradient is dy itself
        d1 = dres if (ctx.nres >= 1 and ctx.needs_input_grad[8]) else None
        d2 = dres if (ctx.nres >= 2 and ctx.needs_input_grad[9]) else None
        return dx, _param_grad(dgamma, weight), _param_grad(dbeta, weight), None, None, None, None, None, d1, d2, None


def _sync_group(bn):
    """(exchange?, group) by ``nn.SyncBatchNorm.forward``'s own condition: the module normalises with batch statistics while it
    trains, ``torch.distributed`` is initialised and the module's group (None: the default one) has more than one rank"""
    if not (isinstance(bn, nn.SyncBatchNorm) and bn.training and dist.is_available() and dist.is_initialized()):
        return False, None
    return dist.get_world_size(bn.process_group) > 1, bn.process_group


def batch_norm_act(x, bn, act="none", resid=None, resid2=None):
    """``act(bn(x) [+ resid] [+ resid2])`` in one pass: ``bn`` an ``nn.BatchNorm2d`` or an ``nn.SyncBatchNorm`` (affine, a float
    ``momentum``), ``act`` "none" or "relu", the addends shaped like ``x`` (``resid2`` only with ``resid``).  In training mode the
    batch statistics (biased variance) normalise and the module's ``running_mean`` / ``running_var`` / ``num_batches_tracked`` are
    updated as ``nn.BatchNorm2d`` updates them (the running variance unbiased); in eval mode the running statistics normalise and
    the backward treats them as constants.  One value per channel in training mode raises ValueError, as torch does.  An
    ``nn.BatchNorm2d`` uses this process's batch alone.  An ``nn.SyncBatchNorm`` that trains inside a process group of more than
    one rank uses every rank's values (the module docstring says what is exchanged); then one value per channel on a rank is
    legal, an empty batch on a rank is not (every rank must call with N >= 1, or the others wait in the gather).  Anywhere else -- eval mode, no process group, a one-rank group -- it computes the bits of an ``nn.BatchNorm2d`` with
    the same state.  Differentiable in x, the affine parameters and the addends.
    Storage: x, the addends and the norm's weight / bias are all float32 or all bfloat16 (a mix raises ValueError); bf16 takes the
    ``acr_bn2d_*_bf16`` entry points, whose outputs are the fp32 ones rounded to bf16, and returns parameter gradients in bf16.  The
    running statistics are float32 in either case: bf16 ones raise ValueError in training mode (keep them fp32, as
    ``train.MasterWeights`` does) and are upcast into a temporary in eval mode, which is exact and leaves the module as it is."""
    if act not in ("none", "relu"):
        raise ValueError("act must be \"none\" or \"relu\", got %r" % (act,))
    if not isinstance(bn, (nn.BatchNorm2d, nn.SyncBatchNorm)) or not bn.affine:
        raise NotImplementedError("batch_norm_act takes an affine nn.BatchNorm2d or nn.SyncBatchNorm, got %s" % type(bn).__name__)
    if bn.momentum is None and bn.track_running_stats:
        raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative average) is not built; give a float momentum")
    if resid2 is not None and resid is None:
        raise ValueError("resid2 given without resid")
    x = _dev32(x, "x")
    if x.shape[1] != bn.num_features:
        raise ValueError("x has %d channels, the norm %d" % (x.shape[1], bn.num_features))
    for r in (resid, resid2):
        if r is not None and (_dev32(r, "resid").shape != x.shape or r.device != x.device):
            raise ValueError("an addend %s on %s does not match x %s on %s" % (tuple(r.shape), r.device, tuple(x.shape), x.device))
        if r is not None and r.dtype != x.dtype:
            raise ValueError("an addend is %s, x %s: one storage type per call" % (r.dtype, x.dtype))
    if bn.weight.dtype != x.dtype or bn.bias.dtype != x.dtype or bn.weight.device != x.device:
        raise ValueError("the norm's parameters must be %s, as x, on %s (got %s / %s)" % (x.dtype, x.device, bn.weight.dtype, bn.bias.dtype))
    training = bn.training or bn.running_mean is None
    sync, group = _sync_group(bn)
    if training and not sync and x.shape[0] * x.shape[2] * x.shape[3] < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    rm, rv = (bn.running_mean, bn.running_var) if bn.track_running_stats else (None, None)
    if rm is not None and (rm.dtype != torch.float32 or rv.dtype != torch.float32):
        if training:
            raise ValueError("the running statistics are %s / %s: keep them float32 (a bf16 running_var updated with momentum 0.1 "
                             "stops moving); train.MasterWeights leaves a norm's buffers fp32" % (rm.dtype, rv.dtype))
        rm, rv = rm.float(), rv.float()                      # eval mode reads them only: an exact upcast into a temporary
    if bn.training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if sync:
        return _SyncBatchNormAct.apply(x, bn.weight, bn.bias, rm, rv, bn.momentum or 0.0, bn.eps, act == "relu", resid, resid2, group)
    return _BatchNormAct.apply(x, bn.weight, bn.bias, rm, rv, training, bn.momentum or 0.0, bn.eps, act == "relu", resid, resid2)


class _Relu(Function):
    @staticmethod
    def forward(ctx, x):
        x = _c16(x)
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            fwd, name = _entry("acr_relu_fwd_f32", x.dtype)
            L.check(fwd(L.ptr(x), x.numel(), L.ptr(y), L.stream_ptr()), name)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        dy = _c16(dy.to(y.dtype))
        dx = torch.empty_like(y)
        with torch.cuda.device(y.device):
            bwd, name = _entry("acr_relu_bwd_f32", y.dtype)
            L.check(bwd(L.ptr(y), L.ptr(dy), y.numel(), L.ptr(dx), L.stream_ptr()), name)
        return dx


def relu(x):
    """``max(x, 0)`` as a new tensor: the leading ``activation(x)`` of a residual unit (blocks.py:330), whose raw ``x`` stays
    untouched for the skip (:343).  (The reference's own ``nn.ReLU(False)`` is out of place for the same reason.)  float32 or
    bfloat16; the gradient has x's dtype."""
    return _Relu.apply(_dev32(x, "x"))


class _Upsample2x(Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        n, c, h, w = x.shape
        y = torch.empty((n, c, 2 * h, 2 * w), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            fwd, name = _entry("acr_upsample2x_fwd", x.dtype)
            L.check(fwd(L.ptr(x), n * c, h, w, 2 * h, 2 * w, L.ptr(y), L.stream_ptr()), name)
        ctx.shape, ctx.dtype = (n, c, h, w), x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c, h, w = ctx.shape
        dy = dy.to(ctx.dtype).contiguous()
        dx = torch.empty((n, c, h, w), dtype=ctx.dtype, device=dy.device)
        with torch.cuda.device(dy.device):
            bwd, name = _entry("acr_upsample2x_bwd", ctx.dtype)
            L.check(bwd(L.ptr(dy), n * c, h, w, 2 * h, 2 * w, L.ptr(dx), L.stream_ptr()), name)
        return dx


def upsample2x(x):
    """``F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)`` (blocks.py:407-409) with its backward.  float32, or bfloat16:
    the fp32 result rounded to bf16."""
    return _Upsample2x.apply(_dev32(x, "x"))


class _Reassemble(Function):
    @staticmethod
    def forward(ctx, y2d, bias, B, T, start, gh, gw, C, s):
        lib = L.load()
        dev = y2d.device
        out = torch.empty((B, C, gh * s, gw * s), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.acr_reassemble_fwd(L.ptr(y2d), y2d.stride(0), L.ptr(bias), B, T, start, gh, gw, C, s, L.ptr(out), L.stream_ptr()),
                    "acr_reassemble_fwd")
        ctx.geom = (B, T, start, gh, gw, C, s)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        B, T, start, gh, gw, C, s = ctx.geom
        dev = dout.device
        need_b = ctx.has_bias and ctx.needs_input_grad[1]
        if not (ctx.needs_input_grad[0] or need_b):
            return (None,) * 9
        with torch.cuda.device(dev):
            dout = dout.to(torch.float32).contiguous()
            dy = torch.empty((B * T, C * s * s), dtype=torch.float32, device=dev)       # every element is written: the skipped rows as zeros
            dbias = torch.empty(C, dtype=torch.float32, device=dev) if need_b else None
            ws = torch.empty(lib.acr_reassemble_ws_bytes(B, gh, gw, C, s), dtype=torch.uint8, device=dev) if need_b else None
            L.check(lib.acr_reassemble_bwd(L.ptr(dout), B, T, start, gh, gw, C, s, L.ptr(dy), dy.stride(0), L.ptr(dbias), L.ptr(ws),
                                           ws.numel() if ws is not None else 0, L.stream_ptr()), "acr_reassemble_bwd")
        return (dy if ctx.needs_input_grad[0] else None, dbias) + (None,) * 7


def reassemble(y2d, bias, B, T, start, gh, gw, C, s):
    """Token-major -> NCHW with the depth-to-space shuffle of a ``ConvTranspose2d`` whose kernel equals its stride ``s`` (DPT/vit.py
    :117-146 with the heads of :263-341): ``y2d`` (B * T, C * s * s) float32 on the GPU, unit inner stride, any row pitch;
    ``out[b, co, i * s + di, j * s + dj] = y2d[b * T + start + i * gw + j, (co * s + di) * s + dj] + bias[co]`` -> (B, C, gh * s,
    gw * s).  ``bias`` (C) or None; ``s`` 1, 2 or 4; ``T == start + gh * gw``; the first ``start`` (0 .. 8) tokens of every sample are
    skipped and receive a zero gradient.  Differentiable in ``y2d`` and ``bias``; forward and backward repeat bit for bit."""
    if not torch.is_tensor(y2d):
        raise ValueError("y2d must be a torch tensor on the GPU, got %s" % type(y2d).__name__)
    L.require_gpu(y2d, bias)
    B, T, start, gh, gw, C, s = (int(v) for v in (B, T, start, gh, gw, C, s))
    if s not in (1, 2, 4):
        raise ValueError("s must be 1, 2 or 4, got %d" % s)
    if min(B, gh, gw, C) < 1 or not 0 <= start <= 8 or T != start + gh * gw:
        raise ValueError("need B, gh, gw, C >= 1, 0 <= start <= 8 and T == start + gh * gw, got B=%d T=%d start=%d gh=%d gw=%d C=%d"
                         % (B, T, start, gh, gw, C))
    if y2d.dtype == torch.bfloat16:
        raise NotImplementedError("reassemble is not built in bf16 (the plain ViT read-outs are fp32 only)")
    if y2d.dtype != torch.float32 or y2d.dim() != 2 or tuple(y2d.shape) != (B * T, C * s * s) or y2d.stride(1) != 1 or y2d.stride(0) < C * s * s:
        raise ValueError("y2d must be a (B * T, C * s * s) = (%d, %d) float32 matrix with a unit inner stride, got %s %s strides %s"
                         % (B * T, C * s * s, y2d.dtype, tuple(y2d.shape), y2d.stride() if y2d.dim() == 2 else None))
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (C,) or bias.device != y2d.device or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous (%d,) float32 tensor on %s, got %s %s" % (C, y2d.device, bias.dtype, tuple(bias.shape)))
    return _Reassemble.apply(y2d, bias, B, T, start, gh, gw, C, s)


class _DeconvProduct(Function):
    """``y2 (M, f * s * s) = z (M, f) . W.view(f, f * s * s)`` with the ``ConvTranspose2d`` weight (ci, co, s, s) as stored: forward
    'nn', input gradient 'nt', weight gradient 'tn' of acr_gemm_f32 -- the weight is neither copied nor transposed"""
    @staticmethod
    def forward(ctx, z, weight, math):
        if z.dtype != torch.float32 or weight.dtype != torch.float32:
            raise NotImplementedError("the read-out's second product is not built in bf16 (fp32 only), got %s / %s" % (z.dtype, weight.dtype))
        f = weight.shape[0]
        w2 = weight.view(f, -1)
        y2 = torch.empty((z.shape[0], w2.shape[1]), dtype=torch.float32, device=z.device)
        with torch.cuda.device(z.device):
            ops.gemm_f32_raw("nn", z, w2, y2, math=math)
        ctx.save_for_backward(z, weight)
        ctx.math = math
        return y2

    @staticmethod
    def backward(ctx, dy2):
        z, weight = ctx.saved_tensors
        f = weight.shape[0]
        w2 = weight.view(f, -1)
        dy2 = _c16(dy2.to(torch.float32))
        dz = dw = None
        with torch.cuda.device(z.device):
            if ctx.needs_input_grad[0]:
                dz = torch.empty_like(z)
                ops.gemm_f32_raw("nt", dy2, w2, dz, math=ctx.math)
            if ctx.needs_input_grad[1]:
                dw = torch.empty_like(w2)
                ops.gemm_f32_raw("tn", z, dy2, dw, math=ctx.math)
                dw = dw.view(weight.shape)
        return dz, dw, None


def readout(tok, start, gh, gw, conv1, deconv, math=0):
    """One read-out head of a plain ViT (DPT/vit.py:263-341, run by :117-146) on the tokens ``tok`` (B, T, D) of its hook, ``T ==
    start + gh * gw``: the 1x1 convolution ``conv1`` (D -> f) as a Linear on ALL tokens (``ops.LinearF32Fn``), then -- for ``deconv``
    an ``nn.ConvTranspose2d(f, f, s, stride=s)``, s 2 or 4 -- the product with its weight as stored, and ``reassemble`` with its
    bias -> (B, f, gh * s, gw * s); ``deconv`` None: ``reassemble`` alone (s = 1, no bias) -> (B, f, gh, gw).  ``math``: a
    ``_lib.MATH`` code; 2 (fp16x2, an opt-in of the block Linears) runs as exact fp32 here."""
    if not torch.is_tensor(tok):
        raise ValueError("tok must be a torch tensor on the GPU, got %s" % type(tok).__name__)
    L.require_gpu(tok)
    if tok.dtype == torch.bfloat16:
        raise NotImplementedError("the read-outs of the plain ViT backbones are not built in bf16 (fp32 only; bf16 decode takes "
                                  "vitb_hybrid)")
    if tok.dtype != torch.float32 or tok.dim() != 3 or tok.numel() == 0:
        raise ValueError("tok must be a non-empty (B, T, D) float32 tensor, got %s %s" % (tok.dtype, tuple(tok.shape)))
    B, T, D = tok.shape
    if not (isinstance(conv1, nn.Conv2d) and conv1.kernel_size == (1, 1) and conv1.stride == (1, 1) and conv1.padding == (0, 0)
            and conv1.groups == 1 and conv1.in_channels == D):
        raise ValueError("conv1 must be an nn.Conv2d(%d, f, 1), got %r" % (D, conv1))
    f, s = conv1.out_channels, 1
    if deconv is not None:
        s = deconv.kernel_size[0] if isinstance(deconv, nn.ConvTranspose2d) else 0
        if not (s in (2, 4) and deconv.kernel_size == (s, s) and deconv.stride == (s, s) and deconv.padding == (0, 0)
                and deconv.output_padding == (0, 0) and deconv.dilation == (1, 1) and deconv.groups == 1
                and deconv.in_channels == f and deconv.out_channels == f):
            raise NotImplementedError("the read-out's second step is an nn.ConvTranspose2d(f, f, s, stride=s) with s 2 or 4 and f = %d, "
                                      "got %r" % (f, deconv))
    if T != start + gh * gw:
        raise ValueError("%d tokens are not %d skipped ones and a %d x %d grid" % (T, start, gh, gw))
    math = 0 if math == L.MATH["f32_fp16x2"] else int(math)
    tok = _c16(tok)
    w1 = conv1.weight.view(f, D)
    if not ops.linear_f32_usable(tok, w1) or f % 4:
        raise NotImplementedError("the fp32 GEMMs take D and f that are multiples of 4 and at least 32, got D=%d f=%d" % (D, f))
    with torch.cuda.device(tok.device):
        z = ops.LinearF32Fn.apply(tok, w1, conv1.bias, None, None, math).reshape(B * T, f)
    if deconv is None:
        return reassemble(z, None, B, T, start, gh, gw, f, 1)
    return reassemble(_DeconvProduct.apply(z, deconv.weight, math), deconv.bias, B, T, start, gh, gw, f, s)


def conv(m, x, math):
    """The ``nn.Conv2d`` ``m`` on x: the hand-written 3x3 / 1x1 kernels where they cover the shape (bias added after), torch's
    convolution otherwise (a stride-2 convolution, channel counts off the tile, a map narrower than 16: the H/32 level at 384^2
    and 448^2)."""
    k, s, p = m.kernel_size, m.stride, m.padding
    if m.groups == 1 and m.dilation == (1, 1) and s == (1, 1):
        y = None
        if k == (3, 3) and p == (1, 1) and ops.conv3x3_fusable(x, m.weight, 1, math):
            y = ops.conv3x3(x, m.weight)
        elif k == (1, 1) and p == (0, 0) and ops.conv1x1_fusable(x, m.weight, 1):
            y = ops.conv1x1(x, m.weight, None, math)
        if y is not None:
            return y if m.bias is None else y + m.bias.view(1, -1, 1, 1)
    return F.conv2d(x, m.weight, m.bias, s, p, m.dilation, m.groups)


# ------------------------------------------------------------------------------------------------
# modules: DPT/blocks.py:277-413, DPT/DPT.py:376-383
# ------------------------------------------------------------------------------------------------
def _relu_only(activation):
    if not isinstance(activation, nn.ReLU):
        raise NotImplementedError("the decoder's activation is nn.ReLU (DPT/ACR.py:18), got %s" % type(activation).__name__)


class ResidualConvUnit_custom(nn.Module):
    """blocks.py:277-345 with ``bn=True``, ``groups=1``: relu, conv1, bn1, relu, conv2, bn2, + x."""
    acr_math = 0

    def __init__(self, features, activation, bn):
        super().__init__()
        _relu_only(activation)
        if bn is not True:
            raise NotImplementedError("ResidualConvUnit_custom is built with bn=True only (DPT/ACR.py:153)")
        self.bn = bn
        self.groups = 1
        self.conv1 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=False, groups=1)
        self.conv2 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=False, groups=1)
        self.bn1 = nn.BatchNorm2d(features)
        self.bn2 = nn.BatchNorm2d(features)
        self.activation = activation

    def forward(self, x, addend=None):
        """``addend``: a second skip added in the same pass as ``+ x`` (the fusion block's ``output + res``, blocks.py:402)"""
        out = relu(x)
        out = conv(self.conv1, out, self.acr_math)
        out = batch_norm_act(out, self.bn1, "relu")              # bn1 and the second activation (:333-335)
        out = conv(self.conv2, out, self.acr_math)
        return batch_norm_act(out, self.bn2, "none", x, addend)


class FeatureFusionBlock_custom(nn.Module):
    """blocks.py:348-413 in the configuration ``_make_fusion_block`` builds (DPT/ACR.py:15-23)."""
    acr_math = 0

    def __init__(self, features, activation, deconv=False, bn=False, expand=False, align_corners=True):
        super().__init__()
        _relu_only(activation)
        if deconv or expand or not align_corners or bn is not True:
            raise NotImplementedError("FeatureFusionBlock_custom is built for bn=True, deconv=False, expand=False, align_corners=True "
                                      "(got bn=%r, deconv=%r, expand=%r, align_corners=%r)" % (bn, deconv, expand, align_corners))
        self.deconv, self.align_corners, self.groups, self.expand = deconv, align_corners, 1, expand
        self.out_conv = nn.Conv2d(features, features, kernel_size=1, stride=1, padding=0, bias=True, groups=1)
        self.resConfUnit1 = ResidualConvUnit_custom(features, activation, bn)
        self.resConfUnit2 = ResidualConvUnit_custom(features, activation, bn)

    def forward(self, *xs):
        if len(xs) not in (1, 2):
            raise ValueError("a fusion block takes one or two inputs, got %d" % len(xs))
        output = xs[0]
        if len(xs) == 2:
            output = self.resConfUnit1(xs[1], addend=output)    # res = unit1(xs[1]); output + res
        output = self.resConfUnit2(output)
        output = upsample2x(output)
        return conv(self.out_conv, output, self.acr_math)


class _Interpolate2x(nn.Module):
    def forward(self, x):
        return upsample2x(x)


class SegmentationHead(nn.Sequential):
    """DPT/DPT.py:376-383 with that ``nn.Sequential``'s state-dict keys (0: 3x3 convolution without bias, 1: BatchNorm, 2: ReLU,
    3: Dropout 0.1, 4: 1x1 convolution to ``num_classes + 1``, 5: x2 upsampling).  Norm and ReLU run as one pass."""
    acr_math = 0

    def __init__(self, features, num_classes):
        super().__init__(nn.Conv2d(features, features, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(features), nn.ReLU(True),
                         nn.Dropout(0.1, False), nn.Conv2d(features, num_classes + 1, kernel_size=1), _Interpolate2x())

    def forward(self, x):
        x = batch_norm_act(conv(self[0], x, self.acr_math), self[1], "relu")
        return self[5](self._f32(conv(self[4], self[3](x), self.acr_math)))

    @staticmethod
    def _f32(logits_half):
        """bf16 mode: the classifier's output (B, K + 1, h / 2, w / 2), the smallest tensor of the stage, is cast to fp32 once; the
        final x2 upsampling and everything behind it (segloss, segpred, featdis' ``seg``) are fp32.  fp32: the tensor itself."""
        return logits_half.float() if logits_half.dtype == torch.bfloat16 else logits_half

    def forward_features(self, x):
        """(logits, feat, logits_half): ``forward``'s logits by the same calls, ``feat`` the tensor the 1x1 classifier ``self[4]``
        reads and ``logits_half`` that classifier's output before the x2 upsampling -- what ``featdis.feature_distance_loss`` takes."""
        feat = self[3](batch_norm_act(conv(self[0], x, self.acr_math), self[1], "relu"))
        logits_half = self._f32(conv(self[4], feat, self.acr_math))
        if feat.dtype == torch.bfloat16:
            feat = feat.float()              # featdis is fp32: a differentiable copy of (B, features, h / 2, w / 2); cost unmeasured
        return self[5](logits_half), feat, logits_half


def make_fusion_block(features, use_bn):
    """DPT/ACR.py:15-23"""
    return FeatureFusionBlock_custom(features, nn.ReLU(False), deconv=False, bn=use_bn, expand=False, align_corners=True)


# ------------------------------------------------------------------------------------------------
# the decoder pass
# ------------------------------------------------------------------------------------------------
def check_precision(model, act_dtype, what, hybrid):
    """The decoder's one precision rule: activations and weights are both float32 or both bfloat16, and bf16 is built for the
    hybrid backbone only (the plain ViT read-outs need the fp32 GEMMs: tap 1 of ``vitb`` has f = 96, off the bf16 GEMM's K % 64)"""
    wd = model.cls_head.weight.dtype
    if act_dtype != wd or wd not in (torch.float32, torch.bfloat16):
        raise NotImplementedError("decode takes fp32 tensors with fp32 weights (math \"f32\" and \"f32_split\") or bf16 tensors with bf16 "
                                  "weights (math \"bf16\"), got %s %s / %s weights" % (act_dtype, what, wd))
    if wd == torch.bfloat16 and not hybrid:
        raise NotImplementedError("bf16 decode is built for the hybrid backbone (vitb_hybrid) only: the read-outs of the plain ViT "
                                  "backbones (readout, reassemble) are fp32, got %s" % model.cur_backbone)


def layers_rn(model, x):
    """``forward_vit`` (DPT/vit.py:103-148) and ``scratch.layerN_rn`` (DPT/DPT.py:274-281) of a ``seg=True`` model:
    the four (B, features, h / 4 .. h / 32, ...) maps the fusion blocks take.  Hybrid: taps 1 and 2 are the stem stages the
    encoder records; taps 3 and 4 drop the class token (``readout="ignore"``), become (B, D, h / 16, w / 16) and go through
    ``act_postprocess3`` / ``act_postprocess4``.  A plain ViT: ``_layers_rn_plain``.  A model without read-out heads (the
    project's own ``vit_tiny``) raises NotImplementedError."""
    from .backbone import HybridEmbed
    if not hasattr(model.scratch, "refinenet1"):
        raise ValueError("decode needs a model built with seg=True")
    vit = model.pretrained.model
    hybrid = isinstance(vit.patch_embed, HybridEmbed)
    if not hybrid and not all(hasattr(model.pretrained, "act_postprocess%d" % i) for i in (1, 2, 3, 4)):
        raise NotImplementedError("decode needs the four read-out heads pretrained.act_postprocess1..4; %s has none" % model.cur_backbone)
    if not torch.is_tensor(x):
        raise ValueError("x must be a torch tensor on the GPU, got %s" % type(x).__name__)
    L.require_gpu(x)
    check_precision(model, x.dtype, "input", hybrid)
    model._encode(x)
    return layers_rn_taps(model, model.pretrained.activations, x.shape[2:])


def layers_rn_taps(model, taps, hw, rows=None):
    """The part of ``layers_rn`` after the encoder pass: ``taps`` is what ``model._encode(x)`` left in
    ``model.pretrained.activations`` for an x of spatial size ``hw`` = (h, w) (``layers_rn`` has checked model and input).
    ``rows``: take the first ``rows`` samples of every tap -- a step that ran both views as one 2B batch (``forward_mirror``)
    decodes view 1 from it, ``rows`` = B."""
    from .backbone import HybridEmbed
    vit = model.pretrained.model
    hybrid = isinstance(vit.patch_embed, HybridEmbed)
    if rows is not None:
        if not 1 <= rows <= taps["4"].shape[0]:
            raise ValueError("rows=%r outside 1..%d, the batch of the pass" % (rows, taps["4"].shape[0]))
        taps = {k: taps[k][:rows] for k in ("1", "2", "3", "4")}
    h, w = hw
    b = taps["4"].shape[0]
    gh, gw = h // vit.patch_size[1], w // vit.patch_size[0]
    skip = vit.num_tokens                                    # 1: the class token (Slice(start_index=1), DPT/vit.py:57-63)
    math = vit.acr_math
    if not hybrid:
        return _layers_rn_plain(model, taps, skip, gh, gw, math)

    def grid(tok):
        return tok[:, skip:].transpose(1, 2).reshape(b, tok.shape[2], gh, gw).contiguous()
    pp, sc = model.pretrained, model.scratch
    layer_3 = conv(pp.act_postprocess3[3], grid(taps["3"]), math)
    layer_4 = conv(pp.act_postprocess4[4], conv(pp.act_postprocess4[3], grid(taps["4"]), math), math)
    return (conv(sc.layer1_rn, taps["1"].contiguous(), math), conv(sc.layer2_rn, taps["2"].contiguous(), math),
            conv(sc.layer3_rn, layer_3, math), conv(sc.layer4_rn, layer_4, math))


def _layers_rn_plain(model, taps, skip, gh, gw, math):
    """``layers_rn`` of a plain ViT (vitb, deit, deit_distilled, vitl; DPT/vit.py:224-353): every tap is the tokens of a block
    (hooks DPT/ACR.py:59-65) and goes through ``readout`` -- x4, x2, x1 and, for tap 4, x1 followed by the stride-2 3x3 convolution,
    which stays on torch's convolution as in the hybrid model.  ``skip`` is 2 for the distilled DeiT (DPT/vit.py:617-632)."""
    pp, sc = model.pretrained, model.scratch
    layer_1 = readout(taps["1"], skip, gh, gw, pp.act_postprocess1[3], pp.act_postprocess1[4], math)
    layer_2 = readout(taps["2"], skip, gh, gw, pp.act_postprocess2[3], pp.act_postprocess2[4], math)
    layer_3 = readout(taps["3"], skip, gh, gw, pp.act_postprocess3[3], None, math)
    layer_4 = conv(pp.act_postprocess4[4], readout(taps["4"], skip, gh, gw, pp.act_postprocess4[3], None, math), math)
    return (conv(sc.layer1_rn, layer_1, math), conv(sc.layer2_rn, layer_2, math), conv(sc.layer3_rn, layer_3, math),
            conv(sc.layer4_rn, layer_4, math))


def fuse(model, l1, l2, l3, l4):
    """``refinenet4 .. 1`` (DPT/DPT.py:283-286) on the four ``layerN_rn`` maps: ``path_1``"""
    sc = model.scratch
    path_4 = sc.refinenet4(l4)
    path_3 = sc.refinenet3(path_4, l3)
    path_2 = sc.refinenet2(path_3, l2)
    return sc.refinenet1(path_2, l1)


def decode(model, x):
    """x (B, 3, h, w) float32 on the GPU, h and w multiples of 32 -> ``path_1`` (B, features, h / 2, w / 2) of an
    ``ACR(..., seg=True)`` with any of the reference's backbones -- vitb_hybrid, vitb, deit, deit_distilled, vitl --
    (DPT/DPT.py:274-286); ``SegmentationHead`` turns it into (B, num_classes + 1, h, w) logits.  A model without read-out heads
    (``vit_tiny``) raises NotImplementedError; bf16 x with bf16 weights is built for vitb_hybrid, a mixed pair is not.  BatchNorm statistics are per process, or those of all ranks after
    ``nn.SyncBatchNorm.convert_sync_batchnorm`` (see the module docstring)."""
    return fuse(model, *layers_rn(model, x))


def decode_taps(model, taps, hw, rows=None):
    """``decode`` from an encoder pass that has already run: ``taps`` = ``model.pretrained.activations`` after ``model._encode(x)``
    (``forward_cls``, ``forward_cam``, ``forward_mirror``) on an x (float32, or bfloat16 as the weights) of spatial size ``hw``; ``rows`` as in
    ``layers_rn_taps``.  On the taps of ``decode``'s own pass the result is ``decode``'s, bit for bit."""
    if not hasattr(model.scratch, "refinenet1"):
        raise ValueError("decode needs a model built with seg=True")
    if any(k not in taps for k in ("1", "2", "3", "4")):
        raise ValueError("taps holds %s: run the encoder pass first (the four taps \"1\" .. \"4\")" % sorted(taps))
    from .backbone import HybridEmbed
    check_precision(model, taps["4"].dtype, "taps", isinstance(model.pretrained.model.patch_embed, HybridEmbed))
    return fuse(model, *layers_rn_taps(model, taps, hw, rows))
