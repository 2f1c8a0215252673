"""ACR model surface -- drop-in for the reference's ``DPT/ACR.py`` (BaseModel :25-37, DPT :40-143, ACR :147-215).

Same constructor, same methods, same state-dict layout; what changes is underneath:
  * both views of ``forward_mirror`` run as ONE 2B batch (exact: every norm is per-sample), and the
    (B,L,T,T) head-mean stack is written slice-by-slice by the attention kernels -- no (B,H,T,T) softmax
    in HBM, no 12 mean kernels, no stack copy (DPT/ACR.py:107-112);
  * ``getam`` reads row 0 of dO V^T / P straight from the saved q,k,v,dO with one small kernel per layer
    instead of materialising two (B,H,T,T) tensors per block (:181-206);
  * there is no CPU fallback: tensors must live on an MI355X and libacr_hip.so must be built.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _derived, ops
from ..backbone import VisionTransformer

# backbone name -> VisionTransformer kwargs, DPT scratch in_shape, the four hooks   (DPT/vit.py:548-632, DPT/blocks.py:26-83,
# DPT/ACR.py:59-65; the hybrid's hooks 0 and 1 are stem stages, not blocks: backbone.ResNetV2 records them)
_BACKBONES = {
    "vitb_rn50_384": (dict(embed_dim=768, depth=12, num_heads=12, hybrid=True), [256, 512, 768, 768], (0, 1, 8, 11)),
    "vitb16_384": (dict(embed_dim=768, depth=12, num_heads=12, hybrid=False), [96, 192, 384, 768], (2, 5, 8, 11)),
    "deitb16_384": (dict(embed_dim=768, depth=12, num_heads=12, hybrid=False), [96, 192, 384, 768], (2, 5, 8, 11)),
    "deitb16_distil_384": (dict(embed_dim=768, depth=12, num_heads=12, hybrid=False, distilled=True),
                           [96, 192, 384, 768], (2, 5, 8, 11)),
    "vitl16_384": (dict(embed_dim=1024, depth=24, num_heads=16, hybrid=False), [256, 512, 1024, 1024], (5, 11, 17, 23)),
    # BASELINE config 1 (plumbing): ViT-tiny/16 @224 assembled from the same parts
    "vit_tiny16_224": (dict(embed_dim=192, depth=12, num_heads=3, hybrid=False, img_size=224), [48, 96, 192, 192], (2, 5, 8, 11)),
}


class AttnPair(list):
    """[attn1, attn2] as the reference returns them, plus ``.stacked``: the (2B,L,T,T) tensor both are
    halves of, so the fused loss can skip the slice/concat round trip."""
    stacked = None


class BaseModel(nn.Module):
    def load(self, path):
        parameters = torch.load(path, map_location=torch.device("cpu"))
        if "optimizer" in parameters:
            parameters = parameters["model"]
        self.load_state_dict(parameters)


class DPT(BaseModel):
    def __init__(self, features=256, backbone="vitb_rn50_384", readout="ignore", channels_last=False, use_bn=False,
                 enable_attention_hooks=False, use_pretrain=True, use_attention=False, seg=False):
        super().__init__()
        if backbone not in _BACKBONES:
            print(f"Backbone '{backbone}' not implemented")
            assert False
        self.channels_last = channels_last
        self.attention = use_attention
        vit_kw, scratch_in, (tap1, tap2, tap3, tap4) = _BACKBONES[backbone]
        # NB use_pretrain: the reference downloads ImageNet weights here (models/helpers.py:177).  There is
        # no network in this build: weights are random-initialised and a checkpoint is loaded via `path`.
        vit = VisionTransformer(**vit_kw)
        vit.tap3, vit.tap4 = tap3, tap4
        if not vit_kw["hybrid"]:
            vit.tap1, vit.tap2 = tap1, tap2
        self.pretrained = nn.Module()
        self.pretrained.model = vit
        self.pretrained.activations = {}
        if backbone in ("vitl16_384", "deitb16_384", "deitb16_distil_384") or (seg and backbone == "vitb16_384"):
            # DPT/blocks.py:29-35,62-82 builds these three without `seg=seg`, so DPT/vit.py:263-341 (default seg=True) attaches
            # the four read-out heads to `pretrained` although the ACR forward never runs them: their 14 tensors are part of
            # every checkpoint of these backbones, and decoder.layers_rn runs them under seg=True (indices 3 / 4 of each
            # Sequential hold the parameters; 0-2 are the parameter-free read-out / transpose / unflatten steps).  vitb16_384
            # gets them under seg=True only (blocks.py:51-57).
            D, f = vit.embed_dim, scratch_in
            tails = ([nn.Conv2d(D, f[0], 1), nn.ConvTranspose2d(f[0], f[0], 4, stride=4)],
                     [nn.Conv2d(D, f[1], 1), nn.ConvTranspose2d(f[1], f[1], 2, stride=2)],
                     [nn.Conv2d(D, f[2], 1)],
                     [nn.Conv2d(D, f[3], 1), nn.Conv2d(f[3], f[3], 3, stride=2, padding=1)])
            for i, tail in enumerate(tails):
                setattr(self.pretrained, "act_postprocess%d" % (i + 1),
                        nn.Sequential(nn.Identity(), nn.Identity(), nn.Identity(), *tail))
        elif seg and backbone == "vitb_rn50_384":
            # DPT/vit.py:444-530: the hybrid's read-outs under seg=True -- taps 1 and 2 are stem stages (nothing to learn), taps 3
            # and 4 a 1x1 projection, tap 4 also the stride-2 3x3 that takes it to H/32.  decoder.layers_rn runs them.
            D, f = vit.embed_dim, scratch_in
            tails = ([], [], [nn.Conv2d(D, f[2], 1)], [nn.Conv2d(D, f[3], 1), nn.Conv2d(f[3], f[3], 3, stride=2, padding=1)])
            for i, tail in enumerate(tails):
                setattr(self.pretrained, "act_postprocess%d" % (i + 1),
                        nn.Sequential(nn.Identity(), nn.Identity(), nn.Identity(), *tail))
        self.scratch = nn.Module()                     # never used in the ACR forward (blocks.py:97-147); decoder.decode runs it
        for i, cin in enumerate(scratch_in):
            setattr(self.scratch, "layer%d_rn" % (i + 1), nn.Conv2d(cin, features, 3, 1, 1, bias=False))
        if seg:                                        # DPT/ACR.py:81-85: the fusion blocks (acr_wsss_amd/decoder.py)
            from ..decoder import make_fusion_block
            for i in (1, 2, 3, 4):
                setattr(self.scratch, "refinenet%d" % i, make_fusion_block(features, use_bn))
        self.cls_head = nn.Linear(vit.embed_dim, self.num_class)
        self.use_gap = True
        self.truncate_at = None                        # GETAM: stop the backward at this block (None = full)

    # -- encoder pass shared by forward_cls / forward_cam --
    def _encode(self, x):
        vit = self.pretrained.model
        if self.channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        b, _, h, w = x.shape
        T = (h // 16) * (w // 16) + vit.num_tokens
        # GETAM passes with a truncated backward: the gradient-free prefix is one hipGraph replay (backbone.PrefixGraph),
        # which owns the MeanStack its blocks write into
        prefix = vit.prefix_graph(x, self.truncate_at) if self.truncate_at else None
        stack = prefix.stack if prefix is not None else ops.MeanStack(b, vit.depth, T, x.device)
        taps = self.pretrained.activations
        taps.clear()
        vit.forward_flex(x, stack=stack, taps=taps, truncate_at=self.truncate_at, prefix=prefix)
        return taps["4"], stack

    def _stack_tensor(self, stack):
        """(B,L,T,T) autograd view of the head-mean buffer the attention kernels filled."""
        vit = self.pretrained.model
        pms = [blk.attn.last_pm for blk in vit.blocks]
        if any(pm is None for pm in pms) or not any(pm.requires_grad for pm in pms):
            return stack.buf
        return ops.StackAliasFn.apply(stack, *pms)

    def forward_cls(self, x):
        layer_4, stack = self._encode(x)
        x_cls = self.cls_head(layer_4[:, 0, :])
        # DPT/ACR.py:100-105 slices [:, 1:] for EVERY backbone -- also for the distilled DeiT, whose distillation token
        # therefore counts as a "patch" here (only getam skips it, :210-211); kept as is
        x_patch_cls = self.cls_head(layer_4[:, 1:, :].mean(dim=1))
        return x_cls, x_patch_cls, self._stack_tensor(stack), None

    def forward_cam(self, x):
        layer_4, stack = self._encode(x)
        x_patch = layer_4[:, 1:, :]                      # DPT/ACR.py:129: [:, 1:] for every backbone (see forward_cls)
        x_cls = self.cls_head(layer_4[:, 0, :])
        x_patch_cls = self.cls_head(x_patch.mean(dim=1))
        if x_patch.requires_grad and torch.is_grad_enabled():
            x_patch_cam = F.relu(self.cls_head(x_patch))
        else:                                           # inference read-out: HIP kernel (K5)
            B, N, D = x_patch.shape
            xp = x_patch.reshape(B * N, D) if x_patch.is_contiguous() else x_patch.contiguous().reshape(B * N, D)
            x_patch_cam = ops.patch_cam(xp, self.cls_head.weight.detach(), self.cls_head.bias.detach())
            x_patch_cam = x_patch_cam.reshape(B, N, -1)
        return x_cls, x_patch_cls, self._stack_tensor(stack), x_patch_cam


class ACR(DPT):
    def __init__(self, num_classes, backbone_name, path=None, math="f32", **kwargs):
        """Reference signature (DPT/ACR.py:148) plus ``math``: how this model's fp32 matrix products are evaluated
        ("f32" exact-fp32 MFMA = the reference's arithmetic, "f32_split" = bf16x3 split products, "f32_fp16x2" = opt-in,
        narrower fp16x2 products for the block Linears only; backbone.set_math)."""
        self.num_class = num_classes
        kwargs["use_bn"] = True
        backbone_dict = {"vitb_hybrid": "vitb_rn50_384", "vitb": "vitb16_384", "deit": "deitb16_384",
                         "deit_distilled": "deitb16_distil_384", "vitl": "vitl16_384", "vit_tiny": "vit_tiny16_224"}
        cur_backbone = backbone_dict[backbone_name]
        self.cur_backbone = cur_backbone
        super().__init__(backbone=cur_backbone, **kwargs)
        self.math = "f32"
        self.set_math(math)
        if path is not None:
            self.load(path)

    def set_math(self, math):
        """"f32" | "f32_split" | "f32_fp16x2" for the fp32 products of this model (a per-model property carried into each C-ABI
        call; "f32_fp16x2" changes the block Linears only and is never the default: backbone.set_math)."""
        from ..backbone import set_math
        from .._lib import MATH
        if math not in MATH:
            raise ValueError("math must be one of %s, got %r" % (sorted(MATH), math))
        set_math(self, math)
        self.math = math
        return self

    def late_gradient_parameters(self):
        """Parameters whose gradients arrive with the very last kernels of backward (the stem's convolutions below its last
        stage, backbone.ResNetV2.late_gradient_parameters): ``dp.GradSync(model.parameters(), late_params=...)`` gives them
        the last bucket to themselves."""
        out = []
        for m in self.modules():
            if m is not self and hasattr(m, "late_gradient_parameters"):
                out += m.late_gradient_parameters()
        return out

    def invalidate_caches(self):
        """After weights were written through ``.data`` (an EMA swap, ``p.data.copy_()``): drop everything derived from the
        weights, since its stamps cannot see such a write (_derived.py): weight images, W^T copies, the stem's frozen weights, the
        captured graphs.  All of it is rebuilt on demand (the W^T copies by the next ``train.refresh_weight_transposes``)."""
        _derived.invalidate(self)
        _derived.drop_graphs(self.modules())
        return self

    def forward_mirror(self, x1, x2):
        """DPT/ACR.py:170-174.  One 2B pass instead of two sequential B passes."""
        b = x1.shape[0]
        x_cls, x_p_cls, attn, _ = self.forward_cls(torch.cat([x1, x2], dim=0))
        pair = AttnPair([attn[:b], attn[b:]])
        pair.stacked = attn
        return [x_cls[:b], x_cls[b:], x_p_cls[:b], x_p_cls[b:], None, None], pair

    def getam(self, batch, start_layer=0, func="grad"):
        """DPT/ACR.py:177-215.  Returns (cls_cam (1,N), attn_list, cam_list) like the reference; cam_list holds
        the per-layer row-0 vectors (1,T) -- the only part of the reference's (1,T,T) maps that is consumed."""
        vit = self.pretrained.model
        rows, attn_list = [], []
        for i, blk in enumerate(vit.blocks):
            attn_list.append(blk.attn.last_pm)
            if i < start_layer:
                continue
            saved = blk.attn.saved_for_getam()
            if saved is None:
                raise RuntimeError("getam(): block %d has no saved forward/backward: call forward_cam + backward first, in eval() mode "
                                   "(a train()-mode forward keeps no attention state unless Attention.keep_state_in_training is set)" % i)
            qkv, d_o, lse2, heads = saved
            row = torch.zeros(qkv.shape[1], dtype=torch.float32, device=qkv.device)
            ops.getam_row_accum(qkv, d_o, lse2, heads, batch, func, row)
            rows.append(row.unsqueeze(0))
        cams = torch.stack(rows).sum(dim=0)
        skip = 2 if self.cur_backbone == "deitb16_distil_384" else 1
        return torch.relu(cams[:, skip:]), attn_list, rows

    def getam_all(self, start_layer=0, func="grad"):
        """``getam`` for EVERY sample of the last forward_cam / backward pair at once: (B, N) class CAM rows, row b equal to
        ``getam(b, start_layer, func)[0]`` up to the order of the fp32 layer sum (one launch per layer for the whole batch,
        accumulated in the kernel, instead of one launch per sample and layer plus a stack + sum: CAM generation batches the
        flipped and the plain pass and several images)."""
        vit = self.pretrained.model
        rows = None
        for i, blk in enumerate(vit.blocks):
            if i < start_layer:
                continue
            saved = blk.attn.saved_for_getam()
            if saved is None:
                raise RuntimeError("getam_all(): block %d has no saved forward/backward: call forward_cam + backward first, in eval() "
                                   "mode (a train()-mode forward keeps no attention state unless Attention.keep_state_in_training is set)" % i)
            qkv, d_o, lse2, heads = saved
            if rows is None:
                rows = torch.zeros((qkv.shape[0], qkv.shape[1]), dtype=torch.float32, device=qkv.device)
            ops.getam_rows_accum(qkv, d_o, lse2, heads, func, rows)
        skip = 2 if self.cur_backbone == "deitb16_distil_384" else 1
        return torch.relu(rows[:, skip:])
