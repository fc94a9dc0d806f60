"""PyTorch custom operators (namespace `cvlite`, torch.library) over the C ABI, with autograd.

SURVEY.md §8b's torch custom-op layer: the kernels behind include/cvlite.h as dispatcher ops that
run on the current HIP stream, so a PyTorch user can call them like built-in ops and take
gradients through them (the reference's `tf.GradientTape` usage, FCOS/train_fcos.py:152-174):

  torch.ops.cvlite.conv2d_nhwc(x, w, b, stride, pad)      Keras Conv2D forward (TF 'same' / valid /
                                                          explicit pad), NHWC bf16, HWIO fp32
                                                          master weights; autograd = the dgrad /
                                                          wgrad / bias-grad kernels
  torch.ops.cvlite.group_conv3x3_nhwc(x, w, stride)       grouped 3x3 conv (pad 1), w [3,3,Cg,C]
                                                          fp32 (the ResNeXt bottleneck); autograd =
                                                          the grouped dgrad / wgrad kernels
  torch.ops.cvlite.fcos_assign(boxes, nbox, img_dim, pad_h, pad_w, C)   fcos.format_data, batched
  torch.ops.cvlite.fcos_loss(reg, cls, targets, C, reg_type)  fcos.model_loss per image
                                                          [B, 3] = (cls, reg, cen); autograd = the
                                                          fused kernel's gradients scaled by the
                                                          upstream per-image, per-term gradients
  torch.ops.cvlite.fcos_paper_assign(boxes, nbox, img_dim, pad_h, pad_w, C, center_radius),
  torch.ops.cvlite.fcos_target_norm(targets, C),
  torch.ops.cvlite.fcos_paper_loss(reg, cls, targets, norm, C)  the FCOS papers' recipe (cvlite
                                                          extension); the loss has autograd as fcos_loss
  torch.ops.cvlite.fcos_atss_assign(boxes, nbox, img_dim, pad_h, pad_w, C, topk, anchor_scale)
                                                          ATSS targets (cvlite extension) for the
                                                          same fcos_target_norm / fcos_paper_loss
  torch.ops.cvlite.fcos_gfl_norm(cls, targets, C),
  torch.ops.cvlite.fcos_gfl_loss(reg, cls, targets, norm, C, reg_max, beta, box_weight, dfl_weight),
  torch.ops.cvlite.fcos_gfl_decode(reg, reg_max)          Generalized Focal Loss on a distribution box
                                                          head (cvlite extension): [B, 3] = (qfl, box,
                                                          dfl) with autograd as fcos_loss, and the
                                                          expected distances for inference
  torch.ops.cvlite.fcos_tal_assign(boxes, nbox, img_dim, pad_h, pad_w, C, dist, cls, topk, alpha, beta, clamp),
  torch.ops.cvlite.fcos_tal_loss(reg, cls, targets, norm, C, beta, box_weight)
                                                          task-aligned assignment from the head outputs
                                                          (cvlite extension) and its loss: [B, 3] = (cls,
                                                          box, 0) with autograd as fcos_loss
  torch.ops.cvlite.retina_atss_assign(boxes, nbox, img_dim, pad, anchor_dims, C, topk),
  torch.ops.cvlite.retina_atss_loss(reg, cls, targets, num_targets, img_weight, A, C)
                                                          ATSS for RetinaNet (cvlite extension): compact
                                                          targets [B, P, A, 8] and [B, 2] = (cls, reg) per
                                                          image / its positive anchors, with autograd
  torch.ops.cvlite.centernet_gauss_assign(boxes, nbox, img_dim, pad_h, pad_w, C, stride, min_overlap),
  torch.ops.cvlite.centernet_gauss_loss(pred, targets, npos, C, alpha, beta)
                                                          CenterNet as "Objects as Points" trains it (cvlite
                                                          extension): Gaussian heat maps [B, H/s, W/s, 4+C] with
                                                          their object counts [B], and [B, 2] = (cls, reg) per
                                                          image / its objects, with autograd on pred
  torch.ops.cvlite.augment_images(images, table, ph, pw)  batched training augmentation (cvlite extension;
                                                          cvlite/augment.py): B decoded images of any sizes
                                                          and their host descriptor table -> [B, ph, pw, 3]
                                                          fp32 in one launch
  torch.ops.cvlite.retina_assign(...) / centernet_splat(...)  RetinaNet / CenterNet targets
  torch.ops.cvlite.sgd_clip_(w, g, v, lr, momentum, inv_bs, clip)  clip_by_global_norm + Keras
                                                          SGD momentum, in place

`NetFunction` makes a whole cvlite network one autograd node: forward = the network's explicit
forward (training-mode BN), backward = its explicit backward (the same kernels FCOSTrainer runs,
so the parameter gradients are bit-identical to the trainer's gradient buffer); the parameters
are its inputs, so torch.autograd.grad(loss, model.trainable_variables) works.
"""
from typing import List, Optional, Tuple

import torch

from . import ops_nn as nn
from . import ops_targets as ot
from .layers import same_pad

BF16 = torch.bfloat16


def _geometry(H, W, k, stride, pad):
    if pad == "same":
        (Ho, pt), (Wo, pl) = same_pad(H, k, stride), same_pad(W, k, stride)
    elif pad == "valid":
        Ho, Wo, pt, pl = (H - k) // stride + 1, (W - k) // stride + 1, 0, 0
    else:
        p = int(pad)
        Ho, Wo, pt, pl = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1, p, p
    return Ho, Wo, pt, pl


def _pad32(n):
    return max(32, (n + 31) // 32 * 32)


def _packs(w, need_dgrad):
    k, _, cin, cout = (int(s) for s in w.shape)
    npad = _pad32(cout)
    wf = torch.empty((npad, k * k * cin), dtype=BF16, device=w.device)
    wd = torch.empty((_pad32(cin), k * k * npad), dtype=BF16, device=w.device) if need_dgrad else None
    nn.pack_conv_weights(w.contiguous(), k, k, cin, cout, cin, npad, wf, _pad32(cin) if need_dgrad else 0,
                         npad if need_dgrad else 0, wd)
    return wf, wd, npad


# ---- conv2d_nhwc --------------------------------------------------------------------------------
@torch.library.custom_op("cvlite::conv2d_nhwc", mutates_args=(), device_types="cuda")
def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], stride: int, pad: str) -> torch.Tensor:
    """x [B,H,W,Cin] bf16 (Cin % 32 == 0), w [k,k,Cin,Cout] fp32 HWIO (Cout % 8 == 0), b [Cout] or
    None -> [B,Ho,Wo,Cout] bf16 (fp32 accumulation, one rounding)."""
    B, H, W, cin = (int(s) for s in x.shape)
    k, cout = int(w.shape[0]), int(w.shape[3])
    Ho, Wo, pt, pl = _geometry(H, W, k, stride, pad)
    wf, _, npad = _packs(w, False)
    out = torch.empty((B, Ho, Wo, cout), dtype=BF16, device=x.device)
    d = nn.make_desc(nn.FWD, B, cin, k, k, stride, pt, pl, npad, cout, cout,
                     [nn.seg(Ho, Wo, H, W, wf, None if b is None else b.contiguous())])
    nn.conv_igemm(d, x.contiguous(), out)
    return out


@conv2d_nhwc.register_fake
def _(x, w, b, stride, pad):
    B, H, W, _ = x.shape
    Ho, Wo, _, _ = _geometry(int(H), int(W), int(w.shape[0]), stride, pad)
    return x.new_empty((B, Ho, Wo, w.shape[3]), dtype=BF16)


def _conv_setup(ctx, inputs, output):
    x, w, b, stride, pad = inputs
    ctx.save_for_backward(x, w)
    ctx.has_bias = b is not None
    ctx.stride, ctx.pad = stride, pad


def _conv_backward(ctx, gy):
    x, w = ctx.saved_tensors
    B, H, W, cin = (int(s) for s in x.shape)
    k, cout = int(w.shape[0]), int(w.shape[3])
    Ho, Wo, pt, pl = _geometry(H, W, k, ctx.stride, ctx.pad)
    wf, wd, npad = _packs(w, True)
    g = torch.zeros((B, Ho, Wo, npad), dtype=BF16, device=x.device)
    g[..., :cout] = gy.to(BF16)
    dx = dw = db = None
    if ctx.needs_input_grad[0]:
        dx = torch.empty_like(x)
        d = nn.make_desc(nn.DGRAD, B, npad, k, k, ctx.stride, pt, pl, _pad32(cin), cin, cin,
                         [nn.seg(H, W, Ho, Wo, wd)])
        nn.conv_igemm(d, g, dx)
    if ctx.needs_input_grad[1]:
        dw = torch.zeros((k, k, cin, cout), dtype=torch.float32, device=x.device)
        d = nn.make_desc(nn.FWD, B, cin, k, k, ctx.stride, pt, pl, npad, cout, npad, [nn.seg(Ho, Wo, H, W, wf)])
        nn.conv_wgrad(d, x.contiguous(), g, dw)
    if ctx.has_bias and ctx.needs_input_grad[2]:
        db = torch.zeros((cout,), dtype=torch.float32, device=x.device)
        nn.bias_grad(g, npad, 0, cout, 0, Ho * Wo, Ho * Wo, B, db)
    return dx, dw, db, None, None


conv2d_nhwc.register_autograd(_conv_backward, setup_context=_conv_setup)


# ---- group_conv3x3_nhwc -----------------------------------------------------------------------------
@torch.library.custom_op("cvlite::group_conv3x3_nhwc", mutates_args=(), device_types="cuda")
def group_conv3x3_nhwc(x: torch.Tensor, w: torch.Tensor, stride: int) -> torch.Tensor:
    """x [B,H,W,C] bf16 (C % 32 == 0), w [3,3,Cg,C] fp32 (Cg in 4/8/16/32; output channel o reads the
    input channels of group o // Cg), ZeroPadding2D(1) + valid, stride 1 or 2 -> [B,Ho,Wo,C] bf16."""
    B, H, W, C = (int(s) for s in x.shape)
    wf = nn.gconv3x3_packed(C, x.device)
    nn.gconv3x3_pack(w.contiguous(), wf, None)
    out = torch.empty((B, (H - 1) // stride + 1, (W - 1) // stride + 1, C), dtype=BF16, device=x.device)
    nn.gconv3x3_fwd(x.contiguous(), wf, out, int(w.shape[2]), stride)
    return out


@group_conv3x3_nhwc.register_fake
def _(x, w, stride):
    B, H, W, C = x.shape
    return x.new_empty((B, (H - 1) // stride + 1, (W - 1) // stride + 1, C), dtype=BF16)


def _gconv_setup(ctx, inputs, output):
    x, w, stride = inputs
    ctx.save_for_backward(x, w)
    ctx.stride = stride


def _gconv_backward(ctx, gy):
    x, w = ctx.saved_tensors
    g = gy.to(BF16).contiguous()
    dx = dw = None
    if ctx.needs_input_grad[0]:
        wd = nn.gconv3x3_packed(int(x.shape[3]), x.device)
        nn.gconv3x3_pack(w.contiguous(), None, wd)
        dx = torch.empty_like(x, memory_format=torch.contiguous_format)
        nn.gconv3x3_dgrad(g, wd, dx, int(w.shape[2]), ctx.stride)
    if ctx.needs_input_grad[1]:
        dw = torch.empty(tuple(w.shape), dtype=torch.float32, device=x.device)
        nn.gconv3x3_wgrad(x.contiguous(), g, dw, ctx.stride)
    return dx, dw, None


group_conv3x3_nhwc.register_autograd(_gconv_backward, setup_context=_gconv_setup)


# ---- targets ------------------------------------------------------------------------------------
@torch.library.custom_op("cvlite::fcos_assign", mutates_args=(), device_types="cuda")
def fcos_assign(boxes: torch.Tensor, nbox: torch.Tensor, img_dim: torch.Tensor, pad_h: int, pad_w: int,
                num_classes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fcos.format_data for a batch: boxes [B,N,5] (yc,xc,h,w,cls), nbox [B] i32, img_dim [B,2]
    -> (targets [B,P,5+C] fp32 level-major, num_targets [B,5] i32)."""
    return ot.fcos_assign(boxes.contiguous(), nbox.contiguous(), img_dim.contiguous(), (pad_h, pad_w), num_classes)


@fcos_assign.register_fake
def _(boxes, nbox, img_dim, pad_h, pad_w, num_classes):
    P = sum(h * w for h, w in ot.fcos_level_shapes(pad_h, pad_w))
    B = boxes.shape[0]
    return boxes.new_empty((B, P, 5 + num_classes)), nbox.new_empty((B, 5))


@torch.library.custom_op("cvlite::retina_assign", mutates_args=(), device_types="cuda")
def retina_assign(boxes: torch.Tensor, nbox: torch.Tensor, img_dim: torch.Tensor, pad: int,
                  anchor_dims: torch.Tensor, num_classes: int, iou_thresh: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """RetinaNet.format_data for a batch -> (targets [B, A*sum S^2, 4+C], num_targets [B])."""
    return ot.retina_assign(boxes.contiguous(), nbox.contiguous(), img_dim.contiguous(), pad, anchor_dims,
                            num_classes, iou_thresh)


@retina_assign.register_fake
def _(boxes, nbox, img_dim, pad, anchor_dims, num_classes, iou_thresh):
    A = anchor_dims.shape[1]
    P = sum(A * (pad // s) ** 2 for s in ot.RETINA_STRIDES)
    return boxes.new_empty((boxes.shape[0], P, 4 + num_classes)), nbox.new_empty((boxes.shape[0],))


@torch.library.custom_op("cvlite::centernet_splat", mutates_args=(), device_types="cuda")
def centernet_splat(boxes: torch.Tensor, nbox: torch.Tensor, img_dim: torch.Tensor, pad_h: int, pad_w: int,
                    num_classes: int, stride: int, sigma: float) -> torch.Tensor:
    """tf_centernet.format_data (heatmap splat) for a batch -> [B, pad_h/s, pad_w/s, 5+C]."""
    return ot.centernet_splat(boxes.contiguous(), nbox.contiguous(), img_dim.contiguous(), (pad_h, pad_w),
                              num_classes, stride, sigma)


@centernet_splat.register_fake
def _(boxes, nbox, img_dim, pad_h, pad_w, num_classes, stride, sigma):
    return boxes.new_empty((boxes.shape[0], pad_h // stride, pad_w // stride, 5 + num_classes))


# ---- fused FCOS loss ------------------------------------------------------------------------------
@torch.library.custom_op("cvlite::fcos_loss", mutates_args=(), device_types="cuda")
def fcos_loss(reg: torch.Tensor, cls: torch.Tensor, targets: torch.Tensor, num_classes: int,
              reg_type: int) -> torch.Tensor:
    """fcos.model_loss per image: reg [B,P,>=5] fp32, cls [B,P,>=C] fp32, targets [B,P,5+C]
    -> [B,3] = (cls, reg, cen) (reg_type: cvl_fcos_loss flags, 0 = smooth-L1, 1 = IoU, +4 focal
    centerness, +8 sigmoid reg)."""
    losses, _, _ = ot.fcos_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), num_classes,
                                reg_type=int(reg_type), with_grad=False)
    return losses


@fcos_loss.register_fake
def _(reg, cls, targets, num_classes, reg_type):
    return reg.new_empty((reg.shape[0], 3))


def _loss_setup(ctx, inputs, output):
    reg, cls, targets, C, reg_type = inputs
    ctx.save_for_backward(reg, cls, targets)
    ctx.C, ctx.reg_type = C, reg_type


def _loss_backward(ctx, g):
    reg, cls, targets = ctx.saved_tensors
    _, d_reg, d_cls = ot.fcos_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), ctx.C,
                                   reg_type=int(ctx.reg_type), grad_scale=1.0)
    g = g.to(torch.float32)
    # cls term -> class logits; reg term -> ltrb channels 0..3; centerness term -> channel 4;
    # padding channels get exactly zero
    cscale = torch.zeros((reg.shape[0], 1, cls.shape[2]), dtype=torch.float32, device=reg.device)
    cscale[:, 0, :ctx.C] = g[:, 0:1]
    rscale = torch.zeros((reg.shape[0], 1, reg.shape[2]), dtype=torch.float32, device=reg.device)
    rscale[:, 0, :4] = g[:, 1:2]
    rscale[:, 0, 4] = g[:, 2]
    return d_reg * rscale, d_cls * cscale, None, None, None


fcos_loss.register_autograd(_loss_backward, setup_context=_loss_setup)


# ---- the FCOS papers' recipe (cvlite extension) ----------------------------------------------------
@torch.library.custom_op("cvlite::fcos_paper_assign", mutates_args=(), device_types="cuda")
def fcos_paper_assign(boxes: torch.Tensor, nbox: torch.Tensor, img_dim: torch.Tensor, pad_h: int, pad_w: int,
                      num_classes: int, center_radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Targets of the FCOS papers (regress ranges (64, 128, 256, 512), centre sampling, smallest area)
    -> (targets [B,P,5+C] fp32 level-major, positive cells per level [B,5] i32)."""
    return ot.fcos_paper_assign(boxes.contiguous(), nbox.contiguous(), img_dim.contiguous(), (pad_h, pad_w),
                                num_classes, center_radius=center_radius)


@fcos_paper_assign.register_fake
def _(boxes, nbox, img_dim, pad_h, pad_w, num_classes, center_radius):
    P = sum(h * w for h, w in ot.fcos_level_shapes(pad_h, pad_w))
    B = boxes.shape[0]
    return boxes.new_empty((B, P, 5 + num_classes)), nbox.new_empty((B, 5))


@torch.library.custom_op("cvlite::fcos_atss_assign", mutates_args=(), device_types="cuda")
def fcos_atss_assign(boxes: torch.Tensor, nbox: torch.Tensor, img_dim: torch.Tensor, pad_h: int, pad_w: int,
                     num_classes: int, topk: int, anchor_scale: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """ATSS targets (the topk nearest grid points per level, IoU threshold mean + std per box, largest
    IoU per cell) -> (targets [B,P,5+C] fp32 level-major, positive cells per level [B,5] i32); the
    loss op is fcos_paper_loss."""
    return ot.fcos_atss_assign(boxes.contiguous(), nbox.contiguous(), img_dim.contiguous(), (pad_h, pad_w),
                               num_classes, topk=topk, anchor_scale=anchor_scale)


@fcos_atss_assign.register_fake
def _(boxes, nbox, img_dim, pad_h, pad_w, num_classes, topk, anchor_scale):
    P = sum(h * w for h, w in ot.fcos_level_shapes(pad_h, pad_w))
    B = boxes.shape[0]
    return boxes.new_empty((B, P, 5 + num_classes)), nbox.new_empty((B, 5))


@torch.library.custom_op("cvlite::fcos_target_norm", mutates_args=(), device_types="cuda")
def fcos_target_norm(targets: torch.Tensor, num_classes: int) -> torch.Tensor:
    """targets [B,P,5+C] -> [B,2] = (number of positive cells, sum of their centerness targets)."""
    return ot.fcos_target_norm(targets.contiguous(), num_classes)


@fcos_target_norm.register_fake
def _(targets, num_classes):
    return targets.new_empty((targets.shape[0], 2))


@torch.library.custom_op("cvlite::fcos_paper_loss", mutates_args=(), device_types="cuda")
def fcos_paper_loss(reg: torch.Tensor, cls: torch.Tensor, targets: torch.Tensor, norm: Optional[torch.Tensor],
                    num_classes: int) -> torch.Tensor:
    """Loss of the FCOS papers per image: reg [B,P,>=5] fp32, cls [B,P,>=C] fp32, targets [B,P,5+C],
    norm [B,2] from fcos_target_norm (None: plain sums) -> [B,3] = (cls, reg, cen)."""
    losses, _, _ = ot.fcos_paper_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), num_classes,
                                      norm=None if norm is None else norm.contiguous(), with_grad=False)
    return losses


@fcos_paper_loss.register_fake
def _(reg, cls, targets, norm, num_classes):
    return reg.new_empty((reg.shape[0], 3))


def _paper_loss_setup(ctx, inputs, output):
    reg, cls, targets, norm, C = inputs
    ctx.save_for_backward(reg, cls, targets, norm)
    ctx.C = C


def _paper_loss_backward(ctx, g):
    reg, cls, targets, norm = ctx.saved_tensors
    _, d_reg, d_cls = ot.fcos_paper_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), ctx.C,
                                         norm=None if norm is None else norm.contiguous(), grad_scale=1.0)
    g = g.to(torch.float32)
    # cls term -> class logits; reg term -> ltrb channels 0..3; centerness term -> channel 4;
    # padding channels get exactly zero
    cscale = torch.zeros((reg.shape[0], 1, cls.shape[2]), dtype=torch.float32, device=reg.device)
    cscale[:, 0, :ctx.C] = g[:, 0:1]
    rscale = torch.zeros((reg.shape[0], 1, reg.shape[2]), dtype=torch.float32, device=reg.device)
    rscale[:, 0, :4] = g[:, 1:2]
    rscale[:, 0, 4] = g[:, 2]
    return d_reg * rscale, d_cls * cscale, None, None, None


fcos_paper_loss.register_autograd(_paper_loss_backward, setup_context=_paper_loss_setup)


# ---- ATSS for RetinaNet (cvlite extension) ------------------------------------------------------------
@torch.library.custom_op("cvlite::retina_atss_assign", mutates_args=(), device_types="cuda")
def retina_atss_assign(boxes: torch.Tensor, nbox: torch.Tensor, img_dim: torch.Tensor, pad: int,
                       anchor_dims: torch.Tensor, num_classes: int, topk: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """ATSS targets for RetinaNet (the topk nearest anchors per level, IoU threshold mean + std per box,
    largest IoU per anchor) -> (compact targets [B,P,A,8] fp32 in the head outputs' row order, positive
    anchors per level [B,5] i32); the loss op is retina_atss_loss."""
    return ot.retina_atss_assign(boxes.contiguous(), nbox.contiguous(), img_dim.contiguous(), pad,
                                 anchor_dims.contiguous(), num_classes, topk=topk)


@retina_atss_assign.register_fake
def _(boxes, nbox, img_dim, pad, anchor_dims, num_classes, topk):
    A = anchor_dims.shape[1]
    P = sum((pad // s) ** 2 for s in ot.RETINA_STRIDES)
    B = boxes.shape[0]
    return boxes.new_empty((B, P, A, 8)), nbox.new_empty((B, 5))


@torch.library.custom_op("cvlite::retina_atss_loss", mutates_args=(), device_types="cuda")
def retina_atss_loss(reg: torch.Tensor, cls: torch.Tensor, targets: torch.Tensor, num_targets: torch.Tensor,
                     img_weight: Optional[torch.Tensor], n_anchors: int, num_classes: int, alpha: float = 0.25,
                     gamma: float = 2.0) -> torch.Tensor:
    """Normalised RetinaNet loss per image: reg [B,P,>=4A] fp32, cls [B,P,>=A*C] fp32, targets [B,P,A,8]
    and num_targets [B,5] from retina_atss_assign, img_weight [B] or None -> [B,2] = (cls, reg)."""
    return ot.retina_atss_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), num_targets.contiguous(),
                               n_anchors, num_classes, img_weight=None if img_weight is None else img_weight.contiguous(),
                               alpha=alpha, gamma=gamma)


@retina_atss_loss.register_fake
def _(reg, cls, targets, num_targets, img_weight, n_anchors, num_classes, alpha=0.25, gamma=2.0):
    return reg.new_empty((reg.shape[0], 2))


def _retina_atss_loss_setup(ctx, inputs, output):
    reg, cls, targets, num_targets, img_weight, A, C, alpha, gamma = inputs
    ctx.save_for_backward(reg, cls, targets, num_targets, img_weight)
    ctx.args = (A, C, alpha, gamma)


def _retina_atss_loss_backward(ctx, g):
    reg, cls, targets, num_targets, img_weight = ctx.saved_tensors
    A, C, alpha, gamma = ctx.args
    # the kernel writes only the anchors' channels: the padding channels stay exactly zero
    d_reg = torch.zeros_like(reg, memory_format=torch.contiguous_format)
    d_cls = torch.zeros_like(cls, memory_format=torch.contiguous_format)
    ot.retina_atss_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), num_targets.contiguous(), A, C,
                        img_weight=None if img_weight is None else img_weight.contiguous(), alpha=alpha, gamma=gamma,
                        grad_scale=1.0, d_reg=d_reg, d_cls=d_cls)
    g = g.to(torch.float32)
    # cls term -> class logits, reg term -> box outputs
    return d_reg * g[:, 1].view(-1, 1, 1), d_cls * g[:, 0].view(-1, 1, 1), None, None, None, None, None, None, None


retina_atss_loss.register_autograd(_retina_atss_loss_backward, setup_context=_retina_atss_loss_setup)


# ---- Generalized Focal Loss (cvlite extension) --------------------------------------------------------
@torch.library.custom_op("cvlite::fcos_gfl_norm", mutates_args=(), device_types="cuda")
def fcos_gfl_norm(cls: torch.Tensor, targets: torch.Tensor, num_classes: int) -> torch.Tensor:
    """cls [B,P,>=C] fp32, targets [B,P,5+C] -> [B,2] = (number of positive cells, sum over them of
    sigmoid(max class logit)).  No gradient flows through it (the loss treats its divisors as constants)."""
    return ot.fcos_gfl_norm(cls.contiguous(), targets.contiguous(), num_classes)


@fcos_gfl_norm.register_fake
def _(cls, targets, num_classes):
    return targets.new_empty((targets.shape[0], 2))


@torch.library.custom_op("cvlite::fcos_gfl_loss", mutates_args=(), device_types="cuda")
def fcos_gfl_loss(reg: torch.Tensor, cls: torch.Tensor, targets: torch.Tensor, norm: Optional[torch.Tensor],
                  num_classes: int, reg_max: int, beta: float = 2.0, box_weight: float = 2.0,
                  dfl_weight: float = 0.25) -> torch.Tensor:
    """Generalized Focal Loss per image: reg [B,P,>=4(reg_max+1)] fp32, cls [B,P,>=C] fp32, targets
    [B,P,5+C], norm [B,2] from fcos_gfl_norm (None: plain sums) -> [B,3] = (qfl, box, dfl)."""
    losses, _, _ = ot.fcos_gfl_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), num_classes, reg_max,
                                    norm=None if norm is None else norm.contiguous(), with_grad=False, beta=beta,
                                    box_weight=box_weight, dfl_weight=dfl_weight)
    return losses


@fcos_gfl_loss.register_fake
def _(reg, cls, targets, norm, num_classes, reg_max, beta=2.0, box_weight=2.0, dfl_weight=0.25):
    return reg.new_empty((reg.shape[0], 3))


def _gfl_loss_setup(ctx, inputs, output):
    reg, cls, targets, norm, C, R, beta, wb, wd = inputs
    ctx.save_for_backward(reg, cls, targets, norm)
    ctx.args = (C, R, beta, wb, wd)


def _gfl_loss_backward(ctx, g):
    reg, cls, targets, norm = ctx.saved_tensors
    C, R, beta, wb, wd = ctx.args
    g = g.to(torch.float32)
    run = lambda b, d: ot.fcos_gfl_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), C, R,  # noqa: E731
                                        norm=None if norm is None else norm.contiguous(), grad_scale=1.0,
                                        beta=beta, box_weight=b, dfl_weight=d)
    # the kernel returns d(qfl + box + dfl); the box rows are linear in the two weights, so one call per
    # term separates them: qfl -> class logits, box and dfl -> the distributions; padding columns get zero
    _, d_box, d_cls = run(wb, 0.0)
    _, d_dfl, _ = run(0.0, wd)
    cscale = torch.zeros((reg.shape[0], 1, cls.shape[2]), dtype=torch.float32, device=reg.device)
    cscale[:, 0, :C] = g[:, 0:1]
    d_reg = d_box * g[:, 1].view(-1, 1, 1) + d_dfl * g[:, 2].view(-1, 1, 1)
    return d_reg, d_cls * cscale, None, None, None, None, None, None, None


fcos_gfl_loss.register_autograd(_gfl_loss_backward, setup_context=_gfl_loss_setup)


@torch.library.custom_op("cvlite::fcos_gfl_decode", mutates_args=(), device_types="cuda")
def fcos_gfl_decode(reg: torch.Tensor, reg_max: int) -> torch.Tensor:
    """reg [B,P,>=4(reg_max+1)] fp32 -> [B,P,8] fp32: columns 0..3 the expected (top, bottom, left, right)
    distances in stride units, columns 4..7 zero (inference; no gradient)."""
    return ot.fcos_gfl_decode(reg.contiguous(), reg_max)


@fcos_gfl_decode.register_fake
def _(reg, reg_max):
    return reg.new_empty(tuple(reg.shape[:-1]) + (8,))


# ---- task-aligned assignment and its loss (cvlite extension) ------------------------------------------
@torch.library.custom_op("cvlite::fcos_tal_assign", mutates_args=(), device_types="cuda")
def fcos_tal_assign(boxes: torch.Tensor, nbox: torch.Tensor, img_dim: torch.Tensor, pad_h: int, pad_w: int,
                    num_classes: int, dist: torch.Tensor, cls: torch.Tensor, topk: int = 13, alpha: float = 1.0,
                    beta: float = 6.0, clamp: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Task-aligned targets from the head outputs (dist [B,P,>=4] fp32 distances in stride units, clamped
    at 0 when `clamp`; cls [B,P,>=C] fp32 logits) -> (targets [B,P,5+C] fp32 level-major with the
    alignment value in slot 4, positive cells per level [B,5] i32); the loss op is fcos_tal_loss.  No
    gradient flows through it (the targets are constants for the loss)."""
    return ot.fcos_tal_assign(boxes.contiguous(), nbox.contiguous(), img_dim.contiguous(), (pad_h, pad_w),
                              num_classes, dist.contiguous(), cls.contiguous(), topk=topk, alpha=alpha, beta=beta,
                              clamp=clamp)


@fcos_tal_assign.register_fake
def _(boxes, nbox, img_dim, pad_h, pad_w, num_classes, dist, cls, topk=13, alpha=1.0, beta=6.0, clamp=True):
    P = sum(h * w for h, w in ot.fcos_level_shapes(pad_h, pad_w))
    B = boxes.shape[0]
    return boxes.new_empty((B, P, 5 + num_classes)), nbox.new_empty((B, 5))


@torch.library.custom_op("cvlite::fcos_tal_loss", mutates_args=(), device_types="cuda")
def fcos_tal_loss(reg: torch.Tensor, cls: torch.Tensor, targets: torch.Tensor, norm: Optional[torch.Tensor],
                  num_classes: int, beta: float = 2.0, box_weight: float = 2.0) -> torch.Tensor:
    """Loss on task-aligned targets per image: reg [B,P,>=5] fp32, cls [B,P,>=C] fp32, targets [B,P,5+C],
    norm [B,2] from fcos_target_norm (None: plain sums) -> [B,3] = (cls, box, 0)."""
    losses, _, _ = ot.fcos_tal_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), num_classes,
                                    norm=None if norm is None else norm.contiguous(), with_grad=False, beta=beta,
                                    box_weight=box_weight)
    return losses


@fcos_tal_loss.register_fake
def _(reg, cls, targets, norm, num_classes, beta=2.0, box_weight=2.0):
    return reg.new_empty((reg.shape[0], 3))


def _tal_loss_setup(ctx, inputs, output):
    reg, cls, targets, norm, C, beta, wb = inputs
    ctx.save_for_backward(reg, cls, targets, norm)
    ctx.args = (C, beta, wb)


def _tal_loss_backward(ctx, g):
    reg, cls, targets, norm = ctx.saved_tensors
    C, beta, wb = ctx.args
    _, d_reg, d_cls = ot.fcos_tal_loss(reg.contiguous(), cls.contiguous(), targets.contiguous(), C,
                                       norm=None if norm is None else norm.contiguous(), grad_scale=1.0, beta=beta,
                                       box_weight=wb)
    g = g.to(torch.float32)
    # cls term -> class logits, box term -> the box outputs (columns 4.. are zero already); the padding
    # columns get exactly zero
    cscale = torch.zeros((reg.shape[0], 1, cls.shape[2]), dtype=torch.float32, device=reg.device)
    cscale[:, 0, :C] = g[:, 0:1]
    return d_reg * g[:, 1].view(-1, 1, 1), d_cls * cscale, None, None, None, None, None


fcos_tal_loss.register_autograd(_tal_loss_backward, setup_context=_tal_loss_setup)


# ---- CenterNet Gaussian targets and penalty-reduced focal loss (cvlite extension) ---------------------
@torch.library.custom_op("cvlite::centernet_gauss_assign", mutates_args=(), device_types="cuda")
def centernet_gauss_assign(boxes: torch.Tensor, nbox: torch.Tensor, img_dim: torch.Tensor, pad_h: int, pad_w: int,
                           num_classes: int, stride: int = 4,
                           min_overlap: float = 0.7) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gaussian-heatmap CenterNet targets for a batch -> (targets [B, pad_h/s, pad_w/s, 4+C] fp32, npos [B]
    i32 = the (cell, class) entries equal to 1.0, the divisor of centernet_gauss_loss)."""
    t = ot.centernet_gauss_assign(boxes.contiguous(), nbox.contiguous(), img_dim.contiguous(), (pad_h, pad_w),
                                  num_classes, stride=stride, min_overlap=min_overlap)
    return t, ot.centernet_gauss_norm(t, num_classes)


@centernet_gauss_assign.register_fake
def _(boxes, nbox, img_dim, pad_h, pad_w, num_classes, stride=4, min_overlap=0.7):
    B = boxes.shape[0]
    return boxes.new_empty((B, pad_h // stride, pad_w // stride, 4 + num_classes)), nbox.new_empty((B,))


def _gauss_rows(pred, targets, num_classes):
    B = int(targets.shape[0])
    return (pred.contiguous().view(B, -1, pred.shape[-1]),
            targets.contiguous().view(B, -1, 4 + num_classes))


@torch.library.custom_op("cvlite::centernet_gauss_loss", mutates_args=(), device_types="cuda")
def centernet_gauss_loss(pred: torch.Tensor, targets: torch.Tensor, npos: torch.Tensor, num_classes: int,
                         alpha: float = 2.0, beta: float = 4.0) -> torch.Tensor:
    """Penalty-reduced focal loss + L1 on the centres per image: pred [B,...,>=4+C] fp32 (box 0..3, class
    logits 4..), targets [B,...,4+C], npos [B] i32 -> [B,2] = (cls, reg), each divided by max(npos, 1)."""
    p, t = _gauss_rows(pred, targets, num_classes)
    losses, _ = ot.centernet_gauss_loss(p, t, npos.contiguous(), num_classes, alpha=alpha, beta=beta)
    return losses


@centernet_gauss_loss.register_fake
def _(pred, targets, npos, num_classes, alpha=2.0, beta=4.0):
    return pred.new_empty((pred.shape[0], 2))


def _gauss_loss_setup(ctx, inputs, output):
    pred, targets, npos, C, alpha, beta = inputs
    ctx.save_for_backward(pred, targets, npos)
    ctx.args = (C, alpha, beta)


def _gauss_loss_backward(ctx, g):
    pred, targets, npos = ctx.saved_tensors
    C, alpha, beta = ctx.args
    p, t = _gauss_rows(pred, targets, C)
    ld = int(p.shape[-1])
    d = torch.empty((p.shape[0], p.shape[1], (ld + 7) // 8 * 8), dtype=BF16, device=p.device)
    ot.centernet_gauss_loss(p, t, npos.contiguous(), C, alpha=alpha, beta=beta, d_pred=d)
    g = g.to(torch.float32)
    # the kernel's gradient is bf16 (the output conv's backward operand); cls term -> class logits, reg
    # term -> box channels 0..3, padding channels exactly zero
    scale = torch.zeros((p.shape[0], 1, ld), dtype=torch.float32, device=p.device)
    scale[:, 0, :4] = g[:, 1:2]
    scale[:, 0, 4:4 + C] = g[:, 0:1]
    return (d[..., :ld].to(torch.float32) * scale).view(pred.shape), None, None, None, None, None


centernet_gauss_loss.register_autograd(_gauss_loss_backward, setup_context=_gauss_loss_setup)


# ---- batched training augmentation (cvlite extension) -------------------------------------------------
@torch.library.custom_op("cvlite::augment_images", mutates_args=(), device_types="cuda")
def augment_images(images: List[torch.Tensor], table: torch.Tensor, ph: int, pw: int) -> torch.Tensor:
    """images: B device uint8 / fp32 [H_i, W_i, 3]; table: host uint8 [B, 144], the images' cvl_augment_desc
    from cvlite.augment.plan_table (every plan padded to ph x pw) -> [B, ph, pw, 3] fp32: zoom-out, crop,
    flip, resize, colour, / 127.5 - 1 and pad of the whole batch in one launch (no gradient)."""
    from . import augment as ag
    imgs = [ag._device_image(im) for im in images]
    out = torch.empty((len(imgs), ph, pw, 3), dtype=torch.float32, device=imgs[0].device)
    ag.launch_table(ag.pinned_table(table, imgs, list(out.unbind(0))))
    return out


@augment_images.register_fake
def _(images, table, ph, pw):
    return images[0].new_empty((len(images), ph, pw, 3), dtype=torch.float32)


# ---- optimizer -----------------------------------------------------------------------------------
@torch.library.custom_op("cvlite::sgd_clip_", mutates_args=("w", "v"), device_types="cuda")
def sgd_clip_(w: torch.Tensor, g: torch.Tensor, v: torch.Tensor, lr: torch.Tensor, momentum: float, inv_bs: float,
              clip: float) -> None:
    """In place: g' = clip_by_global_norm(g * inv_bs, clip); v = momentum*v - lr*g'; w += v."""
    nn.sgd_clip_update(w, g, v, lr, momentum, inv_bs, clip)


# ---- whole-network autograd node ------------------------------------------------------------------
class NetFunction(torch.autograd.Function):
    """outputs = net.forward(x) (training-mode BN); backward = net.backward with the head
    gradients (bf16 [B,P,32-padded] as the fused losses write them), returning the parameter
    gradients from the flat gradient buffer.  Inputs: (net, x, *params) with params the store's
    tensors in store order (so autograd routes gradients to model.trainable_variables)."""

    @staticmethod
    def forward(ctx, net, x, *params):
        reg, cls = net.forward(x, train=True)
        ctx.net = net
        ctx.saved_state = net._saved
        ctx.shapes = (reg.shape, cls.shape)
        return reg, cls

    @staticmethod
    def backward(ctx, g_reg, g_cls):
        net = ctx.net
        B, P = ctx.shapes[0][0], ctx.shapes[0][1]
        # (a Generalized Focal Loss head, FCOSNet(reg_max=R), is wider: its own padding)
        reg_w = net.reg_heads[0].cout_pad if getattr(net, "reg_max", None) is not None else 32
        d_reg = torch.zeros((B, P, reg_w), dtype=BF16, device=net.device)
        d_cls = torch.zeros((B, P, net.cls_ld), dtype=BF16, device=net.device)
        if g_reg is not None:
            d_reg[..., :g_reg.shape[2]] = g_reg.to(BF16)
        if g_cls is not None:
            d_cls[..., :g_cls.shape[2]] = g_cls.to(BF16)
        net._saved = ctx.saved_state
        net.backward(d_reg, d_cls)
        st = net.store
        grads = [st.g(name).clone() for name in st.offsets]
        return (None, None) + tuple(grads)


def net_params(net) -> List[torch.Tensor]:
    st = net.store
    return [st.p(name) for name in st.offsets]
