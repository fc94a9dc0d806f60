"""Device ops for target assignment and the fused detection losses (C ABI: include/cvlite.h)."""
import torch

from . import _lib
from ._lib import ptr

FCOS_STRIDES = (8, 16, 32, 64, 128)      # FCOS/fcos.py:142-143
FCOS_BOUNDS = (32.0, 64.0, 128.0, 256.0)  # FCOS/fcos.py:145-147


def fcos_level_shapes(pad_h, pad_w, strides=FCOS_STRIDES):
    return [(int(pad_h // s), int(pad_w // s)) for s in strides]


def fcos_assign(boxes, nbox, img_dim, pad_hw, num_classes, strides=FCOS_STRIDES, bounds=FCOS_BOUNDS,
                out=None, num_targets=None):
    """Batched FCOS targets.  boxes [B,Nmax,5] f32, nbox [B] i32, img_dim [B,2] f32 (device).
    Returns targets [B, P, 5+C] f32 (level-major cells) and num_targets [B,5] i32."""
    _lib.require_cuda(boxes, nbox, img_dim)
    assert boxes.dtype == torch.float32 and nbox.dtype == torch.int32 and img_dim.dtype == torch.float32
    B, nmax = int(boxes.shape[0]), int(boxes.shape[1])
    P = sum(h * w for h, w in fcos_level_shapes(pad_hw[0], pad_hw[1], strides))
    if out is None:
        out = torch.empty((B, P, 5 + num_classes), device=boxes.device, dtype=torch.float32)
    if num_targets is None:
        num_targets = torch.empty((B, 5), device=boxes.device, dtype=torch.int32)
    st = (_lib.ctypes.c_int32 * 5)(*[int(s) for s in strides])
    bd = (_lib.ctypes.c_float * 4)(*[float(x) for x in bounds])
    _lib.call("cvl_fcos_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]),
              int(pad_hw[1]), int(num_classes), _lib.ctypes.cast(st, _lib.c_void_p),
              _lib.ctypes.cast(bd, _lib.c_void_p), ptr(out), ptr(num_targets), _lib.stream())
    return out, num_targets


def fcos_center_assign(boxes, nbox, img_dim, pad_hw, num_classes, strides=FCOS_STRIDES, b_dim=FCOS_BOUNDS,
                       center_only=False, out=None, num_targets=None):
    """Batched FCOS-center targets (fcos_center.py:149-317) in cvl_fcos_assign's layout:
    targets [B, P, 5+C] f32 level-major, num_targets [B,5] i32."""
    _lib.require_cuda(boxes, nbox, img_dim)
    assert boxes.dtype == torch.float32 and nbox.dtype == torch.int32 and img_dim.dtype == torch.float32
    B, nmax = int(boxes.shape[0]), int(boxes.shape[1])
    P = sum(h * w for h, w in fcos_level_shapes(pad_hw[0], pad_hw[1], strides))
    if out is None:
        out = torch.empty((B, P, 5 + num_classes), device=boxes.device, dtype=torch.float32)
    if num_targets is None:
        num_targets = torch.empty((B, 5), device=boxes.device, dtype=torch.int32)
    st = (_lib.ctypes.c_int32 * 5)(*[int(s) for s in strides])
    bd = (_lib.ctypes.c_float * 4)(*[float(x) for x in b_dim])
    _lib.call("cvl_fcos_center_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]),
              int(pad_hw[1]), int(num_classes), _lib.ctypes.cast(st, _lib.c_void_p),
              _lib.ctypes.cast(bd, _lib.c_void_p), 1 if center_only else 0, ptr(out), ptr(num_targets),
              _lib.stream())
    return out, num_targets


def fcos_center_v1_assign(boxes, nbox, img_dim, pad_hw, num_classes, strides=FCOS_STRIDES, b_dim=FCOS_BOUNDS,
                          out=None, num_targets=None):
    """fcos_center_v1.format_data batched (cvl_fcos_center_v1_assign): centroid cells only,
    (y_off, x_off, h / box_sc, w / box_sc, 1, class bits).  Same layout as fcos_center_assign."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    P = sum(h * w for h, w in fcos_level_shapes(pad_hw[0], pad_hw[1], strides))
    if out is None:
        out = torch.empty((B, P, 5 + num_classes), device=boxes.device, dtype=torch.float32)
    if num_targets is None:
        num_targets = torch.empty((B, 5), device=boxes.device, dtype=torch.int32)
    st = (_lib.ctypes.c_int32 * 5)(*[int(s) for s in strides])
    bd = (_lib.ctypes.c_float * 4)(*[float(x) for x in b_dim])
    _lib.call("cvl_fcos_center_v1_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]),
              int(pad_hw[1]), int(num_classes), _lib.ctypes.cast(st, _lib.c_void_p),
              _lib.ctypes.cast(bd, _lib.c_void_p), ptr(out), ptr(num_targets), _lib.stream())
    return out, num_targets


def fcos_loss(reg_pred, cls_pred, targets, num_classes, reg_type="l1", grad_scale=1.0,
              with_grad=True, grad_dtype=torch.float32, d_reg=None, d_cls=None, cen_type="l1",
              reg_sigmoid=False, cen_in_cls=False, alpha=0.25, gamma=2.0, delta=1.0, float_mask=False,
              losses=None):
    """Fused focal + smooth-L1/IoU + centerness forward and backward.
    reg_pred [B,P,ld_reg>=5] f32, cls_pred [B,P,ld_cls>=C] f32, targets [B,P,5+C] f32.
    Centre variants (fcos_center / fcos_center_v1): cen_type "focal", reg_sigmoid (v1's sigmoid
    reg head), cen_in_cls (centerness logit in class column round_up(C, 8)).
    alpha / gamma / delta: the focal_loss / smooth_l1_loss keywords (fcos.py:380, 443-444);
    float_mask: the regression mask is targets[..., 5] itself (C = 1).  losses: optional [B,3] f32
    output buffer.  Returns (losses [B,3] f32 = (cls, reg, cen) per image, d_reg, d_cls)."""
    _lib.require_cuda(reg_pred, cls_pred, targets)
    B, P = int(targets.shape[0]), int(targets.shape[1])
    assert reg_pred.shape[:2] == (B, P) and cls_pred.shape[:2] == (B, P)
    rt = reg_type if isinstance(reg_type, int) else {"l1": 0, "iou": 1}[reg_type]    # int: raw kernel flags
    rt |= (4 if cen_type.lower() == "focal" else 0) | (8 if reg_sigmoid else 0) | (16 if cen_in_cls else 0)
    rt |= 32 if float_mask else 0
    dev = targets.device
    if losses is None:
        losses = torch.empty((B, 3), device=dev, dtype=torch.float32)
    assert losses.shape == (B, 3) and losses.dtype == torch.float32 and losses.is_contiguous()
    ws = torch.empty(int(_lib.load().cvl_fcos_loss_workspace_size(B, P)), device=dev, dtype=torch.uint8)
    if with_grad:
        if d_reg is None:
            d_reg = torch.empty((B, P, reg_pred.shape[2]), device=dev, dtype=grad_dtype)
        if d_cls is None:
            d_cls = torch.empty((B, P, cls_pred.shape[2]), device=dev, dtype=grad_dtype)
    dt = lambda t: 0 if t is None or t.dtype == torch.float32 else 1  # noqa: E731
    dflt = alpha == 0.25 and gamma == 2.0 and delta == 1.0 and not float_mask
    tail = (ptr(d_reg), int(d_reg.shape[2]) if d_reg is not None else 0, dt(d_reg),
            ptr(d_cls), int(d_cls.shape[2]) if d_cls is not None else 0, dt(d_cls), ptr(ws), ws.numel(),
            _lib.stream())
    head = (ptr(reg_pred), int(reg_pred.shape[2]), ptr(cls_pred), int(cls_pred.shape[2]), ptr(targets), B, P,
            int(num_classes), rt, float(grad_scale))
    if dflt:
        _lib.call("cvl_fcos_loss", *head, ptr(losses), *tail)
    else:
        _lib.call("cvl_fcos_loss_ex", *head, float(alpha), float(gamma), float(delta), ptr(losses), *tail)
    return losses, d_reg, d_cls


# ---- the FCOS papers' recipe (cvlite extension; include/cvlite.h states the rules) ----------------
FCOS_PAPER_BOUNDS = (64.0, 128.0, 256.0, 512.0)   # regress ranges on max(l,t,r,b), Tian et al. 2019


def fcos_paper_assign(boxes, nbox, img_dim, pad_hw, num_classes, strides=FCOS_STRIDES, bounds=FCOS_PAPER_BOUNDS,
                      center_radius=1.5, out=None, num_targets=None):
    """Batched targets of the FCOS papers (cvl_fcos_paper_assign): per-level regress range on
    max(l,t,r,b), centre sampling (center_radius strides about the box centre; <= 0: the whole box),
    smallest-area winner, sqrt centerness, one-hot class.  Inputs and the targets layout are
    fcos_assign's.  Returns targets [B, P, 5+C] f32 and num_targets [B,5] i32 = the number of
    POSITIVE CELLS per level (fcos_assign counts boxes)."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    P = sum(h * w for h, w in fcos_level_shapes(pad_hw[0], pad_hw[1], strides))
    if out is None:
        out = torch.empty((B, P, 5 + num_classes), device=boxes.device, dtype=torch.float32)
    if num_targets is None:
        num_targets = torch.empty((B, 5), device=boxes.device, dtype=torch.int32)
    assert tuple(out.shape) == (B, P, 5 + num_classes) and out.dtype == torch.float32 and out.is_contiguous()
    assert tuple(num_targets.shape) == (B, 5) and num_targets.dtype == torch.int32 and num_targets.is_contiguous()
    st = (_lib.ctypes.c_int32 * 5)(*[int(s) for s in strides])
    bd = (_lib.ctypes.c_float * 4)(*[float(x) for x in bounds])
    _lib.call("cvl_fcos_paper_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]),
              int(pad_hw[1]), int(num_classes), _lib.ctypes.cast(st, _lib.c_void_p),
              _lib.ctypes.cast(bd, _lib.c_void_p), float(center_radius), ptr(out), ptr(num_targets),
              _lib.stream())
    return out, num_targets


def fcos_target_norm(targets, num_classes, out=None):
    """norm [B,2] f32 = (number of positive cells, sum of their centerness targets) per image; a cell
    is positive when its largest class target is >= 1 (cvl_fcos_target_norm)."""
    _lib.require_cuda(targets)
    B, P = int(targets.shape[0]), int(targets.shape[1])
    assert targets.dtype == torch.float32 and targets.is_contiguous() and int(targets.shape[2]) == 5 + num_classes
    if out is None:
        out = torch.empty((B, 2), device=targets.device, dtype=torch.float32)
    assert tuple(out.shape) == (B, 2) and out.dtype == torch.float32 and out.is_contiguous()
    ws = torch.empty(int(_lib.load().cvl_fcos_target_norm_workspace_size(B, P)), device=targets.device,
                     dtype=torch.uint8)
    _lib.call("cvl_fcos_target_norm", ptr(targets), B, P, int(num_classes), ptr(out), ptr(ws), ws.numel(),
              _lib.stream())
    return out


def fcos_paper_loss(reg_pred, cls_pred, targets, num_classes, norm=None, grad_scale=1.0, with_grad=True,
                    grad_dtype=torch.float32, d_reg=None, d_cls=None, alpha=0.25, gamma=2.0, losses=None):
    """Fused loss of the FCOS papers, forward and backward (cvl_fcos_paper_loss): focal / N,
    centerness-weighted GIoU on max(pred, 0) / sum(centerness), BCE centerness on the positives / N,
    with (N, sum centerness) = norm [B,2] as fcos_target_norm returns it (None: plain sums).
    reg_pred [B,P,ld_reg>=5] f32, cls_pred [B,P,ld_cls>=C] f32, targets [B,P,5+C] f32.
    Returns (losses [B,3] f32 = (cls, reg, cen) per image, d_reg, d_cls)."""
    _lib.require_cuda(reg_pred, cls_pred, targets)
    B, P = int(targets.shape[0]), int(targets.shape[1])
    assert reg_pred.shape[:2] == (B, P) and cls_pred.shape[:2] == (B, P)
    assert reg_pred.dtype == torch.float32 and cls_pred.dtype == torch.float32 and targets.dtype == torch.float32
    assert reg_pred.is_contiguous() and cls_pred.is_contiguous() and targets.is_contiguous()
    assert int(targets.shape[2]) == 5 + num_classes
    dev = targets.device
    if norm is not None:
        _lib.require_cuda(norm)
        assert tuple(norm.shape) == (B, 2) and norm.dtype == torch.float32 and norm.is_contiguous()
    if losses is None:
        losses = torch.empty((B, 3), device=dev, dtype=torch.float32)
    assert losses.shape == (B, 3) and losses.dtype == torch.float32 and losses.is_contiguous()
    ws = torch.empty(int(_lib.load().cvl_fcos_loss_workspace_size(B, P)), device=dev, dtype=torch.uint8)
    if with_grad:
        if d_reg is None:
            d_reg = torch.empty((B, P, reg_pred.shape[2]), device=dev, dtype=grad_dtype)
        if d_cls is None:
            d_cls = torch.empty((B, P, cls_pred.shape[2]), device=dev, dtype=grad_dtype)
    for d in (d_reg, d_cls):
        assert d is None or (d.shape[:2] == (B, P) and d.is_contiguous() and d.dtype in (torch.float32, torch.bfloat16))
    dt = lambda t: 0 if t is None or t.dtype == torch.float32 else 1  # noqa: E731
    _lib.call("cvl_fcos_paper_loss", ptr(reg_pred), int(reg_pred.shape[2]), ptr(cls_pred), int(cls_pred.shape[2]),
              ptr(targets), ptr(norm), B, P, int(num_classes), float(grad_scale), float(alpha), float(gamma),
              ptr(losses), ptr(d_reg), int(d_reg.shape[2]) if d_reg is not None else 0, dt(d_reg),
              ptr(d_cls), int(d_cls.shape[2]) if d_cls is not None else 0, dt(d_cls), ptr(ws), ws.numel(),
              _lib.stream())
    return losses, d_reg, d_cls


def fcos_atss_assign(boxes, nbox, img_dim, pad_hw, num_classes, strides=FCOS_STRIDES, topk=9, anchor_scale=8.0,
                     out=None, num_targets=None, return_candidates=False):
    """Batched ATSS targets (cvl_fcos_atss_assign; include/cvlite.h states the rule): per box the topk
    grid points nearest its centre on every level, positives where the anchor IoU (square anchors of
    side anchor_scale * stride) reaches mean + std of the box's own candidates and the point lies
    inside the box; per cell the largest IoU wins.  Inputs, the targets layout and num_targets (positive
    cells per level) are fcos_paper_assign's, and fcos_target_norm / fcos_paper_loss take the result.
    The contest workspace comes from torch's caching allocator, as the neighbours' workspaces do.
    return_candidates: also (cand_cells [B,n_max,5*topk] i32, cand_iou the same shape f32, cand_thr
    [B,n_max] f64), the selection as the kernel saw it."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    P = sum(h * w for h, w in fcos_level_shapes(pad_hw[0], pad_hw[1], strides))
    dev = boxes.device
    if out is None:
        out = torch.empty((B, P, 5 + num_classes), device=dev, dtype=torch.float32)
    if num_targets is None:
        num_targets = torch.empty((B, 5), device=dev, dtype=torch.int32)
    assert tuple(out.shape) == (B, P, 5 + num_classes) and out.dtype == torch.float32 and out.is_contiguous()
    assert tuple(num_targets.shape) == (B, 5) and num_targets.dtype == torch.int32 and num_targets.is_contiguous()
    cand = (None, None, None)
    if return_candidates:
        slots = 5 * max(int(topk), 0)
        cand = (torch.empty((B, nmax, slots), device=dev, dtype=torch.int32),
                torch.empty((B, nmax, slots), device=dev, dtype=torch.float32),
                torch.empty((B, nmax), device=dev, dtype=torch.float64))
    ws = torch.empty(int(_lib.load().cvl_fcos_atss_workspace_size(B, P)), device=dev, dtype=torch.uint8)
    st = (_lib.ctypes.c_int32 * 5)(*[int(s) for s in strides])
    _lib.call("cvl_fcos_atss_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]),
              int(pad_hw[1]), int(num_classes), _lib.ctypes.cast(st, _lib.c_void_p), int(topk),
              float(anchor_scale), ptr(out), ptr(num_targets), ptr(cand[0]), ptr(cand[1]), ptr(cand[2]), ptr(ws),
              ws.numel(), _lib.stream())
    return (out, num_targets) + cand if return_candidates else (out, num_targets)


# ---- Generalized Focal Loss (cvlite extension; include/cvlite.h states the rule) -------------------
def _gfl_rows(reg_pred, cls_pred, targets, num_classes):
    B, P = int(targets.shape[0]), int(targets.shape[1])
    assert reg_pred.shape[:2] == (B, P) and cls_pred.shape[:2] == (B, P)
    assert reg_pred.dtype == torch.float32 and cls_pred.dtype == torch.float32 and targets.dtype == torch.float32
    assert reg_pred.is_contiguous() and cls_pred.is_contiguous() and targets.is_contiguous()
    assert int(targets.shape[2]) == 5 + num_classes
    return B, P


def fcos_gfl_norm(cls_pred, targets, num_classes, out=None):
    """norm [B,2] f32 = (number of positive cells, sum over them of sigmoid(max class logit)) per image
    (cvl_fcos_gfl_norm); cls_pred [B,P,ld_cls>=C] f32, targets [B,P,5+C] f32.  The divisors of
    fcos_gfl_loss; it needs the class outputs, so it runs after the forward."""
    _lib.require_cuda(cls_pred, targets)
    B, P = int(targets.shape[0]), int(targets.shape[1])
    assert cls_pred.shape[:2] == (B, P) and cls_pred.dtype == torch.float32
    assert targets.dtype == torch.float32 and int(targets.shape[2]) == 5 + num_classes
    if out is None:
        out = torch.empty((B, 2), device=targets.device, dtype=torch.float32)
    assert tuple(out.shape) == (B, 2) and out.dtype == torch.float32 and out.is_contiguous()
    ws = torch.empty(int(_lib.load().cvl_fcos_gfl_norm_workspace_size(B, P)), device=targets.device,
                     dtype=torch.uint8)
    _lib.call("cvl_fcos_gfl_norm", ptr(cls_pred), int(cls_pred.shape[2]), ptr(targets), B, P, int(num_classes),
              ptr(out), ptr(ws), ws.numel(), _lib.stream())
    return out


def fcos_gfl_loss(reg_pred, cls_pred, targets, num_classes, reg_max, norm=None, grad_scale=1.0, with_grad=True,
                  grad_dtype=torch.float32, d_reg=None, d_cls=None, beta=2.0, box_weight=2.0, dfl_weight=0.25,
                  losses=None):
    """Fused Generalized Focal Loss, forward and backward (cvl_fcos_gfl_loss): Quality Focal Loss on the
    class logits with the decoded box's IoU as the positives' target / N, GIoU on the expectations of the
    per-side distributions and Distribution Focal Loss, both weighted by sigmoid(max class logit) /
    its sum, with (N, sum) = norm [B,2] as fcos_gfl_norm returns it (None: plain sums).
    reg_pred [B,P,ld_reg>=4(reg_max+1)] f32 (side-major: top, bottom, left, right; reg_max+1 bins each),
    cls_pred [B,P,ld_cls>=C] f32, targets [B,P,5+C] f32 (fcos_atss_assign / fcos_paper_assign).
    Returns (losses [B,3] f32 = (qfl, box, dfl) per image, d_reg, d_cls)."""
    _lib.require_cuda(reg_pred, cls_pred, targets)
    B, P = _gfl_rows(reg_pred, cls_pred, targets, num_classes)
    dev = targets.device
    if norm is not None:
        _lib.require_cuda(norm)
        assert tuple(norm.shape) == (B, 2) and norm.dtype == torch.float32 and norm.is_contiguous()
    if losses is None:
        losses = torch.empty((B, 3), device=dev, dtype=torch.float32)
    assert losses.shape == (B, 3) and losses.dtype == torch.float32 and losses.is_contiguous()
    ws = torch.empty(int(_lib.load().cvl_fcos_gfl_loss_workspace_size(B, P)), device=dev, dtype=torch.uint8)
    if with_grad:
        if d_reg is None:
            d_reg = torch.empty((B, P, reg_pred.shape[2]), device=dev, dtype=grad_dtype)
        if d_cls is None:
            d_cls = torch.empty((B, P, cls_pred.shape[2]), device=dev, dtype=grad_dtype)
    for d in (d_reg, d_cls):
        assert d is None or (d.shape[:2] == (B, P) and d.is_contiguous() and d.dtype in (torch.float32, torch.bfloat16))
    dt = lambda t: 0 if t is None or t.dtype == torch.float32 else 1  # noqa: E731
    _lib.call("cvl_fcos_gfl_loss", ptr(reg_pred), int(reg_pred.shape[2]), ptr(cls_pred), int(cls_pred.shape[2]),
              ptr(targets), ptr(norm), B, P, int(num_classes), int(reg_max), float(grad_scale), float(beta),
              float(box_weight), float(dfl_weight), ptr(losses), ptr(d_reg),
              int(d_reg.shape[2]) if d_reg is not None else 0, dt(d_reg), ptr(d_cls),
              int(d_cls.shape[2]) if d_cls is not None else 0, dt(d_cls), ptr(ws), ws.numel(), _lib.stream())
    return losses, d_reg, d_cls


def fcos_gfl_decode(reg_pred, reg_max, out=None):
    """The distances of a GFL box head (cvl_fcos_gfl_decode): reg_pred [..., ld_reg>=4(reg_max+1)] f32 ->
    [..., 8] f32 with columns 0..3 = the expectations of the (top, bottom, left, right) distributions in
    stride units and columns 4..7 zero: the box rows that cvl_fcos_detect reads with center = 0."""
    _lib.require_cuda(reg_pred)
    assert reg_pred.dtype == torch.float32 and reg_pred.dim() >= 2
    rows = int(reg_pred.numel() // reg_pred.shape[-1])
    if out is None:
        out = torch.empty(tuple(reg_pred.shape[:-1]) + (8,), device=reg_pred.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and int(out.numel() // out.shape[-1]) == rows
    _lib.call("cvl_fcos_gfl_decode", ptr(reg_pred), int(reg_pred.shape[-1]), rows, int(reg_max), ptr(out),
              int(out.shape[-1]), _lib.stream())
    return out


# ---- task-aligned assignment (cvlite extension; include/cvlite.h states the rule) ------------------
def fcos_tal_assign(boxes, nbox, img_dim, pad_hw, num_classes, dist, cls_pred, strides=FCOS_STRIDES, topk=13,
                    alpha=1.0, beta=6.0, clamp=True, out=None, num_targets=None, return_candidates=False):
    """Batched task-aligned targets (cvl_fcos_tal_assign; TOOD, Feng et al. 2021): per box the topk cells
    inside it with the largest sigmoid(class logit)^alpha * IoU(predicted box, box)^beta; per cell the
    selecting box with the largest IoU wins; slot 4 of a won cell is its metric scaled by max IoU / max
    metric of its box.  It reads the head outputs, so it runs after the forward: dist [B,P,ld>=4] f32 =
    (top, bottom, left, right) in stride units (clamp: at 0 first, the 5-output head's raw rows;
    clamp=False: fcos_gfl_decode's rows), cls_pred [B,P,ld>=C] f32 logits.  Boxes, the targets layout and
    num_targets (positive cells per level) are fcos_atss_assign's; fcos_target_norm / fcos_tal_loss take
    the result.  return_candidates: also (cand_cells [B,n_max,topk] i32 by rank or -1, cand_metric and
    cand_iou the same shape f32, box_max [B,n_max,2] f32 = (max metric, max IoU) over the won cells)."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    _lib.require_cuda(dist, cls_pred)
    P = sum(h * w for h, w in fcos_level_shapes(pad_hw[0], pad_hw[1], strides))
    assert dist.dtype == torch.float32 and cls_pred.dtype == torch.float32
    assert tuple(dist.shape[:2]) == (B, P) and tuple(cls_pred.shape[:2]) == (B, P)
    dev = boxes.device
    if out is None:
        out = torch.empty((B, P, 5 + num_classes), device=dev, dtype=torch.float32)
    if num_targets is None:
        num_targets = torch.empty((B, 5), device=dev, dtype=torch.int32)
    assert tuple(out.shape) == (B, P, 5 + num_classes) and out.dtype == torch.float32 and out.is_contiguous()
    assert tuple(num_targets.shape) == (B, 5) and num_targets.dtype == torch.int32 and num_targets.is_contiguous()
    cand = (None, None, None, None)
    if return_candidates:
        k = max(int(topk), 0)
        cand = (torch.empty((B, nmax, k), device=dev, dtype=torch.int32),
                torch.empty((B, nmax, k), device=dev, dtype=torch.float32),
                torch.empty((B, nmax, k), device=dev, dtype=torch.float32),
                torch.empty((B, nmax, 2), device=dev, dtype=torch.float32))
    ws = torch.empty(int(_lib.load().cvl_fcos_tal_workspace_size(B, P, nmax)), device=dev, dtype=torch.uint8)
    st = (_lib.ctypes.c_int32 * 5)(*[int(s) for s in strides])
    _lib.call("cvl_fcos_tal_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]),
              int(pad_hw[1]), int(num_classes), _lib.ctypes.cast(st, _lib.c_void_p), ptr(dist), int(dist.shape[2]),
              1 if clamp else 0, ptr(cls_pred), int(cls_pred.shape[2]), int(topk), float(alpha), float(beta),
              ptr(out), ptr(num_targets), ptr(cand[0]), ptr(cand[1]), ptr(cand[2]), ptr(cand[3]), ptr(ws),
              ws.numel(), _lib.stream())
    return (out, num_targets) + cand if return_candidates else (out, num_targets)


def fcos_tal_loss(reg_pred, cls_pred, targets, num_classes, norm=None, grad_scale=1.0, with_grad=True,
                  grad_dtype=torch.float32, d_reg=None, d_cls=None, beta=2.0, box_weight=2.0, losses=None):
    """Fused loss on task-aligned targets, forward and backward (cvl_fcos_tal_loss): Quality Focal Loss on
    the class logits with targets[..., 4] as the positives' class target, GIoU on max(pred, 0) weighted by
    it, both divided by W = max(sum of targets[..., 4] over the positives, 1) with (count, sum) = norm
    [B,2] as fcos_target_norm returns it (None: W = 1).  reg_pred [B,P,ld_reg>=5] f32 (column 4, the
    head's centerness output, is not read and gets zero gradient), cls_pred [B,P,ld_cls>=C] f32, targets
    [B,P,5+C] f32.  Returns (losses [B,3] f32 = (cls, box, 0) per image, d_reg, d_cls)."""
    _lib.require_cuda(reg_pred, cls_pred, targets)
    B, P = _gfl_rows(reg_pred, cls_pred, targets, num_classes)
    dev = targets.device
    if norm is not None:
        _lib.require_cuda(norm)
        assert tuple(norm.shape) == (B, 2) and norm.dtype == torch.float32 and norm.is_contiguous()
    if losses is None:
        losses = torch.empty((B, 3), device=dev, dtype=torch.float32)
    assert losses.shape == (B, 3) and losses.dtype == torch.float32 and losses.is_contiguous()
    ws = torch.empty(int(_lib.load().cvl_fcos_loss_workspace_size(B, P)), device=dev, dtype=torch.uint8)
    if with_grad:
        if d_reg is None:
            d_reg = torch.empty((B, P, reg_pred.shape[2]), device=dev, dtype=grad_dtype)
        if d_cls is None:
            d_cls = torch.empty((B, P, cls_pred.shape[2]), device=dev, dtype=grad_dtype)
    for d in (d_reg, d_cls):
        assert d is None or (d.shape[:2] == (B, P) and d.is_contiguous() and d.dtype in (torch.float32, torch.bfloat16))
    dt = lambda t: 0 if t is None or t.dtype == torch.float32 else 1  # noqa: E731
    _lib.call("cvl_fcos_tal_loss", ptr(reg_pred), int(reg_pred.shape[2]), ptr(cls_pred), int(cls_pred.shape[2]),
              ptr(targets), ptr(norm), B, P, int(num_classes), float(grad_scale), float(beta), float(box_weight),
              ptr(losses), ptr(d_reg), int(d_reg.shape[2]) if d_reg is not None else 0, dt(d_reg),
              ptr(d_cls), int(d_cls.shape[2]) if d_cls is not None else 0, dt(d_cls), ptr(ws), ws.numel(),
              _lib.stream())
    return losses, d_reg, d_cls


def _boxes_args(boxes, nbox, img_dim):
    _lib.require_cuda(boxes, nbox, img_dim)
    assert boxes.dtype == torch.float32 and nbox.dtype == torch.int32 and img_dim.dtype == torch.float32
    return int(boxes.shape[0]), int(boxes.shape[1])


RETINA_STRIDES = (8, 16, 32, 64, 128)    # RetinaNet/retinanet_module.py:197


def retina_assign(boxes, nbox, img_dim, pad, anchor_dims, num_classes, iou_thresh=0.5,
                  strides=RETINA_STRIDES, out=None, num_targets=None):
    """Batched RetinaNet targets.  anchor_dims: device fp32 [5, A, 2].  Returns (targets
    [B, sum_l A*S_l^2, 4+C] f32 ordered (level, anchor, u, v), num_targets [B] i32)."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    A = int(anchor_dims.shape[1])
    P = sum(A * (pad // s) ** 2 for s in strides)
    if out is None:
        out = torch.empty((B, P, 4 + num_classes), device=boxes.device, dtype=torch.float32)
    nt = torch.empty((B,), device=boxes.device, dtype=torch.int32) if num_targets is None else num_targets
    st = (_lib.ctypes.c_int32 * 5)(*[int(s) for s in strides])
    _lib.call("cvl_retina_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad), int(num_classes),
              ptr(anchor_dims.contiguous()), A, _lib.ctypes.cast(st, _lib.c_void_p), float(iou_thresh), ptr(out),
              ptr(nt), _lib.stream())
    return out, nt


# ---- ATSS for RetinaNet (cvlite extension; include/cvlite.h states the rules) ----------------------
def retina_atss_assign(boxes, nbox, img_dim, pad, anchor_dims, num_classes, strides=RETINA_STRIDES, topk=9,
                       out=None, num_targets=None, return_candidates=False):
    """Batched ATSS targets for RetinaNet (cvl_retina_atss_assign): per box the topk anchors nearest its
    centre on every level (the ceil(topk / A) nearest cells), positives where the anchor IoU reaches
    mean + std of the box's own candidates and the anchor centre lies inside the box; per anchor the
    largest IoU wins.  Inputs as retina_assign (anchor_dims: device fp32 [5, A, 2]).  Returns compact
    targets [B, P, A, 8] f32 in the row order of the head outputs (slots: the four linear box targets,
    label or -1, IoU, box index or -1, 0) and num_targets [B, 5] i32 = positive anchors per level; `out`
    may be any contiguous f32 buffer of B*P*A*8 elements (e.g. [B, P*A, 8]).  return_candidates: also
    (cand_idx [B,n_max,5*topk] i32 = target rows, cand_iou the same shape f32, cand_thr [B,n_max] f64)."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    _lib.require_cuda(anchor_dims)
    assert anchor_dims.dtype == torch.float32 and anchor_dims.dim() == 3 and tuple(anchor_dims.shape[::2]) == (5, 2)
    A = int(anchor_dims.shape[1])
    P = sum((int(pad) // int(s)) ** 2 for s in strides)
    dev = boxes.device
    if out is None:
        out = torch.empty((B, P, A, 8), device=dev, dtype=torch.float32)
    if num_targets is None:
        num_targets = torch.empty((B, 5), device=dev, dtype=torch.int32)
    assert out.numel() == B * P * A * 8 and out.dtype == torch.float32 and out.is_contiguous()
    assert tuple(num_targets.shape) == (B, 5) and num_targets.dtype == torch.int32 and num_targets.is_contiguous()
    cand = (None, None, None)
    if return_candidates:
        slots = 5 * max(int(topk), 0)
        cand = (torch.empty((B, nmax, slots), device=dev, dtype=torch.int32),
                torch.empty((B, nmax, slots), device=dev, dtype=torch.float32),
                torch.empty((B, nmax), device=dev, dtype=torch.float64))
    ws = torch.empty(int(_lib.load().cvl_retina_atss_workspace_size(B, P, A)), device=dev, dtype=torch.uint8)
    st = (_lib.ctypes.c_int32 * 5)(*[int(s) for s in strides])
    _lib.call("cvl_retina_atss_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad), int(num_classes),
              ptr(anchor_dims), A, _lib.ctypes.cast(st, _lib.c_void_p), int(topk), ptr(out), ptr(num_targets),
              ptr(cand[0]), ptr(cand[1]), ptr(cand[2]), ptr(ws), ws.numel(), _lib.stream())
    return (out, num_targets) + cand if return_candidates else (out, num_targets)


def retina_atss_loss(reg, cls, targets, num_targets, A, C, img_weight=None, alpha=0.25, gamma=2.0,
                     grad_scale=1.0, d_reg=None, d_cls=None, losses=None):
    """Focal + smooth-L1 on the compact ATSS targets, forward and backward (cvl_retina_atss_loss), each
    image's sums divided by its positive anchors N = max(sum(num_targets[b]), 1).  reg [B,P,ld>=4A] /
    cls [B,P,ld>=A*C] f32 from the grouped heads, targets B*P*A*8 f32 and num_targets [B,5] i32 from
    retina_atss_assign, img_weight [B] f32 or None.  d_reg / d_cls: bf16 or fp32 buffers written at the
    prediction positions (None = no gradient; padding channels are not touched).  Returns losses [B,2] =
    (cls, reg)."""
    _lib.require_cuda(reg, cls, targets, num_targets, img_weight, d_reg, d_cls)
    B, P = int(reg.shape[0]), int(reg.shape[1])
    assert reg.dtype == torch.float32 and cls.dtype == torch.float32 and targets.dtype == torch.float32
    assert cls.shape[:2] == (B, P) and targets.numel() == B * P * int(A) * 8
    assert tuple(num_targets.shape) == (B, 5) and num_targets.dtype == torch.int32
    assert img_weight is None or (tuple(img_weight.shape) == (B,) and img_weight.dtype == torch.float32)
    dev = targets.device
    if losses is None:
        losses = torch.empty((B, 2), device=dev, dtype=torch.float32)
    assert losses.shape == (B, 2) and losses.dtype == torch.float32 and losses.is_contiguous()
    for d in (d_reg, d_cls):
        assert d is None or (d.shape[:2] == (B, P) and d.dtype in (torch.float32, torch.bfloat16))
    ws = torch.empty(int(_lib.load().cvl_retina_atss_loss_workspace_size(B, P, int(A))), device=dev,
                     dtype=torch.uint8)
    dt = lambda t: 0 if t is None or t.dtype == torch.float32 else 1  # noqa: E731
    _lib.call("cvl_retina_atss_loss", ptr(reg), int(reg.shape[2]), ptr(cls), int(cls.shape[2]), ptr(targets),
              ptr(num_targets), ptr(img_weight), B, P, int(A), int(C), float(grad_scale), float(alpha), float(gamma),
              ptr(losses), ptr(d_reg), int(d_reg.shape[2]) if d_reg is not None else 0, dt(d_reg), ptr(d_cls),
              int(d_cls.shape[2]) if d_cls is not None else 0, dt(d_cls), ptr(ws), ws.numel(), _lib.stream())
    return losses


def centernet_assign(boxes, nbox, img_dim, pad_hw, num_classes, stride=8, out=None):
    """CenterNet hourglass centroid targets -> [B, pad_w/s, pad_h/s, 4+C]."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    if out is None:
        out = torch.empty((B, pad_hw[1] // stride, pad_hw[0] // stride, 4 + num_classes), device=boxes.device,
                      dtype=torch.float32)
    _lib.call("cvl_centernet_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]),
              int(pad_hw[1]), int(num_classes), int(stride), ptr(out), _lib.stream())
    return out


# ---- CenterNet Gaussian targets (cvlite extension; include/cvlite.h states the rules) -----------------
def centernet_gauss_assign(boxes, nbox, img_dim, pad_hw, num_classes, stride=4, min_overlap=0.7, out=None):
    """Gaussian-heatmap CenterNet targets (cvl_centernet_gauss_assign): per kept box a disc of radius
    mmdet's gaussian_radius(min_overlap) about its centre cell, heat exp(-d^2 / (2 sigma^2)) with sigma =
    (2r + 1) / 6, per class the maximum over the boxes, exactly 1.0 at the centres; the box channels are
    centernet_assign's at the centre cells.  Inputs as centernet_assign.  Returns [B, pad_h/s, pad_w/s,
    4+C] f32 (rows along y; centernet_assign's layout for square pads)."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    hm, wm = int(pad_hw[0]) // int(stride), int(pad_hw[1]) // int(stride)
    if out is None:
        out = torch.empty((B, hm, wm, 4 + num_classes), device=boxes.device, dtype=torch.float32)
    assert out.numel() == B * hm * wm * (4 + num_classes) and out.dtype == torch.float32 and out.is_contiguous()
    _lib.call("cvl_centernet_gauss_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]),
              int(pad_hw[1]), int(num_classes), int(stride), float(min_overlap), ptr(out), _lib.stream())
    return out


def centernet_gauss_norm(targets, num_classes, out=None):
    """npos [B] i32 = the (cell, class) entries of each image's target map [B, ..., 4+C] that equal 1.0
    (cvl_centernet_gauss_norm): the divisor N of centernet_gauss_loss, for assigned and loaded maps alike."""
    _lib.require_cuda(targets, out)
    assert targets.dtype == torch.float32 and targets.shape[-1] == 4 + num_classes
    B = int(targets.shape[0])
    P = int(targets.numel() // (B * (4 + num_classes)))
    if out is None:
        out = torch.empty((B,), device=targets.device, dtype=torch.int32)
    assert tuple(out.shape) == (B,) and out.dtype == torch.int32
    _lib.call("cvl_centernet_gauss_norm", ptr(targets), B, P, int(num_classes), ptr(out), _lib.stream())
    return out


def centernet_gauss_loss(pred, targets, npos, num_classes, alpha=2.0, beta=4.0, cls_scale=1.0, reg_scale=1.0,
                         d_pred=None, losses=None):
    """Penalty-reduced focal loss + L1 on the centres, forward and backward (cvl_centernet_gauss_loss), each
    image's sums divided by N = max(npos[b], 1).  pred [B,P,ld] f32 (box 0..3, class logits 4..), targets
    [B,P,4+C] f32, npos [B] i32 from centernet_gauss_norm.  Returns (losses [B,2] = (cls, reg), not scaled,
    d_pred bf16 [B,P,ld_d] of cls_scale*cls + reg_scale*reg, channels >= 4+C zero)."""
    _lib.require_cuda(pred, targets, npos, d_pred, losses)
    B, P = int(targets.shape[0]), int(targets.shape[1])
    assert pred.dtype == torch.float32 and targets.dtype == torch.float32 and npos.dtype == torch.int32
    assert targets.shape[-1] == 4 + num_classes and pred.numel() == B * P * pred.shape[-1]
    assert tuple(npos.shape) == (B,)
    dev = targets.device
    if losses is None:
        losses = torch.empty((B, 2), device=dev, dtype=torch.float32)
    if d_pred is None:
        d_pred = torch.empty((B, P, (4 + num_classes + 7) // 8 * 8), device=dev, dtype=torch.bfloat16)
    assert losses.shape == (B, 2) and losses.dtype == torch.float32
    assert d_pred.dtype == torch.bfloat16 and d_pred.numel() == B * P * d_pred.shape[-1]
    ws = torch.empty(int(_lib.load().cvl_centernet_gauss_loss_workspace_size(B, P)), device=dev, dtype=torch.uint8)
    _lib.call("cvl_centernet_gauss_loss", ptr(pred), int(pred.shape[-1]), ptr(targets), ptr(npos), B, P,
              int(num_classes), float(alpha), float(beta), float(cls_scale), float(reg_scale), ptr(losses),
              ptr(d_pred), int(d_pred.shape[-1]), ptr(ws), _lib.stream())
    return losses, d_pred


def centernet_splat(boxes, nbox, img_dim, pad_hw, num_classes, stride=8, sigma=0.25):
    """CenterNet centre splat targets -> [B, pad_h/s, pad_w/s, 5+C]."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    out = torch.empty((B, pad_hw[0] // stride, pad_hw[1] // stride, 5 + num_classes), device=boxes.device,
                      dtype=torch.float32)
    _lib.call("cvl_centernet_splat", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]),
              int(pad_hw[1]), int(num_classes), int(stride), float(sigma), ptr(out), _lib.stream())
    return out


def det_loss(reg_pred, cls_pred, targets, num_classes, grad_scale_cls=1.0, grad_scale_reg=1.0, with_grad=True):
    """Focal + masked smooth-L1 (CenterNet / RetinaNet).  reg [B,P,>=4], cls [B,P,>=C], targets
    [B,P,4+C] (f32).  Returns (losses [B,2] = (cls, reg), d_reg, d_cls)."""
    _lib.require_cuda(reg_pred, cls_pred, targets)
    B, P = int(targets.shape[0]), int(targets.shape[1])
    dev = targets.device
    losses = torch.empty((B, 2), device=dev, dtype=torch.float32)
    ws = torch.empty(int(_lib.load().cvl_det_loss_workspace_size(B, P)), device=dev, dtype=torch.uint8)
    d_reg = torch.zeros_like(reg_pred) if with_grad else None
    d_cls = torch.zeros_like(cls_pred) if with_grad else None
    _lib.call("cvl_det_loss", ptr(reg_pred), int(reg_pred.shape[-1]), ptr(cls_pred), int(cls_pred.shape[-1]),
              ptr(targets), B, P, int(num_classes), float(grad_scale_cls), float(grad_scale_reg), ptr(losses),
              ptr(d_reg), ptr(d_cls), ptr(ws), _lib.stream())
    return losses, d_reg, d_cls


def retina_loss(reg_pred, cls_pred, targets, level_cells, n_anchors, num_classes, img_weight=None,
                grad_scale=1.0, d_reg=None, d_cls=None, losses=None):
    """RetinaNet.train_loss fwd+bwd (cvl_retina_loss).  reg_pred [B,P,ld>=4A] / cls_pred [B,P,ld>=AC] f32
    from the grouped heads, targets [B, A*P, 4+C] (cvl_retina_assign order).  d_reg / d_cls: bf16
    (fp32 in the parity mode) buffers written at the prediction positions (None = no gradient).
    Returns losses [B,2]."""
    _lib.require_cuda(reg_pred, cls_pred, targets)
    B, P = int(reg_pred.shape[0]), int(reg_pred.shape[1])
    assert sum(level_cells) == P and int(targets.shape[1]) == n_anchors * P
    dev = targets.device
    if losses is None:
        losses = torch.empty((B, 2), device=dev, dtype=torch.float32)
    ws = torch.empty(int(_lib.load().cvl_retina_loss_workspace_size(B, P, n_anchors)), device=dev, dtype=torch.uint8)
    lc = (_lib.ctypes.c_int32 * 5)(*[int(c) for c in level_cells])
    f32 = any(t is not None and t.dtype == torch.float32 for t in (d_reg, d_cls))    # fp32 parity mode
    for t in (d_reg, d_cls):
        assert t is None or t.dtype == (torch.float32 if f32 else torch.bfloat16)
    _lib.call("cvl_retina_loss_f32" if f32 else "cvl_retina_loss", ptr(reg_pred), int(reg_pred.shape[-1]), ptr(cls_pred), int(cls_pred.shape[-1]),
              ptr(targets), B, _lib.ctypes.cast(lc, _lib.c_void_p), int(n_anchors), int(num_classes), ptr(img_weight),
              float(grad_scale), ptr(losses), ptr(d_reg), int(d_reg.shape[-1]) if d_reg is not None else 0,
              ptr(d_cls), int(d_cls.shape[-1]) if d_cls is not None else 0, ptr(ws), _lib.stream())
    return losses


def nms(boxes_xyxy, classes, iou_threshold):
    """boxes [n, 6] float64 (x1, y1, x2, y2, score, cls) device; classes: iterable of class values
    in processing order.  Returns the kept rows in the reference's emission order."""
    _lib.require_cuda(boxes_xyxy)
    n = int(boxes_xyxy.shape[0])
    cls = torch.tensor(list(classes), dtype=torch.float64, device=boxes_xyxy.device)
    ncls = int(cls.numel())
    keep = torch.empty((ncls, n), dtype=torch.int32, device=boxes_xyxy.device)
    nkeep = torch.empty((ncls,), dtype=torch.int32, device=boxes_xyxy.device)
    ws = torch.empty(int(_lib.load().cvl_nms_workspace_size(n, ncls)), dtype=torch.uint8, device=boxes_xyxy.device)
    _lib.call("cvl_nms", ptr(boxes_xyxy), n, ptr(cls), ncls, float(iou_threshold), ptr(keep), ptr(nkeep),
              ptr(ws), _lib.stream())
    nk = nkeep.cpu().tolist()
    idx = torch.cat([keep[c, :nk[c]] for c in range(ncls)]) if ncls else keep.new_zeros(0)
    return boxes_xyxy[idx.long()]


def soft_nms(boxes_xyxy, classes, sigma=0.3):
    """Soft-NMS (cvl_soft_nms): boxes [n, 6] float64 (x1, y1, x2, y2, score, cls) device, classes in
    processing order.  Returns the emitted rows (reference order) with their decayed scores."""
    _lib.require_cuda(boxes_xyxy)
    n = int(boxes_xyxy.shape[0])
    dev = boxes_xyxy.device
    cls = torch.tensor(list(classes), dtype=torch.float64, device=dev)
    ncls = int(cls.numel())
    keep = torch.empty((ncls, n), dtype=torch.int32, device=dev)
    ksc = torch.empty((ncls, n), dtype=torch.float64, device=dev)
    nkeep = torch.empty((ncls,), dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.load().cvl_soft_nms_workspace_size(n, ncls)), dtype=torch.uint8, device=dev)
    _lib.call("cvl_soft_nms", ptr(boxes_xyxy), n, ptr(cls), ncls, float(sigma), ptr(keep), ptr(ksc), ptr(nkeep),
              ptr(ws), _lib.stream())
    nk = nkeep.cpu().tolist()
    idx = torch.cat([keep[c, :nk[c]] for c in range(ncls)]).long()
    rows = boxes_xyxy[idx].clone()
    rows[:, 4] = torch.cat([ksc[c, :nk[c]] for c in range(ncls)])
    return rows


def centernet_loss(pred, targets, num_classes, cls_scale=2.5, reg_scale=1.0, d_pred=None, losses=None):
    """CenterNet model_loss fwd+bwd (tf_centernet_hourglass.py:492-505 in train_step :537-549) off
    the output conv.  pred [B,P,ld] f32 (reg 0..3, cls 4..), targets [B,P,4+C] f32.
    Returns (losses [B,2] = (cls, reg), d_pred bf16 [B,P,ld_d] of cls_scale*cls + reg_scale*reg)."""
    _lib.require_cuda(pred, targets)
    B, P = int(targets.shape[0]), int(targets.shape[1])
    dev = targets.device
    if losses is None:
        losses = torch.empty((B, 2), device=dev, dtype=torch.float32)
    if d_pred is None:
        d_pred = torch.empty((B, P, (4 + num_classes + 7) // 8 * 8), device=dev, dtype=torch.bfloat16)
    ws = torch.empty(int(_lib.load().cvl_det_loss_workspace_size(B, P)), device=dev, dtype=torch.uint8)
    _lib.call("cvl_centernet_loss", ptr(pred), int(pred.shape[-1]), ptr(targets), B, P, int(num_classes),
              float(cls_scale), float(reg_scale), ptr(losses), ptr(d_pred), int(d_pred.shape[-1]), ptr(ws),
              _lib.stream())
    return losses, d_pred


def hourglass_v2_assign(boxes, nbox, raw_dims, img_dims, num_classes, out=None):
    """CenterNet v2 targets of one batch (train_hourglass_voc.py train() :96-160): boxes [B,n_max,5]
    f32 = dataset corner rows + label, nbox [B] i32; returns [B, S, S, 4, 5+C] f32, S = img_dims/8."""
    _lib.require_cuda(boxes, nbox)
    assert boxes.dtype == torch.float32 and nbox.dtype == torch.int32
    B, nmax = int(boxes.shape[0]), int(boxes.shape[1])
    S = int(img_dims) // 8
    if out is None:
        out = torch.empty((B, S, S, 4, 5 + num_classes), device=boxes.device, dtype=torch.float32)
    assert tuple(out.shape) == (B, S, S, 4, 5 + num_classes) and out.is_contiguous()
    _lib.call("cvl_hourglass_v2_assign", ptr(boxes), ptr(nbox), B, nmax, int(raw_dims), int(img_dims),
              int(num_classes), ptr(out), _lib.stream())
    return out


def hourglass_v2_loss(pred, targets, num_classes, loss_type="focal", cls_scale=2.5, reg_scale=1.0, d_pred=None,
                      losses=None, reg_is_prob=False):
    """CenterNet v2 model_loss fwd+bwd (tf_hourglass_net.py:398-413 in train_step :415-447) off the
    head conv.  pred [B,P,ld] f32 (channel sc*(5+C)+j, b_focal folded), targets [B,P,4,5+C] f32.
    reg_is_prob: pred's box channels are the model's sigmoid outputs (model_loss's `outputs`).
    Returns (losses [B,2] = (cls, reg), d_pred bf16 [B,P,ld_d] of cls_scale*cls + reg_scale*reg)."""
    _lib.require_cuda(pred, targets)
    B, P = int(targets.shape[0]), int(targets.shape[1])
    assert tuple(targets.shape[2:]) == (4, 5 + num_classes) and pred.shape[:2] == (B, P)
    dev = targets.device
    if losses is None:
        losses = torch.empty((B, 2), device=dev, dtype=torch.float32)
    if d_pred is None:
        d_pred = torch.empty((B, P, (4 * (5 + num_classes) + 31) // 32 * 32), device=dev, dtype=torch.bfloat16)
    ws = torch.empty(int(_lib.load().cvl_hourglass_v2_loss_workspace_size(B, P)), device=dev, dtype=torch.uint8)
    lt = (1 if loss_type == "sigmoid" else 0) | (2 if reg_is_prob else 0)
    _lib.call("cvl_hourglass_v2_loss", ptr(pred), int(pred.shape[-1]), ptr(targets), B, P, int(num_classes), lt,
              float(cls_scale), float(reg_scale), ptr(losses), ptr(d_pred), int(d_pred.shape[-1]), ptr(ws),
              _lib.stream())
    return losses, d_pred


def centernet_s8_assign(boxes, nbox, img_dim, pad_hw, num_classes, box_scales, stride=8, out=None):
    """tf_centernet_resnet_s8.format_data batched (cvl_centernet_s8_assign): boxes [B,n_max,5]
    normalised (y, x, h, w, cls), img_dim [B,2] the resized size, pad_hw the padded size.
    Returns [B, pad_w/stride, pad_h/stride, n_scales, 4+C] f32."""
    B, nmax = _boxes_args(boxes, nbox, img_dim)
    ns = len(box_scales)
    hm, wm = int(pad_hw[1] / stride), int(pad_hw[0] / stride)
    if out is None:
        out = torch.empty((B, hm, wm, ns, 4 + num_classes), device=boxes.device, dtype=torch.float32)
    assert tuple(out.shape) == (B, hm, wm, ns, 4 + num_classes) and out.is_contiguous()
    sc = (_lib.ctypes.c_float * ns)(*[float(v) for v in box_scales])
    _lib.call("cvl_centernet_s8_assign", ptr(boxes), ptr(nbox), ptr(img_dim), B, nmax, int(pad_hw[0]), int(pad_hw[1]),
              int(num_classes), _lib.ctypes.cast(sc, _lib.c_void_p), ns, int(stride), ptr(out), _lib.stream())
    return out


def centernet_s8_loss(reg, cls, targets, num_classes, n_scales, cls_scale=1.0, reg_scale=1.0, d_reg=None,
                      d_cls=None, losses=None):
    """tf_centernet_resnet_s8.model_loss fwd+bwd off the two head convs: reg [B,P,>=ns*4], cls
    [B,P,>=ns*C] f32 raw logits, targets [B,P,ns,4+C].  Returns (losses [B,2], d_reg, d_cls) with
    bf16 gradients of cls_scale*cls + reg_scale*reg."""
    _lib.require_cuda(reg, cls, targets)
    B, P = int(targets.shape[0]), int(targets.shape[1])
    assert tuple(targets.shape[2:]) == (n_scales, 4 + num_classes)
    dev = targets.device
    if losses is None:
        losses = torch.empty((B, 2), device=dev, dtype=torch.float32)
    if d_reg is None:
        d_reg = torch.empty((B, P, (4 * n_scales + 31) // 32 * 32), device=dev, dtype=torch.bfloat16)
    if d_cls is None:
        d_cls = torch.empty((B, P, (num_classes * n_scales + 31) // 32 * 32), device=dev, dtype=torch.bfloat16)
    ws = torch.empty(int(_lib.load().cvl_centernet_s8_loss_workspace_size(B, P, n_scales)), device=dev,
                     dtype=torch.uint8)
    _lib.call("cvl_centernet_s8_loss", ptr(reg), int(reg.shape[-1]), ptr(cls), int(cls.shape[-1]), ptr(targets), B, P,
              int(n_scales), int(num_classes), float(cls_scale), float(reg_scale), ptr(losses), ptr(d_reg),
              int(d_reg.shape[-1]), ptr(d_cls), int(d_cls.shape[-1]), ptr(ws), _lib.stream())
    return losses, d_reg, d_cls
