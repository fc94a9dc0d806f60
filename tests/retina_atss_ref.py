"""Restatement of the RetinaNet ATSS assignment and its loss (include/cvlite.h, "ATSS target assignment
and a per-image normalised loss for RetinaNet") that the GPU tests compare csrc/retina_atss.hip against.
The assignment is numpy float32 in the kernel's operation order with float64 where the rule names it,
plain loops over images, boxes and levels, and an EXHAUSTIVE top-k over every anchor of a level
(np.lexsort((cell*A + an, d2)): smallest d2, ties to the lowest index, NaN last).  The loss is float64
torch, so autograd gives the reference gradients.  tests/test_retina_atss_ref.py pins this file itself."""
import numpy as np
import torch

from fcos_atss_ref import _order_key, box_geometry, box_label, threshold  # noqa: F401

f32 = np.float32
f64 = np.float64
STRIDES = (8, 16, 32, 64, 128)


def default_anchor_dims():
    """[5, 9, 2] fp32 (h, w): cvlite.retinanet.RetinaNet's default anchors (retinanet_module.py:205-216;
    ratio outer loop, scale inner loop), restated."""
    out = np.zeros((5, 9, 2), f32)
    scales = [2 ** x for x in [0, 1 / 3, 2 / 3]]
    for lv, size in enumerate([32.0, 64.0, 128.0, 256.0, 512.0]):
        area, k = size ** 2, 0
        for ratio in [0.5, 1.0, 2.0]:
            h = np.sqrt(f32(area / ratio))
            w = f32(f32(area) / h)
            for sc in scales:
                out[lv, k] = (f32(f32(sc) * h), f32(f32(sc) * w))
                k += 1
    return out


def level_sizes(pad, strides=STRIDES):
    return [int(pad) // int(s) for s in strides]


def scene(seed, pad, C, n_box):
    """(boxes [n_box,5] f32 normalised (yc, xc, h, w, label), img_dim [2] f32 = (pad, pad)): sides
    log-uniform in [12, 0.9 pad] px, centres uniform with the box inside the image, labels uniform."""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((n_box, 5), f32)
    for k in range(n_box):
        h = float(np.exp(rng.uniform(np.log(12.0), np.log(0.9 * pad))))
        w = float(np.exp(rng.uniform(np.log(12.0), np.log(0.9 * pad))))
        yc, xc = rng.uniform(h / 2, pad - h / 2), rng.uniform(w / 2, pad - w / 2)
        boxes[k] = [yc / pad, xc / pad, h / pad, w / pad, rng.integers(0, C)]
    return boxes, np.array([pad, pad], f32)


def scene_batch(seeds, pad, C, n_box):
    sc = [scene(s, pad, C, n_box) for s in seeds]
    return np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])


def anchor_ious(c0, c1, ah, aw, y0, y1, x0, x1, area):
    """IoU of the box with anchors (arrays) centred at (c0, c1) with dims (ah, aw): fp32, the division in
    float64."""
    zero, half = f32(0), f32(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        ih = np.fmax(np.fmin(y1, c0 + ah * half) - np.fmax(y0, c0 - ah * half), zero)
        iw = np.fmax(np.fmin(x1, c1 + aw * half) - np.fmax(x0, c1 - aw * half), zero)
        inter = ih * iw
        uni = (ah * aw + area) - inter
        return (inter.astype(f64) / uni.astype(f64)).astype(f32)


def atss_assign(boxes, nbox, img_dim, pad, C, anchor_dims=None, strides=STRIDES, topk=9):
    """boxes [B,n_max,5] f32 (yc, xc, h, w, cls) normalised, nbox [B], img_dim [B,2] f32, anchor_dims
    [5,A,2] f32 (None: the default 9 anchors).  Returns (targets [B,P,A,8] f32, positive anchors per
    level [B,5] i32, cand_idx [B,n_max,5*topk] i32, cand_iou the same shape f32, cand_thr [B,n_max] f64,
    positive pairs per anchor [B,P*A] i32, owner [B,P*A] i32 = the winning box or -1)."""
    boxes = np.asarray(boxes, f32)
    img_dim = np.asarray(img_dim, f32)
    adims = default_anchor_dims() if anchor_dims is None else np.asarray(anchor_dims, f32)
    A = adims.shape[1]
    B, n_max = boxes.shape[:2]
    sizes = level_sizes(pad, strides)
    offs = np.concatenate([[0], np.cumsum([S * S for S in sizes])]).astype(int)
    P = int(offs[-1])
    targets = np.zeros((B, P * A, 8), f32)
    targets[:, :, 4] = -1.0
    targets[:, :, 6] = -1.0
    counts = np.zeros((B, 5), np.int32)
    cand_idx = np.full((B, n_max, 5 * topk), -1, np.int32)
    cand_iou = np.zeros((B, n_max, 5 * topk), f32)
    cand_thr = np.zeros((B, n_max), f64)
    npair = np.zeros((B, P * A), np.int32)
    owner = np.full((B, P * A), -1, np.int32)
    eps = f32(0.01)
    for b in range(B):
        H, W = img_dim[b, 0], img_dim[b, 1]
        best = np.full(P * A, -1.0, f32)
        n = min(max(int(nbox[b]), 0), n_max)
        geo = {}
        for i in range(n):
            r = boxes[b, i]
            cls = box_label(r, C)
            with np.errstate(invalid="ignore", over="ignore"):
                yc, xc, y0, y1, x0, x1, area = box_geometry(r, H, W)
            if cls < 0 or not area > 0:
                continue
            geo[i] = (yc, xc, r[2] * H, r[3] * W, cls)
            pairs = []                                   # (row, iou, inside) level-major, then rank
            for lvl, S in enumerate(sizes):
                s = int(strides[lvl])
                pos = (np.arange(S) * s).astype(f32)     # (float)(u*s)
                with np.errstate(invalid="ignore", over="ignore"):
                    dy, dx = pos - yc, pos - xc
                    d2 = (dy * dy)[:, None] + (dx * dx)[None, :]
                key = np.repeat(_order_key(d2).reshape(-1), A)           # every anchor of a cell ties
                k = min(topk, A * S * S)
                sel = np.lexsort((np.arange(key.size), key))[:k]         # indices cell*A + an
                cell, an = sel // A, sel % A
                c0, c1 = pos[cell // S], pos[cell % S]
                iou = anchor_ious(c0, c1, adims[lvl, an, 0], adims[lvl, an, 1], y0, y1, x0, x1, area)
                with np.errstate(invalid="ignore", over="ignore"):
                    inside = (c0 - y0 > eps) & (y1 - c0 > eps) & (c1 - x0 > eps) & (x1 - c1 > eps)
                rows = offs[lvl] * A + sel
                cand_idx[b, i, lvl * topk:lvl * topk + k] = rows
                cand_iou[b, i, lvl * topk:lvl * topk + k] = iou
                pairs += list(zip(rows.tolist(), iou, inside.tolist()))
            thr = threshold([p[1] for p in pairs])
            cand_thr[b, i] = thr
            for row, iou, inside in pairs:
                if not (f64(iou) >= thr and inside):
                    continue
                npair[b, row] += 1
                if iou > best[row]:                      # strict: ties keep the lowest box index
                    best[row] = iou
                    owner[b, row] = i
        for lvl, S in enumerate(sizes):
            s = int(strides[lvl])
            for row in np.nonzero(owner[b, offs[lvl] * A:offs[lvl + 1] * A] >= 0)[0] + offs[lvl] * A:
                i = int(owner[b, row])
                yc, xc, hp, wp, cls = geo[i]
                cell, an = row // A - offs[lvl], row % A
                c0, c1 = f32((cell // S) * s), f32((cell % S) * s)
                ah, aw = adims[lvl, an]
                targets[b, row] = (f32((f64(c0) - f64(yc)) / f64(ah)), f32((f64(c1) - f64(xc)) / f64(aw)),
                                   f32(f64(hp) / f64(ah)), f32(f64(wp) / f64(aw)), f32(cls), best[row], f32(i), 0.0)
                counts[b, lvl] += 1
    return targets.reshape(B, P, A, 8), counts, cand_idx, cand_iou, cand_thr, npair, owner


def focal(y, x, alpha=0.25, gamma=2.0):
    """The focal term of csrc/fcos_focal.h in float64 torch (the stable form)."""
    L = torch.log1p(torch.exp(-x.abs()))
    nlp, nlq = L - x.clamp(max=0), L + x.clamp(min=0)
    p = torch.sigmoid(x)
    return y * alpha * (1 - p) ** gamma * nlp + (1 - y) * (1 - alpha) * p ** gamma * nlq


def atss_loss(reg, cls, targets, num_targets, A, C, img_weight=None, alpha=0.25, gamma=2.0):
    """reg [B,P,>=4A], cls [B,P,>=A*C] float64 torch, targets [B,P,A,8] and num_targets [B,5] numpy ->
    losses [B,2] = (cls, reg) float64 torch: focal over every (anchor, class), smooth-L1 (delta 1) over
    the positive anchors' four box elements, each divided by N = max(sum(num_targets[b]), 1)."""
    tg = torch.as_tensor(np.asarray(targets, f64))
    B, P = tg.shape[:2]
    tg = tg.reshape(B, P, A, 8)
    label = tg[..., 4]
    x = cls[..., :A * C].reshape(B, P, A, C)
    y = (label[..., None] == torch.arange(C, dtype=torch.float64)).to(torch.float64)
    l_cls = focal(y, x, alpha, gamma).sum((1, 2, 3))
    pos = (label >= 0)[..., None]
    t = torch.where(pos, tg[..., :4], torch.zeros(()).double())
    d = t - reg[..., :4 * A].reshape(B, P, A, 4)
    ad = d.abs()
    sl1 = torch.where(ad < 1.0, 0.5 * d * d, ad)
    l_reg = torch.where(pos, sl1, torch.zeros(()).double()).sum((1, 2, 3))
    N = torch.as_tensor(np.maximum(np.asarray(num_targets).sum(1), 1).astype(f64))
    w = torch.ones(B, dtype=torch.float64) if img_weight is None else torch.as_tensor(np.asarray(img_weight, f64))
    return torch.stack([w * l_cls / N, w * l_reg / N], 1)
