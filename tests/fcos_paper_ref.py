"""Restatement of the FCOS papers' recipe (include/cvlite.h, "The FCOS recipe of the FCOS papers") that
the GPU tests compare the kernels against: the assignment in numpy float32 in the kernel's operation
order (bit-identical by construction), the target norm, and the loss in float64 torch (differentiable,
so autograd gives the reference gradients).  tests/test_fcos_paper_ref.py pins this file itself.
Also the two scene families the GPU tests use."""
import numpy as np
import torch

STRIDES = (8, 16, 32, 64, 128)
PAPER_BOUNDS = (64.0, 128.0, 256.0, 512.0)
f32 = np.float32

PAD = (256, 192)                       # non-square: P = 768 + 192 + 48 + 12 + 2 = 1022
BOUNDS_A = (16.0, 32.0, 64.0, 128.0)   # family A: down-scaled ranges, so all five levels get positives


def level_shapes(pad_hw, strides=STRIDES):
    return [(pad_hw[0] // s, pad_hw[1] // s) for s in strides]


def paper_assign(boxes, nbox, img_dim, pad_hw, C, strides=STRIDES, bounds=PAPER_BOUNDS, center_radius=1.5):
    """boxes [B,n_max,5] f32 (yc, xc, h, w, cls) normalised, nbox [B], img_dim [B,2] f32.
    Returns (targets [B,P,5+C] f32, positives per level [B,5] i32, candidates per cell [B,P] i32)."""
    boxes = np.asarray(boxes, f32)
    img_dim = np.asarray(img_dim, f32)
    B, n_max = boxes.shape[:2]
    shapes = level_shapes(pad_hw, strides)
    P = sum(h * w for h, w in shapes)
    targets = np.zeros((B, P, 5 + C), f32)
    counts = np.zeros((B, 5), np.int32)
    ncand = np.zeros((B, P), np.int32)
    lo = [f32(-1.0)] + [f32(v) for v in bounds]
    hi = [f32(v) for v in bounds] + [f32(np.inf)]
    radius = f32(center_radius)
    half = f32(0.5)
    for b in range(B):
        H, W = img_dim[b, 0], img_dim[b, 1]
        n = min(max(int(nbox[b]), 0), n_max)
        off = 0
        for lvl, (Hs, Ws) in enumerate(shapes):
            sf = f32(strides[lvl])
            gy = np.broadcast_to(((np.arange(Hs, dtype=f32) + half) * sf)[:, None], (Hs, Ws))
            gx = np.broadcast_to(((np.arange(Ws, dtype=f32) + half) * sf)[None, :], (Hs, Ws))
            best_area = np.full((Hs, Ws), np.inf, f32)
            best_cls = np.full((Hs, Ws), -1, np.int64)
            win = np.zeros((4, Hs, Ws), f32)            # the winner's pixel distances t, b, l, r
            cand_n = np.zeros((Hs, Ws), np.int32)
            for i in range(n):
                r = boxes[b, i]
                cls = int(r[4])
                if not 0 <= cls < C:
                    continue
                yc, xc, hp, wp = r[0] * H, r[1] * W, r[2] * H, r[3] * W
                y0, y1 = yc - hp * half, yc + hp * half
                x0, x1 = xc - wp * half, xc + wp * half
                area = hp * wp
                t, bt, l, rr = gy - y0, y1 - gy, gx - x0, x1 - gx
                m = np.maximum(np.maximum(t, bt), np.maximum(l, rr))
                if radius <= 0:
                    inside = np.minimum(np.minimum(t, bt), np.minimum(l, rr))
                else:
                    rs = radius * sf
                    sy0, sy1 = np.maximum(y0, yc - rs), np.minimum(y1, yc + rs)
                    sx0, sx1 = np.maximum(x0, xc - rs), np.minimum(x1, xc + rs)
                    inside = np.minimum(np.minimum(gy - sy0, sy1 - gy), np.minimum(gx - sx0, sx1 - gx))
                cand = (inside > 0) & (lo[lvl] <= m) & (m <= hi[lvl])
                cand_n += cand
                better = cand & (area < best_area)      # strict: ties keep the lowest index
                best_area = np.where(better, area, best_area)
                best_cls = np.where(better, cls, best_cls)
                win = np.where(better[None], np.stack([t, bt, l, rr]), win)
            posm = best_cls >= 0
            out = np.zeros((Hs, Ws, 5 + C), f32)
            if posm.any():
                d = win.astype(np.float64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    cen = np.sqrt((np.minimum(d[0], d[1]) / np.maximum(d[0], d[1]))
                                  * (np.minimum(d[2], d[3]) / np.maximum(d[2], d[3]))).astype(f32)
                for k in range(4):
                    out[..., k] = np.where(posm, win[k] / sf, f32(0))
                out[..., 4] = np.where(posm, cen, f32(0))
                ys, xs = np.nonzero(posm)
                out[ys, xs, 5 + best_cls[ys, xs]] = 1.0
            targets[b, off:off + Hs * Ws] = out.reshape(Hs * Ws, 5 + C)
            ncand[b, off:off + Hs * Ws] = cand_n.reshape(-1)
            counts[b, lvl] = int(posm.sum())
            off += Hs * Ws
    return targets, counts, ncand


def target_norm(targets, C):
    """[B,P,5+C] -> [B,2] float64 = (positives, sum of their centerness targets)."""
    targets = np.asarray(targets)
    pos = targets[..., 5:5 + C].max(-1) >= 1
    return np.stack([pos.sum(1).astype(np.float64), (targets[..., 4].astype(np.float64) * pos).sum(1)], 1)


def giou_loss(t, p):
    """1 - GIoU of ltrb boxes about one grid point: t, p [..., 4] torch (top, bottom, left, right),
    the prediction clamped at 0."""
    d = torch.clamp(p, min=0)
    th, tw = t[..., 0] + t[..., 1], t[..., 2] + t[..., 3]
    ph, pw = d[..., 0] + d[..., 1], d[..., 2] + d[..., 3]
    mn, mx = torch.minimum(t, d), torch.maximum(t, d)
    I = (mn[..., 0] + mn[..., 1]) * (mn[..., 2] + mn[..., 3])
    U = th * tw + ph * pw - I + 1e-12
    E = (mx[..., 0] + mx[..., 1]) * (mx[..., 2] + mx[..., 3]) + 1e-12
    return 1.0 - (I / U - (E - U) / E)


def paper_loss(reg, cls, targets, C, norm=None, alpha=0.25, gamma=2.0):
    """reg [B,P,>=5], cls [B,P,>=C] float64 torch (may require grad), targets [B,P,5+C], norm [B,2]
    (the fp32 values the kernel gets) or None -> [B,3] float64 = (cls, reg, cen) per image."""
    tg = torch.as_tensor(targets).double()
    y = tg[..., 5:5 + C]
    x = cls[..., :C]
    sp = torch.nn.functional.softplus
    p = torch.sigmoid(x)
    focal = y * alpha * (1 - p) ** gamma * sp(-x) + (1 - y) * (1 - alpha) * p ** gamma * sp(x)
    pos = (y.max(-1).values >= 1).double()
    t4 = tg[..., 4]
    xc = reg[..., 4]
    cen = (torch.clamp(xc, min=0) - xc * t4 + torch.log1p(torch.exp(-xc.abs()))) * pos
    rg = t4 * giou_loss(tg[..., :4], reg[..., :4]) * pos
    if norm is None:
        N = Wsum = torch.ones(tg.shape[0], dtype=torch.float64)
    else:
        nm = torch.as_tensor(norm).double()
        N = torch.clamp(nm[:, 0], min=1.0)
        Wsum = torch.clamp(nm[:, 1], min=float(f32(1e-6)))
    return torch.stack([focal.sum((1, 2)) / N, rg.sum(1) / Wsum, cen.sum(1) / N], 1)


def scene(seed, family, C, n_box=8, n_max=8):
    """One image of scene family "A" (img_dim = PAD, bounds BOUNDS_A) or "B" (img_dim (250, 181),
    the paper bounds): n_box boxes with log-uniform sides in [10, image side] and uniformly placed
    centres (so some lie partly outside the image).  The geometry does not depend on C (the labels
    come from a stream of their own).  The draw order is fixed: tests/test_fcos_paper_ref.py asserts
    the conditions the GPU tests need of seeds 0..7.  Returns (boxes [n_max,5] f32, img_dim [2] f32,
    bounds)."""
    rng = np.random.default_rng(seed)
    H, W = (float(PAD[0]), float(PAD[1])) if family == "A" else (250.0, 181.0)
    yc = rng.uniform(0, H, n_box)
    h = np.exp(rng.uniform(np.log(10.0), np.log(H), n_box))
    xc = rng.uniform(0, W, n_box)
    w = np.exp(rng.uniform(np.log(10.0), np.log(W), n_box))
    boxes = np.zeros((n_max, 5), f32)
    boxes[:n_box] = np.stack([yc / H, xc / W, h / H, w / W,
                              np.random.default_rng(1000 + seed).integers(0, C, n_box)], 1)
    return boxes, np.array([H, W], f32), (BOUNDS_A if family == "A" else PAPER_BOUNDS)


def loss_inputs(C, ld_reg, ld_cls, seeds=(0, 1), radius=1.5, seed=0):
    """Inputs of the loss tests: targets of family B (one image per scene seed), reg = targets + noise
    with about a quarter of the positive cells' distances made negative (no exact zeros, no p == t
    ties), class logits about -2.  Returns numpy (reg [B,P,ld_reg], cls [B,P,ld_cls], targets)."""
    sc = [scene(s, "B", C) for s in seeds]
    tg, _, _ = paper_assign(np.stack([b for b, _, _ in sc]), [8] * len(sc), np.stack([d for _, d, _ in sc]), PAD, C,
                            bounds=PAPER_BOUNDS, center_radius=radius)
    rng = np.random.default_rng(100 + seed)
    B, P = tg.shape[:2]
    reg = rng.normal(0, 1, (B, P, ld_reg)).astype(f32)
    box = tg[..., :4] + rng.normal(0, 0.5, (B, P, 4)).astype(f32)
    pos = tg[..., 5:].max(-1) >= 1
    flip = (rng.uniform(size=(B, P, 4)) < 0.25) & pos[..., None]
    box = np.where(flip, -np.abs(box) - f32(0.01), box).astype(f32)
    assert (box != 0).all() and (box != tg[..., :4]).all()
    reg[..., :4] = box
    cls = (rng.normal(0, 2, (B, P, ld_cls)) - 2).astype(f32)
    return reg, cls, tg
