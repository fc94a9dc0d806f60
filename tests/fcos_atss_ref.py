"""Restatement of the ATSS assignment (include/cvlite.h, "ATSS target assignment") that the GPU tests
compare csrc/fcos_atss.hip against: numpy float32 in the kernel's operation order with float64 where
the rule names it, plain loops over images, boxes and levels, and an EXHAUSTIVE scan of every level for
the top-k (np.lexsort((index, d2)): smallest d2, ties to the lowest row-major index, NaN last).
tests/test_fcos_atss_ref.py pins this file itself.  Scenes, PAD, level_shapes, target_norm and
paper_loss are those of tests/fcos_paper_ref.py."""
import numpy as np

from fcos_paper_ref import PAD, STRIDES, level_shapes, paper_loss, scene, target_norm  # noqa: F401

f32 = np.float32
f64 = np.float64


def box_geometry(r, H, W):
    """(yc, xc, y0, y1, x0, x1, area) in pixels, fp32, the operation order of cvl_fcos_paper_assign."""
    half = f32(0.5)
    yc, xc, hp, wp = r[0] * H, r[1] * W, r[2] * H, r[3] * W
    return yc, xc, yc - hp * half, yc + hp * half, xc - wp * half, xc + wp * half, hp * wp


def box_label(r, C):
    """(int)label when the box takes part, else -1: the label must lie in [0, C) (NaN does not)."""
    with np.errstate(invalid="ignore"):
        if not (r[4] > f32(-1.0) and r[4] < f32(C)):
            return -1
    return int(r[4])


def level_d2(yc, xc, Hs, Ws, sf):
    """(gy [Hs], gx [Ws], d2 [Hs, Ws]) of one level, fp32."""
    half = f32(0.5)
    gy = (np.arange(Hs, dtype=f32) + half) * sf
    gx = (np.arange(Ws, dtype=f32) + half) * sf
    with np.errstate(invalid="ignore", over="ignore"):
        dy, dx = gy - yc, gx - xc
        d2 = (dy * dy)[:, None] + (dx * dx)[None, :]
    return gy, gx, d2


def _order_key(d2):
    """d2 as the integer the kernel orders by: the fp32 bit pattern (d2 >= 0), NaN above +inf."""
    bits = np.ascontiguousarray(d2, f32).view(np.uint32).astype(np.int64)
    return np.where(np.isnan(d2), np.int64(0x7FC00000), bits)


def select_exhaustive(d2, k):
    """Row-major indices of the k cells with the smallest d2, ties to the lowest index, in that order."""
    flat = _order_key(d2).reshape(-1)
    return np.lexsort((np.arange(flat.size), flat))[:k]


def window_bounds(yc, xc, Hs, Ws, sf, half_width):
    """Inclusive (r0, r1, c0, c1) of the window of `half_width` cells either side of the clamped cell
    (floor(yc/sf), floor(xc/sf)), cut to the level (the kernel's arithmetic: NaN clamps to 0)."""
    def one(c, n):
        with np.errstate(invalid="ignore", over="ignore"):
            fr = np.floor(c / sf)
        fr = np.fmin(np.fmax(fr, f32(0)), f32(n - 1))
        ci = int(fr)
        return max(ci - half_width, 0), min(ci + half_width, n - 1)
    r0, r1 = one(yc, Hs)
    c0, c1 = one(xc, Ws)
    return r0, r1, c0, c1


def select_window(d2, k, bounds):
    """select_exhaustive restricted to the window: the same order, global row-major indices."""
    r0, r1, c0, c1 = bounds
    Ws = d2.shape[1]
    rows, cols = np.meshgrid(np.arange(r0, r1 + 1), np.arange(c0, c1 + 1), indexing="ij")
    idx = (rows * Ws + cols).reshape(-1)
    flat = _order_key(d2).reshape(-1)[idx]
    return idx[np.lexsort((idx, flat))[:k]]


def window_is_safe(yc, xc, Hs, Ws, sf, bounds, kth_d2):
    """The kernel's check that no cell outside the window can displace a selected one: d2 = fl(a_r + b_s)
    is monotone in a_r = dy^2 and b_s = dx^2, so the smallest d2 outside the window is
    min(fl(min_{r outside} a_r + min_s b_s), fl(min_r a_r + min_{s outside} b_s)); the window's answer
    stands when that is strictly larger than the k-th selected d2 (orders as _order_key does)."""
    r0, r1, c0, c1 = bounds
    if r0 == 0 and r1 == Hs - 1 and c0 == 0 and c1 == Ws - 1:
        return True
    half = f32(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        dy = (np.arange(Hs, dtype=f32) + half) * sf - yc
        dx = (np.arange(Ws, dtype=f32) + half) * sf - xc
        a, b = _order_key(dy * dy), _order_key(dx * dx)
        big = np.int64(0x7FC00000)
        back = lambda v: np.array([v], np.int64).astype(np.uint32).view(f32)[0]   # noqa: E731
        a_out = min([big] + [a[r] for r in range(Hs) if not r0 <= r <= r1])
        b_out = min([big] + [b[s] for s in range(Ws) if not c0 <= s <= c1])
        m1 = _order_key(np.array([back(a_out) + back(b.min())], f32))[0]
        m2 = _order_key(np.array([back(a.min()) + back(b_out)], f32))[0]
    return min(m1, m2) > _order_key(np.array([kth_d2], f32))[0]


def anchor_iou(gy, gx, y0, y1, x0, x1, area, ha):
    """IoU of the box with the square anchor of half side ha about (gy, gx): fp32, the division in
    float64."""
    zero = f32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        ih = np.fmax(np.fmin(y1, gy + ha) - np.fmax(y0, gy - ha), zero)
        iw = np.fmax(np.fmin(x1, gx + ha) - np.fmax(x0, gx - ha), zero)
        inter = ih * iw
        uni = ((ha + ha) * (ha + ha) + area) - inter
        return f32(f64(inter) / f64(uni))


def threshold(ious):
    """mean + sample standard deviation of the candidates' IoUs, float64, summed serially in order."""
    n = len(ious)
    if n == 0:
        return f64(0.0)
    s = f64(0.0)
    for v in ious:
        s = s + f64(v)
    mean = s / f64(n)
    std = f64(0.0)
    if n >= 2:
        q = f64(0.0)
        for v in ious:
            d = f64(v) - mean
            q = q + d * d
        std = np.sqrt(q / f64(n - 1))
    return mean + std


def atss_assign(boxes, nbox, img_dim, pad_hw, C, strides=STRIDES, topk=9, anchor_scale=8.0, select=None):
    """boxes [B,n_max,5] f32 (yc, xc, h, w, cls) normalised, nbox [B], img_dim [B,2] f32.
    select(d2, k, yc, xc, Hs, Ws, sf, topk) -> candidate indices; None = the exhaustive scan.
    Returns (targets [B,P,5+C] f32, positives per level [B,5] i32, cand_cells [B,n_max,5*topk] i32,
    cand_iou [B,n_max,5*topk] f32, cand_thr [B,n_max] f64, positive pairs per cell [B,P] i32,
    owner [B,P] i32 = the winning box or -1).  Skipped boxes keep cand_cells -1, cand_iou 0, cand_thr 0."""
    boxes = np.asarray(boxes, f32)
    img_dim = np.asarray(img_dim, f32)
    B, n_max = boxes.shape[:2]
    shapes = level_shapes(pad_hw, strides)
    offs = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])]).astype(int)
    P = int(offs[-1])
    targets = np.zeros((B, P, 5 + C), f32)
    counts = np.zeros((B, 5), np.int32)
    cand_cells = np.full((B, n_max, 5 * topk), -1, np.int32)
    cand_iou = np.zeros((B, n_max, 5 * topk), f32)
    cand_thr = np.zeros((B, n_max), f64)
    npair = np.zeros((B, P), np.int32)
    owner = np.full((B, P), -1, np.int32)
    scale, half, eps = f32(anchor_scale), f32(0.5), f32(0.01)
    for b in range(B):
        H, W = img_dim[b, 0], img_dim[b, 1]
        best_iou = np.full(P, -1.0, f32)
        vals = np.zeros((P, 4), f32)                     # the winner's pixel distances t, b, l, r
        n = min(max(int(nbox[b]), 0), n_max)
        for i in range(n):
            r = boxes[b, i]
            cls = box_label(r, C)
            with np.errstate(invalid="ignore", over="ignore"):
                yc, xc, y0, y1, x0, x1, area = box_geometry(r, H, W)
            if cls < 0 or not area > 0:
                continue
            pairs = []                                   # (cell, iou, t, b, l, r) level-major, then rank
            for lvl, (Hs, Ws) in enumerate(shapes):
                sf = f32(strides[lvl])
                gy, gx, d2 = level_d2(yc, xc, Hs, Ws, sf)
                k = min(topk, Hs * Ws)
                sel = select_exhaustive(d2, k) if select is None else select(d2, k, yc, xc, Hs, Ws, sf, topk)
                ha = scale * sf * half
                for rank, q in enumerate(sel):
                    cy, cx = int(q) // Ws, int(q) % Ws
                    iou = anchor_iou(gy[cy], gx[cx], y0, y1, x0, x1, area, ha)
                    cand_cells[b, i, lvl * topk + rank] = offs[lvl] + int(q)
                    cand_iou[b, i, lvl * topk + rank] = iou
                    with np.errstate(invalid="ignore", over="ignore"):
                        pairs.append((offs[lvl] + int(q), iou, gy[cy] - y0, y1 - gy[cy], gx[cx] - x0, x1 - gx[cx]))
            thr = threshold([p[1] for p in pairs])
            cand_thr[b, i] = thr
            for p, iou, t, bt, l, rr in pairs:
                # each distance is compared on its own, so a NaN distance is never positive
                if not (f64(iou) >= thr and t > eps and bt > eps and l > eps and rr > eps):
                    continue
                npair[b, p] += 1
                if iou > best_iou[p]:                    # strict: ties keep the lowest box index
                    best_iou[p] = iou
                    owner[b, p] = i
                    vals[p] = (t, bt, l, rr)
        for lvl, (Hs, Ws) in enumerate(shapes):
            sf = f32(strides[lvl])
            for p in range(offs[lvl], offs[lvl + 1]):
                i = owner[b, p]
                if i < 0:
                    continue
                t, bt, l, rr = vals[p]
                targets[b, p, :4] = vals[p] / sf
                d = vals[p].astype(f64)
                targets[b, p, 4] = f32(np.sqrt((min(d[0], d[1]) / max(d[0], d[1])) * (min(d[2], d[3]) / max(d[2], d[3]))))
                targets[b, p, 5 + int(boxes[b, i, 4])] = 1.0
                counts[b, lvl] += 1
    return targets, counts, cand_cells, cand_iou, cand_thr, npair, owner


def windowed(half_width_of):
    """A `select` for atss_assign that picks from the window of half_width_of(topk) cells either side."""
    def select(d2, k, yc, xc, Hs, Ws, sf, topk):
        return select_window(d2, k, window_bounds(yc, xc, Hs, Ws, sf, half_width_of(topk)))
    return select
