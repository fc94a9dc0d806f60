"""Reference restatement of the Gaussian CenterNet recipe (include/cvlite.h, "CenterNet as the paper
trains it"): the geometry op by op in numpy float32, the radius and the heat in float64, the loss in
float64 torch (autograd gives the reference gradients), and the scene generator the tests share.
Pure host code: no cvlite import."""
import functools
import math

import numpy as np
import torch

F = np.float32


def gaussian_radius(h, w, m):
    """mmdet's gaussian_radius (the corrected roots) in float64 on a box of h x w cells."""
    h, w, m = float(h), float(w), float(m)
    b1 = h + w
    c1 = w * h * (1.0 - m) / (1.0 + m)
    r1 = (b1 - math.sqrt(b1 * b1 - 4.0 * c1)) / 2.0
    b2 = 2.0 * (h + w)
    c2 = (1.0 - m) * w * h
    r2 = (b2 - math.sqrt(b2 * b2 - 16.0 * c2)) / 8.0
    a3 = 4.0 * m
    b3 = -2.0 * m * (h + w)
    c3 = (m - 1.0) * w * h
    r3 = (b3 + math.sqrt(b3 * b3 - 4.0 * a3 * c3)) / (2.0 * a3)
    return max(0, int(min(r1, r2, r3)))


def box_records(boxes, n, img_dim, pad_hw, C, stride, min_overlap=0.7):
    """One image's box records in the stable ascending-area order: dicts (cy, cx, off4 [4] f32, r, cls,
    kept).  fp32 geometry: every operation on np.float32 scalars, one rounding each."""
    H, W = F(img_dim[0]), F(img_dim[1])
    pad_h, pad_w = F(pad_hw[0]), F(pad_hw[1])
    hm, wm = int(pad_hw[0]) // stride, int(pad_hw[1]) // stride
    sf = F(stride)
    b = np.asarray(boxes, F)[:n]
    area = np.array([(r[2] * H) * (r[3] * W) for r in b], F)
    order = np.argsort(area, kind="stable")
    py = F(int((pad_h - H) / F(2.0)))
    px = F(int((pad_w - W) / F(2.0)))
    out = []
    for i in order:
        r = b[i]
        c0, c1 = (r[0] - F(0.5) * r[2]) * H, (r[1] - F(0.5) * r[3]) * W
        c2, c3 = (r[0] + F(0.5) * r[2]) * H, (r[1] + F(0.5) * r[3]) * W
        ycf, xcf = (c0 + c2) / F(2.0), (c1 + c3) / F(2.0)
        cy, cx = int((py + ycf) / sf), int((px + xcf) / sf)
        off4 = np.array([F(np.float64(cy) + 0.5) - (py + c0) / sf, ((py + c2) / sf - F(cy)) - F(0.5),
                         F(np.float64(cx) + 0.5) - (px + c1) / sf, ((px + c3) / sf - F(cx)) - F(0.5)], F)
        hc, wc = np.ceil((c2 - c0) / sf), np.ceil((c3 - c1) / sf)
        assert hc.dtype == F and off4.dtype == F
        lab = float(r[4])
        cls = int(lab) if 0.0 <= lab < C else -1
        kept = cls >= 0 and 0 <= cy < hm and 0 <= cx < wm
        out.append(dict(cy=cy, cx=cx, off4=off4, r=gaussian_radius(hc, wc, min_overlap), cls=cls, kept=kept,
                        index=int(i)))
    return out


def assign_gather(boxes, nbox, img_dim, pad_hw, C, stride, min_overlap=0.7):
    """Targets [B, hm, wm, 4+C] float64 in the gather form: every cell looks at every kept box.  Box channels
    hold the fp32 values widened; heat = exp(-(dy^2 + dx^2) / (2 sigma^2)), sigma = (2r + 1) / 6, in float64."""
    B = len(nbox)
    hm, wm = int(pad_hw[0]) // stride, int(pad_hw[1]) // stride
    out = np.zeros((B, hm, wm, 4 + C), np.float64)
    ys, xs = np.arange(hm)[:, None], np.arange(wm)[None, :]
    for b in range(B):
        for rec in box_records(boxes[b], int(nbox[b]), img_dim[b], pad_hw, C, stride, min_overlap):
            if not rec["kept"]:
                continue
            dy, dx, r = ys - rec["cy"], xs - rec["cx"], rec["r"]
            here = (dy == 0) & (dx == 0)
            out[b, ..., :4] = np.where(here[..., None], rec["off4"].astype(np.float64), out[b, ..., :4])
            sigma = (2 * r + 1) / 6.0
            d2 = np.ascontiguousarray((dy * dy + dx * dx).astype(np.float64))
            g = np.exp(-d2 / (2 * sigma * sigma))
            inside = (np.abs(dy) <= r) & (np.abs(dx) <= r)
            ch = 4 + rec["cls"]
            out[b, ..., ch] = np.maximum(out[b, ..., ch], np.where(inside, g, 0.0))
    return out


def assign_scatter(boxes, nbox, img_dim, pad_hw, C, stride, min_overlap=0.7):
    """The same map written the way mmdet's gen_gaussian_target does: paste a (2r+1)^2 patch, clipped to
    the map, with np.maximum.  Independent of assign_gather but for box_records."""
    B = len(nbox)
    hm, wm = int(pad_hw[0]) // stride, int(pad_hw[1]) // stride
    out = np.zeros((B, hm, wm, 4 + C), np.float64)
    for b in range(B):
        for rec in box_records(boxes[b], int(nbox[b]), img_dim[b], pad_hw, C, stride, min_overlap):
            if not rec["kept"]:
                continue
            cy, cx, r = rec["cy"], rec["cx"], rec["r"]
            out[b, cy, cx, :4] = rec["off4"]
            sigma = (2 * r + 1) / 6.0
            y, x = np.ogrid[-r:r + 1, -r:r + 1]
            patch = np.exp(-np.ascontiguousarray((x * x + y * y).astype(np.float64)) / (2 * sigma * sigma))
            left, right = min(cx, r), min(wm - cx, r + 1)
            top, bottom = min(cy, r), min(hm - cy, r + 1)
            heat = out[b, cy - top:cy + bottom, cx - left:cx + right, 4 + rec["cls"]]
            np.maximum(heat, patch[r - top:r + bottom, r - left:r + right], out=heat)
    return out


def npos_ref(targets, C):
    """Number of (cell, class) entries equal to 1.0 per image."""
    t = np.asarray(targets)
    return (t.reshape(t.shape[0], -1, 4 + C)[..., 4:] == 1.0).sum((1, 2)).astype(np.int32)


def loss64(pred, targets, npos, C, alpha=2.0, beta=4.0):
    """[B, 2] = (cls, reg) in float64 torch: pred [B, P, >= 4+C] (box 0..3, class logits 4..4+C), targets
    [B, P, 4+C], npos [B].  Penalty-reduced focal loss over every class entry, L1 over the box channels of
    the cells with a class target of exactly 1, both divided by max(npos, 1)."""
    x = pred[..., 4:4 + C]
    y = targets[..., 4:]
    one = y == 1.0
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    nlp, nlq = -torch.nn.functional.logsigmoid(x), -torch.nn.functional.logsigmoid(-x)
    cls = torch.where(one, q ** alpha * nlp, (1.0 - y) ** beta * p ** alpha * nlq)
    cell = one.any(-1, keepdim=True)
    reg = torch.where(cell, (targets[..., :4] - pred[..., :4]).abs(), torch.zeros_like(pred[..., :4]))
    N = torch.clamp(torch.as_tensor(npos, dtype=torch.float64), min=1.0)
    return torch.stack([cls.sum((1, 2)) / N, reg.sum((1, 2)) / N], 1)


def loss_and_grad64(pred32, targets32, npos, C, alpha=2.0, beta=4.0, cls_scale=1.0, reg_scale=1.0):
    """(losses [B,2] float64 numpy, d(cls_scale*cls + reg_scale*reg)/d(pred) float64 numpy) of fp32 inputs."""
    pred = torch.as_tensor(pred32).double().clone().requires_grad_(True)
    L = loss64(pred, torch.as_tensor(targets32).double(), npos, C, alpha, beta)
    (cls_scale * L[:, 0].sum() + reg_scale * L[:, 1].sum()).backward()
    return L.detach().numpy(), pred.grad.numpy()


# ---- scenes ------------------------------------------------------------------------------------------
def _hand_groups(hm, wm, C):
    """Hand-placed boxes in cell units (cy, cx, h, w, label); the boxes of a group share an image."""
    c1 = min(1, C - 1)
    groups = [
        [(hm // 2, wm // 2, 3, 3, 0)],                                         # r = 0
        [(2, 3, 70, 70, 0)],                                                   # r >= 5, clipped top and left
        [(hm - 3, wm - 2, 120, 120, c1)],                                      # r >= 9, clipped bottom and right
        [(hm // 2, wm // 4, 20, 20, C - 1), (hm // 2, wm // 4 + 2, 20, 21, C - 1)],   # overlapping discs, one class
        [(hm // 4, wm // 2, 10, 10, C - 1), (hm // 4, wm // 2, 6, 14, C - 1)],        # one centre cell, one class
        [(hm + 2, 5, 4, 4, 0)],                                                # centre outside the map
        [(5, 5, 4, 4, C), (6, 7, 5, 4, -1)],                                   # labels outside [0, C)
    ]
    if C >= 2:
        groups.insert(5, [(3 * hm // 4, wm // 2, 12, 8, 0), (3 * hm // 4, wm // 2, 9, 9, 1)])   # ..., two classes
    return groups


@functools.lru_cache(maxsize=None)
def scene_batch(seeds, pad_h, pad_w, C, n_box, stride=4, min_overlap=0.7):
    """One image per seed -> (boxes [B, n_box, 5] f32 normalised (yc, xc, h, w, label), nbox [B] i32,
    img_dim [B, 2] f32); the last image has no box.  The hand-placed groups are dealt round the other
    images, random boxes fill each up to n_box.  Images alternate between filling the pad and sitting 8
    px inside it (H == W whenever the pad is square).  What the batch must contain is asserted below on
    box_records' own output.  The arrays are shared between callers: do not write to them."""
    seeds = tuple(seeds)
    B = len(seeds)
    assert B >= 2
    hm, wm = pad_h // stride, pad_w // stride
    boxes = np.zeros((B, n_box, 5), F)
    nbox = np.zeros(B, np.int32)
    dims = np.array([[pad_h - 8 * (b % 2), pad_w - 8 * (b % 2)] for b in range(B)], F)
    cells = [[] for _ in range(B)]
    for g, group in enumerate(_hand_groups(hm, wm, C)):
        cells[g % (B - 1)].extend(group)
    for b in range(B - 1):
        assert len(cells[b]) <= n_box, "n_box too small for the hand-placed boxes"
        rng = np.random.default_rng(seeds[b])
        while len(cells[b]) < n_box:
            h, w = np.exp(rng.uniform(np.log(2.0), np.log(40.0), 2))
            cells[b].append((int(rng.integers(0, hm)), int(rng.integers(0, wm)), float(h), float(w),
                             int(rng.integers(0, C))))
        H, W = float(dims[b, 0]), float(dims[b, 1])
        py, px = int((pad_h - H) / 2), int((pad_w - W) / 2)
        for i, (cy, cx, h, w, lab) in enumerate(cells[b]):
            boxes[b, i] = [((cy + 0.5) * stride - py) / H, ((cx + 0.5) * stride - px) / W, h * stride / H,
                           w * stride / W, lab]
        nbox[b] = n_box
    _check_scene(boxes, nbox, dims, (pad_h, pad_w), C, stride, min_overlap)
    for a in (boxes, nbox, dims):
        a.setflags(write=False)
    return boxes, nbox, dims


def _check_scene(boxes, nbox, dims, pad_hw, C, stride, m):
    hm, wm = pad_hw[0] // stride, pad_hw[1] // stride
    recs = [box_records(boxes[b], int(nbox[b]), dims[b], pad_hw, C, stride, m) for b in range(len(nbox))]
    kept = [[r for r in rs if r["kept"]] for rs in recs]
    flat = [r for rs in kept for r in rs]
    assert any(r["r"] == 0 for r in flat) and any(r["r"] >= 5 for r in flat) and any(r["r"] >= 9 for r in flat)
    overlap = same = other = False
    for rs in kept:
        for i, p in enumerate(rs):
            for q in rs[i + 1:]:
                at_one = (p["cy"], p["cx"]) == (q["cy"], q["cx"])
                same |= at_one and p["cls"] == q["cls"]
                other |= at_one and p["cls"] != q["cls"]
                overlap |= (not at_one and p["cls"] == q["cls"] and abs(p["cy"] - q["cy"]) <= p["r"] + q["r"]
                            and abs(p["cx"] - q["cx"]) <= p["r"] + q["r"])
    assert overlap and same and (other or C < 2)
    assert any(r["cy"] - r["r"] < 0 for r in flat) and any(r["cy"] + r["r"] >= hm for r in flat)
    assert any(r["cx"] - r["r"] < 0 for r in flat) and any(r["cx"] + r["r"] >= wm for r in flat)
    every = [r for rs in recs for r in rs]
    assert any(r["cls"] >= 0 and not (0 <= r["cy"] < hm and 0 <= r["cx"] < wm) for r in every)
    assert any(r["cls"] < 0 for r in every)
    assert int(nbox[-1]) == 0 and all(len(k) >= 1 for k in kept[:-1])


@functools.lru_cache(maxsize=None)
def scene_targets(seeds, pad_h, pad_w, C, n_box, stride=4, min_overlap=0.7):
    """(scene_batch(...), assign_gather of it), computed once per argument set; read-only."""
    scene = scene_batch(tuple(seeds), pad_h, pad_w, C, n_box, stride, min_overlap)
    t = assign_gather(scene[0], scene[1], scene[2], (pad_h, pad_w), C, stride, min_overlap)
    t.setflags(write=False)
    return scene, t
