"""Restatement of the task-aligned assignment and its loss (include/cvlite.h, "Task-aligned assignment")
that the GPU tests compare csrc/fcos_tal.hip against.  The geometry the rule states as a fixed fp32
sequence of IEEE operations (box corners, grid points, the inside test, the intersection and the union)
is evaluated in numpy float32, which is exact; everything a library function or a chain of products
rounds (the sigmoid, the powers, the metric, the IoU quotient, slot 4, the loss and its gradients) is
float64.  Plain loops over images and boxes, an exhaustive sort for the top-k.  tal_loss is float64
torch, differentiable in the box and class outputs with the targets constant, so autograd gives the
reference gradients.  scene() builds the batches the tests run on and decided() says whether float64
can name every selection and every contest winner of a scene; tests/test_fcos_tal_ref.py pins this
file itself.  Importing it needs no GPU."""
import numpy as np
import torch

PAD = (256, 192)
STRIDES = (8, 16, 32, 64, 128)
f32 = np.float32
f64 = np.float64
N_MAX = 10
# fp32 may not tell a metric below this from 0 (its smallest normal number is 1.2e-38)
TINY = 1e-35


def level_shapes(pad_hw, strides=STRIDES):
    return [(int(pad_hw[0] // s), int(pad_hw[1] // s)) for s in strides]


def cell_grid(pad_hw, strides=STRIDES):
    """(gy [P], gx [P], sf [P], level [P]) fp32 / int of the level-major cells."""
    gy, gx, sf, lv = [], [], [], []
    half = f32(0.5)
    for l, (Hs, Ws) in enumerate(level_shapes(pad_hw, strides)):
        s = f32(strides[l])
        y = (np.arange(Hs, dtype=f32) + half) * s
        x = (np.arange(Ws, dtype=f32) + half) * s
        gy.append(np.repeat(y, Ws))
        gx.append(np.tile(x, Hs))
        sf.append(np.full(Hs * Ws, s, f32))
        lv.append(np.full(Hs * Ws, l, np.int64))
    return np.concatenate(gy), np.concatenate(gx), np.concatenate(sf), np.concatenate(lv)


def box_geometry(r, H, W):
    """(y0, y1, x0, x1, area) in pixels, fp32, the operation order of cvl_fcos_atss_assign."""
    half = f32(0.5)
    yc, xc, hp, wp = r[0] * H, r[1] * W, r[2] * H, r[3] * W
    return yc - hp * half, yc + hp * half, xc - wp * half, xc + wp * half, hp * wp


def box_label(r, C):
    """(int)label when the box takes part, else -1: the label must lie in [0, C) (NaN does not)."""
    with np.errstate(invalid="ignore"):
        if not (r[4] > f32(-1.0) and r[4] < f32(C)):
            return -1
    return int(r[4])


def _pow(v, e, plain):
    return v if e == plain else np.power(v, f64(e))


def pair_values(box, H, W, grid, dist, x, clamp, alpha, beta):
    """One box against every cell: (inside [P] bool, tbl [P,4] fp32 pixel distances, u [P] f64,
    m [P] f64), u and m zero outside the box.  dist [P,>=4] fp32, x [P] fp32 = the label's logits."""
    gy, gx, sf, _ = grid
    y0, y1, x0, x1, area = box
    eps, zero = f32(0.01), f32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        t, bt, l, r = gy - y0, y1 - gy, gx - x0, x1 - gx
        inside = (t > eps) & (bt > eps) & (l > eps) & (r > eps)
        d = np.fmax(dist[:, :4], zero) if clamp else dist[:, :4]
        py0, py1 = gy - d[:, 0] * sf, gy + d[:, 1] * sf
        px0, px1 = gx - d[:, 2] * sf, gx + d[:, 3] * sf
        ih = np.fmax(np.fmin(y1, py1) - np.fmax(y0, py0), zero)
        iw = np.fmax(np.fmin(x1, px1) - np.fmax(x0, px0), zero)
        inter = ih * iw
        uni = ((py1 - py0) * (px1 - px0) + area) - inter
        u = np.where(uni > 0, inter.astype(f64) / np.where(uni > 0, uni, f32(1)).astype(f64), 0.0)
        s = 1.0 / (1.0 + np.exp(-x.astype(f64)))
        m = _pow(s, alpha, 1.0) * np.power(u, f64(beta))
    u = np.where(inside, u, 0.0)
    m = np.where(inside, m, 0.0)
    return inside, np.stack([t, bt, l, r], 1), u, m


def tal_assign(boxes, nbox, img_dim, pad_hw, C, dist, cls, strides=STRIDES, topk=13, alpha=1.0, beta=6.0,
               clamp=True):
    """boxes [B,n_max,5] f32 (yc, xc, h, w, cls) normalised, nbox [B], img_dim [B,2] f32, dist [B,P,>=4]
    f32, cls [B,P,>=C] f32.  Returns a dict: targets [B,P,5+C] (columns 0..3 and 5.. exact fp32, slot 4
    float64 rounded to fp32), counts [B,5] i32, cand_cells [B,n_max,topk] i32, cand_metric / cand_iou
    [B,n_max,topk] f64, box_max [B,n_max,2] f64, owner [B,P] i32 (the winning box or -1), and for
    decided(): metrics (per valid box, every candidate's metric in descending order), contests (per
    cell selected by two boxes or more, the selecting boxes' u in descending order), inside [B,P] bool
    (the cell lies inside some valid box)."""
    boxes = np.asarray(boxes, f32)
    img_dim = np.asarray(img_dim, f32)
    dist = np.asarray(dist, f32)
    cls = np.asarray(cls, f32)
    B, n_max = boxes.shape[:2]
    grid = cell_grid(pad_hw, strides)
    P = grid[0].size
    targets64 = np.zeros((B, P, 5 + C), f64)
    counts = np.zeros((B, 5), np.int32)
    cand_cells = np.full((B, n_max, topk), -1, np.int32)
    cand_metric = np.zeros((B, n_max, topk), f64)
    cand_iou = np.zeros((B, n_max, topk), f64)
    box_max = np.zeros((B, n_max, 2), f64)
    owner = np.full((B, P), -1, np.int32)
    any_inside = np.zeros((B, P), bool)
    metrics, contests = [], []
    for b in range(B):
        H, W = img_dim[b, 0], img_dim[b, 1]
        n = min(max(int(nbox[b]), 0), n_max)
        best_u = np.full(P, -1.0, f64)
        nsel = np.zeros(P, np.int64)
        sel_u = [[] for _ in range(P)]
        tbl_of, m_of, lab_of = {}, {}, {}
        for i in range(n):
            r = boxes[b, i]
            lab = box_label(r, C)
            with np.errstate(invalid="ignore", over="ignore"):
                box = box_geometry(r, H, W)
            if lab < 0 or not box[4] > 0:
                continue
            inside, tbl, u, m = pair_values(box, H, W, grid, dist[b], cls[b, :, lab], clamp, alpha, beta)
            any_inside[b] |= inside
            cand = np.nonzero(inside & (m > 0))[0]           # a NaN metric is not > 0
            order = cand[np.lexsort((cand, -m[cand]))]       # largest m, ties to the lowest cell
            metrics.append(m[order])
            sel = order[:topk]
            cand_cells[b, i, :sel.size] = sel
            cand_metric[b, i, :sel.size] = m[sel]
            cand_iou[b, i, :sel.size] = u[sel]
            tbl_of[i], m_of[i], lab_of[i] = tbl, m, lab
            for p in sel:
                sel_u[p].append(u[p])
                nsel[p] += 1
                if u[p] > best_u[p]:                         # strict: ties keep the lowest box index
                    best_u[p] = u[p]
                    owner[b, p] = i
        for p in np.nonzero(nsel >= 2)[0]:
            contests.append(np.sort(np.array(sel_u[p]))[::-1])
        for i in tbl_of:
            won = np.nonzero(owner[b] == i)[0]
            if won.size:
                box_max[b, i] = (m_of[i][won].max(), best_u[won].max())
        gy, gx, sf, lv = grid
        for p in np.nonzero(owner[b] >= 0)[0]:
            i = owner[b, p]
            targets64[b, p, :4] = tbl_of[i][p] / sf[p]       # fp32 quotients, exact in the float64 array
            targets64[b, p, 4] = m_of[i][p] * box_max[b, i, 1] / (box_max[b, i, 0] + 1e-9)
            targets64[b, p, 5 + lab_of[i]] = 1.0
            counts[b, lv[p]] += 1
    return dict(targets=targets64.astype(f32), that=targets64[..., 4], counts=counts, cand_cells=cand_cells,
                cand_metric=cand_metric, cand_iou=cand_iou, box_max=box_max, owner=owner, metrics=metrics,
                contests=contests, inside=any_inside)


def decided_result(res, topk, margin=1e-3):
    """float64 names every selection and every winner of a tal_assign result: per box the metrics of rank
    k and k + 1 differ by more than `margin` relative for every selected rank k, no candidate's metric
    lies where fp32 may round it to 0, and at every contested cell the two best u differ by more than
    `margin` relative."""
    for m in res["metrics"]:
        if m.size and m.min() < TINY:
            return False
        k = min(topk, m.size)
        hi, lo = m[:k], m[1:k + 1]
        if not np.all(hi[:lo.size] - lo > margin * hi[:lo.size]):
            return False
    for u in res["contests"]:
        if not u[0] - u[1] > margin * u[0]:
            return False
    return True


# ---- scenes -------------------------------------------------------------------------------------------
def scene(seed, C, ld_dist=8, ld_cls=None, pad=PAD):
    """A batch of B = 3 images on `pad` with its head outputs.  The first image holds, in this order: one
    box covering the whole pad; one box smaller than a stride-8 cell that contains no grid point of any
    level (zero candidates); one small box with a handful of candidates (fewer than topk = 13); three
    overlapping boxes that contest cells with each other and with the whole-pad box; a NaN-label box; a
    zero-area box.  The second holds two more overlapping boxes, the third has nbox 0 (its rows are
    filled).  The box outputs are the distances to one of the image's boxes, chosen at random per cell,
    jittered multiplicatively and additively (some are negative); the class logits are N(-2, 2).  The
    padding columns of both hold a constant no rule reads.  Returns a dict of numpy arrays."""
    rng = np.random.default_rng(1000 + seed)
    H, W = float(pad[0]), float(pad[1])
    B = 3
    ld_cls = (C + 7) // 8 * 8 if ld_cls is None else ld_cls
    boxes = np.zeros((B, N_MAX, 5), f32)
    lab = lambda: float(rng.integers(0, C))   # noqa: E731

    def big():
        h, w = rng.uniform(50, 120), rng.uniform(45, 100)
        return (H / 2 + rng.uniform(-30, 30), W / 2 + rng.uniform(-20, 20), h, w, lab())
    rows0 = [(H / 2, W / 2, H, W, lab()),
             (128.0, W / 2 + rng.uniform(-20, 20), 4.0, 5.0, lab()),      # no level has a grid line at y = 128
             (rng.uniform(40, H - 40), rng.uniform(40, W - 40), rng.uniform(14, 22), rng.uniform(14, 22), lab()),
             big(), big(), big(),
             (H / 2, W / 2, 80.0, 80.0, float("nan")),
             (H / 2, W / 2, 0.0, 90.0, lab())]
    rows1 = [big(), big()]
    for b, rows in enumerate((rows0, rows1, rows0)):
        for k, (y, x, h, w, c) in enumerate(rows):
            boxes[b, k] = [y / H, x / W, h / H, w / W, c]
    nbox = np.array([len(rows0), len(rows1), 0], np.int32)
    valid = ([0, 2, 3, 4, 5], [0, 1], [0, 2, 3, 4, 5])
    dims = np.array([[H, W]] * B, f32)
    gy, gx, sf, _ = cell_grid(pad)
    P = gy.size
    dist = np.full((B, P, ld_dist), 7.0, f32)
    cls = np.full((B, P, ld_cls), 3.0, f32)
    for b in range(B):
        pick = rng.choice(valid[b], size=P)
        y0, y1, x0, x1, _ = box_geometry(boxes[b, pick].T, f32(H), f32(W))
        true = np.stack([gy - y0, y1 - gy, gx - x0, x1 - gx], 1) / sf[:, None]
        dist[b, :, :4] = true * np.exp(rng.normal(0, 0.35, (P, 4))) + rng.normal(0, 0.5, (P, 4))
        if ld_dist > 4:
            dist[b, :, 4] = rng.normal(0, 1, P)              # the head's centerness output
        cls[b, :, :C] = rng.normal(-2.0, 2.0, (P, C))
    return dict(boxes=boxes, nbox=nbox, dims=dims, dist=dist, cls=cls, pad=tuple(pad), C=C)


def scene_assign(sc, **kw):
    return tal_assign(sc["boxes"], sc["nbox"], sc["dims"], sc["pad"], sc["C"], sc["dist"], sc["cls"], **kw)


# the configurations the GPU tests run: (topk, clamp, alpha, beta)
CONFIGS = [(k, c, a, bt) for k in (1, 13, 32) for c in (1, 0) for (a, bt) in ((1.0, 6.0), (0.5, 2.0))]


def decided(sc, topk=13, clamp=True, alpha=1.0, beta=6.0, margin=1e-3):
    return decided_result(scene_assign(sc, topk=topk, clamp=bool(clamp), alpha=alpha, beta=beta), topk, margin)


def first_decided_seed(C, cfg, limit=2000):
    """The smallest seed whose scene is decided under cfg = (topk, clamp, alpha, beta): how SEEDS was made.
    A box's 32 best of a thousand candidates lie close together, so at topk 32 only a few per cent of the
    seeds qualify; at topk 13 about a quarter, at topk 1 nearly all."""
    for seed in range(limit):
        if decided(scene(seed, C), *cfg):
            return seed
    raise ValueError("no decided seed below %d" % limit)


# a pad whose P = 8525 cells are more than the kernel stages per box (6144), with a decided seed at C = 20 and
# the default configuration: its whole-pad box takes the recompute-per-round path
BIG_PAD = (640, 640)
BIG_SEED = 0

# (C, topk, clamp, alpha, beta) -> the seed of a scene that is decided under that configuration
# (tests/test_fcos_tal_ref.py checks every entry)
SEEDS = {
    (1, 1, 1, 1.0, 6.0): 0,
    (1, 1, 1, 0.5, 2.0): 0,
    (1, 1, 0, 1.0, 6.0): 0,
    (1, 1, 0, 0.5, 2.0): 0,
    (1, 13, 1, 1.0, 6.0): 1,
    (1, 13, 1, 0.5, 2.0): 2,
    (1, 13, 0, 1.0, 6.0): 0,
    (1, 13, 0, 0.5, 2.0): 0,
    (1, 32, 1, 1.0, 6.0): 1,
    (1, 32, 1, 0.5, 2.0): 309,
    (1, 32, 0, 1.0, 6.0): 0,
    (1, 32, 0, 0.5, 2.0): 304,
    (20, 1, 1, 1.0, 6.0): 0,
    (20, 1, 1, 0.5, 2.0): 0,
    (20, 1, 0, 1.0, 6.0): 0,
    (20, 1, 0, 0.5, 2.0): 0,
    (20, 13, 1, 1.0, 6.0): 0,
    (20, 13, 1, 0.5, 2.0): 3,
    (20, 13, 0, 1.0, 6.0): 0,
    (20, 13, 0, 0.5, 2.0): 0,
    (20, 32, 1, 1.0, 6.0): 4,
    (20, 32, 1, 0.5, 2.0): 65,
    (20, 32, 0, 1.0, 6.0): 7,
    (20, 32, 0, 0.5, 2.0): 6,
    (80, 1, 1, 1.0, 6.0): 0,
    (80, 1, 1, 0.5, 2.0): 0,
    (80, 1, 0, 1.0, 6.0): 0,
    (80, 1, 0, 0.5, 2.0): 0,
    (80, 13, 1, 1.0, 6.0): 1,
    (80, 13, 1, 0.5, 2.0): 0,
    (80, 13, 0, 1.0, 6.0): 1,
    (80, 13, 0, 0.5, 2.0): 3,
    (80, 32, 1, 1.0, 6.0): 2,
    (80, 32, 1, 0.5, 2.0): 272,
    (80, 32, 0, 1.0, 6.0): 2,
    (80, 32, 0, 0.5, 2.0): 484,
}


# ---- the loss -----------------------------------------------------------------------------------------
t64 = torch.float64


def _t(a):
    return a.to(t64) if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a), dtype=t64)


def tal_loss(reg, cls, targets, C, norm=None, qfl_beta=2.0, w_box=2.0):
    """losses [B,3] float64 torch = (cls, box, 0) per image.  norm [B,2] as cvl_fcos_target_norm writes it
    (the fp32 values the kernel reads), or None for W = 1.  The box outputs of non-positive cells are
    not read (they may be NaN)."""
    reg, cls, tg = _t(reg), _t(cls), _t(targets)
    x = cls[..., :C]
    hot = tg[..., 5:5 + C] >= 1
    pos = hot.any(-1)
    that = tg[..., 4]
    y = torch.where(hot, that[..., None].expand_as(x), torch.zeros_like(x))
    s = torch.sigmoid(x)
    bce = torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    qfl = (y - s).abs() ** qfl_beta * bce
    B = tg.shape[0]
    Wn = torch.ones(B, dtype=t64)
    if norm is not None:
        Wn = torch.as_tensor(np.maximum(np.asarray(norm, f32)[:, 1], f32(1.0)).astype(f64))
    p4 = torch.where(pos[..., None], reg[..., :4], torch.zeros_like(reg[..., :4]))
    d = torch.clamp(p4, min=0)
    t = tg[..., :4]
    th, tw = t[..., 0] + t[..., 1], t[..., 2] + t[..., 3]
    ph, pw = d[..., 0] + d[..., 1], d[..., 2] + d[..., 3]
    mn, mx = torch.minimum(t, d), torch.maximum(t, d)
    I = (mn[..., 0] + mn[..., 1]) * (mn[..., 2] + mn[..., 3])
    U = th * tw + ph * pw - I + 1e-12
    E = (mx[..., 0] + mx[..., 1]) * (mx[..., 2] + mx[..., 3]) + 1e-12
    giou = I / U - (E - U) / E
    box = torch.where(pos, that * (1.0 - giou), torch.zeros_like(giou)).sum(1)
    return torch.stack([qfl.sum((1, 2)) / Wn, w_box * box / Wn, torch.zeros_like(Wn)], 1)


def target_norm(targets, C):
    """[B,2] fp32 = (number of positive cells, sum of their slot 4), summed in float64."""
    tg = np.asarray(targets, f64)
    pos = tg[..., 5:5 + C].max(-1) >= 1
    return np.stack([pos.sum(1), np.where(pos, tg[..., 4], 0.0).sum(1)], 1).astype(f32)


def tal_loss_reference(reg, cls, targets, C, norm=None, grad_scale=1.0, **kw):
    """(losses [B,3], d_reg, d_cls) float64 numpy: the gradients of grad_scale * sum(losses), full padded
    rows (padding columns, column 4 of d_reg and the rows of non-positive cells zero)."""
    pos = np.asarray(targets, f64)[..., 5:5 + C].max(-1) >= 1
    reg64 = np.where(pos[..., None], np.asarray(reg, f64), 0.0)      # NaN rows of non-positives are not read
    r = torch.tensor(reg64, dtype=t64, requires_grad=True)
    c = torch.tensor(np.asarray(cls, f64), dtype=t64, requires_grad=True)
    losses = tal_loss(r, c, targets, C, norm=norm, **kw)
    (grad_scale * losses.sum()).backward()
    return losses.detach().numpy(), r.grad.numpy(), c.grad.numpy()
