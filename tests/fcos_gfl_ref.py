"""Generalized Focal Loss for the FCOS head, the rule of include/cvlite.h (cvl_fcos_gfl_norm,
cvl_fcos_gfl_loss, cvl_fcos_gfl_decode) restated in float64 torch.  gfl_loss is differentiable in the
box and class logits, with the IoU target q and the weight w detached as the rule says, so autograd
gives the reference gradients.  make_inputs builds the batch the GPU tests run on; its conditions
(checked in tests/test_fcos_gfl_ref.py) keep the fp32 kernel and this restatement on the same branch
of every min / max of the GIoU.  Importing it needs no GPU."""
import numpy as np
import torch

PAD = (256, 192)
STRIDES = (8, 16, 32, 64, 128)
P_CELLS = sum((PAD[0] // s) * (PAD[1] // s) for s in STRIDES)      # 1022: no multiple of any tile
f64 = torch.float64


def clamp_bound(R):
    """The upper clamp of the DFL target: the fp32 value (float)R - 0.1f."""
    return float(np.float32(R) - np.float32(0.1))


def _t64(a):
    return a.to(f64) if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a), dtype=f64)


def _sides(reg, R):
    return reg[..., :4 * (R + 1)].reshape(tuple(reg.shape[:-1]) + (4, R + 1))


def gfl_decode(reg, R):
    """reg [..., >= 4(R+1)] -> [..., 4] float64: d_j = sum_i i softmax(z[j])_i (max-subtracted)."""
    z = _sides(_t64(reg), R)
    p = torch.softmax(z - z.max(-1, keepdim=True).values, -1)
    return (p * torch.arange(R + 1, dtype=f64)).sum(-1)


def positives(targets, C):
    return _t64(targets)[..., 5:5 + C].max(-1).values >= 1


def gfl_norm(cls, targets, C):
    """[B, 2] float64 = (number of positive cells, sum over them of sigmoid(max_c x_c))."""
    pos = positives(targets, C)
    w = torch.sigmoid(_t64(cls)[..., :C].max(-1).values)
    return torch.stack([pos.to(f64).sum(1), torch.where(pos, w, torch.zeros_like(w)).sum(1)], 1).numpy()


def giou_parts(t, d):
    """(I, U, E, GIoU) of ltrb boxes about one point; t, d [..., 4] = (top, bottom, left, right)."""
    th, tw = t[..., 0] + t[..., 1], t[..., 2] + t[..., 3]
    ph, pw = d[..., 0] + d[..., 1], d[..., 2] + d[..., 3]
    mn, mx = torch.minimum(t, d), torch.maximum(t, d)
    I = (mn[..., 0] + mn[..., 1]) * (mn[..., 2] + mn[..., 3])
    U = th * tw + ph * pw - I + 1e-12
    E = (mx[..., 0] + mx[..., 1]) * (mx[..., 2] + mx[..., 3]) + 1e-12
    return I, U, E, I / U - (E - U) / E


def dfl_bins(t, R):
    """(yl as int64, wl, wr) of the clamped distance."""
    tc = torch.clamp(t, 0.0, clamp_bound(R))
    yl = torch.floor(tc)
    return yl.long(), (yl + 1.0) - tc, tc - yl


def gfl_cell_terms(reg, cls, targets, C, R, beta=2.0):
    """Per-cell pieces, all float64: dict(pos [B,P], q, w (detached), qfl [B,P,C], box = 1 - GIoU,
    dfl = dfl_cell [B,P], d [B,P,4])."""
    reg, cls, tg = _t64(reg), _t64(cls), _t64(targets)
    x = cls[..., :C]
    z = _sides(reg, R)
    hot = tg[..., 5:5 + C] >= 1
    pos = hot.any(-1)
    zs = z - z.max(-1, keepdim=True).values.detach()
    p = torch.softmax(zs, -1)
    d = (p * torch.arange(R + 1, dtype=f64)).sum(-1)
    t = tg[..., :4]
    I, U, E, giou = giou_parts(t, d)
    q = (I / U).detach()
    w = torch.sigmoid(x.max(-1).values).detach()
    y = torch.where(pos[..., None] & hot, q[..., None].expand_as(x), torch.zeros_like(x))
    s = torch.sigmoid(x)
    bce = torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    qfl = (y - s).abs() ** beta * bce
    il, wl, wr = dfl_bins(t, R)
    lse = torch.logsumexp(z, -1)
    zl = z.gather(-1, il[..., None])[..., 0]
    zr = z.gather(-1, (il + 1)[..., None])[..., 0]
    dfl = 0.25 * (wl * (lse - zl) + wr * (lse - zr)).sum(-1)
    return dict(pos=pos, q=q, w=w, qfl=qfl, box=1.0 - giou, dfl=dfl, d=d, p=p, y=y)


def gfl_loss(reg, cls, targets, C, R, norm=None, beta=2.0, w_box=2.0, w_dfl=0.25):
    """losses [B, 3] float64 = (qfl, box, dfl) per image.  norm [B, 2] as gfl_norm gives it (the fp32
    values the kernel reads), or None for N = Wsum = 1."""
    c = gfl_cell_terms(reg, cls, targets, C, R, beta)
    B = c["pos"].shape[0]
    N, Wsum = torch.ones(B, dtype=f64), torch.ones(B, dtype=f64)
    if norm is not None:
        nm = np.asarray(norm, np.float32)
        N = torch.as_tensor(np.maximum(nm[:, 0], np.float32(1.0)).astype(np.float64))
        Wsum = torch.as_tensor(np.maximum(nm[:, 1], np.float32(1.0e-6)).astype(np.float64))
    zero = torch.zeros_like(c["dfl"])
    box = torch.where(c["pos"], c["w"] * c["box"], zero).sum(1)
    dfl = torch.where(c["pos"], c["w"] * c["dfl"], zero).sum(1)
    return torch.stack([c["qfl"].sum((1, 2)) / N, w_box * box / Wsum, w_dfl * dfl / Wsum], 1)


def gfl_reference(inp, C, R, norm=None, grad_scale=1.0, **kw):
    """(losses [B,3], d_reg, d_cls) float64 numpy of an input dict of make_inputs: the gradients of
    grad_scale * sum(losses), full padded rows (the padding columns zero)."""
    reg = torch.tensor(np.nan_to_num(inp["reg"], nan=0.0), dtype=f64, requires_grad=True)
    cls = torch.tensor(np.nan_to_num(inp["cls"], nan=0.0), dtype=f64, requires_grad=True)
    L = gfl_loss(reg, cls, inp["targets"], C, R, norm=norm, **kw)
    (grad_scale * L.sum()).backward()
    return L.detach().numpy(), reg.grad.numpy(), cls.grad.numpy()


# ---- the input builder ---------------------------------------------------------------------------------
MIN_GAP = 1.0e-3          # every positive: min_j |d_j - t_j| >= MIN_GAP
POS_FRACTION = 0.08


def _draw_logits(rng, t, R):
    """One cell's [4, R+1] logits: noise plus a bump near each side's target bin."""
    z = rng.normal(0.0, 2.0, (4, R + 1))
    for j in range(4):
        z[j, int(round(min(max(t[j], 0.0), R)))] += 3.0
    return z


def make_inputs(C, R, seed=0, B=3, P=P_CELLS, ld_reg=None, ld_cls=None, pad_value=np.nan):
    """dict(reg [B,P,ld_reg], cls [B,P,ld_cls], targets [B,P,5+C]) float32 and `extreme` = the cells with
    saturated logits.  About POS_FRACTION of the cells of every image but the last are positive (the last
    has none); their distances are U(0.05, 1.25 R), so a fifth or more of the sides lie above R - 0.1;
    some positive rows hold box logits of +-60 and some cells class logits of +-40; the padding columns
    hold pad_value (NaN: a kernel that read them would show it).  Cells whose expected distance falls
    within MIN_GAP of its target are redrawn."""
    rng = np.random.default_rng(seed)
    NB = 4 * (R + 1)
    ld_reg = (NB + 7) // 8 * 8 if ld_reg is None else ld_reg
    ld_cls = (C + 7) // 8 * 8 if ld_cls is None else ld_cls
    assert ld_reg >= NB and ld_cls >= C
    tg = np.zeros((B, P, 5 + C), np.float32)
    reg = np.full((B, P, ld_reg), pad_value, np.float32)
    cls = np.full((B, P, ld_cls), pad_value, np.float32)
    reg[..., :NB] = rng.normal(0.0, 2.0, (B, P, NB))
    cls[..., :C] = rng.normal(0.0, 2.0, (B, P, C)) - 2.0
    pos = rng.random((B, P)) < POS_FRACTION
    pos[B - 1] = False
    cells = np.argwhere(pos)
    for b, p in cells:
        tg[b, p, :4] = rng.uniform(0.05, 1.25 * R, 4)
        tg[b, p, 4] = rng.uniform(0.0, 1.0)              # not read by the rule
        tg[b, p, 5 + rng.integers(0, C)] = 1.0
    hot_box = [tuple(c) for c in cells[rng.choice(len(cells), 6, replace=False)]]
    todo = [tuple(c) for c in cells]
    while todo:
        for b, p in todo:
            if (b, p) in hot_box:
                reg[b, p, :NB] = rng.choice([-60.0, 60.0], NB)
                tg[b, p, :4] = rng.uniform(0.05, 1.25 * R, 4)
            else:
                reg[b, p, :NB] = _draw_logits(rng, tg[b, p, :4], R).reshape(-1)
        idx = np.array(todo)
        d = gfl_decode(reg[idx[:, 0], idx[:, 1]], R).numpy()
        gap = np.abs(d - tg[idx[:, 0], idx[:, 1], :4].astype(np.float64)).min(1)
        todo = [todo[i] for i in np.nonzero(gap < 2 * MIN_GAP)[0]]
    hot_cls = [tuple(c) for c in cells[rng.choice(len(cells), 4, replace=False)]]
    hot_cls += [(int(rng.integers(0, B)), int(rng.integers(0, P))) for _ in range(6)]
    for b, p in hot_cls:
        cls[b, p, :C] = rng.choice([-40.0, 40.0], C)
    return dict(reg=reg, cls=cls, targets=tg, hot_box=hot_box, hot_cls=hot_cls)
