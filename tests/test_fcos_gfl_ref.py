"""Pins tests/fcos_gfl_ref.py, the float64 restatement the GPU tests of the Generalized Focal Loss
compare against: hand-worked cells, the closed-form gradients against autograd, the constants of the
gradient (q and w), and the conditions of the input builder (CPU)."""
import math

import numpy as np
import pytest
import torch

import fcos_gfl_ref as ref

f64 = torch.float64


def _cell(C, R, t, z, x, cls_index=0):
    """One positive cell: targets [1,1,5+C], reg [1,1,4(R+1)], cls [1,1,C] as float64 tensors."""
    tg = np.zeros((1, 1, 5 + C))
    tg[0, 0, :4] = t
    tg[0, 0, 4] = 0.123                                   # not read
    tg[0, 0, 5 + cls_index] = 1.0
    reg = torch.tensor(np.asarray(z, np.float64).reshape(1, 1, 4 * (R + 1)), requires_grad=True)
    cls = torch.tensor(np.asarray(x, np.float64).reshape(1, 1, C), requires_grad=True)
    return tg, reg, cls


def _bce(x, y):
    return max(x, 0.0) - x * y + math.log1p(math.exp(-abs(x)))


def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def test_one_hot_distribution_on_its_target():
    """Each side's mass on one bin, the targets on those bins: d = t, IoU = GIoU = 1, DFL ~ 0, and the
    QFL of the positive class has target 1."""
    C, R = 3, 7
    bins = [2, 5, 0, 6]                                   # (bin R itself lies above the clamp R - 0.1)
    z = np.zeros((4, R + 1))
    for j, k in enumerate(bins):
        z[j, k] = 60.0
    x = [0.3, -1.2, 2.0]
    tg, reg, cls = _cell(C, R, bins, z, x, cls_index=1)
    np.testing.assert_allclose(ref.gfl_decode(reg.detach(), R).numpy()[0, 0], bins, atol=1e-20)
    L = ref.gfl_loss(reg, cls, tg, C, R).detach().numpy()[0]
    s = [_sig(v) for v in x]
    want_qfl = s[0] ** 2 * _bce(x[0], 0.0) + (1.0 - s[1]) ** 2 * _bce(x[1], 1.0) + s[2] ** 2 * _bce(x[2], 0.0)
    np.testing.assert_allclose(L[0], want_qfl, rtol=1e-12)
    assert abs(L[1]) < 1e-12                               # box: w_box w (1 - GIoU), GIoU = 1 (up to the 1e-12 terms)
    assert 0.0 <= L[2] < 1e-24                             # dfl: lse - z[yl] = log(1 + R e^-60)


def test_two_bin_split_reaches_the_entropy_of_its_target():
    """p = (wl, wr) on the two bins about t: d = t exactly and the DFL is at its minimum, the entropy of
    (wl, wr); the weights w and w_dfl / Wsum multiply it."""
    C, R = 1, 16
    t = [2.3, 10.75, 0.5, 15.2]
    z = np.full((4, R + 1), -800.0)                       # exp underflows to exactly 0
    ent = 0.0
    for j, tj in enumerate(t):
        k = int(math.floor(tj))
        wl, wr = k + 1 - tj, tj - k
        z[j, k], z[j, k + 1] = math.log(wl), math.log(wr)
        ent -= wl * math.log(wl) + wr * math.log(wr)
    x = [0.7]
    tg, reg, cls = _cell(C, R, t, z, x)
    np.testing.assert_allclose(ref.gfl_decode(reg.detach(), R).numpy()[0, 0], t, rtol=1e-14)
    c = ref.gfl_cell_terms(reg, cls, tg, C, R)
    np.testing.assert_allclose(float(c["dfl"].detach()[0, 0]), 0.25 * ent, rtol=1e-13)
    np.testing.assert_allclose(float(c["q"][0, 0]), 1.0, rtol=1e-12)
    norm = np.array([[1.0, 0.4]], np.float32)
    L = ref.gfl_loss(reg, cls, tg, C, R, norm=norm, w_dfl=0.5).detach().numpy()[0]
    np.testing.assert_allclose(L[2], 0.5 * _sig(0.7) * 0.25 * ent / float(np.float32(0.4)), rtol=1e-13)


def test_target_above_the_clamp():
    """t > R - 0.1 is clamped to the fp32 value (float)R - 0.1f: bins R-1 and R with weights 0.1 / 0.9
    (as fp32 rounds them), whatever t was."""
    C, R = 1, 7
    bound = ref.clamp_bound(R)
    assert bound == float(np.float32(7) - np.float32(0.1)) and bound != 6.9 and abs(bound - 6.9) < 1e-6
    rng = np.random.default_rng(0)
    z = rng.normal(0, 1, (4, R + 1))
    for t_hi in (6.95, 7.0, 10.0, 1e6):
        t = [1.5, t_hi, 2.0, 3.25]
        tg, reg, cls = _cell(C, R, t, z, [0.0])
        c = ref.gfl_cell_terms(reg, cls, tg, C, R)
        want = 0.0
        for j, tj in enumerate(t):
            tc = min(max(tj, 0.0), bound)
            k = int(math.floor(tc))
            lse = math.log(np.exp(z[j]).sum())
            want += (k + 1 - tc) * (lse - z[j, k]) + (tc - k) * (lse - z[j, k + 1])
        np.testing.assert_allclose(float(c["dfl"].detach()[0, 0]), 0.25 * want, rtol=1e-13)
        il, wl, wr = ref.dfl_bins(torch.tensor([t_hi], dtype=f64), R)
        assert int(il) == R - 1 and float(wl) == R - bound and float(wr) == bound - (R - 1)
    il, wl, wr = ref.dfl_bins(torch.tensor([-3.0, 0.0, 4.0], dtype=f64), R)       # below 0, and on a bin
    assert il.tolist() == [0, 0, 4] and wl.tolist() == [1.0, 1.0, 1.0] and wr.tolist() == [0.0, 0.0, 0.0]


def test_image_without_positives():
    C, R = 4, 3
    rng = np.random.default_rng(1)
    tg = np.zeros((1, 5, 5 + C))
    reg = torch.tensor(rng.normal(0, 1, (1, 5, 4 * (R + 1))), requires_grad=True)
    cls = torch.tensor(rng.normal(0, 2, (1, 5, C)), requires_grad=True)
    x = cls.detach().numpy()
    want = (1.0 / (1.0 + np.exp(-x))) ** 2 * (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x))))
    for norm in (None, np.zeros((1, 2), np.float32)):      # N = max(0, 1), Wsum = max(0, 1e-6)
        L = ref.gfl_loss(reg, cls, tg, C, R, norm=norm)
        np.testing.assert_allclose(L.detach().numpy()[0], [want.sum(), 0.0, 0.0], rtol=1e-13)
        g_reg, = torch.autograd.grad(L.sum(), reg, allow_unused=True)
        assert g_reg is None or not bool(g_reg.any())
    np.testing.assert_array_equal(ref.gfl_norm(cls.detach(), tg, C), [[0.0, 0.0]])


@pytest.fixture(scope="module")
def batch():
    C, R = 3, 7
    inp = ref.make_inputs(C, R, seed=5)
    norm = ref.gfl_norm(inp["cls"], inp["targets"], C).astype(np.float32)
    return C, R, inp, norm


def test_closed_form_gradients_equal_autograd(batch):
    C, R, inp, norm = batch
    NB = 4 * (R + 1)
    L, d_reg, d_cls = ref.gfl_reference(inp, C, R, norm=norm)
    c = ref.gfl_cell_terms(inp["reg"][..., :NB], inp["cls"][..., :C], inp["targets"], C, R)
    N = np.maximum(norm[:, 0], 1.0).astype(np.float64)[:, None, None]
    Wsum = np.maximum(norm[:, 1], np.float32(1e-6)).astype(np.float64)[:, None, None, None]
    # QFL at beta 2: (s - y) [2 s (1 - s) BCE + (s - y)^2] / N
    x = torch.as_tensor(inp["cls"][..., :C].astype(np.float64))
    s, y = torch.sigmoid(x), c["y"]
    bce = torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    want = ((s - y) * (2 * s * (1 - s) * bce + (s - y) ** 2)).numpy() / N
    np.testing.assert_allclose(d_cls[..., :C], want, rtol=1e-10, atol=1e-300)
    assert not d_cls[..., C:].any() and not d_reg[..., NB:].any()
    # DFL alone (w_box = 0): w (w_dfl / Wsum) 0.25 (p - wl e_yl - wr e_yr) on the positives, zero elsewhere
    _, d_dfl, _ = ref.gfl_reference(inp, C, R, norm=norm, w_box=0.0, w_dfl=0.25)
    il, wl, wr = ref.dfl_bins(torch.as_tensor(inp["targets"][..., :4].astype(np.float64)), R)
    hot = torch.zeros_like(c["p"])
    hot.scatter_(-1, il[..., None], wl[..., None])
    hot.scatter_add_(-1, (il + 1)[..., None], wr[..., None])
    want = (c["w"][..., None, None] * 0.25 * 0.25 * (c["p"] - hot)).numpy() / Wsum
    want = np.where(c["pos"].numpy()[..., None, None], want, 0.0).reshape(d_dfl.shape[:2] + (NB,))
    np.testing.assert_allclose(d_dfl[..., :NB], want, rtol=1e-9, atol=1e-18)
    # non-positive cells: all-zero box rows in the full gradient too
    assert not d_reg[~c["pos"].numpy()].any() and d_reg[c["pos"].numpy()].any()
    assert L.shape == (3, 3) and L[2, 1] == 0.0 and L[2, 2] == 0.0 and (L[:2] > 0).all()


def test_q_and_w_are_constants_of_the_gradient(batch):
    C, R, inp, norm = batch
    NB = 4 * (R + 1)
    _, _, d_cls = ref.gfl_reference(inp, C, R, norm=norm)
    # a per-side shift of the box logits leaves every softmax, hence d and q, where it was: the class
    # gradient does not move
    moved = dict(inp)
    shift = np.random.default_rng(2).normal(0, 3, inp["reg"].shape[:2] + (4, 1))
    z = inp["reg"][..., :NB].astype(np.float64).reshape(inp["reg"].shape[:2] + (4, R + 1)) + shift
    moved["reg"] = inp["reg"].astype(np.float64)
    moved["reg"][..., :NB] = z.reshape(inp["reg"].shape[:2] + (NB,))
    _, _, d_cls2 = ref.gfl_reference(moved, C, R, norm=norm)
    np.testing.assert_allclose(d_cls2, d_cls, rtol=1e-9, atol=1e-15)
    # ... and moves when q moves
    other = dict(inp)
    other["reg"] = inp["reg"].copy()
    other["reg"][..., :NB] += np.random.default_rng(3).normal(0, 1, inp["reg"][..., :NB].shape).astype(np.float32)
    _, _, d_cls3 = ref.gfl_reference(other, C, R, norm=norm)
    assert np.abs(d_cls3 - d_cls).max() > 1e-6
    # no gradient reaches the box logits through q, nor the class logits through w
    reg = torch.tensor(np.nan_to_num(inp["reg"]), dtype=f64, requires_grad=True)
    cls = torch.tensor(np.nan_to_num(inp["cls"]), dtype=f64, requires_grad=True)
    L = ref.gfl_loss(reg, cls, inp["targets"], C, R, norm=norm)
    g, = torch.autograd.grad(L[:, 0].sum(), reg, retain_graph=True, allow_unused=True)
    assert g is None or not bool(g.any())
    g, = torch.autograd.grad(L[:, 1:].sum(), cls, allow_unused=True)
    assert g is None or not bool(g.any())


@pytest.mark.parametrize("C,R", [(20, 16), (3, 7), (1, 1), (80, 16)])
def test_builder_conditions(C, R):
    inp = ref.make_inputs(C, R, seed=C * 100 + R)
    tg, reg, cls = inp["targets"], inp["reg"], inp["cls"]
    NB = 4 * (R + 1)
    assert tg.shape == (3, ref.P_CELLS, 5 + C) and ref.P_CELLS == 1022
    assert reg.shape[2] == (NB + 7) // 8 * 8 and cls.shape[2] == (C + 7) // 8 * 8
    assert np.isnan(reg[..., NB:]).all() and np.isnan(cls[..., C:]).all()
    assert np.isfinite(reg[..., :NB]).all() and np.isfinite(cls[..., :C]).all()
    pos = ref.positives(tg, C).numpy()
    frac = pos[:2].mean()
    assert 0.05 < frac < 0.12 and not pos[2].any() and pos[0].any() and pos[1].any()
    assert (tg[~pos] == 0).all()
    d = ref.gfl_decode(reg, R).numpy()[pos]
    t = tg[pos][:, :4].astype(np.float64)
    gap = np.abs(d - t).min(1)
    print("C %d R %d: %d positives, min gap %.2e, sides above the clamp %.1f %%"
          % (C, R, pos.sum(), gap.min(), 100 * (t > R - 0.1).mean()))
    assert gap.min() >= ref.MIN_GAP
    assert 0.05 <= (t > R - 0.1).mean() <= 0.40
    hot = [reg[b, p, :NB] for b, p in inp["hot_box"]]
    assert len(hot) >= 5 and all(pos[b, p] for b, p in inp["hot_box"]) and all((np.abs(h) == 60).all() for h in hot)
    hotc = [cls[b, p, :C] for b, p in inp["hot_cls"]]
    assert len(hotc) >= 5 and all((np.abs(h) == 40).all() for h in hotc)
    assert any(pos[b, p] for b, p in inp["hot_cls"]) and any(not pos[b, p] for b, p in inp["hot_cls"])
    again = ref.make_inputs(C, R, seed=C * 100 + R)
    assert all(np.array_equal(inp[k], again[k], equal_nan=True) for k in ("reg", "cls", "targets"))
    # other leading dimensions on request
    wide = ref.make_inputs(C, R, seed=1, ld_reg=96, ld_cls=C + 12)
    assert wide["reg"].shape[2] == 96 and wide["cls"].shape[2] == C + 12
