"""tests/fcos_tal_ref.py pinned on the CPU: every committed seed is decided, the scenes contain the cases
they promise, the restated assignment does what the rule says on a hand-made case, and the restated
loss's autograd gradients agree with finite differences."""
import numpy as np
import pytest
import torch

import fcos_tal_ref as ref

f32 = np.float32


def test_every_committed_seed_is_decided():
    """Zero exceptions: under its configuration, every box's ranked metrics and every contested cell's two
    best IoUs of a committed scene differ by more than 1e-3 relative, and no metric is near fp32's zero."""
    assert set(ref.SEEDS) == {(C,) + cfg for C in (1, 20, 80) for cfg in ref.CONFIGS}
    for (C, topk, clamp, alpha, beta), seed in ref.SEEDS.items():
        assert ref.decided(ref.scene(seed, C), topk, clamp, alpha, beta, margin=1e-3), (C, topk, clamp, alpha, beta)
    assert ref.decided(ref.scene(ref.BIG_SEED, 20, pad=ref.BIG_PAD))


def test_decided_tells_a_tie():
    """decided_result refuses a near-tie between two ranks, between the last selected and the first
    unselected candidate, at a contested cell, and a metric fp32 could flush."""
    ok = dict(metrics=[np.array([0.5, 0.4, 0.3])], contests=[np.array([0.6, 0.5])])
    assert ref.decided_result(ok, 2)
    assert not ref.decided_result(dict(ok, metrics=[np.array([0.5, 0.49996, 0.3])]), 2)
    assert not ref.decided_result(dict(ok, metrics=[np.array([0.5, 0.4, 0.39997])]), 2)
    assert ref.decided_result(dict(ok, metrics=[np.array([0.5, 0.4, 0.3, 0.29999])]), 2)       # beyond rank topk
    assert not ref.decided_result(dict(ok, contests=[np.array([0.6, 0.59995, 0.1])]), 2)
    assert not ref.decided_result(dict(ok, metrics=[np.array([0.5, 1e-37])]), 2)


@pytest.mark.parametrize("C", [1, 20, 80])
def test_scenes_contain_the_listed_cases(C):
    seed = ref.SEEDS[(C, 13, 1, 1.0, 6.0)]
    sc = ref.scene(seed, C)
    P = sum(h * w for h, w in ref.level_shapes(ref.PAD))
    assert P == 1022 and sc["dist"].shape == (3, P, 8) and sc["cls"].shape[2] >= C
    assert sc["nbox"].tolist() == [8, 2, 0] and sc["boxes"][2].any()          # nbox 0 over filled rows
    res = ref.scene_assign(sc)
    n_cand = [m.size for m in res["metrics"]]                                # valid boxes, in order
    assert len(n_cand) == 8                                                  # 6 + 2: the NaN label and the zero area are skipped
    assert np.isnan(sc["boxes"][0, 6, 4]) and sc["boxes"][0, 7, 2] == 0
    assert (res["cand_cells"][0, 6:] == -1).all()
    grid = ref.cell_grid(ref.PAD)
    whole = ref.pair_values(ref.box_geometry(sc["boxes"][0, 0], f32(256), f32(192)), 256, 192, grid, sc["dist"][0],
                            sc["cls"][0, :, 0], True, 1.0, 6.0)[0]
    assert whole.all()                                                       # every one of P cells inside
    assert n_cand[1] == 0 and (res["cand_cells"][0, 1] == -1).all()          # smaller than a stride-8 cell
    assert 0 < n_cand[2] < 13                                                # fewer than topk candidates
    assert (res["cand_cells"][0, 2, :n_cand[2]] >= 0).all() and (res["cand_cells"][0, 2, n_cand[2]:] == -1).all()
    assert len(res["contests"]) >= 1                                         # overlapping boxes contest cells
    assert (sc["dist"][..., :4] < 0).mean() > 0.02                           # negative before the clamp
    assert res["counts"][:2].sum(1).min() > 0 and not res["counts"][2].any()
    assert not res["targets"][2].any()
    # rows: zero or (distances, that in (0, 1], one-hot)
    tg = res["targets"]
    pos = tg[..., 5:].max(-1) >= 1
    assert pos.sum() == res["counts"].sum() and not tg[~pos].any()
    assert (tg[pos][:, 5:].sum(-1) == 1).all() and (tg[pos][:, :4] > 0).all()
    assert (tg[pos][:, 4] > 0).all() and (tg[pos][:, 4] <= 1).all()


def test_assign_on_a_hand_made_case():
    """Two boxes on one 128 x 128 image, perfect predictions for box 0 everywhere: box 0's cells have
    u = 1, so it wins every cell it selects; the best cell's target is max_u = 1 (up to the 1e-9)."""
    pad = (128, 128)
    gy, gx, sf, _ = ref.cell_grid(pad)
    P = gy.size
    boxes = np.zeros((1, 4, 5), f32)
    boxes[0, 0] = [0.5, 0.5, 0.5, 0.5, 1]         # 32..96
    boxes[0, 1] = [0.5, 0.5, 0.75, 0.75, 0]       # 16..112
    dist = np.zeros((1, P, 4), f32)
    dist[0] = np.stack([gy - 32, 96 - gy, gx - 32, 96 - gx], 1) / sf[:, None]
    cls = np.zeros((1, P, 2), f32)
    cls[0, :, 1] = np.linspace(-3, 3, P)
    cls[0, :, 0] = 1.0
    res = ref.tal_assign(boxes, [2], [[128.0, 128.0]], pad, 2, dist, cls, topk=5)
    c0 = res["cand_cells"][0, 0]
    assert (c0 >= 0).all() and np.allclose(res["cand_iou"][0, 0], 1.0)
    inside0 = (gy > 32) & (gy < 96) & (gx > 32) & (gx < 96)
    assert c0.tolist() == np.nonzero(inside0)[0][::-1][:5].tolist()          # the largest logits inside
    assert (res["owner"][0, c0] == 0).all()
    assert abs(res["that"][0, c0[0]] - 1.0) < 1e-8 and res["box_max"][0, 0, 1] == 1.0
    assert np.all(np.diff(res["that"][0, c0]) < 0)
    # box 1 contains every predicted box, so its u is their area / its own; outside box 0 the clamp at 0
    # lets them grow towards the cell: the best is the stride-8 cell at (20, 20), 76 x 76 of 96 x 96
    assert np.isclose(res["cand_iou"][0, 1, 0], (76 * 76) / (96 * 96))
    p0 = res["cand_cells"][0, 1, 0]
    assert (gy[p0], gx[p0]) == (20.0, 20.0)
    lost = set(res["cand_cells"][0, 1].tolist()) & set(c0.tolist())
    assert all(res["owner"][0, p] == 0 for p in lost)
    assert res["counts"].sum() == len(set(c0.tolist()) | set(res["cand_cells"][0, 1].tolist()))


def test_nan_outside_every_box_changes_nothing():
    C = 20
    sc = ref.scene(ref.SEEDS[(C, 13, 1, 1.0, 6.0)], C)
    want = ref.scene_assign(sc)
    out = ~want["inside"]
    assert out[1].sum() > 100                      # the second image has no whole-pad box
    bad = dict(sc, dist=sc["dist"].copy(), cls=sc["cls"].copy())
    bad["dist"][out] = np.nan
    bad["cls"][out] = np.nan
    got = ref.scene_assign(bad)
    for k in ("targets", "counts", "cand_cells", "cand_metric", "cand_iou", "box_max"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _loss_inputs(C, seed=0):
    sc = ref.scene(ref.SEEDS[(C, 13, 1, 1.0, 6.0)], C)
    tg = ref.scene_assign(sc)["targets"]
    return sc["dist"], sc["cls"], tg


@pytest.mark.parametrize("C", [1, 20])
def test_loss_gradients_against_finite_differences(C):
    reg, cls, tg = _loss_inputs(C)
    norm = ref.target_norm(tg, C)
    assert norm[0, 0] == (tg[0, :, 5:].max(-1) >= 1).sum() and norm[2].tolist() == [0, 0]
    losses, d_reg, d_cls = ref.tal_loss_reference(reg, cls, tg, C, norm=norm, grad_scale=0.37)
    assert losses.shape == (3, 3) and (losses[:, 2] == 0).all() and (losses[:2, :2] > 0).all()
    assert not d_reg[..., 4:].any() and not d_cls[..., C:].any()
    pos = tg[..., 5:].max(-1) >= 1
    assert not d_reg[~pos].any() and np.abs(d_reg[pos][:, :4]).max() > 0

    def total(r, c):
        return 0.37 * float(ref.tal_loss(r, c, tg, C, norm=norm).sum())
    rng = np.random.default_rng(5)
    cells = np.argwhere(pos)
    h = 1e-6
    for b, p in cells[rng.choice(len(cells), 4, replace=False)]:
        for j in range(4):
            if reg[b, p, j] <= 0:
                assert d_reg[b, p, j] == 0         # the clamp's flat side
                continue
            rp, rm = reg.astype(np.float64), reg.astype(np.float64)
            rp[b, p, j] += h
            rm[b, p, j] -= h
            fd = (total(rp, cls) - total(rm, cls)) / (2 * h)
            assert abs(fd - d_reg[b, p, j]) <= 1e-6 * max(1.0, abs(fd)), (b, p, j, fd, d_reg[b, p, j])
        hot = int(np.argmax(tg[b, p, 5:]))
        for c in {hot, (hot + 1) % C}:
            cp, cm = cls.astype(np.float64), cls.astype(np.float64)
            cp[b, p, c] += h
            cm[b, p, c] -= h
            fd = (total(reg, cp) - total(reg, cm)) / (2 * h)
            assert abs(fd - d_cls[b, p, c]) <= 1e-6 * max(1.0, abs(fd)), (b, p, c, fd, d_cls[b, p, c])


def test_loss_does_not_read_non_positive_box_rows():
    C = 20
    reg, cls, tg = _loss_inputs(C)
    pos = tg[..., 5:].max(-1) >= 1
    want = ref.tal_loss_reference(reg, cls, tg, C)
    bad = reg.copy()
    bad[~pos] = np.nan
    got = ref.tal_loss_reference(bad, cls, tg, C)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    # y is the alignment value at the hot class of a positive, 0 elsewhere: a loss without positives is the
    # plain |s|^2 BCE(x, 0) sum
    x = torch.tensor(cls[2:3, :, :C], dtype=torch.float64)
    plain = (torch.sigmoid(x) ** 2 * (torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs())))).sum()
    assert abs(float(want[0][2, 0]) - float(plain)) <= 1e-9 * float(plain)
