"""Pins tests/fcos_paper_ref.py, the restatement the GPU tests of the FCOS papers' recipe compare the
kernels against: hand-enumerable assignment cases, GIoU hand values, and the scene conditions the GPU
tests rely on (CPU; no cvlite code runs here)."""
import numpy as np
import torch

import fcos_paper_ref as ref

f32 = np.float32
PAD = (128, 128)            # levels 16x16, 8x8, 4x4, 2x2, 1x1
OFF = [0, 256, 320, 336, 340, 341]


def _assign(rows, C=2, radius=1.5, pad=PAD, dim=None):
    """rows: pixel (yc, xc, h, w, cls) on an image of size `pad`."""
    H, W = pad if dim is None else dim
    boxes = np.array([[y / H, x / W, h / H, w / W, c] for y, x, h, w, c in rows], f32)[None]
    tg, cnt, ncand = ref.paper_assign(boxes, [len(rows)], np.array([[H, W]], f32), pad, C, center_radius=radius)
    return tg[0], cnt[0], ncand[0]


def _cell(lvl, cy, cx, pad=PAD):
    return OFF[lvl] + cy * (pad[1] // ref.STRIDES[lvl]) + cx


def test_one_box_centred_on_a_grid_point():
    """A 40x40 box centred on (36, 36), the grid point of level-0 cell (4, 4): the whole box covers the
    5x5 cells 2..6 (points 20..52 inside (16, 56)); radius 1.5 keeps the 3x3 cells 3..5 (points within
    12 px of the centre).  Every m <= 36, so only level 0."""
    for radius, cells in ((0.0, range(2, 7)), (1.5, range(3, 6))):
        tg, cnt, _ = _assign([(36, 36, 40, 40, 1)], radius=radius)
        want = {_cell(0, cy, cx) for cy in cells for cx in cells}
        got = set(np.nonzero(tg[:, 5:].max(1) >= 1)[0].tolist())
        assert got == want
        assert cnt.tolist() == [len(want), 0, 0, 0, 0]
        np.testing.assert_array_equal(tg[_cell(0, 4, 4)], f32([2.5, 2.5, 2.5, 2.5, 1.0, 0.0, 1.0]))
        np.testing.assert_array_equal(tg[_cell(0, 3, 4)],
                                      f32([1.5, 3.5, 2.5, 2.5, np.sqrt(12.0 / 28.0), 0.0, 1.0]))
        assert not tg[sorted(set(range(341)) - want)].any()


def test_nested_boxes_smaller_wins():
    """Both boxes cover cell (7, 7) of level 0 (point (60, 60)); the smaller one, given second, wins and
    its class alone is set."""
    tg, _, ncand = _assign([(60, 60, 80, 80, 0), (60, 60, 40, 40, 1)], radius=0.0)
    p = _cell(0, 7, 7)
    assert ncand[p] == 2
    np.testing.assert_array_equal(tg[p], f32([2.5, 2.5, 2.5, 2.5, 1.0, 0.0, 1.0]))
    # outside the small box the large one is alone
    q = _cell(0, 3, 7)      # point (28, 60): t = 8, b = 72 for the large box -> m = 72, level 1 only
    assert ncand[q] == 0 and not tg[q].any()
    q = _cell(0, 4, 7)      # point (36, 60): t = 16, b = 64, l = r = 40 -> m = 64
    assert ncand[q] == 1 and tg[q, 5] == 1 and tg[q, 6] == 0


def test_equal_areas_lowest_index_wins():
    tg, _, ncand = _assign([(60, 60, 40, 40, 1), (60, 60, 40, 40, 0)], radius=0.0)
    p = _cell(0, 7, 7)
    assert ncand[p] == 2 and tg[p, 6] == 1 and tg[p, 5] == 0


def test_point_on_a_box_edge_is_outside():
    """Box rows 20..60: the grid point 20 of row 2 lies on the edge (t = 0), row 3 is inside."""
    tg, _, _ = _assign([(40, 36, 40, 40, 0)], radius=0.0)
    assert not tg[_cell(0, 2, 4)].any()
    assert tg[_cell(0, 3, 4), 5] == 1 and tg[_cell(0, 3, 4), 0] == 1.0
    # the far edge too: box columns 16..56, no grid point on them, but row 7 (point 60) is on y1
    assert not tg[_cell(0, 7, 4)].any() and tg[_cell(0, 6, 4), 5] == 1


def test_m_on_a_bound_is_positive_on_both_levels():
    """Box rows 4..100, columns 8..104.  Level-0 cell (8, 7), point (68, 60): t = 64, b = 32, l = 52,
    r = 44 -> m = 64 = hi_0.  Level-1 cell (3, 4), point (56, 72): t = 52, b = 44, l = 64, r = 32 ->
    m = 64 = lo_1.  Both are positive."""
    tg, cnt, _ = _assign([(52, 56, 96, 96, 0)], C=1, radius=0.0)
    a, b = tg[_cell(0, 8, 7)], tg[_cell(1, 3, 4)]
    np.testing.assert_array_equal(a[:4], f32([64, 32, 52, 44]) / f32(8))
    np.testing.assert_array_equal(b[:4], f32([52, 44, 64, 32]) / f32(16))
    assert a[5] == 1 and b[5] == 1
    # one step further from the edge on level 0 (m = 72) is level 1's alone
    assert not tg[_cell(0, 9, 7)].any()
    assert cnt[0] > 0 and cnt[1] > 0


def test_skipped_boxes_and_counts():
    """A label outside [0, C) and rows past nbox are skipped entirely."""
    H = W = 128.0
    boxes = np.array([[[60 / H, 60 / W, 40 / H, 40 / W, 5], [60 / H, 60 / W, 80 / H, 80 / W, -1],
                       [36 / H, 36 / W, 40 / H, 40 / W, 1]]], f32)
    tg, cnt, _ = ref.paper_assign(boxes, [2], np.array([[H, W]], f32), PAD, 2)
    assert not tg.any() and not cnt.any()
    tg, cnt, _ = ref.paper_assign(boxes, [7], np.array([[H, W]], f32), PAD, 2)      # nbox > n_max: clamped
    assert cnt.tolist() == [[9, 0, 0, 0, 0]]
    nm = ref.target_norm(tg, 2)
    assert nm[0, 0] == 9
    np.testing.assert_allclose(nm[0, 1], 1 + 4 * np.sqrt(12 / 28) + 4 * (12 / 28), rtol=1e-6)


def test_giou_hand_values():
    t = torch.ones(4, dtype=torch.float64)
    for p, want in (((1, 1, 1, 1), 0.0), ((2, 2, 2, 2), 0.75), ((0, 0, 0, 0), 1.0), ((-3, -3, -3, -3), 1.0),
                    ((1, 1, 0, 0), 1.0)):
        pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
        loss = ref.giou_loss(t, pt)
        np.testing.assert_allclose(float(loss.detach()), want, atol=1e-11)
        if p[0] < 0:
            loss.backward()
            assert not pt.grad.any()


def test_loss_terms_and_normalisation():
    """One positive and one negative cell: the three terms by hand, with and without the norm."""
    C = 2
    tg = torch.zeros(1, 2, 5 + C, dtype=torch.float64)
    tg[0, 0] = torch.tensor([1, 1, 1, 1, 0.5, 0, 1], dtype=torch.float64)
    reg = torch.tensor([[[2, 2, 2, 2, 0.3], [1, 1, 1, 1, -0.7]]], dtype=torch.float64)
    cls = torch.tensor([[[0.2, -0.4], [1.5, -2.0]]], dtype=torch.float64)
    out = ref.paper_loss(reg, cls, tg, C)[0]
    sg = lambda v: 1 / (1 + np.exp(-v))   # noqa: E731
    focal = lambda y, x: (-y * 0.25 * (1 - sg(x)) ** 2 * np.log(sg(x))   # noqa: E731
                          - (1 - y) * 0.75 * sg(x) ** 2 * np.log(1 - sg(x)))
    np.testing.assert_allclose(float(out[0]), focal(0, 0.2) + focal(1, -0.4) + focal(0, 1.5) + focal(0, -2.0),
                               rtol=1e-12)
    np.testing.assert_allclose(float(out[1]), 0.5 * 0.75, rtol=1e-12)
    np.testing.assert_allclose(float(out[2]), -(0.5 * np.log(sg(0.3)) + 0.5 * np.log(1 - sg(0.3))), rtol=1e-12)
    norm = np.array([[4.0, 0.25]], f32)
    out_n = ref.paper_loss(reg, cls, tg, C, norm=norm)[0]
    np.testing.assert_allclose(out_n.numpy(), out.numpy() / np.array([4.0, 0.25, 4.0]), rtol=1e-12)
    # no positives: N = 1, Wsum = 1e-6 and zero reg / cen
    out_0 = ref.paper_loss(reg, cls, torch.zeros_like(tg), C, norm=np.zeros((1, 2), f32))[0]
    assert float(out_0[1]) == 0 and float(out_0[2]) == 0 and float(out_0[0]) > 0


SEEDS = range(8)


def _family(family, C, radius):
    res = []
    for seed in SEEDS:
        boxes, dim, bounds = ref.scene(seed, family, C)
        res.append(ref.paper_assign(boxes[None], [8], dim[None], ref.PAD, C, bounds=bounds, center_radius=radius))
    return res


def test_scene_family_b_conditions():
    """Family B: centre sampling changes >= 50 cells in every seed, and at least half of the seeds have a
    cell with two or more candidates under either radius (so the smallest-area rule is exercised)."""
    for C in (3, 20):
        with_r, without = _family("B", C, 1.5), _family("B", C, 0.0)
        amb_r = amb_0 = 0
        for (tr, _, nr), (t0, _, n0) in zip(with_r, without):
            assert int((tr != t0).any(-1).sum()) >= 50
            amb_r += bool((nr >= 2).any())
            amb_0 += bool((n0 >= 2).any())
        assert amb_r >= 4 and amb_0 >= 4


def test_scene_family_a_conditions():
    """Family A: positives on all five levels across the seeds, level 4 included."""
    for C in (3, 20):
        with_r, without = _family("A", C, 1.5), _family("A", C, 0.0)
        cnt = sum(c[0] for _, c, _ in with_r)
        assert (cnt > 0).all(), cnt
        # with these down-scaled ranges the sampling radius covers every box that is in range, so the
        # radius changes nothing here: family B is the one that tests centre sampling
        for (tr, _, _), (t0, _, _) in zip(with_r, without):
            np.testing.assert_array_equal(tr, t0)
