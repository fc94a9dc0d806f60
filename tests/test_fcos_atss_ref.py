"""Pins tests/fcos_atss_ref.py, the restatement the GPU tests of the ATSS assignment compare the kernels
against: a hand case small enough to verify by reading, the scene conditions the GPU tests rely on, the
rule's corner cases, and the window facts csrc/fcos_atss.hip rests on (CPU; no cvlite code runs here)."""
import functools

import numpy as np

import fcos_atss_ref as ref

f32 = np.float32
PAD = ref.PAD               # (256, 192): levels 32x24, 16x12, 8x6, 4x3, 2x1
OFF = [0, 768, 960, 1008, 1020, 1022]


def _px(rows, dim=PAD):
    """Pixel (yc, xc, h, w, cls) rows -> a one-image batch normalised to `dim`."""
    H, W = dim
    return np.array([[y / H, x / W, h / H, w / W, c] for y, x, h, w, c in rows], f32)[None]


def _assign(rows, C=3, dim=PAD, **kw):
    boxes = _px(rows, dim)
    return ref.atss_assign(boxes, [len(rows)], np.array([dim], f32), PAD, C, **kw)


@functools.lru_cache(maxsize=None)
def _scene24(seed, topk=9, select=None):
    boxes, dim, _ = ref.scene(seed, "A", 20, n_box=24, n_max=24)
    return ref.atss_assign(boxes[None], [24], dim[None], PAD, 20, topk=topk, anchor_scale=2.0, select=select)


@functools.lru_cache(maxsize=None)
def _scene8(family, seed, topk=9, select=None):
    boxes, dim, _ = ref.scene(seed, family, 20)
    return ref.atss_assign(boxes[None], [8], dim[None], PAD, 20, topk=topk, select=select)


# ---- the hand case ---------------------------------------------------------------------------------
def test_hand_case_candidates_and_ious():
    """One 100 x 80 px box centred at (128, 96) in the 256 x 192 image: rows 78..178, columns 56..136,
    area 8000.  Level 0 (stride 8): the centre is the corner shared by cells (15, 11), (15, 12),
    (16, 11), (16, 12) = 371, 372, 395, 396, whose points (124 | 132, 92 | 100) are all at d2 = 32; they
    come first, in index order.  Next d2 = 16 + 144 = 160: eight cells, of which the five lowest indices
    347, 348, 370, 373, 394 complete the nine.
    IoU by hand, anchor_scale 8: ha = 8 * 8 * 0.5 = 32, so cell 371's anchor spans rows 92..156 and
    columns 60..124, wholly inside the box: inter = 64 * 64 = 4096, uni = (4096 + 8000) - 4096 = 8000,
    iou = 4096 / 8000 = 0.512.  The same holds for every point within 14 px (rows) / 8 px (columns) of
    the centre line, i.e. the first six.  Cells 370, 373, 394 (columns 84 / 108): the anchor's columns
    52..116 (or 76..140) overhang the box by 4 px: inter = 64 * 60 = 3840, uni = 12096 - 3840 = 8256,
    iou = 0.4651163."""
    _, _, cells, iou, thr, _, _ = _assign([(128, 96, 100, 80, 1)])
    assert cells[0, 0, :9].tolist() == [371, 372, 395, 396, 347, 348, 370, 373, 394]
    np.testing.assert_array_equal(iou[0, 0, :6], f32([0.512] * 6))
    np.testing.assert_array_equal(iou[0, 0, 6:9], f32([3840.0 / 8256.0] * 3))
    np.testing.assert_allclose(iou[0, 0, 6:9], 0.4651163, rtol=1e-7)
    # the threshold over all 9 + 9 + 9 + 9 + 2 candidates, by numpy's own mean / sample std
    n = 9 * 4 + 2
    assert (cells[0, 0] >= 0).sum() == n
    v = iou[0, 0][cells[0, 0] >= 0].astype(np.float64)
    np.testing.assert_allclose(thr[0, 0], v.mean() + v.std(ddof=1), rtol=1e-13)


def test_hand_case_positives():
    """The same box: the level-0 candidates at 0.512 reach the threshold (0.48...), the 0.465 ones do
    not.  Level 1 (stride 16, 128 px anchors, 12 columns): the four cells about the centre, 89, 90, 101,
    102, and of the ring at d2 = 640 the five lowest indices 77, 78, 88, 91, 100.  An anchor that covers
    the whole box has iou = 8000 / 16384 = 0.488..., positive; those of 77 and 78 (point row 104, anchor
    rows 40..168) miss the box's last 10 rows: inter = 90 * 80 = 7200, iou = 7200 / 17184 = 0.419, not
    positive.  So 6 + 7 positives, none above level 1 (IoUs below 0.13 there)."""
    tg, cnt, cells, iou, thr, npair, owner = _assign([(128, 96, 100, 80, 1)])
    assert 0.48 < thr[0, 0] < 0.4883
    pos = np.nonzero(tg[0, :, 5:].max(1) >= 1)[0]
    assert pos.tolist() == [347, 348, 371, 372, 395, 396] + [768 + c for c in (88, 89, 90, 91, 100, 101, 102)]
    assert cells[0, 0, 9:18].tolist() == [768 + c for c in (89, 90, 101, 102, 77, 78, 88, 91, 100)]
    full, cut = f32(8000.0 / 16384.0), f32(7200.0 / 17184.0)
    np.testing.assert_array_equal(iou[0, 0, 9:18], f32([full] * 4 + [cut] * 2 + [full] * 3))
    assert iou[0, 0, 18:].max() < 0.13
    assert cnt[0].tolist() == [6, 7, 0, 0, 0]
    assert cnt[0].sum() == len(pos) and (owner[0, pos] == 0).all() and (npair[0, pos] == 1).all()
    # cell 371: point (124, 92): t = 46, b = 54, l = 36, r = 44, stride 8
    np.testing.assert_array_equal(tg[0, 371, :4], f32([46, 54, 36, 44]) / f32(8))
    np.testing.assert_array_equal(tg[0, 371, 4], f32(np.sqrt((46.0 / 54.0) * (36.0 / 44.0))))
    assert tg[0, 371, 5:].tolist() == [0.0, 1.0, 0.0]


# ---- the scene conditions the GPU tests rely on -------------------------------------------------------
def test_scene_24_boxes_conditions():
    """24 boxes at anchor_scale 2: positives on every level, many contested cells, nearly every box owns
    a cell.  The counts are those of the prototype the rule was written from."""
    want = {0: ([6, 37, 37, 12, 1], 25), 1: ([25, 38, 25, 11, 2], 18)}
    for seed in (0, 1):
        _, cnt, _, _, _, npair, owner = _scene24(seed)
        contested = int((npair >= 2).sum())
        assert cnt[0].tolist() == want[seed][0] and contested == want[seed][1]
        assert (cnt[0] >= 1).all() and contested >= 10
        assert len(set(owner[owner >= 0].tolist())) >= 22


def test_scene_8_boxes_conditions():
    """The default anchor_scale 8 and 8 boxes: the upper levels' anchors exceed this image, so the
    positives fall on levels 0-1 (and 2 at most); every image has positives and at least 7 of the 8
    boxes own a cell."""
    for family in "AB":
        for seed in range(8):
            _, cnt, _, _, _, _, owner = _scene8(family, seed)
            assert cnt[0].sum() > 0 and not cnt[0, 3:].any()
            assert cnt[0, :2].sum() >= 0.9 * cnt[0].sum()
            assert len(set(owner[owner >= 0].tolist())) >= 7


# ---- rule checks ------------------------------------------------------------------------------------
def test_small_level_has_fewer_candidates():
    """The 2 x 1 level of PAD has two cells: k_l = 2 candidates, -1 beyond, and n = 38."""
    _, _, cells, iou, _, _, _ = _assign([(128, 96, 100, 80, 1)])
    assert sorted(cells[0, 0, 36:38].tolist()) == [1020, 1021]
    assert (cells[0, 0, 38:] == -1).all() and not iou[0, 0, 38:].any()
    # the 4 x 3 level holds 12 >= 9 cells, so topk = 16 takes all 12 there
    _, _, cells, _, _, _, _ = _assign([(128, 96, 100, 80, 1)], topk=16)
    assert sorted(cells[0, 0, 48:60].tolist()) == list(range(1008, 1020)) and (cells[0, 0, 60:64] == -1).all()


def test_identical_boxes_lower_index_wins():
    tg, cnt, _, _, _, npair, owner = _assign([(128, 96, 100, 80, 2), (128, 96, 100, 80, 0)])
    pos = owner[0] >= 0
    assert pos.sum() > 0 and (owner[0, pos] == 0).all() and (npair[0, pos] == 2).all()
    assert (tg[0, pos, 7] == 1).all() and not tg[0, pos, 5].any()


def test_box_outside_the_image_has_candidates_but_no_positive():
    tg, cnt, cells, iou, thr, _, _ = _assign([(-60, 300, 40, 40, 1)])
    assert (cells[0, 0, :9] >= 0).all() and cells[0, 0, 0] == 23          # the top-right cell is nearest
    assert not tg.any() and not cnt.any()
    # the small anchors do not reach the box, the upper levels' do: a threshold, and still no positive,
    # because no grid point lies inside the box
    assert not iou[0, 0, :9].any() and iou[0, 0, 27:].max() > 0 and thr[0, 0] > 0
    assert (iou[0, 0].astype(np.float64) >= thr[0, 0]).any()
    # partly outside: candidates with a positive IoU, positives only inside the image
    tg, cnt, _, iou, thr, _, _ = _assign([(-10, 96, 60, 60, 1)])
    assert thr[0, 0] > 0 and cnt.sum() > 0


def test_skipped_boxes_and_nan():
    """Labels -1 and C, zero and negative sides and NaN sizes are skipped (no candidates); a NaN centre
    keeps its candidates (the lowest indices: every distance is NaN) and is never positive."""
    nan = float("nan")
    rows = [(128, 96, 100, 80, -1), (128, 96, 100, 80, 3), (128, 96, 0, 80, 1), (128, 96, -100, 80, 1),
            (128, 96, nan, 80, 1), (128, 96, 100, 80, nan), (nan, 96, 100, 80, 1)]
    tg, cnt, cells, iou, thr, _, _ = _assign(rows)
    assert (cells[0, :6] == -1).all() and not thr[0, :6].any()
    assert cells[0, 6, :9].tolist() == list(range(9)) and cells[0, 6, 9:18].tolist() == list(range(768, 777))
    assert not tg.any() and not cnt.any() and np.isfinite(tg).all()


def test_target_norm_equals_the_counts():
    for seed in (0, 1):
        tg, cnt, _, _, _, _, _ = _scene24(seed)
        nm = ref.target_norm(tg, 20)
        assert nm[0, 0] == cnt.sum()
        pos = tg[0, :, 5:].max(1) >= 1
        np.testing.assert_allclose(nm[0, 1], tg[0, pos, 4].astype(np.float64).sum(), rtol=1e-12)
        assert ((tg[0, pos, 4] > 0) & (tg[0, pos, 4] <= 1)).all() and (tg[0, pos, :4] > 0).all()


# ---- the window facts the kernel rests on ------------------------------------------------------------
HAND_CENTRES = [(128, 96), (8, 8), (64, 128), (248, 184),          # on grid corners of several levels
                (-5, 96), (261, 96), (128, -7), (128, 199),        # outside each image edge
                (0, 0), (256, 192), (0, 192), (-3, -3)]            # at / beyond image corners
WIN = ref.windowed(lambda topk: topk)                              # the kernel's (2 topk + 1)^2 window
WIN_NARROW = ref.windowed(lambda topk: topk - 1)                   # the (2 topk - 1)^2 window


def _same(x, y):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


def test_window_selection_equals_exhaustive():
    """Selecting from the (2 topk + 1)^2 window about the clamped cell of the centre equals the
    exhaustive scan, for every scene above, topk 1, 9 and 16, and the hand centres."""
    for topk in (1, 9, 16):
        for seed in range(4):
            assert _same(_scene24(seed, topk), _scene24(seed, topk, WIN))
        for family in "AB":
            for seed in range(8):
                assert _same(_scene8(family, seed, topk), _scene8(family, seed, topk, WIN))
        rows = [(y, x, 50, 40, 1) for y, x in HAND_CENTRES]
        assert _same(_assign(rows, topk=topk), _assign(rows, topk=topk, select=WIN))


def test_narrow_window_holds_from_topk_2_and_fails_at_1():
    """The (2 topk - 1)^2 window holds the candidates whenever topk >= 2, but not at topk = 1 with the
    centre on a grid corner: cells (15, 11) and (16, 12) are equidistant from (128, 96), the lower
    index 371 is the candidate, and the one-cell window is cell (16, 12) = 396.  Hence the kernel's
    wider window."""
    rows = [(y, x, 50, 40, 1) for y, x in HAND_CENTRES]
    for topk in (2, 9, 16):
        assert _same(_assign(rows, topk=topk), _assign(rows, topk=topk, select=WIN_NARROW))
        for seed in range(2):
            assert _same(_scene24(seed, topk), _scene24(seed, topk, WIN_NARROW))
    full = _assign(rows[:1], topk=1)[2]
    narrow = _assign(rows[:1], topk=1, select=WIN_NARROW)[2]
    assert full[0, 0, 0] == 371 and narrow[0, 0, 0] == 396


def _window_case(yc, xc, lvl, topk):
    """(exhaustive, windowed, safe) for one centre on one level of PAD."""
    Hs, Ws = ref.level_shapes(PAD)[lvl]
    sf = f32(ref.STRIDES[lvl])
    yc, xc = f32(yc), f32(xc)
    _, _, d2 = ref.level_d2(yc, xc, Hs, Ws, sf)
    k = min(topk, Hs * Ws)
    bounds = ref.window_bounds(yc, xc, Hs, Ws, sf, topk)
    ex, win = ref.select_exhaustive(d2, k), ref.select_window(d2, k, bounds)
    return ex, win, ref.window_is_safe(yc, xc, Hs, Ws, sf, bounds, d2.reshape(-1)[win[-1]])


def test_window_check_accepts_the_scenes_and_catches_far_centres():
    """The kernel's separable check (window_is_safe): whenever it accepts, the window's selection IS the
    exhaustive one; it accepts every centre in or near the image; and a centre so far off that the fp32
    distances round together (where the lowest indices win, far from the window) is rejected, which
    sends the kernel to the whole-level scan."""
    rng = np.random.default_rng(0)
    near = [(rng.uniform(-100, 356), rng.uniform(-100, 292)) for _ in range(200)] + HAND_CENTRES
    for yc, xc in near:
        for lvl in range(3):
            for topk in (1, 9):
                ex, win, safe = _window_case(yc, xc, lvl, topk)
                assert safe and np.array_equal(ex, win), (yc, xc, lvl, topk)
    rejected = 0
    for yc, xc in [(1e9, 96), (128, -1e9), (3e38, 3e38), (float("nan"), 96), (1e6, 1e6), (5000, 96), (128, 1e5)]:
        for topk in (1, 9):
            ex, win, safe = _window_case(yc, xc, 0, topk)
            assert (not safe) or np.array_equal(ex, win), (yc, xc, topk)
            rejected += not safe
    assert rejected >= 6
    # (1e9, 96): dy^2 swallows dx^2, so every column of the best rows ties and column 0 wins, which the
    # window about column 12 does not hold
    ex, win, safe = _window_case(1e9, 96, 0, 1)
    assert not safe and ex[0] % 24 == 0 and win[0] % 24 != 0
