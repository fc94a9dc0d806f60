"""Host side of the batched augmentation (cvlite/augment.py; CPU): the composition of the colour map, the
boxes through a plan, and the invariants of the planner's draws, against the restatements of
tests/augment_ref.py."""
import numpy as np
import pytest

import augment_ref as ar
from cvlite import augment as ag
from cvlite.data_preprocess import box_targets, padded_size

f32 = np.float32
HW = (37, 53)                                    # H x W of the planner layouts
ONE = np.array([[8, 6, 45, 31]], f32)            # pixel (x1, y1, x2, y2)
THREE = np.array([[2, 3, 20, 18], [25, 10, 50, 34], [10, 20, 30, 35]], f32)
NORM = np.array([HW[1], HW[0], HW[1], HW[0]], f32)
CROP_ONLY = dict(flip=0.0, brightness=0.0, contrast=None, saturation=None, hue=0.0, swap_channels=False, expand=None)


# ---- colour ----------------------------------------------------------------------------------------------
def test_saturation_zero_is_grey():
    m, t = ag.colour_affine(saturation=0.0)
    assert np.array_equal(m[0], m[1]) and np.array_equal(m[1], m[2]) and not t.any()
    v = ar.apply_affine_f32(np.random.default_rng(0).uniform(0, 255, (50, 3)), m, t)
    assert np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(v[:, 1], v[:, 2])
    m, t = ag.colour_affine(brightness=7.0, contrast=1.3, saturation=0.0, hue=11.0)
    assert np.array_equal(m[0], m[1]) and np.array_equal(m[1], m[2]) and t[0] == t[1] == t[2]


def test_identity_parameters_give_the_identity_exactly():
    m, t = ag.colour_affine(saturation=1.0, hue=0.0)
    assert np.array_equal(m, np.eye(3, dtype=f32)) and np.array_equal(t, np.zeros(3, f32))
    assert m.dtype == f32 and t.dtype == f32
    assert np.array_equal(ag.saturation_matrix(1.0), np.eye(3)) and np.array_equal(ag.hue_matrix(0.0), np.eye(3))


def test_hue_is_periodic():
    assert np.abs(ag.hue_matrix(360.0) - ag.hue_matrix(0.0)).max() <= 1e-12
    assert np.abs(ag.hue_matrix(-170.0) - ag.hue_matrix(190.0)).max() <= 1e-12
    # a rotation about the grey axis: grey pixels stay put, the luma of any pixel stays put
    h = ag.hue_matrix(37.0)
    assert np.abs(h @ np.ones(3) - 1.0).max() <= 1e-6
    assert np.abs(ar.BT601 @ h - ar.BT601).max() <= 1e-6


def test_permutation_permutes_rows():
    kw = dict(brightness=-9.0, contrast=0.8, saturation=1.4, hue=-12.0)
    m0, t0 = ag.colour_affine(**kw)
    for perm in ((0, 1, 2), (2, 0, 1), (1, 0, 2), (2, 1, 0)):
        m, t = ag.colour_affine(perm=perm, **kw)
        assert np.array_equal(m, m0[list(perm)]) and np.array_equal(t, t0[list(perm)])
    with pytest.raises(ValueError):
        ag.colour_affine(perm=(0, 0, 1))


def test_composition_matches_stepwise_float64():
    """The fp32 affine map applied in the kernel's order against the photometric chain applied one step at
    a time in float64, over pixels in [0, 255] and the default policy's parameter ranges.  Measured
    largest difference: 6.50e-5 (outputs reach several hundred, where one fp32 ulp is 3.1e-5 to 6.1e-5);
    bound = 4 x that."""
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.uniform(0, 255, (200, 3)), [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0]]]).astype(f32)
    worst = 0.0
    for k in range(300):
        kw = dict(brightness=rng.uniform(-32, 32), contrast=rng.uniform(0.5, 1.5), saturation=rng.uniform(0.5, 1.5),
                  hue=rng.uniform(-18, 18), perm=tuple(rng.permutation(3)), contrast_first=bool(k % 2))
        m, t = ag.colour_affine(**kw)
        worst = max(worst, np.abs(ar.apply_affine_f32(v, m, t) - ar.colour_steps(v.astype(np.float64), **kw)).max())
    print("fp32 affine vs stepwise float64: %.3e" % worst)
    assert worst <= 4 * 6.50e-5


def test_contrast_order_matters_only_with_brightness():
    a = ag.colour_affine(brightness=10.0, contrast=1.5, contrast_first=True)
    b = ag.colour_affine(brightness=10.0, contrast=1.5, contrast_first=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])       # both scale the offset
    a = ag.colour_affine(contrast=1.5, saturation=0.7, hue=5.0, contrast_first=True)
    b = ag.colour_affine(contrast=1.5, saturation=0.7, hue=5.0, contrast_first=False)
    np.testing.assert_allclose(a[0], b[0], rtol=1e-6)


# ---- boxes -----------------------------------------------------------------------------------------------
def _plan_with(boxes_px, canvas, crop, flip):
    """The planner's box path for explicit geometry (crop in the kernel's (y0, x0, hh, ww) order)."""
    H, W = HW
    px = boxes_px / NORM * np.array([W, H, W, H], f32) + np.array([canvas[3], canvas[2]] * 2, f32)
    patch = (crop[1], crop[0], crop[1] + crop[3], crop[0] + crop[2])
    kept, mask = ag.crop_boxes(px, patch)
    return box_targets(kept / np.array([crop[3], crop[2]] * 2, f32), flip), np.nonzero(mask)[0]


def test_boxes_hand_worked():
    # crop_boxes on pixel boxes (x1, y1, x2, y2), patch (10, 5, 40, 25): centre strictly inside keeps
    px = np.array([[12, 6, 20, 10],        # inside: translated by (-10, -5)
                   [0, 0, 30, 20],         # centre (15, 10) inside: clipped at the left / top edges
                   [30, 20, 60, 40],       # centre (45, 30) outside: dropped
                   [36, 21, 44, 29],       # centre (40, 25) on the corner: not strictly inside, dropped
                   [35, 20, 43, 28]], f32)  # centre (39, 24) inside: clipped at the right / bottom edges
    kept, mask = ag.crop_boxes(px, (10, 5, 40, 25))
    assert mask.tolist() == [True, True, False, False, True]
    np.testing.assert_array_equal(kept, np.array([[2, 1, 10, 5], [0, 0, 20, 15], [25, 15, 30, 20]], f32))
    # mirror + (yc, xc, h, w): a 30 x 20 crop, box (2, 1, 10, 5) -> x in (20, 28) after the mirror
    t = box_targets(kept[:1] / np.array([30, 20, 30, 20], f32), True)
    np.testing.assert_allclose(t, [[3 / 20, 24 / 30, 4 / 20, 8 / 30]], rtol=1e-6)
    # translate by a zoom-out: source 37 x 53 at (oy, ox) = (10, 20) on a 100 x 120 canvas, no crop
    p = ag.plan_geometry(37, 53, canvas=(100, 120, 10, 20), size=64)
    assert (p.y0, p.x0, p.hh, p.ww) == (0, 0, 100, 120)
    got, keep = _plan_with(ONE, (100, 120, 10, 20), (0, 0, 100, 120), False)
    np.testing.assert_allclose(got, [[(16 + 41) / 2 / 100, (28 + 65) / 2 / 120, 25 / 100, 37 / 120]], rtol=1e-6)
    assert keep.tolist() == [0]


def test_boxes_match_the_restatement():
    rng = np.random.default_rng(2)
    for k in range(100):
        ch, cw = int(rng.integers(37, 120)), int(rng.integers(53, 150))
        oy, ox = int(rng.integers(0, ch - 37 + 1)), int(rng.integers(0, cw - 53 + 1))
        hh, ww = int(rng.integers(1, ch + 1)), int(rng.integers(1, cw + 1))
        y0, x0 = int(rng.integers(0, ch - hh + 1)), int(rng.integers(0, cw - ww + 1))
        flip = bool(k % 2)
        got, keep = _plan_with(THREE, (ch, cw, oy, ox), (y0, x0, hh, ww), flip)
        ref, rkeep = ar.boxes_through(THREE / NORM, HW, (ch, cw, oy, ox), (y0, x0, hh, ww), flip)
        np.testing.assert_array_equal(keep, rkeep)
        np.testing.assert_array_equal(got, ref)


def test_identity_policy_is_todays_path():
    """Boxes bit for bit data_preprocess.box_targets, the rng left where padded_size leaves it."""
    pol = ag.AugmentPolicy.identity()
    flips = set()
    for seed in range(40):
        r1, r2 = np.random.default_rng(seed), np.random.default_rng(seed)
        p = ag.plan_image((375, 500), THREE / NORM, [4, 5, 6], pol, r1, jitter=[480, 544], min_side=512.0,
                          max_side=640.0)
        flip, new_shape, side = padded_size((375, 500), [480, 544], 512.0, 640.0, r2)
        assert p.flip == flip and (p.ph, p.pw) == (side, side)
        np.testing.assert_array_equal(p.new_shape, new_shape)
        assert (p.oh, p.ow) == (int(new_shape[0]), int(new_shape[1]))
        np.testing.assert_array_equal(p.boxes, box_targets(THREE / NORM, flip))
        assert p.labels.tolist() == [4, 5, 6] and p.keep.tolist() == [0, 1, 2]
        assert (p.ch, p.cw, p.oy, p.ox, p.y0, p.x0, p.hh, p.ww) == (375, 500, 0, 0, 0, 0, 375, 500)
        assert np.array_equal(p.m, np.eye(3, dtype=f32)) and not p.t.any()
        assert r1.bit_generator.state == r2.bit_generator.state
        flips.add(flip)
    assert flips == {False, True}


# ---- planner ---------------------------------------------------------------------------------------------
def _check_plan(p, boxes_px, policy):
    """The invariants of one draw; returns the mode."""
    H, W = HW
    assert 0 <= p.oy <= p.ch - H and 0 <= p.ox <= p.cw - W                       # the source inside the canvas
    assert p.y0 >= 0 and p.x0 >= 0 and p.hh >= 1 and p.ww >= 1                  # the patch inside the canvas
    assert p.y0 + p.hh <= p.ch and p.x0 + p.ww <= p.cw
    assert len(p.boxes) >= 1 and len(p.boxes) == len(p.labels) == len(p.keep)
    if p.mode == 1.0:
        assert (p.y0, p.x0, p.hh, p.ww) == (0, 0, p.ch, p.cw)
        return p.mode
    assert 0.5 <= p.hh / p.ww <= 2.0
    assert p.hh >= int(policy.min_crop * p.ch) - 1 and p.ww >= int(policy.min_crop * p.cw) - 1
    patch = (p.x0, p.y0, p.x0 + p.ww, p.y0 + p.hh)
    px = boxes_px + np.array([p.ox, p.oy, p.ox, p.oy], f32)
    assert min(ar.iou(patch, b) for b in px) >= p.mode
    for i, b in enumerate(px):
        cx, cy = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2
        inside = patch[0] < cx < patch[2] and patch[1] < cy < patch[3]
        assert inside == (i in p.keep)
    return p.mode


def _same(p, q):
    return all(np.array_equal(a, b) for a, b in zip(p, q))


@pytest.mark.parametrize("expand", [None, (1.0, 4.0)])
def test_planner_one_box(expand):
    pol = ag.AugmentPolicy(**dict(CROP_ONLY, expand=expand))
    modes = set()
    for seed in range(400):
        p = ag.plan_image(HW, ONE / NORM, [7], pol, np.random.default_rng(seed), size=64)
        modes.add(_check_plan(p, ONE, pol))
        assert _same(p, ag.plan_image(HW, ONE / NORM, [7], pol, np.random.default_rng(seed), size=64))
        assert (p.oh, p.ow, p.ph, p.pw) == (64, 64, 64, 64) and p.labels.tolist() == [7]
    if expand is None:
        assert modes >= {1.0, 0.1, 0.3, 0.5, 0.7, 0.0}        # 0.9 is rare (3 of 400): not asserted


def test_planner_three_boxes():
    """No patch overlaps all three boxes by 0.3: the planner still terminates, through modes 1, 0.1 and 0."""
    pol = ag.AugmentPolicy(**CROP_ONLY)
    modes = set()
    for seed in range(400):
        p = ag.plan_image(HW, THREE / NORM, [1, 2, 3], pol, np.random.default_rng(seed), size=64)
        modes.add(_check_plan(p, THREE, pol))
        assert p.labels.tolist() == [1 + int(i) for i in p.keep]
    assert modes == {1.0, 0.1, 0.0}


def test_planner_no_boxes_makes_no_crop_draws():
    pol, off = ag.AugmentPolicy(**CROP_ONLY), ag.AugmentPolicy(**dict(CROP_ONLY, min_ious=None))
    for seed in range(20):
        r1, r2 = np.random.default_rng(seed), np.random.default_rng(seed)
        p = ag.plan_image(HW, np.zeros((0, 4), f32), [], pol, r1, jitter=[60, 70], stride=32.0)
        q = ag.plan_image(HW, np.zeros((0, 4), f32), [], off, r2, jitter=[60, 70], stride=32.0)
        assert (p.y0, p.x0, p.hh, p.ww) == (0, 0, 37, 53) and p.mode == 1.0 and len(p.boxes) == 0
        assert _same(p, q) and r1.bit_generator.state == r2.bit_generator.state


def test_full_policy_draws():
    """The default policy over the three-box layout: every part is taken sometimes, the plan stays valid,
    the jitter mode's sizes follow the crop."""
    pol = ag.AugmentPolicy()
    seen = dict(flip=0, expand=0, crop=0, colour=0, perm=0)
    rng = np.random.default_rng(11)
    for _ in range(200):
        p = ag.plan_image(HW, THREE / NORM, [1, 2, 3], pol, rng, jitter=[60, 70], min_side=64.0, max_side=128.0,
                          stride=32.0)
        _check_plan(p, THREE, pol)
        assert 37 <= p.ch <= 4 * 37 and 53 <= p.cw <= 4 * 53
        assert p.oh <= p.ph and p.ow <= p.pw and p.ph == p.pw and p.ph % 32 == 0
        assert min(p.oh, p.ow) <= 70 and max(p.oh, p.ow) <= 128
        np.testing.assert_array_equal(p.new_shape.astype(np.int64), [p.oh, p.ow])
        np.testing.assert_array_equal(p.fill, np.array(pol.fill, f32))
        seen["flip"] += p.flip
        seen["expand"] += (p.ch, p.cw) != HW
        seen["crop"] += p.mode != 1.0
        seen["colour"] += not np.array_equal(p.m, np.eye(3, dtype=f32)) or bool(p.t.any())
        seen["perm"] += sorted(np.count_nonzero(p.m, axis=1).tolist()) == [1, 1, 1] and not np.array_equal(
            p.m != 0, np.eye(3, dtype=bool))
    assert all(20 <= v < 200 for k, v in seen.items() if k != "perm") and seen["perm"] >= 1, seen
