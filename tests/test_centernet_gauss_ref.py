"""The Gaussian CenterNet restatement checked against itself on the host (CPU): the gather form against
an independently written scatter form, the radius table, the loss at hand-computed points and under
gradcheck, and the definition of N."""
import math

import numpy as np
import pytest
import torch

import centernet_gauss_ref as ref

SEEDS = tuple(range(8))


@pytest.mark.parametrize("pad_h,pad_w,stride", [(128, 128, 4), (128, 96, 4), (120, 100, 4), (128, 128, 8)])
@pytest.mark.parametrize("C,n_box", [(1, 4), (3, 24), (20, 4)])
def test_gather_equals_scatter(pad_h, pad_w, stride, C, n_box):
    (boxes, nbox, dims), gather = ref.scene_targets(SEEDS, pad_h, pad_w, C, n_box, stride)
    scatter = ref.assign_scatter(boxes, nbox, dims, (pad_h, pad_w), C, stride)
    assert gather.dtype == np.float64 and gather.shape == (8, pad_h // stride, pad_w // stride, 4 + C)
    assert np.array_equal(gather.view(np.int64), scatter.view(np.int64))
    heat = gather[..., 4:]
    assert heat.max() == 1.0 and heat.min() == 0.0 and not gather[-1].any()
    # exact ones sit on kept centres only, and every kept centre holds one
    for b in range(8):
        recs = [r for r in ref.box_records(boxes[b], int(nbox[b]), dims[b], (pad_h, pad_w), C, stride) if r["kept"]]
        want = {(r["cy"], r["cx"], r["cls"]) for r in recs}
        got = {tuple(int(v) for v in i) for i in np.argwhere(heat[b] == 1.0)}
        assert got == want


def test_radius_table():
    """min_overlap 0.7: r = 0 for squares up to 8 cells and for 3 x 32, 1 at 16, 2 at 28 and 32, 5 at 64."""
    r = lambda h, w: ref.gaussian_radius(h, w, 0.7)  # noqa: E731
    assert [r(s, s) for s in range(1, 9)] == [0] * 8
    assert r(3, 32) == 0 and r(32, 3) == 0
    assert r(16, 16) == 1 and r(28, 28) == 2 and r(32, 32) == 2 and r(64, 64) == 5
    assert r(0, 0) == 0 and r(0, 9) == 0
    # the three roots of a square of side s are s (1 - sqrt(2m / (1 + m))), s (1 - sqrt(m)) / 2 and
    # s (1 / sqrt(m) - 1) / 2: the second is the smallest
    for s in (100, 333):
        assert r(s, s) == int(s * (1 - math.sqrt(0.7)) / 2)


def test_loss_at_hand_computed_points():
    C = 2
    # one image, three cells: a centre of class 0, a cell at heat 0.5 / 0, an empty cell
    t = torch.tensor([[[1.0, 2.0, 3.0, 4.0, 1.0, 0.0],
                       [0.0, 0.0, 0.0, 0.0, 0.5, 0.0],
                       [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]], dtype=torch.float64)
    x = torch.zeros((1, 3, 6), dtype=torch.float64)
    x[0, 0, :4] = torch.tensor([1.5, 2.0, 1.0, 7.0])          # |d| = 0.5, 0, 2, 3
    x[0, 1, :4] = 100.0                                       # not a centre: ignored
    L = ref.loss64(x, t, [1], C).numpy()
    ln2 = math.log(2.0)
    # p = 0.5 everywhere: centre 0.25 ln2; five negatives 0.25 ln2 (1 - y)^4, y = 0.5 once
    assert L[0, 0] == pytest.approx(0.25 * ln2 * (1 + 4 + 0.5 ** 4), rel=1e-14)
    assert L[0, 1] == pytest.approx(5.5, rel=1e-14)
    # N divides both; N = 0 counts as 1
    L2 = ref.loss64(x, t, [2], C).numpy()
    np.testing.assert_allclose(L2, L / 2, rtol=1e-14)
    np.testing.assert_allclose(ref.loss64(x, t, [0], C).numpy(), L, rtol=1e-14)
    # a confident right answer costs nothing, a confident wrong one -log
    x2 = x.clone()
    x2[0, 0, 4] = 40.0
    x2[0, 2, 5] = -40.0
    x2[0, 1, 4] = 40.0                                        # p = 1 at heat 0.5: (0.5)^4 * 40
    L3 = ref.loss64(x2, t, [1], C).numpy()
    assert L3[0, 0] == pytest.approx(0.25 * ln2 * 3 + 0.5 ** 4 * 40.0, rel=1e-12)
    # gradients: L1 is sign(x - t), zero at equality and off the centres
    _, g = ref.loss_and_grad64(x.float(), t.float(), [1], C, cls_scale=0.0, reg_scale=1.0)
    np.testing.assert_array_equal(g[0, 0, :4], [1.0, 0.0, -1.0, 1.0])
    assert not g[0, 1:].any() and not g[0, :, 4:].any()


def test_loss_gradcheck():
    """float64 gradcheck away from the L1 kinks (box errors of at least 0.25), other exponents included."""
    g = torch.Generator().manual_seed(3)
    C, P = 3, 6
    t = torch.zeros((2, P, 4 + C), dtype=torch.float64)
    t[..., 4:] = torch.rand((2, P, C), generator=g, dtype=torch.float64) * 0.9
    t[0, 1, 5] = 1.0
    t[0, 4, 4] = 1.0
    t[0, 4, 6] = 1.0
    t[1, 2, 6] = 1.0
    t[..., :4] = torch.randn((2, P, 4), generator=g, dtype=torch.float64)
    x = torch.randn((2, P, 4 + C), generator=g, dtype=torch.float64) * 2
    sgn = torch.where(torch.rand((2, P, 4), generator=g) < 0.5, -1.0, 1.0).double()
    x[..., :4] = t[..., :4] + sgn * (0.25 + torch.rand((2, P, 4), generator=g, dtype=torch.float64))
    x.requires_grad_(True)
    for alpha, beta in ((2.0, 4.0), (1.5, 3.0)):
        assert torch.autograd.gradcheck(lambda v: ref.loss64(v, t, [3, 1], C, alpha, beta), (x,), eps=1e-6,
                                        atol=1e-7, rtol=1e-5)


def test_n_counts_a_doubly_hit_centre_once():
    C, pad, stride = 3, (64, 64), 4
    dims = np.array([[64.0, 64.0]], np.float32)
    c = lambda cy, cx, h, w, lab: [(cy + 0.5) * stride / 64.0, (cx + 0.5) * stride / 64.0, h * stride / 64.0,  # noqa: E731
                                   w * stride / 64.0, lab]
    # two class-1 boxes on cell (5, 6), a class-2 box on the same cell, a class-1 box elsewhere
    boxes = np.array([[c(5, 6, 4, 4, 1), c(5, 6, 6, 3, 1), c(5, 6, 5, 5, 2), c(9, 9, 4, 4, 1)]], np.float32)
    t = ref.assign_gather(boxes, [4], dims, pad, C, stride)
    assert ref.npos_ref(t, C).tolist() == [3]
    assert t[0, 5, 6, 5] == 1.0 and t[0, 5, 6, 6] == 1.0 and t[0, 9, 9, 5] == 1.0
    # the box channels of the shared cell are the largest box's (ascending area, the last writer wins)
    recs = ref.box_records(boxes[0], 4, dims[0], pad, C, stride)
    big = [r for r in recs if r["index"] == 2][0]
    assert np.array_equal(t[0, 5, 6, :4], big["off4"].astype(np.float64))
    # an empty image has N = 0 (the loss uses max(N, 1))
    assert ref.npos_ref(ref.assign_gather(boxes, [0], dims, pad, C, stride), C).tolist() == [0]
