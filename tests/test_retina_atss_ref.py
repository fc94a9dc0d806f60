"""Pins tests/retina_atss_ref.py, the restatement the GPU tests of csrc/retina_atss.hip stand on (CPU):
hand-worked cases with the candidates and thresholds written out, an independently written brute force,
a hand-computed loss, and the properties of the generated scenes that the GPU tests rely on."""
import math
import statistics

import numpy as np
import torch

import retina_atss_ref as ref

f32 = np.float32
PAD = 128                                   # S = 16, 8, 4, 2, 1; level offsets 0, 256, 320, 336, 340; P = 341
OFF = (0, 256, 320, 336, 340)


def _one_box(label=1, n=1):
    """n copies (labels label, label+1, ...) of the 32 x 32 box centred at (32, 40)."""
    boxes = np.zeros((1, max(n, 1), 5), f32)
    for k in range(n):
        boxes[0, k] = [32 / PAD, 40 / PAD, 32 / PAD, 32 / PAD, label + k]
    return boxes, np.array([[PAD, PAD]], f32)


def _iou(c0, c1, ah, aw, box=(16.0, 48.0, 24.0, 56.0)):
    """Plain float64 IoU of the box (y0, y1, x0, x1) with the anchor (ah, aw) centred at (c0, c1)."""
    y0, y1, x0, x1 = box
    ih = max(min(y1, c0 + ah / 2) - max(y0, c0 - ah / 2), 0.0)
    iw = max(min(x1, c1 + aw / 2) - max(x0, c1 - aw / 2), 0.0)
    return ih * iw / (ah * aw + (y1 - y0) * (x1 - x0) - ih * iw)


def test_one_box_on_one_anchor():
    """A = 1, square anchors 32 .. 512, topk 1.  The box IS the level-0 anchor of cell (4, 5).  Nearest
    cells: level 0 (4,5) = 69; level 1 (stride 16): y 32 is cell 2, x 40 ties 32 | 48 -> the lower, (2,2) =
    18; level 2 (stride 32): (1,1) = 5; level 3 (stride 64): y ties 0 | 64 -> 0, x 40 is nearer 64,
    (0,1) = 1; level 4: 0.  IoUs 1, 1/4, 1/16, 1/64, 1/256 (the anchors contain the box): mean
    0.26640625, squared deviations summing to 0.7118042, sample std 0.4218424, threshold 0.6882487."""
    adims = np.array([[[s, s]] for s in (32, 64, 128, 256, 512)], f32)
    boxes, dims = _one_box()
    tg, cnt, idx, iou, thr, npair, owner = ref.atss_assign(boxes, [1], dims, PAD, 3, anchor_dims=adims, topk=1)
    assert idx[0, 0].tolist() == [69, 256 + 18, 320 + 5, 336 + 1, 340]
    assert iou[0, 0].tolist() == [1.0, 0.25, 0.0625, 0.015625, 0.00390625]
    ious = [1.0, 0.25, 0.0625, 0.015625, 0.00390625]
    want_thr = statistics.mean(ious) + statistics.stdev(ious)
    assert abs(want_thr - 0.6882487) < 1e-7 and abs(thr[0, 0] - want_thr) < 1e-15
    assert cnt.tolist() == [[1, 0, 0, 0, 0]] and np.nonzero(owner[0] >= 0)[0].tolist() == [69]
    assert tg.shape == (1, 341, 1, 8)
    assert tg[0, 69, 0].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    rest = np.delete(tg[0, :, 0], 69, 0)
    assert (rest == np.array([0, 0, 0, 0, -1, 0, -1, 0], f32)).all()


def test_two_equal_boxes_tie_goes_to_the_lower_index():
    adims = np.array([[[s, s]] for s in (32, 64, 128, 256, 512)], f32)
    boxes, dims = _one_box(label=1, n=2)
    tg, cnt, idx, iou, thr, npair, owner = ref.atss_assign(boxes, [2], dims, PAD, 3, anchor_dims=adims, topk=1)
    assert idx[0, 0].tolist() == idx[0, 1].tolist() and thr[0, 0] == thr[0, 1]
    assert npair[0, 69] == 2 and owner[0, 69] == 0 and cnt.tolist() == [[1, 0, 0, 0, 0]]
    assert tg[0, 69, 0, 4] == 1.0 and tg[0, 69, 0, 6] == 0.0               # box 0's label, box 0
    # the other way round: the second box alone gives its own label and index
    tg1 = ref.atss_assign(boxes, [2], dims, PAD, 3, anchor_dims=adims, topk=1)[0]
    boxes[0, 0, 4] = 7.0                                                   # box 0 invalid (label >= C)
    tg2, _, _, _, _, _, owner2 = ref.atss_assign(boxes, [2], dims, PAD, 3, anchor_dims=adims, topk=1)
    assert owner2[0, 69] == 1 and tg2[0, 69, 0, 4] == 2.0 and tg2[0, 69, 0, 6] == 1.0
    assert (tg1[0, 69, 0, :4] == tg2[0, 69, 0, :4]).all()


ADIMS3 = np.array([[[4 * s, 4 * s], [4 * s, 8 * s], [8 * s, 4 * s]] for s in (8, 16, 32, 64, 128)], f32)


def _cells_of_the_box():
    """Cells by rank for the box centred at (32, 40): level 0 (4,5) = 69 then the four at d2 = 64, the lowest
    index (3,5) = 53; level 1 the tie (2,2) = 18, (2,3) = 19; level 2 (1,1) = 5 at d2 64, then (1,2) = 6 at
    576; level 3 (0,1) = 1 and (1,1) = 3 tie at 1600; level 4 has the one cell."""
    return [(69, 53), (18, 19), (5, 6), (1, 3), (0, None)]


def _expect(topk, A=3):
    rows, ious = [], []
    for lvl, cells in enumerate(_cells_of_the_box()):
        S, s = PAD // ref.STRIDES[lvl], ref.STRIDES[lvl]
        for j in range(topk):
            cell = cells[j // A]
            if cell is None:
                rows.append(-1)
                continue
            an = j % A
            rows.append((OFF[lvl] + cell) * A + an)
            ious.append(_iou(float((cell // S) * s), float((cell % S) * s), float(ADIMS3[lvl, an, 0]),
                             float(ADIMS3[lvl, an, 1])))
    return rows, ious


def test_topk_below_the_anchor_count():
    """A = 3, topk 2: anchors 0 and 1 of the nearest cell of every level."""
    boxes, dims = _one_box()
    _, cnt, idx, iou, thr, _, owner = ref.atss_assign(boxes, [1], dims, PAD, 3, anchor_dims=ADIMS3, topk=2)
    assert idx[0, 0].tolist() == [207, 208, 822, 823, 975, 976, 1011, 1012, 1020, 1021]
    rows, ious = _expect(2)
    assert rows == idx[0, 0].tolist()
    np.testing.assert_allclose(iou[0, 0], ious, rtol=1e-6)
    assert abs(thr[0, 0] - (statistics.mean(ious) + statistics.stdev(ious))) < 1e-7
    # the level-0 anchor 0 (32 x 32 at (32, 40)) is the box itself; anchor 1 (32 x 64) has IoU 1/2
    assert iou[0, 0, 0] == 1.0 and iou[0, 0, 1] == 0.5
    assert owner[0, 207] == 0 and cnt[0, 0] >= 1


def test_topk_no_multiple_of_the_anchor_count():
    """A = 3, topk 4: the nearest cell in full and anchor 0 of the second; level 4 has only 3 anchors."""
    boxes, dims = _one_box()
    _, _, idx, iou, thr, _, _ = ref.atss_assign(boxes, [1], dims, PAD, 3, anchor_dims=ADIMS3, topk=4)
    assert idx[0, 0].tolist() == [207, 208, 209, 159, 822, 823, 824, 825, 975, 976, 977, 978, 1011, 1012, 1013,
                                  1017, 1020, 1021, 1022, -1]
    rows, ious = _expect(4)
    assert rows == idx[0, 0].tolist() and len(ious) == 19
    got = iou[0, 0][idx[0, 0] >= 0]
    np.testing.assert_allclose(got, ious, rtol=1e-6)
    assert iou[0, 0, 19] == 0.0
    assert abs(thr[0, 0] - (statistics.mean(ious) + statistics.stdev(ious))) < 1e-7


def _brute(boxes, nbox, dims, pad, C, adims, topk):
    """Written independently: every anchor of the image in one table, a stable argsort per level, a
    dictionary contest.  float64 where exactness does not matter for the decision, fp32 where it does."""
    B, n_max = boxes.shape[:2]
    A = adims.shape[1]
    sizes = [pad // s for s in ref.STRIDES]
    owner_all, cand_all = [], []
    for b in range(B):
        table = []                                   # (level, cell, an, c0, c1, ah, aw), row order
        for lvl, S in enumerate(sizes):
            for cell in range(S * S):
                for an in range(A):
                    table.append((lvl, cell, an, f32((cell // S) * ref.STRIDES[lvl]), f32((cell % S) * ref.STRIDES[lvl]),
                                  adims[lvl, an, 0], adims[lvl, an, 1]))
        lv = np.array([t[0] for t in table])
        c0 = np.array([t[3] for t in table], f32)
        c1 = np.array([t[4] for t in table], f32)
        ah = np.array([t[5] for t in table], f32)
        aw = np.array([t[6] for t in table], f32)
        contest, cands = {}, []
        for i in range(min(max(int(nbox[b]), 0), n_max)):
            r = boxes[b, i]
            H, W = dims[b]
            yc, xc, hp, wp = r[0] * H, r[1] * W, r[2] * H, r[3] * W
            if not (-1 < r[4] < C) or not hp * wp > 0:
                cands.append(None)
                continue
            y0, y1, x0, x1 = yc - hp * f32(0.5), yc + hp * f32(0.5), xc - wp * f32(0.5), xc + wp * f32(0.5)
            d2 = (c0 - yc) * (c0 - yc) + (c1 - xc) * (c1 - xc)
            picked = []
            for lvl in range(5):
                rows = np.nonzero(lv == lvl)[0]
                picked += rows[np.argsort(d2[rows], kind="stable")[:topk]].tolist()
            picked = np.array(picked)
            iou = ref.anchor_ious(c0[picked], c1[picked], ah[picked], aw[picked], y0, y1, x0, x1, hp * wp)
            thr = np.float64(0)
            for v in iou:
                thr = thr + np.float64(v)
            mean = thr / len(iou)
            q = np.float64(0)
            for v in iou:
                q = q + (np.float64(v) - mean) ** 2
            thr = mean + np.sqrt(q / (len(iou) - 1))
            cands.append((picked.tolist(), thr))
            for row, v in zip(picked, iou):
                inside = min(c0[row] - y0, y1 - c0[row], c1[row] - x0, x1 - c1[row]) > f32(0.01)
                if np.float64(v) >= thr and inside and (row not in contest or v > contest[row][0]):
                    contest[row] = (v, i)
        owner_all.append({int(k): int(v[1]) for k, v in contest.items()})
        cand_all.append(cands)
    return owner_all, cand_all


def test_agrees_with_a_brute_force():
    for pad, n_box, topk in ((128, 4, 9), (256, 24, 9), (256, 24, 27)):
        seeds = (0, 1) if pad == 256 else tuple(range(8))
        boxes, dims = ref.scene_batch(seeds, pad, 20, n_box)
        adims = ref.default_anchor_dims()
        _, _, idx, _, thr, _, owner = ref.atss_assign(boxes, [n_box] * len(seeds), dims, pad, 20, topk=topk)
        b_owner, b_cand = _brute(boxes, [n_box] * len(seeds), dims, pad, 20, adims, topk)
        for b in range(len(seeds)):
            got = {int(r): int(owner[b, r]) for r in np.nonzero(owner[b] >= 0)[0]}
            assert got == b_owner[b] and len(got) > 0
            for i in range(n_box):
                rows, t = b_cand[b][i]
                assert idx[b, i][idx[b, i] >= 0].tolist() == rows and thr[b, i] == t


def test_loss_of_a_two_anchor_example():
    """P = 1, A = 2, C = 2, logits 0: a focal element is 0.25 * 0.25 * ln 2 at the label and
    0.75 * 0.25 * ln 2 elsewhere, so the class sum is (1/16 + 3 * 3/16) ln 2 = 0.625 ln 2.  Anchor 0 is
    positive with t = (0.5, 0, 1, 1) against (0, 0, 0, 3): smooth-L1 0.125 + 0 + 1 + 2 = 3.125 (|d| = 1 takes
    the linear branch); anchor 1 is not positive, its NaN box slots are never used."""
    nan = float("nan")
    tg = np.array([[[[0.5, 0, 1, 1, 1, 0.8, 0, 0], [nan, nan, nan, nan, -1, 0, -1, 0]]]], f32)
    reg = torch.tensor([[[0.0, 0, 0, 3, 5, 5, 5, 5, 9]]], dtype=torch.float64, requires_grad=True)
    cls = torch.zeros((1, 1, 6), dtype=torch.float64, requires_grad=True)
    L = ref.atss_loss(reg, cls, tg, np.array([[1, 0, 0, 0, 0]]), 2, 2)
    L.sum().backward()
    L = L.detach()
    assert abs(float(L[0, 0]) - 0.625 * math.log(2)) < 1e-15 and float(L[0, 1]) == 3.125
    assert reg.grad[0, 0].tolist() == [-0.5, 0.0, -1.0, 1.0, 0, 0, 0, 0, 0]
    assert cls.grad[0, 0, 4:].tolist() == [0, 0] and bool((cls.grad[0, 0, :4] != 0).all())
    # N = 2 halves both, a weight scales them, N = 0 counts as 1
    L2 = ref.atss_loss(reg, cls, tg, np.array([[1, 1, 0, 0, 0]]), 2, 2, img_weight=[3.0]).detach()
    assert abs(float(L2[0, 0]) - 1.5 * 0.625 * math.log(2)) < 1e-15 and float(L2[0, 1]) == 1.5 * 3.125
    L0 = ref.atss_loss(reg, cls, tg, np.zeros((1, 5), np.int32), 2, 2).detach()
    assert float(L0[0, 1]) == 3.125


def test_default_anchor_dims_are_the_modules():
    from cvlite.retinanet import RetinaNet
    np.testing.assert_array_equal(np.array(RetinaNet(3, {}).anchor_boxes, f32), ref.default_anchor_dims())


def test_scene_properties_the_gpu_tests_stand_on():
    """Seeds 0..7 with the default anchors: positives in every image; contested anchors in every image with
    24 boxes; every box of the topk 9 scenes wins an anchor; level 4 gets candidates and no positive."""
    for pad, n_box, topk in ((128, 4, 9), (256, 8, 9), (256, 24, 9), (256, 24, 27)):
        boxes, dims = ref.scene_batch(range(8), pad, 80, n_box)
        assert (boxes[..., 2] * pad >= 12 - 1e-3).all() and (boxes[..., 2] * pad <= 0.9 * pad + 1e-3).all()
        assert (boxes[..., 0] - boxes[..., 2] / 2 >= -1e-6).all() and (boxes[..., 1] + boxes[..., 3] / 2 <= 1 + 1e-6).all()
        _, cnt, idx, _, _, npair, owner = ref.atss_assign(boxes, [n_box] * 8, dims, pad, 80, topk=topk)
        assert (cnt.sum(1) >= 5 * n_box).all()
        assert (idx[:, :, 4 * topk] >= 0).all() and not cnt[:, 4].any()
        if n_box == 24:
            assert ((npair >= 2).sum(1) >= (2 if topk == 9 else 18)).all()
        if topk == 9:
            assert all(len(set(owner[b][owner[b] >= 0].tolist())) == n_box for b in range(8))
        if pad == 256:
            assert (cnt[:, :3].sum(0) > 0).all()          # positives on levels 0..2 somewhere in the batch
