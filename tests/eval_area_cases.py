"""The hand-worked ranged COCO case (exact rational APs) and the random exact-grid generator shared by
tests/test_eval_area_ref.py (the restatement, CPU) and tests/test_gpu_eval_area.py (the kernels)."""
from fractions import Fraction as F

import numpy as np

import eval_cases as ec

SIDES = (8, 16, 32, 64, 96, 128)          # areas land on and beside 32^2 = 1024 and 96^2 = 9216


def hand_case():
    """One image, one class.  Ground truths: 10 x 10 (small), 50 x 50 (medium), 200 x 200 (large), a
    40 x 40 crowd.  Detections by score: a 60 x 60 miss, the medium box, the small box, a 20 x 20
    miss, the large box, a 10 x 10 box inside the crowd, the medium box again."""
    gts = [([0, 0, 10, 10], 0, 0), ([100, 100, 150, 150], 0, 0), ([300, 300, 500, 500], 0, 0),
           ([600, 600, 640, 640], 0, 1)]
    boxes = [[800, 800, 860, 860], [100, 100, 150, 150], [0, 0, 10, 10], [700, 700, 720, 720], [300, 300, 500, 500],
             [605, 605, 615, 615], [100, 100, 150, 150]]
    scores = [0.95, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4]
    return [ec.image(0, [(s, b, 0) for s, b in zip(scores, boxes)], gts)]


# (all, small, medium, large) per slot, threshold 0.5
HAND_NPOS = [3, 1, 1, 1]
HAND_TP = {1: (1, 0, 1, 0), 2: (1, 1, 0, 0), 4: (1, 0, 0, 1)}
HAND_IGN = {0: (0, 1, 0, 1), 1: (0, 1, 0, 1), 2: (0, 0, 1, 1), 3: (0, 0, 1, 1), 4: (0, 1, 1, 0), 5: (1, 1, 1, 1),
            6: (0, 1, 0, 1)}
HAND_AP = [F(976, 1515), F(1), F(1, 2), F(1)]            # AP, APs, APm, APl at max_dets 100
HAND_AP_RANK2, HAND_RECALL_RANK2 = F(17, 101), F(1, 3)   # view (all, 2)
HAND_AP_RANK1, HAND_RECALL_RANK1 = F(0), F(0)            # view (all, 1)


def random_images(rng, B, T, G, C, id0=0, crowds=True, gt_area=False, area_scale=False, span=320):
    """Integer corners, sides from SIDES: detections are ground truths shifted by multiples of a
    quarter side (IoUs on and beside the thresholds, equal IoUs) or random boxes; scores multiples of
    1/16 (ties); short valid counts, empty images, out-of-range classes.  gt_area: a mask area of
    1, 1/2 or 1/4 of the box's; area_scale: 1/4, 1, 9/4 or 4 per image."""
    out = []
    for b in range(B):
        ng = 0 if (G == 0 or rng.random() < 0.1) else int(rng.integers(1, G + 1))
        gts = []
        for _ in range(ng):
            h, w = (int(SIDES[i]) for i in rng.integers(0, len(SIDES), 2))
            y1, x1 = (int(v) * 8 for v in rng.integers(0, span // 8, 2))
            lab = int(rng.integers(-1, C + 1)) if rng.random() < 0.1 else int(rng.integers(0, C))
            gts.append(([y1, x1, y1 + h, x1 + w], lab, int(crowds and rng.random() < 0.2)))
        nv = T if rng.random() < 0.6 else int(rng.integers(0, T + 1))
        dets = []
        for _ in range(T):
            if gts and rng.random() < 0.7:
                (y1, x1, y2, x2), c, _ = gts[int(rng.integers(0, len(gts)))]
                h, w = y2 - y1, x2 - x1
                dy, dx = (int(v) for v in rng.integers(-2, 3, 2) * (rng.random(2) < 0.5))
                box = [y1 + dy * h // 4, x1 + dx * w // 4, y2 + dy * h // 4, x2 + dx * w // 4]
                c = c if rng.random() < 0.9 else int(rng.integers(0, C))
            else:
                h, w = (int(SIDES[i]) for i in rng.integers(0, len(SIDES), 2))
                y1, x1 = (int(v) * 8 for v in rng.integers(0, span // 8, 2))
                box, c = [y1, x1, y1 + h, x1 + w], int(rng.integers(0, C))
            cv = float(c)
            r = rng.random()
            if r < 0.03:
                cv = float(C)
            elif r < 0.05:
                cv = float("nan")
            s = float(rng.integers(1, 17)) / 16.0
            dets.append((s, box, cv))
        im = ec.image(id0 + b, dets, gts, T=T, G=G)
        im["valid"] = nv
        if gt_area:
            boxes = im["gt_boxes"].astype(np.float64)
            frac = np.array([1.0, 0.5, 0.25])[rng.integers(0, 3, len(boxes))]
            im["gt_area"] = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) * frac).astype(np.float32)
        if area_scale:
            im["area_scale"] = float(np.array([0.25, 1.0, 2.25, 4.0])[int(rng.integers(0, 4))])
        out.append(im)
    return out
