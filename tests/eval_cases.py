"""Hand-worked evaluation cases (exact rational APs) and the random exact-grid generator shared by
tests/test_eval_ref.py (the restatement, CPU) and tests/test_gpu_eval.py (the kernels)."""
from fractions import Fraction as F

import numpy as np


def image(img_id, dets, gts, T=None, G=None):
    """dets: [(score, box, class)], gts: [(box, class, flag)] -> an eval_ref image dict, padded to
    T detection and G ground-truth slots."""
    T = max(T or 0, len(dets), 1)
    G = max(G or 0, len(gts))
    im = dict(id=img_id, boxes=np.zeros((T, 4), np.float32), scores=np.zeros(T, np.float32),
              classes=np.zeros(T, np.float32), valid=len(dets), gt_boxes=np.zeros((G, 4), np.float32),
              gt_labels=np.zeros(G, np.int32), gt_flags=np.zeros(G, np.uint8), gt_count=len(gts))
    for t, (s, box, c) in enumerate(dets):
        im["boxes"][t], im["scores"][t], im["classes"][t] = box, s, c
    for g, (box, c, fl) in enumerate(gts):
        im["gt_boxes"][g], im["gt_labels"][g], im["gt_flags"][g] = box, c, fl
    return im


SQ = [0, 0, 10, 10]


def case_a():
    """Duplicate detection + a detection whose IoU is exactly 0.8."""
    return [image(0, [(0.9, SQ, 0), (0.8, SQ, 0)], [(SQ, 0, 0)]),
            image(1, [(0.7, [0, 0, 10, 8], 0)], [(SQ, 0, 0)])]


CASE_A = {"voc07": F(28, 33), "voc12": F(5, 6), "coco": F(223, 303)}
CASE_A_COCO_K = [F(253, 303)] * 7 + [F(51, 101)] * 3


def case_b(with_flagged=True):
    """Two matches of one flagged ground truth (both ignored), a TP and an FP."""
    gts = [(SQ, 0, 0)] + ([([20, 20, 40, 40], 0, 1)] if with_flagged else [])
    return [image(0, [(0.9, [20, 20, 40, 38], 0), (0.8, SQ, 0), (0.7, [20, 20, 40, 40], 0),
                      (0.6, [50, 50, 60, 60], 0)], gts)]


def case_tie():
    """IoU exactly 1/3 with both ground truths: voc takes the first, coco the last; the second
    detection sits on the first ground truth."""
    return [image(0, [(0.9, [0, 5, 10, 15], 0), (0.8, SQ, 0)], [(SQ, 0, 0), ([0, 10, 10, 20], 0, 0)])]


def case_crowd_after_match():
    """IoU 0.6 with a plain ground truth, 1.0 (inter / ad) with a crowd listed first."""
    return [image(0, [(0.9, [0, 0, 10, 6], 0)], [([0, 0, 20, 20], 0, 1), (SQ, 0, 0)])]


def case_score_tie():
    """Equal scores in two images: image 3's FP is accumulated before image 5's TP."""
    return [image(5, [(0.5, SQ, 0)], [(SQ, 0, 0)]), image(3, [(0.5, SQ, 0)], [])]


def random_images(rng, B, T, G, C, id0=0, grid=32):
    """Integer corners on a 0..grid lattice (equal IoUs and IoUs exactly on a threshold occur), scores
    multiples of 1/16 (ties), ~20 % flagged ground truths, short valid counts, empty images and
    out-of-range class values.  Detections are jittered copies of ground truths or random boxes."""
    out = []
    for b in range(B):
        ng = 0 if (G == 0 or rng.random() < 0.15) else int(rng.integers(1, G + 1))
        gts = []
        for _ in range(ng):
            y1, x1 = rng.integers(0, grid - 2, 2)
            h, w = rng.integers(2, 13, 2)
            gts.append(([y1, x1, min(grid, y1 + h), min(grid, x1 + w)], int(rng.integers(-1, C + 1)) if
                        rng.random() < 0.1 else int(rng.integers(0, C)), int(rng.random() < 0.2)))
        nv = T if rng.random() < 0.5 else int(rng.integers(0, T + 1))
        dets = []
        for _ in range(T):                      # slots past nv hold data too: they must be dropped
            if gts and rng.random() < 0.7:
                box, c, _ = gts[int(rng.integers(0, len(gts)))]
                box = list(np.clip(np.array(box) + rng.integers(-2, 3, 4) * (rng.random(4) < 0.4), 0, grid))
                if box[2] <= box[0] or box[3] <= box[1]:
                    box = [0, 0, 4, 4]
                c = c if rng.random() < 0.9 else int(rng.integers(0, C))
            else:
                y1, x1 = rng.integers(0, grid - 2, 2)
                h, w = rng.integers(2, 13, 2)
                box, c = [y1, x1, min(grid, y1 + h), min(grid, x1 + w)], int(rng.integers(0, C))
            cv = float(c)
            r = rng.random()
            if r < 0.03:
                cv = float(C)
            elif r < 0.06:
                cv = -1.0
            elif r < 0.08:
                cv = float("nan")
            s = float(rng.integers(1, 17)) / 16.0
            if rng.random() < 0.02:
                s = float("nan")
            dets.append((s, box, cv))
        im = image(id0 + b, dets, gts, T=T, G=G)
        im["valid"] = nv
        out.append(im)
    return out
