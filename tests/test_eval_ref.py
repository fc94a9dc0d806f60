"""The numpy restatement of the evaluation contract (tests/eval_ref.py) against hand-worked cases
whose APs are exact rationals (CPU; compared at 1e-15)."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import eval_cases as ec
import eval_ref

PROTOCOLS = ("voc07", "voc12", "coco")


def _close(got, frac):
    assert abs(got - float(frac)) <= 1e-15, (got, frac)


def test_iou_exact_values():
    assert eval_ref.iou([0, 0, 10, 8], ec.SQ) == 0.8 == (50 + 5 * 6) / 100.0
    assert eval_ref.iou([0, 5, 10, 15], ec.SQ) == 50.0 / 150.0
    assert eval_ref.iou([0, 0, 10, 6], [0, 0, 20, 20], crowd=True) == 1.0
    assert eval_ref.iou([0, 0, 0, 0], [0, 0, 0, 0]) == 0.0            # denominator <= 0
    assert eval_ref.iou([0, 0, 0, 5], ec.SQ, crowd=True) == 0.0       # ad <= 0
    # no "+1 pixel": touching boxes do not overlap
    assert eval_ref.iou([0, 10, 10, 20], ec.SQ) == 0.0


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_case_a(protocol):
    r = eval_ref.evaluate(ec.case_a(), 1, protocol)
    _close(r["mAP"], ec.CASE_A[protocol])
    assert list(r["npos"]) == [2]
    if protocol == "coco":
        for k, want in enumerate(ec.CASE_A_COCO_K):      # 0.80 == the IoU: still a match
            _close(r["ap"][k, 0], want)
        _close(r["AP50"], F(253, 303))
        _close(r["AP75"], F(253, 303))
        _close(r["AR"], F(7 * 2 + 3 * 1, 20))
        assert r["records"][(1, 0)] == (0, 0b0001111111, 0)
    else:
        assert r["records"][(0, 0)] == (0, 1, 0) and r["records"][(0, 1)] == (0, 0, 0)


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_case_b(protocol):
    r = eval_ref.evaluate(ec.case_b(), 1, protocol)
    assert r["mAP"] == 1.0 and list(r["npos"]) == [1]
    K = len(r["thresholds"])
    full = (1 << K) - 1
    assert r["records"][(0, 0)] == (0, 0, full)          # both matches of the flagged one: ignored
    assert r["records"][(0, 2)] == (0, 0, full)
    assert r["records"][(0, 1)] == (0, full, 0)
    assert r["records"][(0, 3)] == (0, 0, 0)
    r = eval_ref.evaluate(ec.case_b(with_flagged=False), 1, protocol)
    _close(r["mAP"], F(1, 2))


def test_class_without_ground_truth_is_nan_and_excluded():
    im = ec.image(0, [(0.9, ec.SQ, 0), (0.8, ec.SQ, 1)], [(ec.SQ, 0, 0), (ec.SQ, 2, 0)])
    for protocol in PROTOCOLS:
        r = eval_ref.evaluate([im], 4, protocol)
        ap = r["ap"]
        assert (ap[:, 0] == 1.0).all()
        assert np.isnan(ap[:, 1]).all() and np.isnan(ap[:, 3]).all()      # npos == 0
        assert (ap[:, 2] == 0.0).all()                                    # ground truth, no detections
        assert r["mAP"] == 0.5
    assert math.isnan(eval_ref.evaluate([ec.image(0, [(0.5, ec.SQ, 0)], [])], 2, "voc07")["mAP"])


def test_best_iou_tie_voc_first_coco_last():
    thr = [0.3]
    r = eval_ref.evaluate(ec.case_tie(), 1, "voc12", iou_thresholds=thr)
    assert r["records"][(0, 0)] == (0, 1, 0) and r["records"][(0, 1)] == (0, 0, 0)     # first taken: dup FP
    _close(r["mAP"], F(1, 2))
    r = eval_ref.evaluate(ec.case_tie(), 1, "coco", iou_thresholds=thr)
    assert r["records"][(0, 0)] == (0, 1, 0) and r["records"][(0, 1)] == (0, 1, 0)     # last taken: both TP
    assert r["mAP"] == 1.0


def test_non_crowd_match_not_displaced_by_crowd():
    r = eval_ref.evaluate(ec.case_crowd_after_match(), 1, "coco")
    # IoU 0.6 with the plain ground truth: TP up to thr 0.60; above it the crowd (IoU 1) takes it
    assert r["records"][(0, 0)] == (0, 0b0000000111, 0b1111111000)
    # under voc the flag is "difficult": plain IoU, the first strictly largest is the plain one
    r = eval_ref.evaluate(ec.case_crowd_after_match(), 1, "voc07")
    assert r["records"][(0, 0)] == (0, 1, 0)


def test_max_dets_truncation():
    im = ec.image(0, [(0.9, [50, 50, 60, 60], 0), (0.8, ec.SQ, 0), (0.7, ec.SQ, 1)], [(ec.SQ, 0, 0), (ec.SQ, 1, 0)])
    r = eval_ref.evaluate([im], 2, "coco", max_dets=1)
    assert r["records"][(0, 1)] == (None, 0, 0)                  # second of class 0: dropped
    assert (r["ap"][:, 0] == 0.0).all() and (r["ap"][:, 1] == 1.0).all()
    r = eval_ref.evaluate([im], 2, "voc07", max_dets=1)          # voc has no cap
    assert r["records"][(0, 1)] == (0, 1, 0)


def test_score_tie_across_images_ordered_by_image_id():
    for protocol in PROTOCOLS:
        a = eval_ref.evaluate(ec.case_score_tie(), 1, protocol)
        b = eval_ref.evaluate(ec.case_score_tie()[::-1], 1, protocol)
        assert a["mAP"] == b["mAP"]
    _close(eval_ref.evaluate(ec.case_score_tie(), 1, "voc12")["mAP"], F(1, 2))


def test_dropped_detections():
    im = ec.image(0, [(0.9, ec.SQ, 1.0), (float("nan"), ec.SQ, 0), (0.8, ec.SQ, -1.0), (0.7, ec.SQ, 0),
                      (0.6, ec.SQ, 0)], [(ec.SQ, 0, 0)])
    im["valid"] = 4
    r = eval_ref.evaluate([im], 1, "voc07")
    assert [r["records"][(0, t)][0] for t in range(5)] == [None, None, None, 0, None]
    assert r["mAP"] == 1.0


def test_random_protocol_consistency():
    """On the random exact-grid images AP never leaves [0, 1] in any protocol."""
    rng = np.random.default_rng(0)
    imgs = ec.random_images(rng, 6, 12, 5, 3)
    for protocol in PROTOCOLS:
        r = eval_ref.evaluate(imgs, 3, protocol)
        ap = r["ap"][~np.isnan(r["ap"])]
        assert ((ap >= 0) & (ap <= 1)).all()
