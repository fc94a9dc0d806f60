"""Host-side checks of the evaluation API (CPU; no kernel runs): the ctypes table, argument
validation in cvlite.evaluate, and the CVL_EINVAL paths of cvl_eval_match / cvl_eval_ap that return
before anything is enqueued."""
import ctypes

import numpy as np
import pytest
import torch


def test_signatures_registered():
    from cvlite import _lib
    c_int, P, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    res, args = _lib.SIGNATURES["cvl_eval_match"]
    assert res is c_int and args == [P] * 9 + [c_int] * 4 + [P] + [c_int] * 3 + [P] * 5 + [i64, P, P]
    res, args = _lib.SIGNATURES["cvl_eval_ap"]
    assert res is c_int and args == [P] * 4 + [i64] + [c_int] * 3 + [P] * 3
    lib = _lib.load()
    assert hasattr(lib, "cvl_eval_match") and hasattr(lib, "cvl_eval_ap")


def test_evaluator_argument_validation():
    from cvlite import evaluate as E
    with pytest.raises(ValueError):
        E.Evaluator(20, protocol="voc")
    with pytest.raises(ValueError):
        E.Evaluator(20, "coco", iou_thresholds=[0.5 + 0.01 * k for k in range(17)])
    with pytest.raises(ValueError):
        E.Evaluator(20, "coco", iou_thresholds=[])
    with pytest.raises(ValueError):
        E.Evaluator(0)
    with pytest.raises(ValueError):
        E.Evaluator(3, max_dets=0)
    ev = E.Evaluator(3, "coco", iou_thresholds=[0.5 + 0.01 * k for k in range(16)])      # 16 are allowed
    assert len(ev.thresholds) == 16
    assert E.Evaluator(3, "coco").thresholds == [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
    assert E.Evaluator(3, "voc07").thresholds == E.Evaluator(3, "voc12").thresholds == [0.5]


def _args(B=2, T=4, G=3):
    return dict(boxes=torch.zeros(B, T, 4), scores=torch.zeros(B, T), classes=torch.zeros(B, T),
                valid=torch.zeros(B, dtype=torch.int32), gt_boxes=torch.zeros(B, G, 4),
                gt_labels=torch.zeros(B, G, dtype=torch.int32), gt_count=torch.zeros(B, dtype=torch.int32))


@pytest.mark.parametrize("key,bad", [
    ("boxes", torch.zeros(2, 4, 5)), ("scores", torch.zeros(2, 5)), ("classes", torch.zeros(3, 4)),
    ("valid", torch.zeros(3, dtype=torch.int32)), ("gt_boxes", torch.zeros(3, 3, 4)),
    ("gt_labels", torch.zeros(2, 4, dtype=torch.int32)), ("gt_count", torch.zeros(1, dtype=torch.int32)),
    ("gt_flags", torch.zeros(2, 2, dtype=torch.uint8)), ("image_ids", [1, 2, 3]),
    ("boxes", torch.zeros(2, 0, 4)),
])
def test_add_shape_mismatches(key, bad):
    from cvlite import evaluate as E
    a = _args()
    a[key] = bad
    if key == "boxes" and bad.shape[1] == 0:
        a["scores"] = a["classes"] = torch.zeros(2, 0)
    with pytest.raises(ValueError):
        E.Evaluator(3).add(**a)


def test_add_limits_and_rows_validation():
    from cvlite import evaluate as E
    with pytest.raises(ValueError):
        E.Evaluator(3).add(**_args(T=E.MAX_T + 1))
    with pytest.raises(ValueError):
        E.Evaluator(3).add(**_args(G=E.MAX_G + 1))
    with pytest.raises(ValueError):
        E.Evaluator(3).add_rows([np.zeros((1, 6))], [np.zeros((0, 5))], fmt="xywh")
    with pytest.raises(ValueError):
        E.Evaluator(3).add_rows([np.zeros((1, 6))], [])


def test_no_cpu_fallback():
    from cvlite import _lib
    from cvlite import evaluate as E
    if torch.cuda.is_available():
        return                                   # the loud-failure path is for CPU-only hosts
    with pytest.raises(_lib.CvlError):
        E.Evaluator(3).add(**_args())


def test_gt_from_labels_on_host():
    from cvlite.evaluate import gt_from_labels
    bx = np.array([[[0.5, 0.25, 0.5, 0.25, 2.0]]], np.float32)
    gtb, gtl, gtc = gt_from_labels(bx, [1], (64, 128))
    np.testing.assert_array_equal(gtb.numpy(), np.array([[[16.0, 16.0, 48.0, 48.0]]], np.float32))
    assert gtl.dtype == torch.int32 and int(gtl[0, 0]) == 2 and gtc.tolist() == [1]


def test_einval_paths_without_device():
    """Out-of-range sizes, unknown protocol / mode and NULL arrays return CVL_EINVAL (1) before any
    HIP call: nothing is dereferenced or enqueued."""
    from cvlite import _lib
    lib = _lib.load()
    thr = (ctypes.c_double * 16)(*[0.5] * 16)
    buf = (ctypes.c_char * 64)()                    # any non-NULL address: never read on these paths
    p = ctypes.cast(buf, ctypes.c_void_p)
    t = ctypes.cast(thr, ctypes.c_void_p)

    def match(B=1, T=4, G=2, C=3, K=1, protocol=0, max_dets=100, off=0, thresholds=t, boxes=p):
        return lib.cvl_eval_match(boxes, p, p, p, p, p, None, p, p, B, T, G, C, thresholds, K, protocol, max_dets,
                                  p, p, p, p, p, off, p, None)

    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(T=1025), dict(G=-1), dict(G=1025), dict(C=0), dict(C=65536),
               dict(K=0), dict(K=17), dict(protocol=2), dict(protocol=-1), dict(max_dets=0), dict(off=-1),
               dict(thresholds=None), dict(boxes=None)):
        assert match(**kw) == 1, kw

    def ap(n=0, C=3, K=1, mode=0, seg=p):
        return lib.cvl_eval_ap(None, None, seg, p, n, C, K, mode, p, p, None)

    for kw in (dict(n=-1), dict(C=0), dict(K=0), dict(K=17), dict(mode=3), dict(mode=-1), dict(seg=None),
               dict(n=5)):                           # n > 0 needs the record arrays
        assert ap(**kw) == 1, kw
