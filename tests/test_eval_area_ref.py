"""The numpy restatement of the ranged COCO contract (tests/eval_area_ref.py) against a hand-worked
case whose numbers are exact rationals (compared at 1e-15) and against tests/eval_ref.py with the
single unbounded range; the host-only parts of cvlite.evaluate that go with it (merge_states,
gather_states over gloo, argument validation, the ctypes table, the CVL_EINVAL paths that return
before anything is enqueued) and cvlite.coco_json.  CPU; no kernel runs."""
import ctypes
import math
import os
import pickle
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as tdist
import torch.multiprocessing as mp

import eval_area_cases as eac
import eval_area_ref as ear
import eval_cases as ec
import eval_ref
from conftest import GOLDEN, PKG, ROOT

INF = math.inf


def _close(got, frac):
    assert abs(got - float(frac)) <= 1e-15, (got, frac)


def _bit(v):
    return tuple(int(b) for b in v)


# ---- the hand case ------------------------------------------------------------------------------------
def test_hand_case_bits_and_npos():
    r = ear.evaluate(eac.hand_case(), 1, iou_thresholds=[0.5])
    assert r["npos_area"][:, 0].tolist() == eac.HAND_NPOS
    for t in range(7):
        c, rank, tpb, igb = r["records"][(0, t)]
        assert (c, rank) == (0, t)
        assert _bit(tpb) == eac.HAND_TP.get(t, (0, 0, 0, 0)), t
        assert _bit(igb) == eac.HAND_IGN[t], t


def test_hand_case_summary_numbers():
    r = ear.evaluate(eac.hand_case(), 1, iou_thresholds=[0.5])
    for v, want in enumerate(eac.HAND_AP):
        _close(r["ap"][v, 0, 0], want)
    _close(r["mAP"], eac.HAND_AP[0])
    _close(r["AP50"], eac.HAND_AP[0])
    assert math.isnan(r["AP75"])                     # 0.75 is not among the thresholds
    _close(r["APs"], 1), _close(r["APm"], eac.HAND_AP[2]), _close(r["APl"], 1)
    _close(r["AR100"], 1), _close(r["ARs"], 1), _close(r["ARm"], 1), _close(r["ARl"], 1)
    _close(r["AR1"], eac.HAND_RECALL_RANK1), _close(r["AR10"], 1)
    _close(r["ap"][4, 0, 0], eac.HAND_AP_RANK1)
    assert len(r["summary"]) == 12
    r2 = ear.evaluate(eac.hand_case(), 1, iou_thresholds=[0.5], views=[(0, 2), (0, 1)])
    _close(r2["ap"][0, 0, 0], eac.HAND_AP_RANK2)
    _close(r2["AR_view"][0], eac.HAND_RECALL_RANK2)
    _close(r2["ap"][1, 0, 0], eac.HAND_AP_RANK1)
    _close(r2["AR_view"][1], eac.HAND_RECALL_RANK1)


# ---- range ends, gt_area, area_scale --------------------------------------------------------------------
def _one(box, gt_box=None, **extra):
    im = ec.image(0, [(0.9, box, 0)], [(box if gt_box is None else gt_box, 0, 0)])
    im.update(extra)
    return im


def test_range_ends_are_inclusive():
    r = ear.evaluate([_one([0, 0, 32, 32])], 1, iou_thresholds=[0.5])          # area exactly 1024
    assert r["npos_area"][:, 0].tolist() == [1, 1, 1, 0]
    assert _bit(r["records"][(0, 0)][2]) == (1, 1, 1, 0) and _bit(r["records"][(0, 0)][3]) == (0, 0, 0, 1)
    assert (r["APs"], r["APm"]) == (1.0, 1.0) and math.isnan(r["APl"])
    r = ear.evaluate([_one([0, 0, 96, 96])], 1, iou_thresholds=[0.5])          # exactly 9216
    assert r["npos_area"][:, 0].tolist() == [1, 0, 1, 1]


def test_gt_area_overrides_the_box_area():
    big = [0, 0, 100, 100]
    r = ear.evaluate([_one(big, gt_area=np.array([900.0], np.float32))], 1, iou_thresholds=[0.5])
    assert r["npos_area"][:, 0].tolist() == [1, 1, 0, 0]               # the ground truth counts as small
    tpb, igb = r["records"][(0, 0)][2:]
    # matched to it: a TP in "small"; in medium / large the ground truth is ignored, and so is the match
    assert _bit(tpb) == (1, 1, 0, 0) and _bit(igb) == (0, 0, 1, 1)
    # an unmatched detection is judged by its own box area (large)
    r = ear.evaluate([_one(big, gt_box=[500, 500, 600, 600], gt_area=np.array([900.0], np.float32))], 1,
                     iou_thresholds=[0.5])
    assert _bit(r["records"][(0, 0)][2]) == (0, 0, 0, 0) and _bit(r["records"][(0, 0)][3]) == (0, 1, 1, 0)


def test_area_scale_moves_a_box_between_ranges():
    box = [0, 0, 20, 20]                                                        # 400 -> 1600
    r = ear.evaluate([_one(box)], 1, iou_thresholds=[0.5])
    assert r["npos_area"][:, 0].tolist() == [1, 1, 0, 0]
    r = ear.evaluate([_one(box, area_scale=4.0)], 1, iou_thresholds=[0.5])
    assert r["npos_area"][:, 0].tolist() == [1, 0, 1, 0]
    assert _bit(r["records"][(0, 0)][2]) == (1, 0, 1, 0) and _bit(r["records"][(0, 0)][3]) == (0, 1, 0, 1)
    # a supplied gt_area is used as is
    r = ear.evaluate([_one(box, area_scale=4.0, gt_area=np.array([400.0], np.float32))], 1, iou_thresholds=[0.5])
    assert r["npos_area"][:, 0].tolist() == [1, 1, 0, 0]


# ---- the single unbounded range is eval_ref's coco --------------------------------------------------------
def _unbounded_equals_eval_ref(images, C, **kw):
    ref = eval_ref.evaluate(images, C, "coco", **kw)
    max_dets = kw.get("max_dets", 100)
    got = ear.evaluate(images, C, [("all", -INF, INF)], kw.get("iou_thresholds"), max_dets, views=[(0, max_dets)])
    np.testing.assert_array_equal(got["npos_area"][0], ref["npos"])
    assert got["ap"][0].tobytes() == ref["ap"].tobytes()
    assert set(got["records"]) == set(ref["records"])
    for key, (c, tpb, igb) in ref["records"].items():
        gc, _, gtp, gig = got["records"][key]
        assert (gc, gtp[0], gig[0]) == (c, tpb, igb), key


def test_unbounded_range_equals_eval_ref_on_every_case():
    for images in (ec.case_a(), ec.case_b(True), ec.case_b(False), ec.case_crowd_after_match(), ec.case_score_tie()):
        _unbounded_equals_eval_ref(images, 1)
    _unbounded_equals_eval_ref(ec.case_tie(), 1, iou_thresholds=[0.3])
    im = ec.image(0, [(0.9, [50, 50, 60, 60], 0), (0.8, ec.SQ, 0), (0.7, ec.SQ, 1)], [(ec.SQ, 0, 0), (ec.SQ, 1, 0)])
    _unbounded_equals_eval_ref([im], 2, max_dets=1)
    rng = np.random.default_rng(11)
    _unbounded_equals_eval_ref(ec.random_images(rng, 6, 30, 8, 4), 4)
    _unbounded_equals_eval_ref(ec.random_images(rng, 3, 12, 5, 3, grid=16), 3, max_dets=3)


def test_ranged_first_range_equals_eval_ref():
    """The unbounded "all" of the four COCO ranges gives eval_ref's table too (the other ranges do
    not disturb it)."""
    images = eac.random_images(np.random.default_rng(4), 3, 20, 8, 3)
    ref = eval_ref.evaluate(images, 3, "coco")
    got = ear.evaluate(images, 3)
    assert got["ap"][0].tobytes() == ref["ap"].tobytes()
    for k in ("mAP", "AP50", "AP75"):
        np.testing.assert_equal(got[k], ref[k])
    np.testing.assert_equal(got["AR100"], ref["AR"])


# ---- merging ----------------------------------------------------------------------------------------------
def _by_key(state):
    o = np.argsort(state["records"]["key"], kind="stable")
    return {k: v[o] for k, v in state["records"].items()}


def _same_state(a, b):
    assert a["config"] == b["config"]
    np.testing.assert_array_equal(a["npos"], b["npos"])
    ra, rb = _by_key(a), _by_key(b)
    assert set(ra) == set(rb) == {"score", "cls", "key", "tp", "ign", "rank"}
    for k in ra:
        assert ra[k].dtype == rb[k].dtype and ra[k].tobytes() == rb[k].tobytes(), k


def test_merge_states_split_equals_whole_in_both_orders():
    from cvlite.evaluate import merge_states
    images = eac.random_images(np.random.default_rng(2), 6, 16, 6, 3, gt_area=True)
    whole = ear.state(images, 3)
    assert whole["npos"].sum() > 0 and (whole["records"]["cls"] < 3).any()
    a, b = ear.state(images[0::2], 3), ear.state(images[1::2], 3)
    _same_state(merge_states([a, b]), whole)
    _same_state(merge_states([b, a]), whole)
    _same_state(merge_states([whole]), whole)
    three = [ear.state(images[i::3], 3) for i in (2, 0, 1)]
    _same_state(merge_states(three), whole)


def test_merge_states_refuses_duplicates_and_other_configs():
    from cvlite.evaluate import merge_states
    images = eac.random_images(np.random.default_rng(3), 4, 8, 4, 2)
    a, b = ear.state(images[:2], 2), ear.state(images[1:], 2)                 # image 1 in both
    with pytest.raises(ValueError):
        merge_states([a, b])
    with pytest.raises(ValueError):
        merge_states([ear.state(images[:2], 2), ear.state(images[2:], 2, max_dets=10)])
    with pytest.raises(ValueError):
        merge_states([ear.state(images[:2], 2), ear.state(images[2:], 2, ranges=ear.COCO_RANGES[:2])])
    with pytest.raises(ValueError):
        merge_states([])


def test_reference_state_matches_the_evaluator_config():
    from cvlite.evaluate import Evaluator
    ev = Evaluator(3, "coco", area_ranges="coco")
    assert ev.config() == ear.state([], 3)["config"]
    st = ev.state()                                   # nothing added: no device needed
    assert st["npos"].shape == (4, 3) and st["records"]["tp"].shape == (0, 4) and len(st["records"]["rank"]) == 0
    assert sorted(Evaluator(3, "coco").state()["records"]) == ["cls", "ign", "key", "score", "tp"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, out_dir):
    import sys
    sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    from cvlite.evaluate import gather_states
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    images = eac.random_images(np.random.default_rng(6), 5, 12, 5, 3, area_scale=True)
    merged = gather_states(ear.state(images[rank::world], 3))
    with open(os.path.join(out_dir, "merged_%d.pkl" % rank), "wb") as f:
        pickle.dump(merged, f)
    tdist.barrier()
    tdist.destroy_process_group()


def test_gather_states_over_gloo():
    """Two fresh host processes each hold a shard's state; every rank ends with the whole set's."""
    world = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_gather_worker, args=(world, _free_port(), td), nprocs=world, join=True)
        got = []
        for r in range(world):
            with open(os.path.join(td, "merged_%d.pkl" % r), "rb") as f:
                got.append(pickle.load(f))
    images = eac.random_images(np.random.default_rng(6), 5, 12, 5, 3, area_scale=True)
    whole = ear.state(images, 3)
    for g in got:
        _same_state(g, whole)


# ---- host-side API ------------------------------------------------------------------------------------------
def test_area_ranges_validation():
    from cvlite import evaluate as E
    for protocol in ("voc07", "voc12"):
        with pytest.raises(ValueError):
            E.Evaluator(3, protocol, area_ranges="coco")
    with pytest.raises(ValueError):
        E.Evaluator(3, "coco", area_ranges="pascal")
    with pytest.raises(ValueError):
        E.Evaluator(3, "coco", area_ranges=[("r%d" % i, 0, 1) for i in range(5)])
    with pytest.raises(ValueError):
        E.Evaluator(3, "coco", area_ranges=[])
    ev = E.Evaluator(3, "coco", area_ranges="coco")
    assert [r[0] for r in ev.area_ranges] == ["all", "small", "medium", "large"]
    assert ev.area_ranges[0][1:] == (-INF, INF) and ev.area_ranges[1][1:] == (0.0, 1024.0)
    assert ev.area_ranges[2][1:] == (1024.0, 9216.0) and ev.area_ranges[3][1:] == (9216.0, 1e10)
    assert ev.views() == [(0, 100), (1, 100), (2, 100), (3, 100), (0, 1), (0, 10)]
    assert E.Evaluator(3, "coco", area_ranges=[("tiny", 0, 64)]).views() == [(0, 100), (0, 1), (0, 10)]
    assert E.Evaluator(3, "coco").area_ranges is None
    z = lambda *s, **k: torch.zeros(*s, **k)
    args = (z(2, 4, 4), z(2, 4), z(2, 4), z(2, dtype=torch.int32), z(2, 3, 4), z(2, 3, dtype=torch.int32),
            z(2, dtype=torch.int32))
    with pytest.raises(ValueError):                    # the area inputs need area ranges
        E.Evaluator(3, "coco").add(*args, gt_area=z(2, 3))
    with pytest.raises(ValueError):
        ev.add(*args, gt_area=z(2, 4))
    with pytest.raises(ValueError):
        ev.add(*args, area_scale=z(3))
    with pytest.raises(ValueError):                    # the area column: every image or none
        ev.add_rows([np.zeros((1, 6)), np.zeros((1, 6))], [np.zeros((1, 7)), np.zeros((1, 6))])
    with pytest.raises(ValueError):
        ev.add_rows([np.zeros((1, 6))], [np.zeros((1, 7))], area_scale=[1.0, 2.0])


def test_signatures_registered():
    from cvlite import _lib
    c_int, P, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    res, args = _lib.SIGNATURES["cvl_eval_match_areas"]
    assert res is c_int and args == [P] * 9 + [c_int] * 4 + [P] + [c_int] * 3 + [P, c_int] + [P] * 8 + [i64, P, P]
    res, args = _lib.SIGNATURES["cvl_eval_ap_views"]
    assert res is c_int and args == [P] * 5 + [i64] + [c_int] * 3 + [P, c_int] + [P] * 3
    lib = _lib.load()
    assert hasattr(lib, "cvl_eval_match_areas") and hasattr(lib, "cvl_eval_ap_views")


def test_einval_paths_without_device():
    """A protocol other than COCO, A or R outside their limits, a bad view and NULL arrays return
    CVL_EINVAL (1) before any HIP call: nothing is dereferenced or enqueued."""
    from cvlite import _lib
    lib = _lib.load()
    thr = (ctypes.c_double * 16)(*[0.5] * 16)
    rng = (ctypes.c_double * 8)(*[-INF, INF] * 4)
    buf = (ctypes.c_char * 64)()                    # any non-NULL address: never read on these paths
    p, t, g = (ctypes.cast(x, ctypes.c_void_p) for x in (buf, thr, rng))

    def match(B=1, T=4, G=2, C=3, K=1, protocol=1, max_dets=100, A=4, ranges=g, rank=p, boxes=p, off=0):
        return lib.cvl_eval_match_areas(boxes, p, p, p, p, p, None, p, p, B, T, G, C, t, K, protocol, max_dets, ranges,
                                        A, None, None, p, p, p, p, p, rank, off, p, None)

    for kw in (dict(protocol=0), dict(protocol=2), dict(A=0), dict(A=5), dict(ranges=None), dict(rank=None),
               dict(boxes=None), dict(B=0), dict(T=1025), dict(G=1025), dict(K=17), dict(C=65536), dict(max_dets=0),
               dict(off=-1)):
        assert match(**kw) == 1, kw

    def ap(n=0, C=3, K=1, A=4, R=2, views=(0, 100, 3, 1), seg=p, rank=None, vnull=False):
        v = (ctypes.c_int32 * 16)(*views)
        return lib.cvl_eval_ap_views(None, None, rank, seg, p, n, C, K, A, None if vnull else ctypes.cast(
            v, ctypes.c_void_p), R, p, p, None)

    for kw in (dict(R=0), dict(R=9), dict(A=0), dict(A=5), dict(vnull=True), dict(seg=None), dict(n=-1), dict(K=17),
               dict(C=0), dict(views=(4, 100, 0, 1)), dict(views=(-1, 100, 0, 1)), dict(views=(0, 0, 0, 1)),
               dict(n=5)):                          # n > 0 needs the record arrays
        assert ap(**kw) == 1, kw


def test_read_coco_json():
    from cvlite.coco_json import read_coco_json
    path = os.path.join(GOLDEN, "coco_tiny.json")
    out = read_coco_json(path)
    assert [d["file_name"] for d in out] == ["a.jpg", "b.jpg", "c.jpg"]          # the file's image order
    assert [d["image_id"] for d in out] == [7, 3, 9]
    a, b, c = out
    assert a["orig_dim"] == [100, 200] and c["orig_dim"] == [50, 80]
    # categories 1, 18, 44 -> labels 0, 1, 2; category 99 is not listed under "categories": left out
    assert a["label"].tolist() == [1, 0] and a["iscrowd"].tolist() == [0, 1]
    np.testing.assert_array_equal(a["area"], np.array([2500.5, 1800.0], np.float32))
    # (x, y, w, h) = (20, 10, 100, 40) in a 100 x 200 image -> (yc, xc, h, w) = (0.3, 0.35, 0.4, 0.5)
    np.testing.assert_array_equal(a["bbox"], np.array([[0.3, 0.35, 0.4, 0.5], [0.25, 0.125, 0.5, 0.25]], np.float32))
    assert b["label"].tolist() == [2, 0]
    np.testing.assert_array_equal(b["bbox"][0], np.array([0.5, 0.5, 0.5, 0.5], np.float32))
    assert c["bbox"].shape == (0, 4) and c["label"].shape == (0,) and c["area"].dtype == np.float32
    assert a["bbox"].dtype == np.float32 and a["iscrowd"].dtype == np.uint8
    # a chosen subset: the bottle is left out, person -> 0, dog -> 1
    a2, b2, _ = read_coco_json(path, category_ids=[18, 1])
    assert a2["label"].tolist() == [1, 0] and b2["label"].tolist() == [0] and b2["area"].tolist() == [700.0]
    # the dicts feed the drivers' ground truth: pixel corners from the normalised boxes
    from cvlite.evaluate import gt_from_labels
    bx = np.concatenate([a["bbox"], a["label"][:, None].astype(np.float32)], 1)[None]
    gtb, gtl, _ = gt_from_labels(bx, [2], a["orig_dim"])
    np.testing.assert_allclose(gtb[0, 0].numpy(), [10.0, 20.0, 50.0, 120.0], rtol=0, atol=1e-4)
