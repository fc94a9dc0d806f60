"""GPU parity of the ranged COCO evaluation (csrc/det_eval.hip: cvl_eval_match_areas,
cvl_eval_ap_views) through cvlite.evaluate vs the numpy restatement tests/eval_area_ref.py: the TP /
ignored bit sets per range, the ranks, the dropped slots, npos and the final TP counts exactly; AP
within 1e-12 absolute, the bound tests/test_gpu_eval.py derives from the formats (integer counts,
exact fp64 quotients, a sum of at most 101 terms of at most 1)."""
import functools
import math

import numpy as np
import pytest
import torch

import eval_area_cases as eac
import eval_area_ref as ear
import eval_cases as ec
import test_eval_area_ref as host

pytestmark = pytest.mark.gpu

TOL = 1e-12
INF = math.inf


def _same_shape(images):
    T = max(len(im["scores"]) for im in images)
    G = max(len(im["gt_boxes"]) for im in images)
    out = []
    for im in images:
        dets = [(im["scores"][t], im["boxes"][t], im["classes"][t]) for t in range(len(im["scores"]))]
        gts = [(im["gt_boxes"][g], im["gt_labels"][g], im["gt_flags"][g]) for g in range(len(im["gt_boxes"]))]
        p = ec.image(im["id"], dets, gts, T=T, G=G)
        p["valid"], p["gt_count"] = im["valid"], im["gt_count"]
        if im.get("gt_area") is not None:
            p["gt_area"] = np.zeros(G, np.float32)
            p["gt_area"][:len(im["gt_area"])] = im["gt_area"]
        if im.get("area_scale") is not None:
            p["area_scale"] = im["area_scale"]
        out.append(p)
    return out


def _stack(images, ranged=True):
    """eval_ref image dicts of one (T, G) -> the device tensors of Evaluator.add."""
    cat = lambda k, dt: torch.from_numpy(np.stack([np.asarray(im[k]) for im in images]).astype(dt)).cuda()
    out = dict(boxes=cat("boxes", np.float32), scores=cat("scores", np.float32), classes=cat("classes", np.float32),
               valid=torch.tensor([im["valid"] for im in images], dtype=torch.int32).cuda(),
               gt_boxes=cat("gt_boxes", np.float32), gt_labels=cat("gt_labels", np.int32),
               gt_count=torch.tensor([im["gt_count"] for im in images], dtype=torch.int32).cuda(),
               gt_flags=cat("gt_flags", np.uint8), image_ids=[im["id"] for im in images])
    if ranged and images[0].get("gt_area") is not None:
        out["gt_area"] = cat("gt_area", np.float32)
    if ranged and images[0].get("area_scale") is not None:
        out["area_scale"] = torch.tensor([im["area_scale"] for im in images], dtype=torch.float32).cuda()
    return out


def _run(images, C, batches=None, area_ranges="coco", **kw):
    from cvlite.evaluate import Evaluator
    ev = Evaluator(C, "coco", area_ranges=area_ranges, **kw)
    for chunk in (batches or [list(range(len(images)))]):
        ev.add(**_stack([images[i] for i in chunk], ranged=area_ranges is not None))
    return ev, ev.result()


def _check(ev, got, images, C, ranges=None, **kw):
    """Records (bits, ranks, dropped slots) and npos against the restatement's state exactly; every
    view's final TP count exactly and AP within TOL; the summary numbers within TOL."""
    want = ear.state(images, C, ranges, kw.get("iou_thresholds"), kw.get("max_dets", 100))
    host._same_state(ev.state(), want)
    ref = ear.evaluate(images, C, ranges, kw.get("iou_thresholds"), kw.get("max_dets", 100))
    A = len(ref["npos_area"])
    assert ref["views"] == ev.views()
    np.testing.assert_array_equal(got["npos_area"], ref["npos_area"])
    np.testing.assert_array_equal(got["tp_total_area"], ref["tp_total"][:A])
    np.testing.assert_array_equal(np.isnan(got["ap_area"]), np.isnan(ref["ap"][:A]))
    print("max |ap - ref| =", np.nanmax(np.abs(got["ap_area"] - ref["ap"][:A]), initial=0.0))
    np.testing.assert_allclose(got["ap_area"], ref["ap"][:A], rtol=0, atol=TOL)
    pairs = [(got["AP_area"][a], ref["AP_view"][a]) for a in range(A)]
    pairs += [(got["AR_area"][a], ref["AR_view"][a]) for a in range(A)]
    pairs += [(got["AR1"], ref["AR_view"][A]), (got["AR10"], ref["AR_view"][A + 1]), (got["AR100"], ref["AR_view"][0])]
    if "summary" in ref:
        pairs += list(zip(got["summary"], ref["summary"]))
    for g, r in pairs:
        assert (math.isnan(r) and math.isnan(g)) or abs(g - r) <= TOL, (g, r)
    return ref


# ---- the hand case and the random exact-grid cases ----------------------------------------------------
def test_hand_case():
    images = eac.hand_case()
    ev, got = _run(images, 1, iou_thresholds=[0.5])
    _check(ev, got, images, 1, iou_thresholds=[0.5])
    rec = ev.records()
    assert rec["rank"].tolist() == list(range(7))
    for t in range(7):
        assert tuple(rec["tp"][t]) == eac.HAND_TP.get(t, (0, 0, 0, 0)) and tuple(rec["ign"][t]) == eac.HAND_IGN[t]
    assert got["npos_area"][:, 0].tolist() == eac.HAND_NPOS
    for a, want in enumerate(eac.HAND_AP):
        assert abs(got["ap_area"][a, 0, 0] - float(want)) <= TOL
    assert got["AR100"] == 1.0 and got["AR10"] == 1.0 and got["AR1"] == 0.0
    assert got["APs"] == 1.0 and abs(got["APm"] - 0.5) <= TOL and got["APl"] == 1.0
    ev2, got2 = _run(images, 1, iou_thresholds=[0.5], max_dets=2)          # view (all, 2) as a max_dets cut
    assert abs(got2["mAP"] - float(eac.HAND_AP_RANK2)) <= TOL and abs(got2["AR100"] - 1.0 / 3.0) <= TOL
    assert ev2.records()["rank"].tolist() == [0, 1] + [0xffff] * 5          # slots past the cut are dropped


RANDOM = {"plain": dict(crowds=False), "crowds": dict(), "gt_area": dict(gt_area=True),
          "area_scale": dict(area_scale=True), "all": dict(gt_area=True, area_scale=True)}
SEEDS = {"plain": 21, "crowds": 22, "gt_area": 30, "area_scale": 24, "all": 25}      # checked on the CPU (below)


@functools.lru_cache(maxsize=None)
def _random_case(name):
    B, T, G, C = 3, 40, 12, 3
    return _same_shape(eac.random_images(np.random.default_rng(SEEDS[name]), B, T, G, C, **RANDOM[name])), C


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_random_exact_grid(name):
    images, C = _random_case(name)
    ref = ear.evaluate(images, C)
    # the case must make the ranges matter: positives in every range, a ranged AP unlike the overall one
    assert ((ref["npos_area"] > 0).sum(1) > 0).all(), ref["npos_area"]
    assert any(not math.isnan(ref[k]) and ref[k] != ref["mAP"] for k in ("APs", "APm", "APl"))
    ev, got = _run(images, C)
    _check(ev, got, images, C)


def test_ranged_equals_unranged_bitwise():
    """Range "all" is unbounded, so ap / mAP / AP50 / AP75 of a ranged evaluator are the unranged
    evaluator's bit for bit, and AR100 its AR."""
    images, C = _random_case("crowds")
    batches = [[0, 1], [2]]
    _, ranged = _run(images, C, batches=batches)
    _, plain = _run(images, C, batches=batches, area_ranges=None)
    assert ranged["ap"].tobytes() == plain["ap"].tobytes() and not np.isnan(plain["ap"]).all()
    np.testing.assert_array_equal(ranged["npos"], plain["npos"])
    np.testing.assert_array_equal(ranged["tp_total"], plain["tp_total"])
    for k in ("mAP", "AP50", "AP75", "AR"):
        np.testing.assert_equal(ranged[k], plain[k])
    np.testing.assert_equal(ranged["AR100"], plain["AR"])
    # a single unbounded range: the records are cvl_eval_match's
    ev1, _ = _run(images, C, area_ranges=[("all", -INF, INF)])
    ev0, _ = _run(images, C, area_ranges=None)
    r1, r0 = ev1.records(), ev0.records()
    for k in ("image_id", "slot", "cls", "score"):
        np.testing.assert_array_equal(r1[k], r0[k])
    np.testing.assert_array_equal(r1["tp"][:, 0], r0["tp"])
    np.testing.assert_array_equal(r1["ign"][:, 0], r0["ign"])


# ---- shapes where the kernels can go wrong ----------------------------------------------------------------
@pytest.mark.parametrize("B,T,G", [(1, 1, 0), (1, 1, 1), (2, 7, 3)])
def test_smallest_shapes(B, T, G):
    images = _same_shape(eac.random_images(np.random.default_rng(B * 100 + T * 10 + G), B, T, G, 2))
    for im in images:
        im["valid"] = T
    ev, got = _run(images, 2)
    _check(ev, got, images, 2)


@pytest.mark.parametrize("A", [1, 4])
@pytest.mark.parametrize("K", [1, 16])
def test_range_and_threshold_counts(A, K):
    images, C = _random_case("all")
    thr = [0.5 + 0.03 * k for k in range(K)]
    ranges = ear.COCO_RANGES[:A] if A == 4 else [("medium", 1024.0, 9216.0)]
    ev, got = _run(images, C, area_ranges=ranges, iou_thresholds=thr)
    _check(ev, got, images, C, ranges=ranges, iou_thresholds=thr)


def test_ap_chunks_with_rank_views():
    """One class segment of 1280 records (cvl_eval_ap_views walks it in chunks of 1024): the views
    (all, 1) and (all, 10) skip records in the middle of both chunks."""
    rng = np.random.default_rng(7)
    B, T, G = 5, 256, 8
    images = []
    for b in range(B):
        gts = [([40 * g, 0, 40 * g + int(rng.choice(eac.SIDES[:3])), int(rng.choice(eac.SIDES))], 0,
                int(rng.random() < 0.2)) for g in range(G)]
        dets = []
        for t in range(T):
            y1, x1, y2, x2 = gts[int(rng.integers(0, G))][0]
            box = [y1, x1, y2, x2] if rng.random() < 0.5 else [y1, x1, y2, x1 + int(rng.choice(eac.SIDES))]
            dets.append((float(rng.integers(1, 129)) / 128.0, box, 0.0))
        images.append(ec.image(b, dets, gts))
    kw = dict(iou_thresholds=[0.5, 0.75], max_dets=T)
    ev, got = _run(images, 1, **kw)
    assert int((ev.records()["cls"] == 0).sum()) == B * T > 1024
    ref = _check(ev, got, images, 1, **kw)
    assert 0 < ref["AR_view"][4] < ref["AR_view"][5] < ref["AR_view"][0]


def test_one_launch_at_the_limits():
    """T = G = 1024, K = 16, A = 4: the largest LDS carve-up the entry launches (63 KiB)."""
    rng = np.random.default_rng(8)
    T = G = 1024
    C, K = 64, 16
    gts, dets = [], []
    for g in range(G):
        h, w = (int(v) for v in rng.choice(eac.SIDES, 2))
        y1, x1 = (int(v) * 8 for v in rng.integers(0, 64, 2))
        gts.append(([y1, x1, y1 + h, x1 + w], int(rng.integers(0, C)), int(rng.random() < 0.1)))
    for t in range(T):
        (y1, x1, y2, x2), c, _ = gts[int(rng.integers(0, G))]
        d = int(rng.integers(-1, 2)) * (y2 - y1) // 4
        dets.append((float(rng.integers(1, 65)) / 64.0, [y1 + d, x1, y2 + d, x2], float(c)))
    images = [ec.image(0, dets, gts)]
    thr = [0.5 + 0.03 * k for k in range(K)]
    ev, got = _run(images, C, iou_thresholds=thr, max_dets=T)
    _check(ev, got, images, C, iou_thresholds=thr, max_dets=T)
    assert (got["npos_area"].sum(1) > 0).all()


# ---- merging, launch counts ---------------------------------------------------------------------------------
def test_batching_invariance_through_states():
    from cvlite.evaluate import Evaluator, merge_states
    images, C = _random_case("all")
    images = images + _same_shape(eac.random_images(np.random.default_rng(31), 3, 40, 12, C, id0=10, gt_area=True,
                                                    area_scale=True))
    _, whole = _run(images, C)
    ev_a, _ = _run(images[:3], C)
    ev_b, _ = _run(images[3:], C, batches=[[2], [0, 1]])
    for order in ([ev_a, ev_b], [ev_b, ev_a]):
        merged = Evaluator.from_state(merge_states([e.state() for e in order]))
        res = merged.result()
        for k in ("ap", "ap_area", "tp_total_area", "npos_area"):
            assert res[k].tobytes() == whole[k].tobytes(), k
        np.testing.assert_equal(res["summary"], whole["summary"])
    with pytest.raises(ValueError):
        merge_states([ev_a.state(), ev_a.state()])


def test_launch_counts(monkeypatch):
    from cvlite import _lib
    images, C = _random_case("plain")
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    _run(images, C, batches=[[0], [1, 2]])
    assert calls == ["cvl_eval_match_areas", "cvl_eval_match_areas", "cvl_eval_ap_views"]
    del calls[:]
    _run(images, C, batches=[[0], [1, 2]], area_ranges=None)
    assert calls == ["cvl_eval_match", "cvl_eval_match", "cvl_eval_ap"]


def test_einval_paths():
    host.test_einval_paths_without_device()


# ---- drivers ----------------------------------------------------------------------------------------------------
def _samples(rng, n, S, C, area=False):
    out = []
    for i in range(n):
        k = int(rng.integers(1, 4))
        hw = rng.uniform(0.1, 0.8, (k, 2))
        c = rng.uniform(hw / 2, 1 - hw / 2)
        s = dict(image=rng.uniform(-1, 1, (S, S, 3)).astype(np.float32),
                 bbox=np.concatenate([c, hw], 1).astype(np.float32), label=rng.integers(0, C, k),
                 iscrowd=(rng.random(k) < 0.3).astype(np.uint8), orig_dim=[2 * S, 3 * S])
        if area:
            s["area"] = (hw[:, 0] * hw[:, 1] * 6 * S * S * 0.7).astype(np.float32)
        out.append(s)
    return out


def test_evaluate_fcos_shards_merge_to_the_whole():
    from cvlite import fcos
    from cvlite.evaluate import Evaluator, evaluate_fcos, merge_states
    C, S = 3, 256
    samples = _samples(np.random.default_rng(2), 3, S, C)
    model = fcos.build_model(C)
    kw = dict(batch_size=2, protocol="coco", area_ranges="coco", cls_thresh=0.0101, max_total_size=40)
    whole = evaluate_fcos(model, samples, C, **kw)
    assert whole["npos_area"][0].sum() > 0 and len(whole["summary"]) == 12
    states = [evaluate_fcos(model, samples, C, shard=(r, 2), return_state=True, **kw)[1] for r in (0, 1)]
    ids = [set((st["records"]["key"] >> 32).tolist()) for st in states]
    assert {0, 2} <= ids[0] and 1 in ids[1] and not ids[0] & ids[1]           # global indices as image ids
    for order in (states, states[::-1]):
        res = Evaluator.from_state(merge_states(order)).result()
        for k in ("ap_area", "tp_total_area", "npos_area"):
            assert res[k].tobytes() == whole[k].tobytes(), k
        np.testing.assert_equal(res["summary"], whole["summary"])
    # orig_dim reaches the kernel: the areas are 6 x the network-pixel ones, so the ranges see other boxes
    plain = evaluate_fcos(model, [{k: v for k, v in s.items() if k != "orig_dim"} for s in samples], C, **kw)
    assert plain["ap"].tobytes() == whole["ap"].tobytes()
    assert not np.array_equal(plain["npos_area"], whole["npos_area"])


def _finite_or_nan_summary(res, C):
    assert len(res["summary"]) == 12 and res["ap_area"].shape[0] == 4 and res["ap_area"].shape[2] == C
    for v in res["summary"]:
        assert math.isnan(v) or 0.0 <= v <= 1.0
    assert res["npos_area"][0].sum() > 0


def test_evaluate_hourglass_v2_runs():
    from cvlite import tf_hourglass_net as hg2
    from cvlite.evaluate import evaluate_hourglass_v2
    C, S = 3, 128
    samples = _samples(np.random.default_rng(12), 3, S, C, area=True)
    model = hg2.build_model(12, C, n_features=64)
    pred = model(np.stack([s["image"] for s in samples[:2]]), training=False)
    rows = hg2.decode_detections(pred[0], thresh=0.005, img_rows=S, img_cols=S)
    print("hourglass v2 rows of image 0:", len(rows))
    assert len(rows) > 0, "the threshold must let detections through"
    res = evaluate_hourglass_v2(model, samples, C, batch_size=2, protocol="coco", area_ranges="coco", thresh=0.005)
    _finite_or_nan_summary(res, C)


def test_evaluate_centernet_s8_runs():
    from cvlite import tf_centernet_resnet_s8 as s8
    from cvlite.evaluate import evaluate_centernet_s8
    C, S, scales = 3, 128, [32.0, 96.0]
    samples = _samples(np.random.default_rng(13), 3, S, C, area=True)
    model = s8.build_model(C, n_scales=2)
    pred = model(np.stack([s["image"] for s in samples[:2]]), training=False)
    kept = s8.decode_detections(pred[0], scales, thresh=0.005, img_rows=S, img_cols=S)[1]
    print("centernet s8 rows of image 0:", len(kept))
    assert len(kept) > 0, "the threshold must let detections through"
    res = evaluate_centernet_s8(model, samples, C, scales, batch_size=2, protocol="coco", area_ranges="coco",
                                thresh=0.005)
    _finite_or_nan_summary(res, C)
