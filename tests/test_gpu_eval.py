"""GPU parity of the evaluation kernels (csrc/det_eval.hip: cvl_eval_match, cvl_eval_ap) through
cvlite.evaluate vs the numpy restatement tests/eval_ref.py: TP / ignored bit sets, dropped slots
and npos exactly, ap / mAP within 1e-12 absolute (integer counts, exact fp64 quotients, a sum of at
most 101 terms of at most 1 -- or, all-point, one term per TP of the small cases here -- so the bound
is derived from the formats, not measured)."""
import math

import numpy as np
import pytest
import torch

import eval_cases as ec
import eval_ref

pytestmark = pytest.mark.gpu

PROTOCOLS = ("voc07", "voc12", "coco")
TOL = 1e-12


def _stack(images):
    """eval_ref image dicts of one (T, G) -> the device tensors of Evaluator.add."""
    cat = lambda k, dt: torch.from_numpy(np.stack([np.asarray(im[k]) for im in images]).astype(dt)).cuda()
    return dict(boxes=cat("boxes", np.float32), scores=cat("scores", np.float32), classes=cat("classes", np.float32),
                valid=torch.tensor([im["valid"] for im in images], dtype=torch.int32).cuda(),
                gt_boxes=cat("gt_boxes", np.float32), gt_labels=cat("gt_labels", np.int32),
                gt_count=torch.tensor([im["gt_count"] for im in images], dtype=torch.int32).cuda(),
                gt_flags=cat("gt_flags", np.uint8), image_ids=[im["id"] for im in images])


def _same_shape(images):
    T = max(len(im["scores"]) for im in images)
    G = max(len(im["gt_boxes"]) for im in images)
    out = []
    for im in images:
        dets = [(im["scores"][t], im["boxes"][t], im["classes"][t]) for t in range(len(im["scores"]))]
        gts = [(im["gt_boxes"][g], im["gt_labels"][g], im["gt_flags"][g]) for g in range(len(im["gt_boxes"]))]
        p = ec.image(im["id"], dets, gts, T=T, G=G)
        p["valid"], p["gt_count"] = im["valid"], im["gt_count"]
        out.append(p)
    return out


def _run(images, C, protocol, batches=None, **kw):
    from cvlite.evaluate import Evaluator
    images = _same_shape(images)
    ev = Evaluator(C, protocol, **kw)
    for chunk in (batches or [list(range(len(images)))]):
        ev.add(**_stack([images[i] for i in chunk]))
    return ev, ev.result()


def _check(ev, got, ref, C):
    np.testing.assert_array_equal(got["npos"], ref["npos"])
    rec = ev.records()
    assert len(rec["slot"]) >= len(ref["records"])         # + the slots a smaller image was padded with
    for i in range(len(rec["slot"])):
        c, tpb, igb = ref["records"].get((int(rec["image_id"][i]), int(rec["slot"][i])), (None, 0, 0))
        want = (C if c is None else c, tpb, igb)
        assert (int(rec["cls"][i]), int(rec["tp"][i]), int(rec["ign"][i])) == want, (i, want)
    np.testing.assert_array_equal(np.isnan(got["ap"]), np.isnan(ref["ap"]))
    print("max |ap - ref| =", np.nanmax(np.abs(got["ap"] - ref["ap"]), initial=0.0))
    np.testing.assert_allclose(got["ap"], ref["ap"], rtol=0, atol=TOL)
    for k in ("mAP", "AP50", "AP75", "AR"):
        if k in ref:
            assert (math.isnan(ref[k]) and math.isnan(got[k])) or abs(got[k] - ref[k]) <= TOL, (k, got[k], ref[k])


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_hand_cases(protocol):
    ev, got = _run(ec.case_a(), 1, protocol)
    _check(ev, got, eval_ref.evaluate(ec.case_a(), 1, protocol), 1)
    assert abs(got["mAP"] - float(ec.CASE_A[protocol])) <= TOL
    if protocol == "coco":
        for k, want in enumerate(ec.CASE_A_COCO_K):
            assert abs(got["ap"][k, 0] - float(want)) <= TOL
    for flagged, want in ((True, 1.0), (False, 0.5)):
        ev, got = _run(ec.case_b(flagged), 1, protocol)
        _check(ev, got, eval_ref.evaluate(ec.case_b(flagged), 1, protocol), 1)
        assert abs(got["mAP"] - want) <= TOL
    thr = [0.3]
    ev, got = _run(ec.case_tie(), 1, protocol, iou_thresholds=thr)
    _check(ev, got, eval_ref.evaluate(ec.case_tie(), 1, protocol, iou_thresholds=thr), 1)
    ev, got = _run(ec.case_crowd_after_match(), 1, protocol)
    _check(ev, got, eval_ref.evaluate(ec.case_crowd_after_match(), 1, protocol), 1)
    ev, got = _run(ec.case_score_tie(), 1, protocol)
    _check(ev, got, eval_ref.evaluate(ec.case_score_tie(), 1, protocol), 1)


def test_hand_cases_classes_and_max_dets():
    im = ec.image(0, [(0.9, ec.SQ, 0), (0.8, ec.SQ, 1)], [(ec.SQ, 0, 0), (ec.SQ, 2, 0)])
    for protocol in PROTOCOLS:
        ev, got = _run([im], 4, protocol)
        _check(ev, got, eval_ref.evaluate([im], 4, protocol), 4)
        assert got["mAP"] == 0.5 and np.isnan(got["ap"][:, 1]).all() and (got["ap"][:, 2] == 0).all()
    im = ec.image(0, [(0.9, [50, 50, 60, 60], 0), (0.8, ec.SQ, 0), (0.7, ec.SQ, 1)], [(ec.SQ, 0, 0), (ec.SQ, 1, 0)])
    for protocol in ("coco", "voc07"):
        ev, got = _run([im], 2, protocol, max_dets=1)
        _check(ev, got, eval_ref.evaluate([im], 2, protocol, max_dets=1), 2)
    ev, got = _run([ec.image(0, [(0.5, ec.SQ, 0)], [])], 2, "voc07")         # no ground truth at all
    assert math.isnan(got["mAP"]) and np.isnan(got["ap"]).all()


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_random_exact_grid(protocol):
    rng = np.random.default_rng(11)
    B, T, G, C = 16, 100, 20, 20
    images = ec.random_images(rng, B, T, G, C)
    ref = eval_ref.evaluate(images, C, protocol)
    assert (ref["npos"] > 0).sum() >= C // 2
    on_thr = sum(1 for im in images for t in range(im["valid"]) for g in range(im["gt_count"])
                 if eval_ref.iou(im["boxes"][t], im["gt_boxes"][g]) == 0.5)
    assert on_thr > 0, "the grid must produce IoUs exactly on a threshold"
    ev, got = _run(images, C, protocol)
    _check(ev, got, ref, C)


@pytest.mark.parametrize("B,T,G,C", [(3, 8, 5, 3), (1, 1, 0, 2), (1, 1, 1, 1), (2, 300, 40, 4)])
def test_small_and_odd_shapes(B, T, G, C):
    rng = np.random.default_rng(B * 1000 + T)
    images = ec.random_images(rng, B, T, G, C, grid=16)
    for protocol in PROTOCOLS:
        ev, got = _run(images, C, protocol, max_dets=100 if T < 300 else 7)
        _check(ev, got, eval_ref.evaluate(images, C, protocol, max_dets=100 if T < 300 else 7), C)


def test_ap_chunk_boundaries():
    """cvl_eval_ap walks a class segment in chunks of 1024 records: class 0 holds two chunks plus one
    detection, class 1 exactly one chunk, class 2 one record short of a chunk."""
    CH = 1024
    rng = np.random.default_rng(3)
    want = {0: 2 * CH + 1, 1: CH, 2: CH - 1}
    T, B = 256, 17
    pool = [c for c, n in want.items() for _ in range(n)]
    pool += [3] * (B * T - len(pool))                    # class 3: out of range with C = 3 -> dropped
    pool = rng.permutation(np.array(pool))
    images = []
    for b in range(B):
        gts = [([4 * g, 0, 4 * g + 4, 4], int(rng.integers(0, 3)), int(rng.random() < 0.2)) for g in range(4)]
        dets = []
        for t in range(T):
            g = int(rng.integers(0, 4))
            box = list(gts[g][0]) if rng.random() < 0.5 else [4 * g, 0, 4 * g + 4, int(rng.integers(1, 9))]
            dets.append((float(rng.integers(1, 65)) / 64.0, box, float(pool[b * T + t])))
        images.append(ec.image(b, dets, gts))
    for protocol in PROTOCOLS:
        ev, got = _run(images, 3, protocol, max_dets=T)
        rec = ev.records()
        assert {c: int((rec["cls"] == c).sum()) for c in want} == want
        _check(ev, got, eval_ref.evaluate(images, 3, protocol, max_dets=T), 3)


def test_batching_invariance_and_add_rows():
    from cvlite.evaluate import Evaluator
    rng = np.random.default_rng(5)
    C = 6
    images = ec.random_images(rng, 32, 24, 6, C, id0=100)
    for im in images:               # add_rows takes the valid rows only: keep the dropped slots inside valid
        im["valid"] = len(im["scores"])
    for protocol in PROTOCOLS:
        _, a = _run(images, C, protocol, batches=[list(range(16)), list(range(16, 32))])
        _, b = _run(images, C, protocol, batches=[list(range(8 * i, 8 * i + 8))[::-1] for i in (3, 2, 1, 0)])
        ev = Evaluator(C, protocol)
        for lo in (20, 0):
            chunk = images[lo:lo + 20] if lo == 0 else images[20:]
            ev.add_rows([np.concatenate([im["boxes"], im["scores"][:, None], im["classes"][:, None]], 1)
                         for im in chunk],
                        [np.concatenate([im["gt_boxes"], im["gt_labels"][:, None], im["gt_flags"][:, None]],
                                        1)[:im["gt_count"]] for im in chunk], image_ids=[im["id"] for im in chunk])
        c = ev.result()
        assert a["ap"].tobytes() == b["ap"].tobytes() == c["ap"].tobytes()
        np.testing.assert_array_equal(a["npos"], c["npos"])
        ref = eval_ref.evaluate(images, C, protocol)
        np.testing.assert_allclose(a["ap"], ref["ap"], rtol=0, atol=TOL)


def test_add_rows_xyxy_and_growth():
    """fmt="xyxy" swaps the corner order; a capacity of one record grows by reallocation."""
    from cvlite.evaluate import Evaluator
    imgs = ec.case_a()
    ev = Evaluator(1, "voc07", capacity=1)
    for im in imgs:
        rows = np.concatenate([im["boxes"][:, [1, 0, 3, 2]], im["scores"][:, None], im["classes"][:, None]], 1)
        ev.add_rows([rows[:im["valid"]]], [np.concatenate([im["gt_boxes"], im["gt_labels"][:, None]], 1)], fmt="xyxy")
    assert abs(ev.result()["mAP"] - float(ec.CASE_A["voc07"])) <= TOL
    ev.reset()
    assert math.isnan(ev.result()["mAP"]) and ev.npos().sum() == 0


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_teacher_is_perfect(protocol):
    """Ground-truth boxes fed back as detections with score 1: mAP == 1.0 exactly."""
    from cvlite.evaluate import Evaluator
    rng = np.random.default_rng(9)
    B, G, C = 8, 12, 5
    gt = np.zeros((B, G, 4), np.float32)
    lab = rng.integers(0, C, (B, G)).astype(np.int32)
    cnt = rng.integers(0, G + 1, B).astype(np.int32)
    cnt[0] = G
    for b in range(B):
        for g in range(G):          # disjoint cells: no detection overlaps another ground truth
            y, x = 20.0 * g, 20.0 * b
            gt[b, g] = [y + rng.uniform(0, 3), x + rng.uniform(0, 3), y + rng.uniform(8, 19), x + rng.uniform(8, 19)]
    ev = Evaluator(C, protocol)
    g_ = torch.from_numpy(gt).cuda()
    ev.add(g_, torch.ones((B, G), device="cuda"), torch.from_numpy(lab).float().cuda(), torch.from_numpy(cnt).cuda(),
           g_, torch.from_numpy(lab).cuda(), torch.from_numpy(cnt).cuda())
    r = ev.result()
    assert r["mAP"] == 1.0 and (r["ap"][:, r["npos"] > 0] == 1.0).all()
    if protocol == "coco":
        assert r["AP50"] == 1.0 and r["AP75"] == 1.0 and r["AR"] == 1.0


def test_gt_from_labels():
    from cvlite.evaluate import gt_from_labels
    bx = np.array([[[0.5, 0.25, 0.5, 0.25, 2.0], [0, 0, 0, 0, 0]]], np.float32)
    gtb, gtl, gtc = gt_from_labels(torch.from_numpy(bx).cuda(), torch.tensor([1]).cuda(), np.array([[64.0, 128.0]]))
    np.testing.assert_array_equal(gtb[0, 0].cpu().numpy(), np.array([16.0, 16.0, 48.0, 48.0], np.float32))
    assert int(gtl[0, 0]) == 2 and int(gtc[0]) == 1 and gtb.is_cuda


# ---- end to end ---------------------------------------------------------------------------------------
def _samples(rng, n, S, C):
    out = []
    for i in range(n):
        k = int(rng.integers(1, 4))
        hw = rng.uniform(0.2, 0.8, (k, 2))
        c = rng.uniform(hw / 2, 1 - hw / 2)
        out.append(dict(image=rng.uniform(-1, 1, (S, S, 3)).astype(np.float32),
                        bbox=np.concatenate([c, hw], 1).astype(np.float32), label=rng.integers(0, C, k),
                        difficult=(rng.random(k) < 0.3).astype(np.uint8)))
    return out


def _ref_images(samples, dets, S):
    """eval_ref images from the samples' ground truth and per-image (boxes, scores, classes, valid)."""
    from cvlite.evaluate import gt_from_labels
    out = []
    for i, (s, d) in enumerate(zip(samples, dets)):
        n = len(s["label"])
        bx = np.concatenate([s["bbox"], np.asarray(s["label"], np.float32)[:, None]], 1)[None]
        gtb, gtl, _ = gt_from_labels(bx, [n], (S, S))
        out.append(dict(id=i, boxes=d[0], scores=d[1], classes=d[2], valid=d[3], gt_boxes=gtb[0].numpy(),
                        gt_labels=gtl[0].numpy(), gt_flags=s["difficult"], gt_count=n))
    return out


def test_evaluate_fcos_end_to_end():
    from cvlite import fcos
    from cvlite.evaluate import Evaluator, evaluate_fcos
    from cvlite.infer_fcos import image_detections
    C, S = 3, 256
    rng = np.random.default_rng(2)
    samples = _samples(rng, 3, S, C)
    model = fcos.build_model(C)
    kw = dict(cls_thresh=0.0101, max_total_size=40)
    # by hand, in the driver's batches of 2: [0, 1] and [2, zero image with valid = 0 / gt_count = 0]
    batches = [np.stack([samples[0]["image"], samples[1]["image"]]),
               np.stack([samples[2]["image"], np.zeros((S, S, 3), np.float32)])]
    outs = [image_detections(x, model, C, **kw) for x in batches]
    dets = [(outs[i // 2].nmsed_boxes[i % 2].cpu().numpy(), outs[i // 2].nmsed_scores[i % 2].cpu().numpy(),
             outs[i // 2].nmsed_classes[i % 2].cpu().numpy(), int(outs[i // 2].valid_detections[i % 2]))
            for i in range(3)]
    assert min(d[3] for d in dets) > 0
    imgs = _ref_images(samples, dets, S)
    G = max(len(s["label"]) for s in samples)
    for protocol in ("voc07", "coco"):
        got = evaluate_fcos(model, samples, C, batch_size=2, protocol=protocol, **kw)
        ev = Evaluator(C, protocol)
        for bi, det in enumerate(outs):
            gtb, gtl, gtf = np.zeros((2, G, 4), np.float32), np.zeros((2, G), np.int32), np.zeros((2, G), np.uint8)
            cnt = np.zeros(2, np.int32)
            valid = det.valid_detections.clone()
            for b in range(2):
                if 2 * bi + b < 3:
                    im = imgs[2 * bi + b]
                    n = cnt[b] = im["gt_count"]
                    gtb[b, :n], gtl[b, :n], gtf[b, :n] = im["gt_boxes"], im["gt_labels"], im["gt_flags"]
                else:
                    valid[b] = 0
            ev.add(det.nmsed_boxes, det.nmsed_scores, det.nmsed_classes, valid, torch.from_numpy(gtb).cuda(),
                   torch.from_numpy(gtl).cuda(), torch.from_numpy(cnt).cuda(), gt_flags=torch.from_numpy(gtf).cuda(),
                   image_ids=[2 * bi, 2 * bi + 1])
        hand = ev.result()
        assert got["ap"].tobytes() == hand["ap"].tobytes()
        np.testing.assert_equal(got["mAP"], hand["mAP"])
        np.testing.assert_array_equal(got["npos"], hand["npos"])
        _check(ev, hand, eval_ref.evaluate(imgs, C, protocol), C)


def test_evaluate_retinanet_end_to_end():
    from cvlite.evaluate import Evaluator, evaluate_retinanet
    from cvlite.retinanet import RetinaNet
    C, S = 3, 256
    rng = np.random.default_rng(4)
    samples = _samples(rng, 2, S, C)
    net = RetinaNet(C, {}, anchor_sizes=[20.0, 40.0, 80.0, 160.0, 320.0])
    x = torch.from_numpy(np.stack([s["image"] for s in samples])).cuda()
    shapes, _, _ = net.model.layout(2, S, S)
    reg, cls = net.model.forward(x, train=False)
    rows = [r[:1024] for r in net.decode_detections(reg, cls, shapes, iou_thresh=0.5, cls_thresh=0.0101)]
    assert min(len(r) for r in rows) > 0
    T = max(len(r) for r in rows)
    dets = []
    for r in rows:
        p = np.zeros((T, 6), np.float32)
        p[:len(r)] = r
        dets.append((p[:, :4], p[:, 4], p[:, 5], len(r)))
    imgs = _ref_images(samples, dets, S)
    for protocol in ("coco", "voc12"):
        got = evaluate_retinanet(net, samples, batch_size=2, protocol=protocol, cls_thresh=0.0101)
        ev = Evaluator(C, protocol)
        ev.add_rows(rows, [np.concatenate([im["gt_boxes"], im["gt_labels"][:, None], im["gt_flags"][:, None]], 1)
                           for im in imgs])
        hand = ev.result()
        assert got["ap"].tobytes() == hand["ap"].tobytes()
        np.testing.assert_equal(got["mAP"], hand["mAP"])
        _check(ev, hand, eval_ref.evaluate(imgs, C, protocol), C)


def test_evaluate_centernet_runs():
    """The separable-hourglass driver end to end (random weights: the numbers mean nothing; the
    decode's rows reach the evaluator in its corner order and every class with ground truth counts)."""
    from cvlite import centernet_hourglass as ch
    from cvlite.evaluate import evaluate_centernet
    C, S = 3, 128
    samples = _samples(np.random.default_rng(6), 3, S, C)
    model = ch.build_model(C, n_filters=64)
    pred = model(np.stack([s["image"] for s in samples[:2]]), training=False)
    kept = ch.decode_detections(pred[0], thresh=0.005, downsample=4, img_rows=S, img_cols=S)[1]
    print("centernet rows of image 0:", len(kept))
    assert len(kept) > 0, "the threshold must let detections through"
    r = evaluate_centernet(model, samples, C, batch_size=2, protocol="voc12", thresh=0.005)
    assert r["ap"].shape == (1, C) and r["npos"].sum() > 0
    ap = r["ap"][0, r["npos"] > 0]
    assert ((ap >= 0) & (ap <= 1)).all()


def _label_seq(text):
    return [ln.split(":")[0] for ln in text.splitlines() if ln.strip() and not ln.startswith("-")]


def test_train_eval_hook(tmp_path, capsys):
    from cvlite import fcos
    from cvlite.train_fcos import SGD, train
    C, S = 3, 128
    data = _samples(np.random.default_rng(8), 4, S, C)
    model = fcos.build_model(C)
    args = dict(init_lr=5e-4, display_step=1, step_save=10, step_cool=10, weight_decay=0.0,
                save_loss_file=str(tmp_path / "loss.csv"))
    train(data, [], model, 2, SGD(5e-4, 0.9), "", None, 0, 2, **args)
    base = capsys.readouterr().out
    assert "Eval mAP" not in base and "Average Loss" in base
    train(data, [], model, 2, SGD(5e-4, 0.9), "", None, 0, 2, eval_data=data[:3], eval_every=1, **args)
    out = capsys.readouterr().out
    evals = [ln for ln in out.splitlines() if ln.startswith("Eval mAP:")]
    assert len(evals) == 2 and all(np.isfinite(float(ln.split(":")[1])) for ln in evals)
    # everything else the loop prints is as without the hook
    assert [l for l in _label_seq(out) if l != "Eval mAP"] == _label_seq(base)
