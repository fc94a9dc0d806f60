"""numpy float64 restatement of the ranged COCO evaluation contract (include/cvlite.h
cvl_eval_match_areas / cvl_eval_ap_views; INTEGRATION.md "Evaluation"): pycocotools' evaluateImg per
area range and accumulate per maxDets, in plain loops with an explicit operation order.  The IoU and
the AP of one (class, threshold) are eval_ref's; nothing is shared with cvlite.evaluate or
csrc/det_eval.hip.

An image is an eval_ref image dict plus two optional entries: gt_area [G] (used as is in place of
the ground truths' box areas) and area_scale (a number: every box-derived area is multiplied by its
fp32 value once).
"""
import math

import numpy as np

from eval_ref import _mn, average_precision, default_thresholds, iou

INF = math.inf
COCO_RANGES = [("all", -INF, INF), ("small", 0.0, 32.0 ** 2), ("medium", 32.0 ** 2, 96.0 ** 2),
               ("large", 96.0 ** 2, 1e10)]
SUMMARY = ("mAP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def coco_views(max_dets=100):
    return [(0, max_dets), (1, max_dets), (2, max_dets), (3, max_dets), (0, 1), (0, 10)]


def box_area(box, scale=None):
    y1, x1, y2, x2 = (float(np.float32(v)) for v in box)
    a = (y2 - y1) * (x2 - x1)
    return a if scale is None else a * float(np.float32(scale))


def outside(v, lo, hi):
    return v < lo or v > hi


def match_image(img, C, thresholds, ranges, max_dets):
    """-> (records {slot: (class or None when dropped, score, rank or None, tp bits [A], ign bits
    [A])}, npos [A][C])."""
    A = len(ranges)
    T = len(img["scores"])
    valid = min(max(int(img["valid"]), 0), T)
    G = 0 if img.get("gt_boxes") is None else len(img["gt_boxes"])
    ng = min(max(int(img["gt_count"]), 0), G) if G else 0
    flags = img.get("gt_flags")
    scale = img.get("area_scale")
    gts = []                            # (g, label, crowd, area)
    for g in range(ng):
        lab = int(img["gt_labels"][g])
        if 0 <= lab < C:
            crowd = bool(flags[g]) if flags is not None else False
            if img.get("gt_area") is not None:
                area = float(np.float32(img["gt_area"][g]))
            else:
                area = box_area(img["gt_boxes"][g], scale)
            gts.append((g, lab, crowd, area))
    npos = [[0] * C for _ in range(A)]
    kept = {}
    for t in range(T):
        s = np.float32(img["scores"][t])
        c = np.float32(img["classes"][t])
        if t >= valid or s != s or not (c >= 0 and c < C):
            continue
        kept[t] = (int(c), float(s))
    rec = {t: [None, 0.0, None, [0] * A, [0] * A] for t in range(T)}
    ious = {}                           # (slot, g) -> IoU: the same value for every range and threshold

    def pair_iou(t, g, crowd):
        if (t, g) not in ious:
            ious[(t, g)] = iou(img["boxes"][t], img["gt_boxes"][g], crowd=crowd)
        return ious[(t, g)]

    for c in range(C):
        cg = [x for x in gts if x[1] == c]
        for a, (_, lo, hi) in enumerate(ranges):
            npos[a][c] += sum(1 for (_, _, crowd, area) in cg if not (crowd or outside(area, lo, hi)))
        slots = sorted((t for t in kept if kept[t][0] == c), key=lambda t: (-kept[t][1], t))[:max_dets]
        for rank, t in enumerate(slots):
            rec[t][0], rec[t][1], rec[t][2] = c, kept[t][1], rank
        for a, (_, lo, hi) in enumerate(ranges):
            ign = {g: (crowd or outside(area, lo, hi)) for (g, _, crowd, area) in cg}
            visit = [x for x in cg if not ign[x[0]]] + [x for x in cg if ign[x[0]]]
            for k, thr in enumerate(thresholds):
                used = set()
                for t in slots:
                    box = img["boxes"][t]
                    best, m = _mn(thr, 1 - 1e-10), -1
                    for (g, _, crowd, _) in visit:
                        if g in used and not crowd:
                            continue
                        if m >= 0 and not ign[m] and ign[g]:
                            break
                        ov = pair_iou(t, g, crowd)
                        if ov < best:
                            continue
                        best, m = ov, g
                    if m >= 0:
                        used.add(m)
                        rec[t][4 if ign[m] else 3][a] |= 1 << k
                    elif outside(box_area(box, scale), lo, hi):
                        rec[t][4][a] |= 1 << k
    return {t: (v[0], v[1], v[2], tuple(v[3]), tuple(v[4])) for t, v in rec.items()}, npos


def evaluate(images, num_classes, ranges=None, iou_thresholds=None, max_dets=100, views=None):
    """-> records {(image id, slot): (class or None, rank or None, tp bits [A], ign bits [A])},
    npos_area [A, C], ap / tp_total [R, K, C] over the views [(area index, max_rank)] (default: one
    view per range at max_dets, then (0, 1) and (0, 10)), and the summary numbers."""
    C = num_classes
    ranges = COCO_RANGES if ranges is None else list(ranges)
    A = len(ranges)
    thr = list(default_thresholds("coco") if iou_thresholds is None else iou_thresholds)
    K = len(thr)
    views = [(a, max_dets) for a in range(A)] + [(0, 1), (0, 10)] if views is None else list(views)
    npos = np.zeros((A, C), np.int64)
    records, rows = {}, []
    for img in images:
        rec, np_img = match_image(img, C, thr, ranges, max_dets)
        npos += np.array(np_img, np.int64).reshape(A, C)
        for t, (c, s, rank, tpb, igb) in rec.items():
            records[(int(img["id"]), t)] = (c, rank, tpb, igb)
            if c is not None:
                rows.append((c, s, int(img["id"]), t, rank, tpb, igb))
    R = len(views)
    ap = np.full((R, K, C), np.nan)
    tpf = np.zeros((R, K, C), np.int64)
    for c in range(C):
        seg = sorted((r for r in rows if r[0] == c), key=lambda r: (-r[1], r[2], r[3]))
        for v, (a, max_rank) in enumerate(views):
            for k in range(K):
                fl = [bool((r[5][a] >> k) & 1) for r in seg if not ((r[6][a] >> k) & 1 or r[4] >= max_rank)]
                ap[v, k, c], tpf[v, k, c] = average_precision(fl, int(npos[a, c]), "coco")
    out = {"ap": ap, "tp_total": tpf, "npos_area": npos, "records": records, "thresholds": thr, "views": views}
    out.update(summary_numbers(ap, tpf, npos, views, thr))
    return out


def _mean_ap(ap, cnt, k=None):
    if not cnt.any():
        return math.nan
    return float(np.mean(ap[:, cnt] if k is None else ap[k, cnt]))


def _mean_ar(tpf, np_a):
    cnt = np_a > 0
    return float(np.mean(tpf[:, cnt] / np_a[cnt])) if cnt.any() else math.nan


def summary_numbers(ap, tpf, npos, views, thr):
    """The per-view means: AP_view / AR_view lists, and the twelve COCO names when the views are
    coco_views()."""
    out = {"AP_view": [_mean_ap(ap[v], npos[a] > 0) for v, (a, _) in enumerate(views)],
           "AR_view": [_mean_ar(tpf[v], npos[a]) for v, (a, _) in enumerate(views)]}
    if len(views) == 6 and [a for a, _ in views] == [0, 1, 2, 3, 0, 0]:
        cnt = npos[0] > 0
        out["mAP"] = out["AP_view"][0]
        for name, val in (("AP50", 0.5), ("AP75", 0.75)):
            ks = [k for k in range(len(thr)) if thr[k] == val]
            out[name] = _mean_ap(ap[0], cnt, ks[0]) if ks else math.nan
        out["APs"], out["APm"], out["APl"] = out["AP_view"][1:4]
        out["AR1"], out["AR10"], out["AR100"] = out["AR_view"][4], out["AR_view"][5], out["AR_view"][0]
        out["ARs"], out["ARm"], out["ARl"] = out["AR_view"][1:4]
        out["summary"] = [out[k] for k in SUMMARY]
    return out


def state(images, num_classes, ranges=None, iou_thresholds=None, max_dets=100):
    """The cvlite.evaluate.Evaluator.state() the contract implies for these images added in this
    order (one record per slot): what the device records are compared with, and what the host-only
    merging tests merge."""
    ranges = COCO_RANGES if ranges is None else list(ranges)
    A, C = len(ranges), num_classes
    thr = list(default_thresholds("coco") if iou_thresholds is None else iou_thresholds)
    npos = np.zeros((A, C), np.int32)
    n = sum(len(im["scores"]) for im in images)
    rec = dict(score=np.zeros(n, np.float32), cls=np.full(n, C, np.int32), key=np.zeros(n, np.int64),
               tp=np.zeros((n, A), np.uint16), ign=np.zeros((n, A), np.uint16), rank=np.full(n, 0xffff, np.uint16))
    i = 0
    for im in images:
        kept, np_img = match_image(im, C, thr, ranges, max_dets)
        npos += np.array(np_img, np.int32).reshape(A, C)
        for t in range(len(im["scores"])):
            c, s, rank, tpb, igb = kept[t]
            rec["key"][i] = (int(im["id"]) << 32) | t
            if c is not None:
                rec["score"][i], rec["cls"][i], rec["rank"][i], rec["tp"][i], rec["ign"][i] = s, c, rank, tpb, igb
            i += 1
    for k in ("tp", "ign", "rank"):
        rec[k] = rec[k].view(np.int16)
    cfg = dict(num_classes=C, protocol="coco", thresholds=thr, max_dets=max_dets,
               area_ranges=[(str(nm), float(lo), float(hi)) for nm, lo, hi in ranges])
    return dict(config=cfg, records=rec, npos=npos,
                next_id=max([int(im["id"]) for im in images] + [-1]) + 1)
