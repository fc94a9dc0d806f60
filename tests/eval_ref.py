"""numpy float64 restatement of the detection-evaluation contract (INTEGRATION.md "Evaluation";
include/cvlite.h "Detection evaluation"): VOC AP (07 11-point, 12 all-point) and COCO-style mAP
(area "all").  Written from the contract, plain loops, explicit operation order; it shares no code
with cvlite.evaluate or csrc/det_eval.hip.

An image is a dict: id (int), boxes [T,4] (y1, x1, y2, x2), scores [T], classes [T] (float class
values), valid (int), gt_boxes [G,4], gt_labels [G], gt_flags [G] (or None), gt_count (int).
"""
import math

import numpy as np

PROTOCOLS = {"voc07": "voc", "voc12": "voc", "coco": "coco"}


def default_thresholds(protocol):
    if protocol == "coco":
        return [(50 + 5 * k) / 100.0 for k in range(10)]
    return [0.5]


def _mx(a, b):
    return b if b > a else a


def _mn(a, b):
    return b if b < a else a


def iou(d, g, crowd=False):
    """float64 from the fp32 corners, one operation per step."""
    y1d, x1d, y2d, x2d = (float(np.float32(v)) for v in d)
    y1g, x1g, y2g, x2g = (float(np.float32(v)) for v in g)
    ih = _mx(0.0, _mn(y2d, y2g) - _mx(y1d, y1g))
    iw = _mx(0.0, _mn(x2d, x2g) - _mx(x1d, x1g))
    inter = ih * iw
    ad = (y2d - y1d) * (x2d - x1d)
    if crowd:
        return 0.0 if ad <= 0.0 else inter / ad
    ag = (y2g - y1g) * (x2g - x1g)
    den = (ad + ag) - inter
    return 0.0 if den <= 0.0 else inter / den


def match_image(img, C, thresholds, matching, max_dets):
    """-> (records {slot: (class or None when dropped, score, tp_bits, ign_bits)}, npos [C])."""
    T = len(img["scores"])
    valid = min(max(int(img["valid"]), 0), T)
    G = 0 if img.get("gt_boxes") is None else len(img["gt_boxes"])
    ng = min(max(int(img["gt_count"]), 0), G) if G else 0
    flags = img.get("gt_flags")
    gts = []
    npos = [0] * C
    for g in range(ng):
        lab = int(img["gt_labels"][g])
        fl = bool(flags[g]) if flags is not None else False
        if 0 <= lab < C:
            gts.append((g, lab, fl))
            if not fl:
                npos[lab] += 1
    kept = {}
    for t in range(T):
        s = np.float32(img["scores"][t])
        c = np.float32(img["classes"][t])
        if t >= valid or s != s or not (c >= 0 and c < C):
            continue
        kept[t] = (int(c), float(s))
    rec = {t: [None, 0.0, 0, 0] for t in range(T)}
    for c in sorted(set(v[0] for v in kept.values())):
        slots = sorted((t for t in kept if kept[t][0] == c), key=lambda t: (-kept[t][1], t))
        if matching == "coco":
            slots = slots[:max_dets]
        for t in slots:
            rec[t][0], rec[t][1] = c, kept[t][1]
        cg = [(g, fl) for g, lab, fl in gts if lab == c]
        for k, thr in enumerate(thresholds):
            used = set()
            for t in slots:
                box = img["boxes"][t]
                if matching == "voc":
                    ovmax, jmax, jflag = -math.inf, -1, False
                    for g, fl in cg:
                        ov = iou(box, img["gt_boxes"][g])
                        if ov > ovmax:
                            ovmax, jmax, jflag = ov, g, fl
                    if jmax >= 0 and ovmax >= thr:
                        if jflag:
                            rec[t][3] |= 1 << k
                        elif jmax not in used:
                            rec[t][2] |= 1 << k
                            used.add(jmax)
                else:
                    best, m, mcrowd = _mn(thr, 1 - 1e-10), -1, False
                    for g, fl in [x for x in cg if not x[1]] + [x for x in cg if x[1]]:
                        if g in used and not fl:
                            continue
                        if m >= 0 and not mcrowd and fl:
                            break
                        ov = iou(box, img["gt_boxes"][g], crowd=fl)
                        if ov < best:
                            continue
                        best, m, mcrowd = ov, g, fl
                    if m >= 0:
                        used.add(m)
                        rec[t][3 if mcrowd else 2] |= 1 << k
    return {t: tuple(v) for t, v in rec.items()}, npos


def average_precision(tp_flags, npos, mode):
    """tp_flags: the non-ignored detections of one (class, threshold) in accumulation order (True =
    TP).  -> (ap, final tp)."""
    if npos == 0:
        return math.nan, sum(1 for f in tp_flags if f)
    tps, fps, tp, fp = [], [], 0, 0
    for f in tp_flags:
        tp += 1 if f else 0
        fp += 0 if f else 1
        tps.append(tp)
        fps.append(fp)
    n = len(tps)
    env = [0.0] * n
    run = 0.0
    for i in range(n - 1, -1, -1):
        p = tps[i] / (tps[i] + fps[i])
        run = p if p > run else run
        env[i] = run
    if mode == "voc12":
        tot, prev = 0.0, 0             # sum of (tp_i - tp_prev) / npos * envelope_i, the division hoisted
        for i in range(n):
            if tps[i] > prev:
                tot += (tps[i] - prev) * env[i]
            prev = tps[i]
        return tot / npos, tp
    nl = 100 if mode == "coco" else 10
    tot, i = 0.0, 0
    for k in range(nl + 1):             # tp never falls: the first point reaching k / nl moves right with k
        while i < n and nl * tps[i] < k * npos:
            i += 1
        if i == n:
            break
        tot += env[i]
    return tot / (nl + 1), tp


def evaluate(images, num_classes, protocol="voc07", iou_thresholds=None, max_dets=100):
    C = num_classes
    matching = PROTOCOLS[protocol]
    thr = list(default_thresholds(protocol) if iou_thresholds is None else iou_thresholds)
    K = len(thr)
    npos = np.zeros(C, np.int64)
    records = {}
    rows = []                       # (class, score, image id, slot, tp bits, ign bits)
    for img in images:
        rec, np_img = match_image(img, C, thr, matching, max_dets)
        npos += np.array(np_img)
        for t, (c, s, tpb, igb) in rec.items():
            records[(int(img["id"]), t)] = (c, tpb, igb)
            if c is not None:
                rows.append((c, s, int(img["id"]), t, tpb, igb))
    ap = np.full((K, C), np.nan)
    tpf = np.zeros((K, C), np.int64)
    for c in range(C):
        seg = sorted((r for r in rows if r[0] == c), key=lambda r: (-r[1], r[2], r[3]))
        for k in range(K):
            flags = [bool((r[4] >> k) & 1) for r in seg if not (r[5] >> k) & 1]
            ap[k, c], tpf[k, c] = average_precision(flags, int(npos[c]), protocol)
    cnt = npos > 0
    out = {"ap": ap, "npos": npos, "records": records, "thresholds": thr,
           "mAP": float(np.mean(ap[:, cnt])) if cnt.any() else math.nan}
    if protocol == "coco":
        for name, v in (("AP50", 0.5), ("AP75", 0.75)):
            ks = [k for k in range(K) if thr[k] == v]
            out[name] = float(np.mean(ap[ks[0], cnt])) if ks and cnt.any() else math.nan
        out["AR"] = float(np.mean(tpf[:, cnt] / npos[cnt])) if cnt.any() else math.nan
    return out
