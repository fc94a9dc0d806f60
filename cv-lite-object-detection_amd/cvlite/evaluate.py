"""Detection evaluation on MI355X: VOC AP (07 11-point, 12 all-point) and COCO-style mAP.

The reference publishes no accuracy and has no evaluator; this is the project's own,
behind include/cvlite.h "Detection evaluation" (csrc/det_eval.hip) -- the contract and its
deviations from the VOC devkit / pycocotools are in INTEGRATION.md "Evaluation":

  Evaluator(num_classes, protocol)      device-resident state: one record per detection slot
    .add(...)                           one cvl_eval_match launch per batch, no host sync
    .add_rows(...)                      the [k, 6] row lists of the RetinaNet / CenterNet decodes
    .result()                           two-key stable sort (plumbing: torch.sort) + cvl_eval_ap
  gt_from_labels(bx, nbox, img_dim)     the trainers' normalised (yc, xc, h, w, cls) -> pixel corners
  evaluate_fcos / evaluate_retinanet / evaluate_centernet / evaluate_hourglass_v2 /
  evaluate_centernet_s8                 inference forward in batches + the family's decode + add

Evaluator(..., protocol="coco", area_ranges="coco") also scores the small / medium / large area
ranges and AR@1 / 10 / 100 -- the twelve-number COCO summary -- through cvl_eval_match_areas (one
launch per add) and cvl_eval_ap_views (one launch per result()); without area_ranges the path and
its two entries are as before.  state() / merge_states / from_state / gather_states combine the
records of several evaluators (data-parallel ranks that each scored a shard): pure host code over
the record arrays, and through the order key the merged result equals one evaluator fed every image,
bit for bit, in any merge order.

There is no CPU fallback: the hot path is the HIP kernels.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

PROTOCOLS = {"voc07": (0, 0), "voc12": (0, 1), "coco": (1, 2)}      # -> (matching protocol, AP mode)
MAX_THRESHOLDS, MAX_T, MAX_G, MAX_CLASSES = 16, 1024, 1024, 65535   # include/cvlite.h CVL_EVAL_MAX_*
MAX_AREAS, MAX_VIEWS = 4, 8
# "all" is unbounded (pycocotools: [0, 1e10]) so that a ranged evaluator's ap equals the unranged one's
COCO_AREA_RANGES = [("all", -math.inf, math.inf), ("small", 0.0, 32.0 ** 2), ("medium", 32.0 ** 2, 96.0 ** 2),
                    ("large", 96.0 ** 2, 1e10)]
SUMMARY_KEYS = ("mAP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def default_thresholds(protocol):
    """The doubles nearest to the decimals: 0.5 (VOC), 0.50:0.05:0.95 (COCO)."""
    return [(50 + 5 * k) / 100.0 for k in range(10)] if protocol == "coco" else [0.5]


def _parse_area_ranges(spec):
    if spec is None:
        return None
    if isinstance(spec, str):
        if spec != "coco":
            raise ValueError("area_ranges must be None, 'coco' or a list of (name, lo, hi), not %r" % (spec,))
        return list(COCO_AREA_RANGES)
    out = [(str(n), float(lo), float(hi)) for n, lo, hi in spec]
    if not 1 <= len(out) <= MAX_AREAS:
        raise ValueError("between 1 and %d area ranges, not %d" % (MAX_AREAS, len(out)))
    return out


def summary(result):
    """The twelve COCO numbers of a ranged result, in pycocotools' order (SUMMARY_KEYS)."""
    return [result[k] for k in SUMMARY_KEYS]


class Evaluator(object):
    def __init__(self, num_classes, protocol="voc07", iou_thresholds=None, max_dets=100, capacity=1 << 16,
                 area_ranges=None):
        if protocol not in PROTOCOLS:
            raise ValueError("protocol must be 'voc07', 'voc12' or 'coco', not %r" % (protocol,))
        self.area_ranges = _parse_area_ranges(area_ranges)
        if self.area_ranges is not None and protocol != "coco":
            raise ValueError("area_ranges need protocol='coco', not %r" % (protocol,))
        self._A = 0 if self.area_ranges is None else len(self.area_ranges)
        self._rng = (ctypes.c_double * (2 * max(self._A, 1)))(*[v for r in self.area_ranges or [] for v in r[1:]])
        thr = default_thresholds(protocol) if iou_thresholds is None else [float(v) for v in iou_thresholds]
        if not 1 <= len(thr) <= MAX_THRESHOLDS:
            raise ValueError("between 1 and %d IoU thresholds, not %d" % (MAX_THRESHOLDS, len(thr)))
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError("num_classes must be in [1, %d]" % MAX_CLASSES)
        if int(max_dets) < 1:
            raise ValueError("max_dets must be >= 1")
        self.C, self.protocol, self.thresholds, self.max_dets = int(num_classes), protocol, thr, int(max_dets)
        self._match, self._mode = PROTOCOLS[protocol]
        self._thr = (ctypes.c_double * len(thr))(*thr)
        self._cap0 = max(1, int(capacity))
        self._buf = None                 # allocated on the first add (the constructor needs no device)
        self.reset()

    # ---- state ---------------------------------------------------------------------------------------
    def reset(self):
        self._pos = 0                    # records in use: host arithmetic over the fixed strides B * T
        self._next_id = 0
        if self._buf is not None:
            self._npos.zero_()

    def _alloc(self, cap, dev):
        """score, class, key, tp, ign; with area ranges tp / ign are [cap, A] and the rank follows."""
        bits = (cap, self._A) if self._A else cap
        buf = (torch.empty(cap, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
               torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(bits, dtype=torch.int16, device=dev),
               torch.empty(bits, dtype=torch.int16, device=dev))
        return buf + (torch.empty(cap, dtype=torch.int16, device=dev),) if self._A else buf

    def _reserve(self, n, dev):
        """Capacity for n more records; grows by reallocation (between batches only)."""
        if self._buf is None:
            self._buf = self._alloc(max(self._cap0, n), dev)
            self._npos = torch.zeros((self._A, self.C) if self._A else self.C, dtype=torch.int32, device=dev)
        cap = self._buf[0].numel()
        if self._pos + n > cap:
            while self._pos + n > cap:
                cap *= 2
            new = self._alloc(cap, dev)
            for o, nw in zip(self._buf, new):
                nw[:self._pos].copy_(o[:self._pos])
            self._buf = new

    # ---- adding batches --------------------------------------------------------------------------------
    def add(self, boxes, scores, classes, valid, gt_boxes, gt_labels, gt_count, gt_flags=None, image_ids=None,
            gt_area=None, area_scale=None):
        """Device tensors, the form cvl_fcos_detect returns: boxes [B,T,4] (y1, x1, y2, x2), scores /
        classes [B,T] fp32, valid [B] int32; gt_boxes [B,G,4] fp32 pixel corners, gt_labels [B,G],
        gt_count [B], gt_flags [B,G] bytes (VOC difficult / COCO iscrowd).  image_ids [B] (ints in
        [0, 2^31); default: a running counter) make the result independent of the batching.  With
        area ranges: gt_area [B,G] fp32 replaces the ground truths' box areas (COCO's `area`), and
        area_scale [B] fp32 multiplies every box-derived area (original pixels^2 per network
        pixel^2).  One launch, no host synchronisation."""
        if (gt_area is not None or area_scale is not None) and not self._A:
            raise ValueError("gt_area / area_scale need an Evaluator with area_ranges")
        if boxes.dim() != 3 or boxes.shape[-1] != 4:
            raise ValueError("boxes must be [B, T, 4]")
        B, T = int(boxes.shape[0]), int(boxes.shape[1])
        if tuple(scores.shape) != (B, T) or tuple(classes.shape) != (B, T) or tuple(valid.shape) != (B,):
            raise ValueError("scores / classes must be [B, T] and valid [B] for boxes [B, T, 4]")
        if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[-1] != 4:
            raise ValueError("gt_boxes must be [B, G, 4]")
        G = int(gt_boxes.shape[1])
        if tuple(gt_labels.shape) != (B, G) or tuple(gt_count.shape) != (B,):
            raise ValueError("gt_labels must be [B, G] and gt_count [B] for gt_boxes [B, G, 4]")
        if gt_flags is not None and tuple(gt_flags.shape) != (B, G):
            raise ValueError("gt_flags must be [B, G]")
        if image_ids is not None and len(image_ids) != B:
            raise ValueError("image_ids must hold B ids")
        if gt_area is not None and tuple(gt_area.shape) != (B, G):
            raise ValueError("gt_area must be [B, G]")
        if area_scale is not None and tuple(area_scale.shape) != (B,):
            raise ValueError("area_scale must be [B]")
        if B < 1 or not 1 <= T <= MAX_T or G > MAX_G:
            raise ValueError("B >= 1, 1 <= T <= %d and G <= %d" % (MAX_T, MAX_G))
        _lib.require_cuda(boxes, scores, classes, valid, gt_boxes, gt_labels, gt_count, gt_flags, gt_area, area_scale)
        dev = boxes.device
        f32 = lambda t: t if t.dtype == torch.float32 else t.float()
        i32 = lambda t: t if t.dtype == torch.int32 else t.to(torch.int32)
        boxes, scores, classes, gt_boxes = f32(boxes), f32(scores), f32(classes), f32(gt_boxes)
        valid, gt_labels, gt_count = i32(valid), i32(gt_labels), i32(gt_count)
        if gt_flags is not None and gt_flags.dtype != torch.uint8:
            gt_flags = (gt_flags != 0).to(torch.uint8)
        if image_ids is None:
            ids = torch.arange(self._next_id, self._next_id + B, dtype=torch.int64, device=dev)
        else:
            ids = torch.as_tensor(image_ids, dtype=torch.int64).to(dev).contiguous()
        self._next_id += B
        self._reserve(B * T, dev)
        if self._A:
            gt_area = None if gt_area is None or not G else f32(gt_area)
            area_scale = None if area_scale is None else f32(area_scale)
            sc, cl, key, tp, ig, rk = self._buf
            _lib.call("cvl_eval_match_areas", _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(classes), _lib.ptr(valid),
                      _lib.ptr(gt_boxes) if G else None, _lib.ptr(gt_labels) if G else None,
                      _lib.ptr(gt_flags) if G else None, _lib.ptr(gt_count) if G else None, _lib.ptr(ids), B, T, G,
                      self.C, ctypes.cast(self._thr, ctypes.c_void_p), len(self.thresholds), self._match,
                      self.max_dets, ctypes.cast(self._rng, ctypes.c_void_p), self._A, _lib.ptr(gt_area),
                      _lib.ptr(area_scale), _lib.ptr(sc), _lib.ptr(cl), _lib.ptr(key), _lib.ptr(tp), _lib.ptr(ig),
                      _lib.ptr(rk), self._pos, _lib.ptr(self._npos), _lib.stream())
            self._pos += B * T
            return
        sc, cl, key, tp, ig = self._buf
        _lib.call("cvl_eval_match", _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(classes), _lib.ptr(valid),
                  _lib.ptr(gt_boxes) if G else None, _lib.ptr(gt_labels) if G else None,
                  _lib.ptr(gt_flags) if G else None, _lib.ptr(gt_count) if G else None, _lib.ptr(ids), B, T, G,
                  self.C, ctypes.cast(self._thr, ctypes.c_void_p), len(self.thresholds), self._match, self.max_dets,
                  _lib.ptr(sc), _lib.ptr(cl), _lib.ptr(key), _lib.ptr(tp), _lib.ptr(ig), self._pos,
                  _lib.ptr(self._npos), _lib.stream())
        self._pos += B * T

    def add_rows(self, rows_per_image, gts_per_image, fmt="yxyx", image_ids=None, area_scale=None):
        """rows_per_image: one [k, 6] array per image, (y1, x1, y2, x2, score, class) with
        fmt="yxyx" (RetinaNet.decode_detections) or (x1, y1, x2, y2, score, class) with fmt="xyxy"
        (the CenterNet decode_detections' NMS rows); gts_per_image: one [n, 5], [n, 6] or [n, 7] array
        per image, (y1, x1, y2, x2, class[, flag[, area]]) in pixels -- the area column (every image
        or none; with area ranges only) is add's gt_area, area_scale [B] its area_scale.  Row i is
        detection slot i."""
        if fmt not in ("yxyx", "xyxy"):
            raise ValueError("fmt must be 'yxyx' or 'xyxy', not %r" % (fmt,))
        if len(rows_per_image) != len(gts_per_image) or len(rows_per_image) < 1:
            raise ValueError("one row array and one ground-truth array per image")
        rows = [np.asarray(r, np.float32).reshape(-1, 6) for r in rows_per_image]
        gts = [np.asarray(g, np.float32) for g in gts_per_image]
        gts = [g.reshape(-1, g.shape[-1] if g.ndim == 2 and g.shape[-1] in (5, 6, 7) else 5) for g in gts]
        widths = set(g.shape[1] for g in gts if len(g))
        if 7 in widths and widths != {7}:
            raise ValueError("the area column must be given for every image or for none")
        if area_scale is not None and len(area_scale) != len(rows):
            raise ValueError("area_scale must hold one value per image")
        B = len(rows)
        T = max(1, max(len(r) for r in rows))
        G = max(len(g) for g in gts)
        det = np.zeros((B, T, 6), np.float32)
        gt = np.zeros((B, G, 7), np.float32)
        nv, ng = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            r = rows[b][:, [1, 0, 3, 2, 4, 5]] if fmt == "xyxy" else rows[b]
            det[b, :len(r)], nv[b] = r, len(r)
            gt[b, :len(gts[b]), :gts[b].shape[1]], ng[b] = gts[b], len(gts[b])
        _lib.require_cuda()
        d, g = torch.from_numpy(det).cuda(), torch.from_numpy(gt).cuda()
        self.add(d[..., :4].contiguous(), d[..., 4].contiguous(), d[..., 5].contiguous(),
                 torch.from_numpy(nv).cuda(), g[..., :4].contiguous(), g[..., 4].to(torch.int32).contiguous(),
                 torch.from_numpy(ng).cuda(), gt_flags=(g[..., 5] != 0).to(torch.uint8).contiguous(),
                 image_ids=image_ids, gt_area=g[..., 6].contiguous() if 7 in widths else None,
                 area_scale=None if area_scale is None else torch.tensor(area_scale, dtype=torch.float32).cuda())

    # ---- results ---------------------------------------------------------------------------------------
    def records(self):
        """The raw records (host copies; tests and debugging): dict of arrays over every slot added
        so far -- image_id, slot, class (num_classes = dropped), score, tp / ign bit sets; with area
        ranges tp / ign are [n, A] and rank (0xffff = dropped) is added."""
        if self._buf is None:
            z = np.zeros(0, np.int64)
            out = dict(image_id=z, slot=z, cls=z, score=np.zeros(0, np.float32), tp=z, ign=z)
            if self._A:
                out.update(tp=np.zeros((0, self._A), np.int64), ign=np.zeros((0, self._A), np.int64), rank=z)
            return out
        sc, cl, key, tp, ig = (t[:self._pos].cpu().numpy() for t in self._buf[:5])
        out = dict(image_id=key >> 32, slot=key & 0xffffffff, cls=cl.astype(np.int64), score=sc,
                   tp=tp.view(np.uint16).astype(np.int64), ign=ig.view(np.uint16).astype(np.int64))
        if self._A:
            out["rank"] = self._buf[5][:self._pos].cpu().numpy().view(np.uint16).astype(np.int64)
        return out

    def npos(self):
        """[C]; with area ranges [A, C]."""
        if self._buf is None:
            return np.zeros((self._A, self.C) if self._A else self.C, np.int64)
        return self._npos.cpu().numpy().astype(np.int64)

    def _sorted(self, n, dev):
        """The first n records' order by (class, score descending, key) -- three stable passes, least
        significant key first -- and where each class starts in it."""
        sc, cl, key = (t[:n] for t in self._buf[:3])
        order = torch.sort(key, stable=True).indices
        order = order[torch.sort(sc[order], descending=True, stable=True).indices]
        cls_sorted, idx = torch.sort(cl[order], stable=True)
        seg = torch.searchsorted(cls_sorted, torch.arange(self.C + 1, dtype=torch.int32, device=dev)).to(torch.int64)
        return order[idx], seg

    def _means(self, ap, tpf, npos):
        """mAP, and for coco AP50 / AP75 / AR, of one [K, C] table."""
        K = len(self.thresholds)
        cnt = npos > 0
        nan = float("nan")
        out = {"mAP": float(np.mean(ap[:, cnt])) if cnt.any() else nan}
        if self.protocol == "coco":
            for name, v in (("AP50", 0.5), ("AP75", 0.75)):
                ks = [k for k in range(K) if self.thresholds[k] == v]
                out[name] = float(np.mean(ap[ks[0], cnt])) if ks and cnt.any() else nan
            out["AR"] = float(np.mean(tpf[:, cnt] / npos[cnt])) if cnt.any() else nan
        return out

    def result(self):
        """dict: ap [K, C] float64 (NaN where a class has no unflagged ground truth), mAP (mean over
        thresholds and the classes counted), npos [C], thresholds; coco also AP50, AP75 and AR (the
        mean of the final tp / npos).  With area ranges, see _result_areas."""
        _lib.require_cuda()
        K, C, n = len(self.thresholds), self.C, self._pos
        if self._buf is None:
            self._reserve(0, torch.device("cuda"))
        dev = self._npos.device
        if self._A:
            return self._result_areas(K, C, n, dev)
        tp, ig = (t[:n] for t in self._buf[3:5])
        order, seg = self._sorted(n, dev)
        tp_s, ig_s = tp[order].contiguous(), ig[order].contiguous()
        ap = torch.empty((K, C), dtype=torch.float64, device=dev)
        tpf = torch.empty((K, C), dtype=torch.int32, device=dev)
        _lib.call("cvl_eval_ap", _lib.ptr(tp_s) if n else None, _lib.ptr(ig_s) if n else None, _lib.ptr(seg),
                  _lib.ptr(self._npos), n, C, K, self._mode, _lib.ptr(ap), _lib.ptr(tpf), _lib.stream())
        ap, tpf, npos = ap.cpu().numpy(), tpf.cpu().numpy().astype(np.int64), self.npos()
        out = {"ap": ap, "npos": npos, "thresholds": list(self.thresholds), "tp_total": tpf}
        out.update(self._means(ap, tpf, npos))
        return out

    def views(self):
        """The (area index, max_rank) views of one result(): every range at max_dets, then the
        first range at 1 and at 10 detections per (image, class)."""
        return [(a, self.max_dets) for a in range(self._A)] + [(0, 1), (0, 10)]

    def _result_areas(self, K, C, n, dev):
        """The same three sorts and one cvl_eval_ap_views launch over views().  ap / npos / tp_total /
        mAP / AP50 / AP75 / AR are the first range's at max_dets (range "all": bitwise what an
        evaluator without area ranges gives); ap_area / tp_total_area [A, K, C], npos_area [A, C],
        AP_area / AR_area [A] (the means, NaN-skipping as mAP / AR), area_names; AR1 / AR10 / AR100
        (the first range at 1 / 10 / max_dets); for ranges named small / medium / large APs / APm /
        APl and ARs / ARm / ARl, and with all three `summary`, the twelve numbers (SUMMARY_KEYS)."""
        A, views = self._A, self.views()
        R = len(views)
        tp, ig, rk = (t[:n] for t in self._buf[3:6])
        order, seg = self._sorted(n, dev)
        tp_s, ig_s, rk_s = tp[order].contiguous(), ig[order].contiguous(), rk[order].contiguous()
        ap = torch.empty((R, K, C), dtype=torch.float64, device=dev)
        tpf = torch.empty((R, K, C), dtype=torch.int32, device=dev)
        vw = (ctypes.c_int32 * (2 * R))(*[v for pair in views for v in pair])
        _lib.call("cvl_eval_ap_views", _lib.ptr(tp_s) if n else None, _lib.ptr(ig_s) if n else None,
                  _lib.ptr(rk_s) if n else None, _lib.ptr(seg), _lib.ptr(self._npos), n, C, K, A,
                  ctypes.cast(vw, ctypes.c_void_p), R, _lib.ptr(ap), _lib.ptr(tpf), _lib.stream())
        ap, tpf, npos = ap.cpu().numpy(), tpf.cpu().numpy().astype(np.int64), self.npos()
        names = [r[0] for r in self.area_ranges]
        out = {"ap": ap[0], "npos": npos[0], "thresholds": list(self.thresholds), "tp_total": tpf[0],
               "ap_area": ap[:A], "tp_total_area": tpf[:A], "npos_area": npos, "area_names": names}
        means = [self._means(ap[v], tpf[v], npos[a]) for v, (a, _) in enumerate(views)]
        out.update(means[0])
        out["AP_area"] = [m["mAP"] for m in means[:A]]
        out["AR_area"] = [m["AR"] for m in means[:A]]
        out["AR1"], out["AR10"], out["AR100"] = means[A]["AR"], means[A + 1]["AR"], means[0]["AR"]
        for name, letter in (("small", "s"), ("medium", "m"), ("large", "l")):
            if name in names:
                out["AP" + letter], out["AR" + letter] = means[names.index(name)]["mAP"], means[names.index(name)]["AR"]
        if all(k in out for k in SUMMARY_KEYS):
            out["summary"] = summary(out)
        return out

    def summary(self):
        """result()'s twelve COCO numbers in pycocotools' order: AP, AP50, AP75, APs, APm, APl, AR1,
        AR10, AR100, ARs, ARm, ARl (area_ranges="coco")."""
        return summary(self.result())

    # ---- merging ---------------------------------------------------------------------------------------
    def config(self):
        return dict(num_classes=self.C, protocol=self.protocol, thresholds=list(self.thresholds),
                    max_dets=self.max_dets,
                    area_ranges=None if self.area_ranges is None else [tuple(r) for r in self.area_ranges])

    def state(self):
        """Host dict: config, the records added so far (numpy arrays: score, cls, key, tp, ign and,
        with area ranges, rank) and npos.  Small, picklable: what merge_states / gather_states take."""
        names = ("score", "cls", "key", "tp", "ign", "rank")
        if self._buf is None:
            buf = self._alloc(0, torch.device("cpu"))
            npos = np.zeros((self._A, self.C) if self._A else self.C, np.int32)
        else:
            buf, npos = self._buf, self._npos.cpu().numpy()
        return dict(config=self.config(), records={k: t[:self._pos].cpu().numpy() for k, t in zip(names, buf)},
                    npos=npos, next_id=self._next_id)

    def load_state(self, state):
        """Replaces the evaluator's records by a state()'s (of an evaluator with the same config)."""
        if state["config"] != self.config():
            raise ValueError("the state's config differs from this evaluator's")
        _lib.require_cuda()
        rec = state["records"]
        n = len(rec["key"])
        self._buf = None
        self.reset()
        self._reserve(n, torch.device("cuda"))
        for t, k in zip(self._buf, ("score", "cls", "key", "tp", "ign", "rank")):
            t[:n].copy_(torch.from_numpy(np.ascontiguousarray(rec[k])))
        self._npos.copy_(torch.from_numpy(np.ascontiguousarray(state["npos"], dtype=np.int32)))
        self._pos, self._next_id = n, int(state.get("next_id", 0))
        return self

    @classmethod
    def from_state(cls, state):
        """The inverse of state()."""
        c = state["config"]
        ev = cls(c["num_classes"], c["protocol"], iou_thresholds=c["thresholds"], max_dets=c["max_dets"],
                 capacity=max(1, len(state["records"]["key"])), area_ranges=c["area_ranges"])
        return ev.load_state(state)


def merge_states(states):
    """Evaluator.state() dicts of evaluators that saw disjoint images -> one state: the records
    concatenated, npos added (pure host code).  The evaluation orders records by (class, score, image
    id << 32 | slot), so the merged result does not depend on the order of `states`.  Raises
    ValueError when the configs differ or two states hold the same image id."""
    states = list(states)
    if not states:
        raise ValueError("merge_states needs at least one state")
    cfg = states[0]["config"]
    seen = np.zeros(0, np.int64)
    for s in states:
        if s["config"] != cfg:
            raise ValueError("the states' configs differ: %r / %r" % (cfg, s["config"]))
        ids = np.unique(np.asarray(s["records"]["key"], np.int64) >> 32)
        both = np.intersect1d(seen, ids)
        if len(both):
            raise ValueError("image id %d is in two states" % int(both[0]))
        seen = np.concatenate([seen, ids])
    rec = {k: np.concatenate([s["records"][k] for s in states]) for k in states[0]["records"]}
    npos = states[0]["npos"].copy()
    for s in states[1:]:
        npos += s["npos"]
    return dict(config=cfg, records=rec, npos=npos, next_id=max(int(s.get("next_id", 0)) for s in states))


def gather_states(state, group=None):
    """All ranks of `group` (None: the default group) exchange their states
    (torch.distributed.all_gather_object: host objects, so gloo and RCCL alike) and every rank returns
    the merged state."""
    import torch.distributed as tdist
    out = [None] * tdist.get_world_size(group)
    tdist.all_gather_object(out, state, group=group)
    return merge_states(out)


def gt_from_labels(bx, nbox, img_dim):
    """The trainers' boxes bx [B, n, 5] = (yc, xc, h, w, class) normalised to img_dim [B, 2] (h, w; or
    one (h, w) pair) -> (gt_boxes [B, n, 4] fp32 pixel corners (y1, x1, y2, x2), gt_labels [B, n]
    int32, gt_count [B] int32), on bx's device (host arrays -> host tensors)."""
    bx = torch.as_tensor(bx, dtype=torch.float32)
    nb = torch.as_tensor(nbox).to(bx.device, torch.int32)
    dim = torch.as_tensor(img_dim, dtype=torch.float32).to(bx.device).reshape(-1, 1, 2).expand(bx.shape[0], 1, 2)
    half = bx[..., 2:4] / 2.0
    gt = torch.cat([(bx[..., 0:2] - half) * dim, (bx[..., 0:2] + half) * dim], -1)
    return gt.contiguous(), bx[..., 4].to(torch.int32).contiguous(), nb.contiguous()


# -------------------------------------------------------------------------------------------------------
# drivers over pre-processed samples of one padded size: the dict form train() accepts -- image
# [Hp, Wp, 3] in [-1, 1], bbox [N, 4] normalised (yc, xc, h, w), label [N], optional img_dim [h, w]
# -- plus optional per-sample arrays: `difficult` or `iscrowd` [N] (the ground-truth flag) and, read
# with area_ranges only, `area` [N] (COCO's area, original pixels^2: Evaluator.add's gt_area; every
# sample or none) and `orig_dim` [h, w] (the image's size before it was resized to img_dim: with
# img_dim it gives add's area_scale).
# Common keywords: area_ranges (Evaluator's); shard=(rank, world): score samples[rank::world] under
# their global indices as image ids; group: a torch.distributed group -- the ranks' states are
# gathered and merged before result(), so every rank returns the whole set's result;
# return_state=True: -> (result, state) for merging by hand (merge_states).
# -------------------------------------------------------------------------------------------------------
def _shard(samples, shard):
    if shard is None:
        return samples, 0, 1
    rank, world = int(shard[0]), int(shard[1])
    if not 0 <= rank < world:
        raise ValueError("shard must be (rank, world) with 0 <= rank < world, not %r" % (shard,))
    return samples[rank::world], rank, world


def _sample_batches(samples, batch_size, shard=None, areas=False):
    """-> per batch (images [bs, Hp, Wp, 3] host fp32, gt (boxes, labels, count, flags) host tensors,
    image ids, real count, area = dict(gt_area [bs, n] or None, area_scale [bs] or None; both None
    unless `areas`)); a partial last batch is padded with zero images and gt_count = 0.  Sample j of
    the shard (rank, world) has the id rank + world * j, the padding included, so the ids of
    different ranks never meet."""
    samples, rank, world = _shard(samples, shard)
    if not len(samples):
        return
    n_max = max(1, max(len(s["label"]) for s in samples))
    H, W = np.asarray(samples[0]["image"]).shape[:2]
    with_area = areas and samples[0].get("area") is not None
    with_scale = areas and any(s.get("orig_dim") is not None for s in samples)
    for i0 in range(0, len(samples), batch_size):
        chunk = samples[i0:i0 + batch_size]
        real = len(chunk)
        imgs = np.zeros((batch_size, H, W, 3), np.float32)
        bx = np.zeros((batch_size, n_max, 5), np.float32)
        nb = np.zeros(batch_size, np.int32)
        dims = np.tile(np.array([[H, W]], np.float32), (batch_size, 1))
        flags = np.zeros((batch_size, n_max), np.uint8)
        area = np.zeros((batch_size, n_max), np.float32) if with_area else None
        scale = np.ones(batch_size, np.float32) if with_scale else None
        for k, s in enumerate(chunk):
            n = len(s["label"])
            imgs[k] = np.asarray(s["image"], np.float32)
            bx[k, :n, :4] = np.asarray(s["bbox"], np.float32).reshape(n, 4)
            bx[k, :n, 4] = s["label"]
            nb[k] = n
            dims[k] = s.get("img_dim", (H, W))
            fl = s.get("difficult") if s.get("difficult") is not None else s.get("iscrowd")
            if fl is not None:
                flags[k, :n] = np.asarray(fl) != 0
            if with_area:
                area[k, :n] = np.asarray(s["area"], np.float32)
            if with_scale and s.get("orig_dim") is not None:
                oh, ow = (float(v) for v in s["orig_dim"])
                scale[k] = (oh * ow) / (float(dims[k, 0]) * float(dims[k, 1]))
        gtb, gtl, gtc = gt_from_labels(bx, nb, dims)
        extra = dict(gt_area=None if area is None else torch.from_numpy(area),
                     area_scale=None if scale is None else torch.from_numpy(scale))
        yield (imgs, (gtb, gtl, gtc, torch.from_numpy(flags)), [rank + world * j for j in range(i0, i0 + batch_size)],
               real, extra)


def _finish(ev, group, return_state):
    if group is not None:
        ev = Evaluator.from_state(gather_states(ev.state(), group))
    res = ev.result()
    return (res, ev.state()) if return_state else res


def _gt_rows(gt, real, gt_area=None):
    gtb, gtl, gtc, gtf = (t.numpy() for t in gt)
    cols = lambda b: [gtb[b, :gtc[b]], gtl[b, :gtc[b], None], gtf[b, :gtc[b], None]] + (
        [] if gt_area is None else [gt_area.numpy()[b, :gtc[b], None]])
    return [np.concatenate(cols(b), 1).astype(np.float32) for b in range(real)]


def _row_scale(extra, real):
    return None if extra["area_scale"] is None else extra["area_scale"].numpy()[:real]


def evaluate_fcos(model, samples, num_classes, batch_size=16, protocol="voc07", center=False, iou_thresholds=None,
                  max_dets=100, fold_bn=False, area_ranges=None, shard=None, group=None, return_state=False,
                  clamp_reg=False, **detect_kwargs):
    """FCOS (cvlite.fcos.build_model or its FCOSNet): infer_fcos.image_detections per batch, then
    Evaluator.add on its device outputs.  detect_kwargs: iou_thresh, cls_thresh, max_detections,
    max_total_size of image_detections.  fold_bn: the forwards run with the backbone's BatchNorms
    folded into its convs (folded once, before the first batch).  clamp_reg: image_detections' clamp of
    the box outputs at 0 (networks trained with the FCOS papers' recipe).  A network built with reg_max
    (Generalized Focal Loss) is decoded through its distributions, as image_detections does.  Returns
    Evaluator.result()."""
    from .infer_fcos import image_detections
    ev = Evaluator(num_classes, protocol, iou_thresholds=iou_thresholds, max_dets=max_dets, area_ranges=area_ranges)
    for imgs, gt, ids, real, extra in _sample_batches(samples, batch_size, shard, areas=area_ranges is not None):
        det = image_detections(torch.from_numpy(imgs).cuda(), model, num_classes, center=center, fold_bn=fold_bn,
                               clamp_reg=clamp_reg, **detect_kwargs)
        valid = det.valid_detections.clone()
        valid[real:] = 0
        gtb, gtl, gtc, gtf = (t.cuda() for t in gt)
        ev.add(det.nmsed_boxes, det.nmsed_scores, det.nmsed_classes, valid, gtb, gtl, gtc, gt_flags=gtf,
               image_ids=ids, **{k: v.cuda() for k, v in extra.items() if v is not None})
    return _finish(ev, group, return_state)


def evaluate_retinanet(retina, samples, num_classes=None, batch_size=16, protocol="coco", iou_thresholds=None,
                       max_dets=100, iou_thresh=0.5, cls_thresh=0.05, fold_bn=False, area_ranges=None, shard=None,
                       group=None, return_state=False):
    """RetinaNet (cvlite.retinanet.RetinaNet): inference forward per batch, decode_detections
    (decode + NMS on the device, rows to the host as that API returns them), Evaluator.add_rows.
    fold_bn: the forwards run with the backbone's BatchNorms folded into its convs."""
    C = retina.n_class if num_classes is None else int(num_classes)
    ev = Evaluator(C, protocol, iou_thresholds=iou_thresholds, max_dets=max_dets, area_ranges=area_ranges)
    net = retina.model
    for imgs, gt, ids, real, extra in _sample_batches(samples, batch_size, shard, areas=area_ranges is not None):
        x = torch.from_numpy(imgs).cuda()
        shapes, _, _ = net.layout(int(x.shape[0]), int(x.shape[1]), int(x.shape[2]))
        reg, cls = net.forward(x, train=False, folded=bool(fold_bn))
        rows = retina.decode_detections(reg, cls, shapes, iou_thresh=iou_thresh, cls_thresh=cls_thresh)
        # NMS emits its rows best score first: the slot limit keeps the MAX_T best of an image
        ev.add_rows([r[:MAX_T] for r in rows[:real]], _gt_rows(gt, real, extra["gt_area"]), fmt="yxyx",
                    image_ids=ids[:real], area_scale=_row_scale(extra, real))
    return _finish(ev, group, return_state)


def evaluate_centernet(model, samples, num_classes, batch_size=16, protocol="voc07", iou_thresholds=None,
                       max_dets=100, area_ranges=None, shard=None, group=None, return_state=False, decode="nms",
                       K=100, **decode_kwargs):
    """The separable-hourglass CenterNet (cvlite.centernet_hourglass.build_model): inference forward
    per batch, then Evaluator.add_rows on rows (x1, y1, x2, y2, score, class).  decode="nms" (default):
    centernet_hourglass.decode_detections per image (the reference's threshold + NMS); decode_kwargs:
    thresh, iou_thresh, downsample (default: the model's stride).  decode="peak": one batched
    centernet_hourglass.peak_detections call per batch (3x3 max-pool peaks, the K best per image, no
    per-image host synchronisation) -- the decode that heat maps trained with targets="gaussian" are
    made for; decode_kwargs: thresh, downsample."""
    from .centernet_hourglass import decode_detections, peak_detections
    if decode not in ("nms", "peak"):
        raise ValueError("decode must be 'nms' or 'peak', not %r" % (decode,))
    ev = Evaluator(num_classes, protocol, iou_thresholds=iou_thresholds, max_dets=max_dets, area_ranges=area_ranges)
    for imgs, gt, ids, real, extra in _sample_batches(samples, batch_size, shard, areas=area_ranges is not None):
        H, W = imgs.shape[1:3]
        pred = model(torch.from_numpy(imgs).cuda(), training=False)
        kw = dict(decode_kwargs)
        kw.setdefault("downsample", H // int(pred.shape[1]))
        if decode == "peak":
            dets = peak_detections(pred, K=int(K), num_classes=num_classes, **kw)
            rows = [d[:MAX_T][:, [1, 0, 3, 2, 4, 5]] for d in dets[:real]]
        else:
            rows = [decode_detections(pred[b], img_rows=H, img_cols=W, **kw)[1][:MAX_T] for b in range(real)]
        ev.add_rows(rows, _gt_rows(gt, real, extra["gt_area"]), fmt="xyxy", image_ids=ids[:real],
                    area_scale=_row_scale(extra, real))
    return _finish(ev, group, return_state)


def evaluate_hourglass_v2(model, samples, num_classes, batch_size=16, protocol="voc07", iou_thresholds=None,
                          max_dets=100, area_ranges=None, shard=None, group=None, return_state=False,
                          **decode_kwargs):
    """The v2 hourglass CenterNet (cvlite.tf_hourglass_net.build_model; padded sizes are multiples of
    64): inference forward per batch, tf_hourglass_net.decode_detections per image -- rows (lower
    corner along the row axis, along the column axis, extent along rows, along columns, int(100 p),
    class) of every cell over the threshold; that decode has no NMS -- best score first, the MAX_T
    best kept, Evaluator.add_rows.  decode_kwargs: thresh, img_scale of decode_detections."""
    from .tf_hourglass_net import decode_detections
    ev = Evaluator(num_classes, protocol, iou_thresholds=iou_thresholds, max_dets=max_dets, area_ranges=area_ranges)
    for imgs, gt, ids, real, extra in _sample_batches(samples, batch_size, shard, areas=area_ranges is not None):
        H, W = imgs.shape[1:3]
        pred = model(torch.from_numpy(imgs).cuda(), training=False)
        rows = []
        for b in range(real):
            r = np.asarray(decode_detections(pred[b], img_rows=H, img_cols=W, **decode_kwargs), np.float64)
            r = r.reshape(-1, 6)
            r = r[np.argsort(-r[:, 4], kind="stable")][:MAX_T]
            rows.append(np.stack([r[:, 0], r[:, 1], r[:, 0] + r[:, 2], r[:, 1] + r[:, 3], r[:, 4], r[:, 5]], 1))
        ev.add_rows(rows, _gt_rows(gt, real, extra["gt_area"]), fmt="yxyx", image_ids=ids[:real],
                    area_scale=_row_scale(extra, real))
    return _finish(ev, group, return_state)


def evaluate_centernet_s8(model, samples, num_classes, box_scales, batch_size=16, protocol="voc07",
                          iou_thresholds=None, max_dets=100, area_ranges=None, shard=None, group=None,
                          return_state=False, **decode_kwargs):
    """The stride-8 multi-scale CenterNet (cvlite.tf_centernet_resnet_s8.build_model; box_scales: its
    per-scale box sizes, as in training): inference forward per batch,
    tf_centernet_resnet_s8.decode_detections per image (threshold + NMS; rows (x1, y1, x2, y2, score,
    class)), Evaluator.add_rows.  decode_kwargs: thresh, iou_thresh, downsample of decode_detections."""
    from .tf_centernet_resnet_s8 import decode_detections
    ev = Evaluator(num_classes, protocol, iou_thresholds=iou_thresholds, max_dets=max_dets, area_ranges=area_ranges)
    for imgs, gt, ids, real, extra in _sample_batches(samples, batch_size, shard, areas=area_ranges is not None):
        H, W = imgs.shape[1:3]
        pred = model(torch.from_numpy(imgs).cuda(), training=False)
        rows = [decode_detections(pred[b], box_scales, img_rows=H, img_cols=W, **decode_kwargs)[1][:MAX_T]
                for b in range(real)]
        ev.add_rows(rows, _gt_rows(gt, real, extra["gt_area"]), fmt="xyxy", image_ids=ids[:real],
                    area_scale=_row_scale(extra, real))
    return _finish(ev, group, return_state)
