"""Detection evaluation on MI355X: VOC AP (07 11-point, 12 all-point) and COCO-style mAP.

The reference publishes no accuracy and has no evaluator; this is the project's own,
behind include/cvlite.h "Detection evaluation" (csrc/det_eval.hip) -- the contract and its
deviations from the VOC devkit / pycocotools are in INTEGRATION.md "Evaluation":

  Evaluator(num_classes, protocol)      device-resident state: one record per detection slot
    .add(...)                           one cvl_eval_match launch per batch, no host sync
    .add_rows(...)                      the [k, 6] row lists of the RetinaNet / CenterNet decodes
    .result()                           two-key stable sort (plumbing: torch.sort) + cvl_eval_ap
  gt_from_labels(bx, nbox, img_dim)     the trainers' normalised (yc, xc, h, w, cls) -> pixel corners
  evaluate_fcos / evaluate_retinanet / evaluate_centernet
                                        inference forward in batches + the family's decode + add

There is no CPU fallback: the hot path is the two HIP kernels.
"""
import ctypes

import numpy as np
import torch

from . import _lib

PROTOCOLS = {"voc07": (0, 0), "voc12": (0, 1), "coco": (1, 2)}      # -> (matching protocol, AP mode)
MAX_THRESHOLDS, MAX_T, MAX_G, MAX_CLASSES = 16, 1024, 1024, 65535   # include/cvlite.h CVL_EVAL_MAX_*


def default_thresholds(protocol):
    """The doubles nearest to the decimals: 0.5 (VOC), 0.50:0.05:0.95 (COCO)."""
    return [(50 + 5 * k) / 100.0 for k in range(10)] if protocol == "coco" else [0.5]


class Evaluator(object):
    def __init__(self, num_classes, protocol="voc07", iou_thresholds=None, max_dets=100, capacity=1 << 16):
        if protocol not in PROTOCOLS:
            raise ValueError("protocol must be 'voc07', 'voc12' or 'coco', not %r" % (protocol,))
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
        return (torch.empty(cap, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int16, device=dev),
                torch.empty(cap, dtype=torch.int16, device=dev))

    def _reserve(self, n, dev):
        """Capacity for n more records; grows by reallocation (between batches only)."""
        if self._buf is None:
            self._buf = self._alloc(max(self._cap0, n), dev)
            self._npos = torch.zeros(self.C, dtype=torch.int32, device=dev)
        cap = self._buf[0].numel()
        if self._pos + n > cap:
            while self._pos + n > cap:
                cap *= 2
            new = self._alloc(cap, dev)
            for o, nw in zip(self._buf, new):
                nw[:self._pos].copy_(o[:self._pos])
            self._buf = new

    # ---- adding batches --------------------------------------------------------------------------------
    def add(self, boxes, scores, classes, valid, gt_boxes, gt_labels, gt_count, gt_flags=None, image_ids=None):
        """Device tensors, the form cvl_fcos_detect returns: boxes [B,T,4] (y1, x1, y2, x2), scores /
        classes [B,T] fp32, valid [B] int32; gt_boxes [B,G,4] fp32 pixel corners, gt_labels [B,G],
        gt_count [B], gt_flags [B,G] bytes (VOC difficult / COCO iscrowd).  image_ids [B] (ints in
        [0, 2^31); default: a running counter) make the result independent of the batching.  One
        launch, no host synchronisation."""
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
        if B < 1 or not 1 <= T <= MAX_T or G > MAX_G:
            raise ValueError("B >= 1, 1 <= T <= %d and G <= %d" % (MAX_T, MAX_G))
        _lib.require_cuda(boxes, scores, classes, valid, gt_boxes, gt_labels, gt_count, gt_flags)
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
        sc, cl, key, tp, ig = self._buf
        _lib.call("cvl_eval_match", _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(classes), _lib.ptr(valid),
                  _lib.ptr(gt_boxes) if G else None, _lib.ptr(gt_labels) if G else None,
                  _lib.ptr(gt_flags) if G else None, _lib.ptr(gt_count) if G else None, _lib.ptr(ids), B, T, G,
                  self.C, ctypes.cast(self._thr, ctypes.c_void_p), len(self.thresholds), self._match, self.max_dets,
                  _lib.ptr(sc), _lib.ptr(cl), _lib.ptr(key), _lib.ptr(tp), _lib.ptr(ig), self._pos,
                  _lib.ptr(self._npos), _lib.stream())
        self._pos += B * T

    def add_rows(self, rows_per_image, gts_per_image, fmt="yxyx", image_ids=None):
        """rows_per_image: one [k, 6] array per image, (y1, x1, y2, x2, score, class) with
        fmt="yxyx" (RetinaNet.decode_detections) or (x1, y1, x2, y2, score, class) with fmt="xyxy"
        (the CenterNet decode_detections' NMS rows); gts_per_image: one [n, 5] or [n, 6] array per
        image, (y1, x1, y2, x2, class[, flag]) in pixels.  Row i is detection slot i."""
        if fmt not in ("yxyx", "xyxy"):
            raise ValueError("fmt must be 'yxyx' or 'xyxy', not %r" % (fmt,))
        if len(rows_per_image) != len(gts_per_image) or len(rows_per_image) < 1:
            raise ValueError("one row array and one ground-truth array per image")
        rows = [np.asarray(r, np.float32).reshape(-1, 6) for r in rows_per_image]
        gts = [np.asarray(g, np.float32) for g in gts_per_image]
        gts = [g.reshape(-1, g.shape[-1] if g.ndim == 2 and g.shape[-1] in (5, 6) else 5) for g in gts]
        B = len(rows)
        T = max(1, max(len(r) for r in rows))
        G = max(len(g) for g in gts)
        det = np.zeros((B, T, 6), np.float32)
        gt = np.zeros((B, G, 6), np.float32)
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
                 image_ids=image_ids)

    # ---- results ---------------------------------------------------------------------------------------
    def records(self):
        """The raw records (host copies; tests and debugging): dict of arrays over every slot added
        so far -- image_id, slot, class (num_classes = dropped), score, tp / ign bit sets."""
        if self._buf is None:
            z = np.zeros(0, np.int64)
            return dict(image_id=z, slot=z, cls=z, score=np.zeros(0, np.float32), tp=z, ign=z)
        sc, cl, key, tp, ig = (t[:self._pos].cpu().numpy() for t in self._buf)
        return dict(image_id=key >> 32, slot=key & 0xffffffff, cls=cl.astype(np.int64), score=sc,
                    tp=tp.view(np.uint16).astype(np.int64), ign=ig.view(np.uint16).astype(np.int64))

    def npos(self):
        return np.zeros(self.C, np.int64) if self._buf is None else self._npos.cpu().numpy().astype(np.int64)

    def result(self):
        """dict: ap [K, C] float64 (NaN where a class has no unflagged ground truth), mAP (mean over
        thresholds and the classes counted), npos [C], thresholds; coco also AP50, AP75 and AR (the
        mean of the final tp / npos)."""
        _lib.require_cuda()
        K, C, n = len(self.thresholds), self.C, self._pos
        if self._buf is None:
            self._reserve(0, torch.device("cuda"))
        dev = self._npos.device
        sc, cl, key, tp, ig = (t[:n] for t in self._buf)
        # (class, score descending, key): three stable passes, least significant key first
        order = torch.sort(key, stable=True).indices
        order = order[torch.sort(sc[order], descending=True, stable=True).indices]
        cls_sorted, idx = torch.sort(cl[order], stable=True)
        order = order[idx]
        tp_s, ig_s = tp[order].contiguous(), ig[order].contiguous()
        seg = torch.searchsorted(cls_sorted, torch.arange(C + 1, dtype=torch.int32, device=dev)).to(torch.int64)
        ap = torch.empty((K, C), dtype=torch.float64, device=dev)
        tpf = torch.empty((K, C), dtype=torch.int32, device=dev)
        _lib.call("cvl_eval_ap", _lib.ptr(tp_s) if n else None, _lib.ptr(ig_s) if n else None, _lib.ptr(seg),
                  _lib.ptr(self._npos), n, C, K, self._mode, _lib.ptr(ap), _lib.ptr(tpf), _lib.stream())
        ap, tpf, npos = ap.cpu().numpy(), tpf.cpu().numpy().astype(np.int64), self.npos()
        cnt = npos > 0
        nan = float("nan")
        out = {"ap": ap, "npos": npos, "thresholds": list(self.thresholds), "tp_total": tpf,
               "mAP": float(np.mean(ap[:, cnt])) if cnt.any() else nan}
        if self.protocol == "coco":
            for name, v in (("AP50", 0.5), ("AP75", 0.75)):
                ks = [k for k in range(K) if self.thresholds[k] == v]
                out[name] = float(np.mean(ap[ks[0], cnt])) if ks and cnt.any() else nan
            out["AR"] = float(np.mean(tpf[:, cnt] / npos[cnt])) if cnt.any() else nan
        return out


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
# -- plus an optional `difficult` [N] array (the ground-truth flag)
# -------------------------------------------------------------------------------------------------------
def _sample_batches(samples, batch_size):
    """-> per batch (images [bs, Hp, Wp, 3] host fp32, gt (boxes, labels, count, flags) host tensors,
    image ids, real count); a partial last batch is padded with zero images and gt_count = 0."""
    n_max = max(1, max(len(s["label"]) for s in samples))
    H, W = np.asarray(samples[0]["image"]).shape[:2]
    for i0 in range(0, len(samples), batch_size):
        chunk = samples[i0:i0 + batch_size]
        real = len(chunk)
        imgs = np.zeros((batch_size, H, W, 3), np.float32)
        bx = np.zeros((batch_size, n_max, 5), np.float32)
        nb = np.zeros(batch_size, np.int32)
        dims = np.tile(np.array([[H, W]], np.float32), (batch_size, 1))
        flags = np.zeros((batch_size, n_max), np.uint8)
        for k, s in enumerate(chunk):
            n = len(s["label"])
            imgs[k] = np.asarray(s["image"], np.float32)
            bx[k, :n, :4] = np.asarray(s["bbox"], np.float32).reshape(n, 4)
            bx[k, :n, 4] = s["label"]
            nb[k] = n
            dims[k] = s.get("img_dim", (H, W))
            if s.get("difficult") is not None:
                flags[k, :n] = np.asarray(s["difficult"]) != 0
        gtb, gtl, gtc = gt_from_labels(bx, nb, dims)
        yield imgs, (gtb, gtl, gtc, torch.from_numpy(flags)), list(range(i0, i0 + batch_size)), real


def evaluate_fcos(model, samples, num_classes, batch_size=16, protocol="voc07", center=False, iou_thresholds=None,
                  max_dets=100, fold_bn=False, **detect_kwargs):
    """FCOS (cvlite.fcos.build_model or its FCOSNet): infer_fcos.image_detections per batch, then
    Evaluator.add on its device outputs.  detect_kwargs: iou_thresh, cls_thresh, max_detections,
    max_total_size of image_detections.  fold_bn: the forwards run with the backbone's BatchNorms
    folded into its convs (folded once, before the first batch).  Returns Evaluator.result()."""
    from .infer_fcos import image_detections
    ev = Evaluator(num_classes, protocol, iou_thresholds=iou_thresholds, max_dets=max_dets)
    for imgs, gt, ids, real in _sample_batches(samples, batch_size):
        det = image_detections(torch.from_numpy(imgs).cuda(), model, num_classes, center=center, fold_bn=fold_bn,
                               **detect_kwargs)
        valid = det.valid_detections.clone()
        valid[real:] = 0
        gtb, gtl, gtc, gtf = (t.cuda() for t in gt)
        ev.add(det.nmsed_boxes, det.nmsed_scores, det.nmsed_classes, valid, gtb, gtl, gtc, gt_flags=gtf,
               image_ids=ids)
    return ev.result()


def _gt_rows(gt, real):
    gtb, gtl, gtc, gtf = (t.numpy() for t in gt)
    return [np.concatenate([gtb[b, :gtc[b]], gtl[b, :gtc[b], None], gtf[b, :gtc[b], None]], 1).astype(np.float32)
            for b in range(real)]


def evaluate_retinanet(retina, samples, num_classes=None, batch_size=16, protocol="coco", iou_thresholds=None,
                       max_dets=100, iou_thresh=0.5, cls_thresh=0.05, fold_bn=False):
    """RetinaNet (cvlite.retinanet.RetinaNet): inference forward per batch, decode_detections
    (decode + NMS on the device, rows to the host as that API returns them), Evaluator.add_rows.
    fold_bn: the forwards run with the backbone's BatchNorms folded into its convs."""
    C = retina.n_class if num_classes is None else int(num_classes)
    ev = Evaluator(C, protocol, iou_thresholds=iou_thresholds, max_dets=max_dets)
    net = retina.model
    for imgs, gt, ids, real in _sample_batches(samples, batch_size):
        x = torch.from_numpy(imgs).cuda()
        shapes, _, _ = net.layout(int(x.shape[0]), int(x.shape[1]), int(x.shape[2]))
        reg, cls = net.forward(x, train=False, folded=bool(fold_bn))
        rows = retina.decode_detections(reg, cls, shapes, iou_thresh=iou_thresh, cls_thresh=cls_thresh)
        # NMS emits its rows best score first: the slot limit keeps the MAX_T best of an image
        ev.add_rows([r[:MAX_T] for r in rows[:real]], _gt_rows(gt, real), fmt="yxyx", image_ids=ids[:real])
    return ev.result()


def evaluate_centernet(model, samples, num_classes, batch_size=16, protocol="voc07", iou_thresholds=None,
                       max_dets=100, **decode_kwargs):
    """The separable-hourglass CenterNet (cvlite.centernet_hourglass.build_model): inference forward
    per batch, centernet_hourglass.decode_detections per image (threshold + NMS; rows (x1, y1, x2,
    y2, score, class)), Evaluator.add_rows.  decode_kwargs: thresh, iou_thresh, downsample (default:
    the model's stride) of decode_detections."""
    from .centernet_hourglass import decode_detections
    ev = Evaluator(num_classes, protocol, iou_thresholds=iou_thresholds, max_dets=max_dets)
    for imgs, gt, ids, real in _sample_batches(samples, batch_size):
        H, W = imgs.shape[1:3]
        pred = model(torch.from_numpy(imgs).cuda(), training=False)
        kw = dict(decode_kwargs)
        kw.setdefault("downsample", H // int(pred.shape[1]))
        rows = [decode_detections(pred[b], img_rows=H, img_cols=W, **kw)[1][:MAX_T] for b in range(real)]
        ev.add_rows(rows, _gt_rows(gt, real), fmt="xyxy", image_ids=ids[:real])
    return ev.result()
