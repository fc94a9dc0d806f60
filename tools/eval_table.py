"""Times the device-resident evaluator (cvlite.evaluate.Evaluator: cvl_eval_match per batch,
torch.sort + cvl_eval_ap in result()) on a synthetic COCO-sized validation set -- --images 5000
images, 100 detections each, 80 classes, about 7 ground truths per image -- next to what it sits
beside in an evaluation pass and what it replaces:
  (a) Evaluator.add per batch of 16 (inputs staged on the device beforehand; HIP events around the
      whole sequence of adds of one pass, divided by the batches: launch gaps included);
  (b) Evaluator.result() (host clock; it ends in the device-to-host copy of ap, a synchronise);
  (c) the numpy restatement tests/eval_ref.evaluate on the same data (host clock, run once);
  (d) one FCOS R50-FPN inference forward + cvl_fcos_detect at 512 x 512, batch 16 (HIP events).
Records the ratios (a) / (d) and ((a) x batches + (b)) / (c); there is no threshold.  (a), (b), (d):
warm-up passes first, then the median of --reps timed passes.  The device result is also compared
with the restatement's (max |ap - ref|), so the times are of code that computes the same thing.
--area-ranges coco also times an Evaluator(area_ranges="coco") (cvl_eval_match_areas per batch,
cvl_eval_ap_views in result(): the small / medium / large ranges and AR@1 / 10 / 100) on the same
batches, its passes alternating with the unranged evaluator's, and compares all its views with
tests/eval_area_ref.evaluate: rows (a'), (b'), (c').
usage: eval_table.py [--images 5000] [--reps 5] [--protocol coco] [--area-ranges coco] [--out profiles/eval_table.md]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

T, C, G, BS = 100, 80, 16, 16


def synthetic(n_img, seed=0):
    """[n_img] arrays: ground truths 1 + Poisson(6) per image (<= G, ~7 % crowd), detections = jittered
    copies of ground truths (70 %) or random boxes, scores U(0, 1) rounded to 1/1024 (ties occur)."""
    rng = np.random.default_rng(seed)
    ng = np.minimum(1 + rng.poisson(6.0, n_img), G).astype(np.int32)
    yx = rng.uniform(0, 400, (n_img, G, 2))
    hw = np.exp(rng.uniform(np.log(16), np.log(200), (n_img, G, 2)))
    gtb = np.concatenate([yx, yx + hw], -1).astype(np.float32)
    gtl = rng.integers(0, C, (n_img, G)).astype(np.int32)
    gtf = (rng.random((n_img, G)) < 0.07).astype(np.uint8)
    src = (rng.random((n_img, T)) * ng[:, None]).astype(np.int64)
    ii = np.arange(n_img)[:, None]
    from_gt = rng.random((n_img, T)) < 0.7
    jit = gtb[ii, src] + rng.normal(0, 6.0, (n_img, T, 4))
    ryx = rng.uniform(0, 400, (n_img, T, 2))
    rnd = np.concatenate([ryx, ryx + np.exp(rng.uniform(np.log(16), np.log(200), (n_img, T, 2)))], -1)
    boxes = np.where(from_gt[..., None], jit, rnd).astype(np.float32)
    cls = np.where(from_gt & (rng.random((n_img, T)) < 0.9), gtl[ii, src], rng.integers(0, C, (n_img, T)))
    scores = (np.round(rng.random((n_img, T)) * 1024) / 1024).astype(np.float32)
    valid = np.full(n_img, T, np.int32)
    return boxes, scores, cls.astype(np.float32), valid, gtb, gtl, gtf, ng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--protocol", default="coco")
    ap.add_argument("--area-ranges", default=None, choices=["coco"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_table.py times GPU work: it needs the GPU")
    import eval_ref
    from cvlite import fcos
    from cvlite.evaluate import Evaluator
    from cvlite.infer_fcos import image_detections

    data = synthetic(args.images)
    n = args.images
    batches = []
    for i0 in range(0, n, BS):
        sl = slice(i0, min(n, i0 + BS))
        b, s, c, v, gb, gl, gf, gc = (torch.from_numpy(np.ascontiguousarray(a[sl])).cuda() for a in data)
        batches.append((b, s, c, v, gb, gl, gc, gf, torch.arange(sl.start, sl.stop, dtype=torch.int64, device="cuda")))
    evs = [Evaluator(C, args.protocol, capacity=n * T)]
    if args.area_ranges:
        evs.append(Evaluator(C, args.protocol, capacity=n * T, area_ranges=args.area_ranges))

    def one_pass(ev):
        ev.reset()
        for b, s, c, v, gb, gl, gc, gf, ids in batches:
            ev.add(b, s, c, v, gb, gl, gc, gt_flags=gf, image_ids=ids)

    for _ in range(2):
        for ev in evs:
            one_pass(ev)
            ev.result()
    t_add, t_res, results = [[] for _ in evs], [[] for _ in evs], [None] * len(evs)
    for _ in range(args.reps):
        for i, ev in enumerate(evs):                 # the configurations alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            one_pass(ev)
            e1.record()
            torch.cuda.synchronize()
            t_add[i].append(e0.elapsed_time(e1) / len(batches))
            h0 = time.perf_counter()
            results[i] = ev.result()
            t_res[i].append((time.perf_counter() - h0) * 1e3)
    a_ms, b_ms, res = statistics.median(t_add[0]), statistics.median(t_res[0]), results[0]

    images = [dict(id=i, boxes=data[0][i], scores=data[1][i], classes=data[2][i], valid=int(data[3][i]),
                   gt_boxes=data[4][i], gt_labels=data[5][i], gt_flags=data[6][i], gt_count=int(data[7][i]))
              for i in range(n)]
    h0 = time.perf_counter()
    ref = eval_ref.evaluate(images, C, args.protocol)
    c_ms = (time.perf_counter() - h0) * 1e3
    err = float(np.nanmax(np.abs(res["ap"] - ref["ap"])))
    if args.area_ranges:
        import eval_area_ref
        a2_ms, b2_ms, res2 = statistics.median(t_add[1]), statistics.median(t_res[1]), results[1]
        h0 = time.perf_counter()
        ref2 = eval_area_ref.evaluate(images, C)
        c2_ms = (time.perf_counter() - h0) * 1e3
        err2 = float(np.nanmax(np.abs(res2["ap_area"] - ref2["ap"][:4])))
        err_s = max(abs(g - r) for g, r in zip(res2["summary"], ref2["summary"]) if r == r)
        same = res2["ap"].tobytes() == res["ap"].tobytes()

    model = fcos.build_model(20)
    x = (torch.rand((BS, 512, 512, 3)) * 2 - 1).cuda()
    for _ in range(3):
        image_detections(x, model, 20)
    t_det = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(5):
            image_detections(x, model, 20)
        e1.record()
        torch.cuda.synchronize()
        t_det.append(e0.elapsed_time(e1) / 5)
    d_ms = statistics.median(t_det)

    total = a_ms * len(batches) + b_ms
    lines = [
        "Device-resident evaluation on a synthetic validation set: %d images x %d detections, %d classes, %.1f ground "
        "truths per image, protocol %s, %s; median of %d passes." % (
            n, T, C, float(data[7].mean()), args.protocol, torch.cuda.get_device_name(0), args.reps),
        "Command: `python tools/eval_table.py --images %d --reps %d --protocol %s%s`" % (
            n, args.reps, args.protocol, " --area-ranges coco" if args.area_ranges else ""), "",
        "| | what | time |", "|---|---|---|",
        "| (a) | Evaluator.add, per batch of %d (%d batches per pass; HIP events, launch gaps included) | %.3f ms |" % (
            BS, len(batches), a_ms),
        "| (b) | Evaluator.result() (3 stable sorts + cvl_eval_ap + copy to host; host clock) | %.2f ms |" % b_ms,
        "| (c) | numpy restatement tests/eval_ref.evaluate, same data (host clock, one run) | %.0f ms |" % c_ms,
        "| (d) | FCOS R50-FPN inference forward + cvl_fcos_detect, 512 x 512, batch %d (HIP events) | %.2f ms |" % (
            BS, d_ms),
        "", "(a) / (d) = %.4f" % (a_ms / d_ms),
        "((a) x batches + (b)) / (c) = %.5f  (%.1f ms against %.0f ms)" % (total / c_ms, total, c_ms),
        "mAP %.6f; max |ap - restatement| = %.3g over the %d x %d table." % (res["mAP"], err, len(res["thresholds"]), C)]
    if args.area_ranges:
        total2 = a2_ms * len(batches) + b2_ms
        lines += [
            "", "With `--area-ranges coco` (Evaluator(area_ranges=\"coco\"): four ranges, six views), same batches, passes "
            "alternating with the unranged evaluator's:", "", "| | what | time |", "|---|---|---|",
            "| (a') | Evaluator.add (cvl_eval_match_areas), per batch of %d | %.3f ms |" % (BS, a2_ms),
            "| (b') | Evaluator.result() (3 stable sorts + cvl_eval_ap_views + copy to host; host clock) | %.2f ms |" % b2_ms,
            "| (c') | numpy restatement tests/eval_area_ref.evaluate, same data (host clock, one run) | %.0f ms |" % c2_ms,
            "", "(a') / (a) = %.2f; (a') / (d) = %.4f" % (a2_ms / a_ms, a2_ms / d_ms),
            "((a') x batches + (b')) / (c') = %.5f  (%.1f ms against %.0f ms)" % (total2 / c2_ms, total2, c2_ms),
            "max |ap_area - restatement| = %.3g over the 4 x %d x %d table; max |summary - restatement| = %.3g; "
            "ap of range \"all\" bitwise equal to the unranged evaluator's: %s." % (
                err2, len(res2["thresholds"]), C, err_s, same),
            "summary (AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl): " +
            " ".join("%.4f" % v for v in res2["summary"])]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
