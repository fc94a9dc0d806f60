"""Times the task-aligned assignment, its loss and the whole targets="tal" training step at 512 x 512,
batch 16, C = 20, in one process, by the method of tools/fcos_gfl_table.py (HIP events around a HIP graph
of --iters calls, median of --reps passes after --warmup passes):
  kernels   cvl_fcos_tal_assign at 1 + Poisson(1.4) boxes per image (the synthetic training batch) and at
            32 boxes per image, on head outputs that overlap the boxes (the distances to one of the image's
            boxes per cell, jittered; class logits N(-2, 2)), beside cvl_fcos_atss_assign on the same boxes;
            cvl_fcos_tal_loss beside cvl_fcos_paper_loss and cvl_fcos_target_norm on the same targets (bf16
            gradient rows as the trainer passes them), with the bytes each loss call has to move
  step      the whole FCOSTrainer step (two graph replays) for targets="tal" and targets="atss", each as
            median and min .. max over the passes (the run-to-run spread)
With CVL_LIB pointing at a build of the parent revision (tools/build_base.sh) the task-aligned rows are
left out and the others are the parent's figures on the same box.
usage: fcos_tal_table.py [--size 512] [--batch 16] [--iters 20] [--reps 7] [--out FILE] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fcos_atss_table import passes  # noqa: E402
from fcos_paper_table import graphed  # noqa: E402


def dense_boxes(B, n, D, C, seed):
    """n boxes per image, log-uniform sides in [12, D] px, as synthetic_batch draws them."""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((B, n, 5), np.float32)
    for b in range(B):
        for k in range(n):
            h, w = np.exp(rng.uniform(np.log(12.0), np.log(D), 2))
            boxes[b, k] = [rng.uniform(h / 2, D - h / 2) / D, rng.uniform(w / 2, D - w / 2) / D, h / D, w / D,
                           rng.integers(0, C)]
    return torch.from_numpy(boxes).cuda(), torch.full((B,), n, dtype=torch.int32, device="cuda")


def head_outputs(boxes, nbox, D, C, seed):
    """reg [B,P,8] and cls [B,P,32] fp32: per cell the distances (stride units) to one of its image's boxes,
    times exp(N(0, 0.35)) plus N(0, 0.5); class logits N(-2, 2)."""
    from cvlite.ops_targets import FCOS_STRIDES, fcos_level_shapes
    rng = np.random.default_rng(seed)
    gy, gx, sf = [], [], []
    for (Hs, Ws), s in zip(fcos_level_shapes(D, D), FCOS_STRIDES):
        y, x = (np.arange(Hs) + 0.5) * s, (np.arange(Ws) + 0.5) * s
        gy.append(np.repeat(y, Ws))
        gx.append(np.tile(x, Hs))
        sf.append(np.full(Hs * Ws, float(s)))
    gy, gx, sf = np.concatenate(gy), np.concatenate(gx), np.concatenate(sf)
    P = gy.size
    bx, nb = boxes.cpu().numpy().astype(np.float64) * D, nbox.cpu().numpy()
    B = bx.shape[0]
    reg = np.zeros((B, P, 8), np.float32)
    cls = np.zeros((B, P, 32), np.float32)
    for b in range(B):
        r = bx[b, rng.integers(0, max(int(nb[b]), 1), P)]
        true = np.stack([gy - (r[:, 0] - r[:, 2] / 2), (r[:, 0] + r[:, 2] / 2) - gy,
                         gx - (r[:, 1] - r[:, 3] / 2), (r[:, 1] + r[:, 3] / 2) - gx], 1) / sf[:, None]
        reg[b, :, :4] = true * np.exp(rng.normal(0, 0.35, (P, 4))) + rng.normal(0, 0.5, (P, 4))
        reg[b, :, 4] = rng.normal(0, 1, P)
        cls[b, :, :C] = rng.normal(-2.0, 2.0, (P, C))
    return torch.from_numpy(reg).cuda(), torch.from_numpy(cls).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fcos_tal_table.py times GPU work: it needs the GPU")
    from cvlite import _lib
    from cvlite import ops_targets as ot
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer, synthetic_batch

    have_tal = hasattr(_lib.load(), "cvl_fcos_tal_assign")
    B, D, C = args.batch, args.size, args.classes
    imgs, boxes, nbox = synthetic_batch(B, D, D, C, seed=7)
    dims = torch.full((B, 2), float(D), device="cuda")
    bf = torch.bfloat16
    kernels = []
    loss_tg = None
    for label, (bx, nb) in (("1 + Poisson(1.4) boxes per image", (boxes, nbox)),
                            ("32 boxes per image", dense_boxes(B, 32, D, C, 11))):
        reg, cls = head_outputs(bx, nb, D, C, 5)
        tg, nt = ot.fcos_atss_assign(bx, nb, dims, (D, D), C)
        kernels.append(("cvl_fcos_atss_assign, " + label, None,
                        lambda bx=bx, nb=nb, tg=tg, nt=nt: ot.fcos_atss_assign(bx, nb, dims, (D, D), C, out=tg,
                                                                                num_targets=nt)))
        if have_tal:
            tg2, nt2 = torch.zeros_like(tg), torch.zeros_like(nt)
            kernels.append(("cvl_fcos_tal_assign, " + label, None,
                            lambda bx=bx, nb=nb, reg=reg, cls=cls, tg2=tg2, nt2=nt2: ot.fcos_tal_assign(
                                bx, nb, dims, (D, D), C, reg, cls, out=tg2, num_targets=nt2)))
            kernels[-1][2]()
            tg = tg2
        if loss_tg is None:
            loss_tg, loss_reg, loss_cls = tg, reg, cls
    torch.cuda.synchronize()
    P = int(loss_tg.shape[1])
    npos = int((loss_tg[..., 5:].amax(-1) >= 1).sum())
    cells = B * P
    t_row, c_row = (5 + C) * 4, 32 * 4
    d_reg = torch.zeros((B, P, 32), dtype=bf, device="cuda")
    d_cls = torch.zeros((B, P, 32), dtype=bf, device="cuda")
    losses = torch.zeros((B, 3), device="cuda")
    norm = ot.fcos_target_norm(loss_tg, C)
    kernels += [("cvl_fcos_paper_loss", cells * (t_row + c_row + 32 + 64 + 64),
                 lambda: ot.fcos_paper_loss(loss_reg, loss_cls, loss_tg, C, norm=norm, d_reg=d_reg, d_cls=d_cls,
                                            losses=losses)),
                ("cvl_fcos_target_norm", cells * t_row, lambda: ot.fcos_target_norm(loss_tg, C, out=norm))]
    if have_tal:
        kernels.append(("cvl_fcos_tal_loss", cells * (t_row + c_row + 64 + 64) + npos * 32,
                        lambda: ot.fcos_tal_loss(loss_reg, loss_cls, loss_tg, C, norm=norm, d_reg=d_reg, d_cls=d_cls,
                                                 losses=losses)))
    rows = []
    for name, nbytes, fn in kernels:
        gr = graphed(fn, args.iters)
        us = statistics.median(passes(gr.replay, 1, args.reps, args.warmup)) / args.iters * 1000.0
        del gr
        rows.append(dict(call=name, us=round(us, 2), mbytes=None if nbytes is None else round(nbytes / 1e6, 2),
                         tbps=None if nbytes is None else round(nbytes / (us * 1e-6) / 1e12, 3)))
        print(rows[-1], flush=True)
    steps = []
    for kind in ("atss", "tal") if have_tal else ("atss",):
        net = FCOSNet(C, device=torch.device("cuda", 0), seed=0)
        tr = FCOSTrainer(net, B, (D, D), use_graph=True, targets=kind)
        tr.load_batch(imgs, boxes, nbox)
        ms = passes(tr.step, args.iters, args.reps, args.warmup)
        steps.append(dict(targets=kind, median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4),
                          max_ms=round(max(ms), 4)))
        print(steps[-1], flush=True)
        del tr, net
    lib = os.environ.get("CVL_LIB") or "of this tree"
    lines = ["Task-aligned assignment, %d x %d, batch %d, C = %d (P = %d cells per image, %d positive cells in the "
             "sparse batch), %s, library %s; HIP events around a HIP graph of %d calls, median of %d passes after %d "
             "warm-up passes." % (D, D, B, C, P, npos, torch.cuda.get_device_name(0), lib, args.iters, args.reps,
                                  args.warmup),
             "Command: `python tools/fcos_tal_table.py --size %d --batch %d --iters %d --reps %d`"
             % (D, B, args.iters, args.reps), "",
             "| call | per call | bytes to move | rate |", "|---|---|---|---|"]
    for r in rows:
        lines.append("| `%s` | %.1f us | %s | %s |" % (r["call"], r["us"],
                                                      "" if r["mbytes"] is None else "%.1f MB" % r["mbytes"],
                                                      "" if r["tbps"] is None else "%.2f TB/s" % r["tbps"]))
    lines += ["", "| whole step (two graph replays) | median | min .. max of the passes |", "|---|---|---|"]
    lines += ["| `FCOSTrainer(targets=\"%s\")` | %.3f ms | %.3f .. %.3f ms |"
              % (s["targets"], s["median_ms"], s["min_ms"], s["max_ms"]) for s in steps]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "library": lib, "size": D, "batch": B, "classes": C,
                       "cells": P, "positives": npos, "iters": args.iters, "reps": args.reps, "warmup": args.warmup,
                       "kernels": rows, "steps": steps}, f, indent=1)


if __name__ == "__main__":
    main()
