"""Times the CenterNet target / loss calls of both recipes at the benchmark geometry (512 x 512, batch 8,
C = 20, stride 4: P = 16384 cells, train_centernet.synthetic_batch), in one process, by the method of
tools/retina_atss_table.py (HIP events around a HIP graph of --iters calls, median of --reps passes after
--warmup passes):
  kernels   cvl_centernet_assign and cvl_centernet_loss (the reference recipe), cvl_centernet_gauss_assign,
            cvl_centernet_gauss_norm (its memset node included) and cvl_centernet_gauss_loss; each with the
            bytes it must move (arithmetic from the shapes: every output written once, every input read
            once) and the rate that gives.  The two losses read and write the same tensors, so their rates
            compare the strided row walk with the coalesced one directly.
  step      the whole CenterNetTrainer step (two graph replays) for targets="reference" and
            targets="gaussian", each as median and min .. max over the passes (the run-to-run spread)
With CVL_LIB pointing at a build of the parent revision (tools/build_base.sh) the gaussian rows are left
out and the others are the parent's figures on the same box.
usage: centernet_gauss_table.py [--size 512] [--batch 8] [--iters 20] [--reps 7] [--out FILE] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from fcos_atss_table import passes  # noqa: E402
from fcos_paper_table import graphed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="kernel rows only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("centernet_gauss_table.py times GPU work: it needs the GPU")
    from cvlite import _lib
    from cvlite import ops_targets as ot
    from cvlite.hourglass_net import HourglassNet
    from cvlite.train_centernet import CenterNetTrainer, synthetic_batch

    have_gauss = hasattr(_lib.load(), "cvl_centernet_gauss_assign")
    B, S, C, stride = args.batch, args.size, args.classes, 4
    imgs, boxes, nbox = synthetic_batch(B, S, S, C, n_max=16, seed=777)
    dims = torch.full((B, 2), float(S), device="cuda")
    Hs = S // stride
    P = Hs * Hs
    row = 4 + C
    ld = (row + 31) // 32 * 32                                            # the output conv's padded rows
    g = torch.Generator(device="cpu").manual_seed(1)
    pred = torch.randn((B, P, ld), generator=g).cuda()
    pred[..., 4:] -= 4.0                                                  # about the prior of the focal bias
    d = torch.zeros((B, P, ld), dtype=torch.bfloat16, device="cuda")
    losses = torch.zeros((B, 2), device="cuda")
    tg = torch.zeros((B, Hs, Hs, row), device="cuda")
    map_bytes = B * P * row * 4
    loss_bytes = map_bytes + B * P * ld * 4 + B * P * ld * 2              # targets + fp32 rows read, bf16 rows written
    kernels = [
        ("cvl_centernet_assign", map_bytes, lambda: ot.centernet_assign(boxes, nbox, dims, (S, S), C, stride=stride,
                                                                        out=tg)),
        ("cvl_centernet_loss", loss_bytes, lambda: ot.centernet_loss(pred, tg.view(B, P, row), C, 2.5, 1.0, d_pred=d,
                                                                     losses=losses)),
    ]
    if have_gauss:
        gt = torch.zeros((B, Hs, Hs, row), device="cuda")
        npos = torch.zeros((B,), dtype=torch.int32, device="cuda")
        ot.centernet_gauss_assign(boxes, nbox, dims, (S, S), C, stride=stride, out=gt)
        ot.centernet_gauss_norm(gt, C, out=npos)
        kernels += [
            ("cvl_centernet_gauss_assign", map_bytes,
             lambda: ot.centernet_gauss_assign(boxes, nbox, dims, (S, S), C, stride=stride, out=gt)),
            ("cvl_centernet_gauss_norm", map_bytes, lambda: ot.centernet_gauss_norm(gt, C, out=npos)),
            ("cvl_centernet_gauss_loss", loss_bytes,
             lambda: ot.centernet_gauss_loss(pred, gt.view(B, P, row), npos, C, cls_scale=2.5, reg_scale=1.0, d_pred=d,
                                             losses=losses)),
        ]
    ot.centernet_assign(boxes, nbox, dims, (S, S), C, stride=stride, out=tg)
    rows = []
    for name, nbytes, fn in kernels:
        gr = graphed(fn, args.iters)
        ms = statistics.median(passes(gr.replay, 1, args.reps, args.warmup)) / args.iters
        del gr
        rows.append((name, ms * 1000.0, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e9))
        print("%s: %.1f us, %.1f MB, %.0f GB/s" % rows[-1], flush=True)
    steps = []
    if not args.no_step:
        for kind in (("reference", "gaussian") if have_gauss else ("reference",)):
            net = HourglassNet(C, seed=0)
            kw = dict(targets=kind) if have_gauss else {}
            tr = CenterNetTrainer(net, B, (S, S), sub_batch_sz=2, n_max=16, use_graph=True, **kw)
            tr.load_batch(imgs, boxes, nbox)
            ms = passes(tr.step, args.iters, args.reps, args.warmup)
            steps.append((kind, statistics.median(ms), min(ms), max(ms)))
            print("CenterNetTrainer(targets=%r) step: %.3f ms (%.3f .. %.3f)" % steps[-1], flush=True)
            del tr, net
    lib = os.environ.get("CVL_LIB") or "of this tree"
    lines = ["CenterNet targets and loss, %d x %d, batch %d, C = %d, stride %d (P = %d cells, rows of %d floats, "
             "prediction rows of %d), %s, library %s; HIP events around a HIP graph of %d calls, median of %d passes "
             "after %d warm-up passes.  Times are measured; bytes are arithmetic from the shapes; rates are their "
             "quotient." % (S, S, B, C, stride, P, row, ld, torch.cuda.get_device_name(0), lib, args.iters, args.reps,
                            args.warmup),
             "Command: `python tools/centernet_gauss_table.py --size %d --batch %d --iters %d --reps %d`"
             % (S, B, args.iters, args.reps), "",
             "| call | per call | bytes it must move | rate |", "|---|---|---|---|"]
    lines += ["| `%s` | %.1f us | %.1f MB | %.0f GB/s |" % r for r in rows]
    if steps:
        lines += ["", "| whole step (two graph replays) | median | min .. max of the passes |", "|---|---|---|"]
        lines += ["| `CenterNetTrainer(targets=\"%s\")` | %.3f ms | %.3f .. %.3f ms |" % s for s in steps]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "library": lib, "size": S, "batch": B, "classes": C,
                       "cells": P, "iters": args.iters, "reps": args.reps, "warmup": args.warmup,
                       "kernels": [dict(call=r[0], us=round(r[1], 2), mbytes=round(r[2], 2), gbps=round(r[3], 1))
                                   for r in rows],
                       "steps": [dict(targets=s[0], median_ms=round(s[1], 4), min_ms=round(s[2], 4),
                                      max_ms=round(s[3], 4)) for s in steps]}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
