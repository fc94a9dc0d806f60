"""Times the RetinaNet target / loss triple of both recipes at the benchmark geometry (640 x 640, batch 8,
C = 80, 24 candidates, synthetic_coco_batch), in one process, by the method of tools/fcos_atss_table.py
(HIP events around a HIP graph of --iters calls, median of --reps passes after --warmup passes):
  kernels   cvl_retina_assign, the target cvl_gather_rows and cvl_retina_loss, and their ATSS counterparts
            cvl_retina_atss_assign (its two memset nodes included), cvl_gather_rows on the compact rows
            and cvl_retina_atss_loss; each with the bytes it must move (arithmetic from the shapes: every
            output written once, every input read once) and the rate that gives.  To show where the ATSS
            assignment's time goes: the same call with every box skipped (nbox = 0: memsets and write-out)
  step      the whole RetinaTrainer step (two graph replays) for targets="reference" and targets="atss",
            each as median and min .. max over the passes (the run-to-run spread)
With CVL_LIB pointing at a build of the parent revision (tools/build_base.sh) the ATSS rows are left out
and the others are the parent's figures on the same box.
usage: retina_atss_table.py [--size 640] [--batch 8] [--candidates 3] [--iters 20] [--reps 7] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd")]
import torch  # noqa: E402

from fcos_atss_table import passes  # noqa: E402
from fcos_paper_table import graphed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--candidates", type=int, default=3)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retina_atss_table.py times GPU work: it needs the GPU")
    from cvlite import _lib
    from cvlite import ops_nn as nn
    from cvlite import ops_targets as ot
    from cvlite.retinanet import RetinaNet
    from cvlite.train_retinanet import RetinaTrainer, synthetic_coco_batch

    have_atss = hasattr(_lib.load(), "cvl_retina_atss_assign")
    B, S, C = args.batch, args.size, args.classes
    nc = args.candidates * B
    rn = RetinaNet(C, {}, anchor_sizes=[20.0, 40.0, 80.0, 160.0, 320.0])
    A = rn.n_anchors
    adims = rn.anchor_dims_device()
    imgs, boxes, nbox = synthetic_coco_batch(nc, S, C, n_max=50, seed=4321)
    dims = torch.full((nc, 2), float(S), device="cuda")
    cells = [(S // s) ** 2 for s in rn.strides]
    P = sum(cells)
    T = P * A
    ld_reg, ld_cls = 4 * A + (-4 * A) % 32, A * C + (-A * C) % 32          # the heads' padded rows
    g = torch.Generator(device="cpu").manual_seed(1)
    reg = torch.randn((B, P, ld_reg), generator=g).cuda()
    cls = (torch.randn((B, P, ld_cls), generator=g) - 2).cuda()
    d_reg = torch.zeros((B, P, ld_reg), dtype=torch.bfloat16, device="cuda")
    d_cls = torch.zeros((B, P, ld_cls), dtype=torch.bfloat16, device="cuda")
    losses = torch.zeros((B, 2), device="cuda")
    sel = torch.arange(0, B, dtype=torch.int32, device="cuda") * args.candidates
    w = torch.ones((B,), device="cuda")
    pred = B * P * (A * C + 4 * A) * (4 + 2)                               # fp32 outputs read, bf16 gradients written

    # the reference triple
    row = 4 + C
    c_tg = torch.zeros((nc, T, row), device="cuda")
    c_nt = torch.zeros((nc,), dtype=torch.int32, device="cuda")
    tg = torch.zeros((B, T, row), device="cuda")
    kernels = [
        ("cvl_retina_assign", nc * T * row * 4,
         lambda: ot.retina_assign(boxes, nbox, dims, S, adims, C, out=c_tg, num_targets=c_nt)),
        ("cvl_gather_rows (targets)", 2 * B * T * row * 4, lambda: nn.gather_rows(c_tg, sel, tg)),
        ("cvl_retina_loss", B * T * row * 4 + pred,
         lambda: ot.retina_loss(reg, cls, tg, cells, A, C, img_weight=w, d_reg=d_reg, d_cls=d_cls, losses=losses)),
    ]
    if have_atss:
        a_tg = torch.zeros((nc, T, 8), device="cuda")
        a_nt = torch.zeros((nc, 5), dtype=torch.int32, device="cuda")
        atg = torch.zeros((B, T, 8), device="cuda")
        ant = torch.zeros((B, 5), dtype=torch.int32, device="cuda")
        none = torch.zeros_like(nbox)
        assign_bytes = nc * T * (8 + 8 + 32)                                # keys cleared, keys read, rows written
        kernels += [
            ("cvl_retina_atss_assign", assign_bytes,
             lambda: ot.retina_atss_assign(boxes, nbox, dims, S, adims, C, out=a_tg, num_targets=a_nt)),
            ("cvl_retina_atss_assign, nbox = 0", assign_bytes,
             lambda: ot.retina_atss_assign(boxes, none, dims, S, adims, C, out=a_tg, num_targets=a_nt)),
            ("cvl_gather_rows (compact targets)", 2 * B * T * 32, lambda: nn.gather_rows(a_tg, sel, atg)),
        ]
        ot.retina_atss_assign(boxes, nbox, dims, S, adims, C, out=a_tg, num_targets=a_nt)
        nn.gather_rows(a_tg, sel, atg)
        torch.index_select(a_nt, 0, sel, out=ant)
        kernels.append(("cvl_retina_atss_loss", B * T * 32 + pred,
                        lambda: ot.retina_atss_loss(reg, cls, atg, ant, A, C, img_weight=w, d_reg=d_reg, d_cls=d_cls,
                                                    losses=losses)))
    ot.retina_assign(boxes, nbox, dims, S, adims, C, out=c_tg, num_targets=c_nt)
    nn.gather_rows(c_tg, sel, tg)
    rows = []
    for name, nbytes, fn in kernels:
        gr = graphed(fn, args.iters)
        ms = statistics.median(passes(gr.replay, 1, args.reps, args.warmup)) / args.iters
        del gr
        rows.append((name, ms * 1000.0, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e9))
        print("%s: %.1f us, %.1f MB, %.0f GB/s" % rows[-1], flush=True)
    del c_tg, tg
    steps = []
    for kind in (("reference", "atss") if have_atss else ("reference",)):
        net = RetinaNet(C, {}, anchor_sizes=[20.0, 40.0, 80.0, 160.0, 320.0])
        kw = dict(targets=kind) if have_atss else {}
        tr = RetinaTrainer(net.model, net, B, S, n_max=50, candidates=args.candidates, use_graph=True, **kw)
        tr.load_candidates(imgs, boxes, nbox)
        ms = passes(tr.step, args.iters, args.reps, args.warmup)
        steps.append((kind, statistics.median(ms), min(ms), max(ms)))
        print("RetinaTrainer(targets=%r) step: %.3f ms (%.3f .. %.3f)" % steps[-1], flush=True)
        del tr, net
    lines = ["RetinaNet targets and loss, %d x %d, batch %d, %d candidates, C = %d (P = %d cells, %d anchors per image), "
             "%s, library %s; HIP events around a HIP graph of %d calls, median of %d passes after %d warm-up passes.  "
             "Times are measured; bytes are arithmetic from the shapes; rates are their quotient."
             % (S, S, B, nc, C, P, T, torch.cuda.get_device_name(0), os.environ.get("CVL_LIB") or "of this tree",
                args.iters, args.reps, args.warmup),
             "Command: `python tools/retina_atss_table.py --size %d --batch %d --iters %d --reps %d`"
             % (S, B, args.iters, args.reps), "",
             "| call | per call | bytes it must move | rate |", "|---|---|---|---|"]
    lines += ["| `%s` | %.1f us | %.1f MB | %.0f GB/s |" % r for r in rows]
    lines += ["", "| whole step (two graph replays) | median | min .. max of the passes |", "|---|---|---|"]
    lines += ["| `RetinaTrainer(targets=\"%s\")` | %.3f ms | %.3f .. %.3f ms |" % s for s in steps]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
