"""Times the ATSS assignment next to the other two FCOS assignments at 512 x 512, batch 16, C = 20, in
one process, by the method of tools/fcos_paper_table.py (HIP events around a HIP graph of --iters
calls, median of --reps passes after --warmup passes):
  kernels   cvl_fcos_atss_assign (its two memset nodes included) beside cvl_fcos_paper_assign and
            cvl_fcos_assign; and, to show where its time goes, the same call with topk 1 and 16 (the
            selection rounds), with every box skipped (nbox = 0: the memsets and the write-out alone) and
            with 16 boxes in every image
  step      the whole FCOSTrainer step (two graph replays) for targets="atss" and targets="paper", each
            as median and min .. max over the passes (the run-to-run spread)
With CVL_LIB pointing at a build of the parent revision (tools/build_base.sh) the ATSS rows are left out
and the others are the parent's figures on the same box.
usage: fcos_atss_table.py [--size 512] [--batch 16] [--iters 20] [--reps 7] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd")]
import torch  # noqa: E402

from fcos_paper_table import graphed  # noqa: E402


def passes(fn, iters, reps, warmup):
    """HIP-event time of iters calls / iters, in ms, for each of reps passes after warmup passes."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fcos_atss_table.py times GPU work: it needs the GPU")
    from cvlite import _lib
    from cvlite import ops_targets as ot
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer, synthetic_batch

    have_atss = hasattr(_lib.load(), "cvl_fcos_atss_assign")
    B, D, C = args.batch, args.size, args.classes
    imgs, boxes, nbox = synthetic_batch(B, D, D, C, seed=7)
    # 16 boxes in every image: the first box of each image of 16 more draws
    extra = [synthetic_batch(B, D, D, C, seed=20 + k)[1][:, :1] for k in range(16)]
    full = torch.cat(extra, 1).contiguous()
    nfull = torch.full_like(nbox, 16)
    none = torch.zeros_like(nbox)
    dims = torch.full((B, 2), float(D), device="cuda")
    tg, nt = ot.fcos_assign(boxes, nbox, dims, (D, D), C)
    P = int(tg.shape[1])
    kw = dict(out=tg, num_targets=nt)
    kernels = [
        ("cvl_fcos_assign (reference)", lambda: ot.fcos_assign(boxes, nbox, dims, (D, D), C, **kw)),
        ("cvl_fcos_paper_assign", lambda: ot.fcos_paper_assign(boxes, nbox, dims, (D, D), C, **kw)),
    ]
    if have_atss:
        kernels += [
            ("cvl_fcos_atss_assign", lambda: ot.fcos_atss_assign(boxes, nbox, dims, (D, D), C, **kw)),
            ("cvl_fcos_atss_assign, topk 1", lambda: ot.fcos_atss_assign(boxes, nbox, dims, (D, D), C, topk=1, **kw)),
            ("cvl_fcos_atss_assign, topk 16", lambda: ot.fcos_atss_assign(boxes, nbox, dims, (D, D), C, topk=16, **kw)),
            ("cvl_fcos_atss_assign, nbox = 0", lambda: ot.fcos_atss_assign(boxes, none, dims, (D, D), C, **kw)),
            ("cvl_fcos_atss_assign, 16 boxes per image", lambda: ot.fcos_atss_assign(full, nfull, dims, (D, D), C, **kw)),
            ("cvl_fcos_paper_assign, 16 boxes per image", lambda: ot.fcos_paper_assign(full, nfull, dims, (D, D), C, **kw)),
        ]
    rows = []
    for name, fn in kernels:
        gr = graphed(fn, args.iters)
        ms = statistics.median(passes(gr.replay, 1, args.reps, args.warmup)) / args.iters
        del gr
        rows.append((name, ms * 1000.0))
        print("%s: %.1f us" % rows[-1], flush=True)
    steps = []
    for kind in (("atss", "paper") if have_atss else ("paper",)):
        net = FCOSNet(C, device=torch.device("cuda", 0), seed=0)
        tr = FCOSTrainer(net, B, (D, D), use_graph=True, targets=kind)
        tr.load_batch(imgs, boxes, nbox)
        ms = passes(tr.step, args.iters, args.reps, args.warmup)
        steps.append((kind, statistics.median(ms), min(ms), max(ms)))
        print("FCOSTrainer(targets=%r) step: %.3f ms (%.3f .. %.3f)" % steps[-1], flush=True)
        del tr, net
    lines = ["FCOS assignments, %d x %d, batch %d, C = %d (P = %d cells per image), %s, library %s; HIP events around a "
             "HIP graph of %d calls, median of %d passes after %d warm-up passes."
             % (D, D, B, C, P, torch.cuda.get_device_name(0), os.environ.get("CVL_LIB") or "of this tree", args.iters,
                args.reps, args.warmup),
             "Command: `python tools/fcos_atss_table.py --size %d --batch %d --iters %d --reps %d`"
             % (D, B, args.iters, args.reps), "",
             "| call | per call |", "|---|---|"]
    lines += ["| `%s` | %.1f us |" % r for r in rows]
    lines += ["", "| whole step (two graph replays) | median | min .. max of the passes |", "|---|---|---|"]
    lines += ["| `FCOSTrainer(targets=\"%s\")` | %.3f ms | %.3f .. %.3f ms |" % s for s in steps]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
