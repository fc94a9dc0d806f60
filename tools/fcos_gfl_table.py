"""Times the Generalized Focal Loss kernels and the whole GFL training step at 512 x 512, batch 16,
C = 20 (synthetic batches of 1 + Poisson(1.4) boxes per image), in one process, by the method of
tools/fcos_atss_table.py (HIP events around a HIP graph of --iters calls, median of --reps passes after
--warmup passes):
  kernels   cvl_fcos_gfl_loss (bf16 gradient rows as the trainer passes them: reg_max 16 with d_reg 96
            and 128 wide, reg_max 7 with d_reg 32 wide), cvl_fcos_gfl_norm and cvl_fcos_gfl_decode beside
            cvl_fcos_paper_loss and cvl_fcos_target_norm, on ATSS targets; with the bytes each call has
            to move (targets and class rows read, the positives' box rows read, both gradient rows
            written) and the rate that makes
  step      the whole FCOSTrainer step (two graph replays) for targets="gfl" at reg_max 16 with the reg
            head's GEMM padding 96 and 128, at reg_max 7, and for targets="atss", each as median and
            min .. max over the passes (the run-to-run spread)
With CVL_LIB pointing at a build of the parent revision (tools/build_base.sh) the GFL rows are left out
and the others are the parent's figures on the same box.
usage: fcos_gfl_table.py [--size 512] [--batch 16] [--iters 20] [--reps 7] [--out FILE]"""
import argparse
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fcos_gfl_table.py times GPU work: it needs the GPU")
    from cvlite import _lib
    from cvlite import ops_targets as ot
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer, synthetic_batch

    have_gfl = hasattr(_lib.load(), "cvl_fcos_gfl_loss")
    B, D, C = args.batch, args.size, args.classes
    imgs, boxes, nbox = synthetic_batch(B, D, D, C, seed=7)
    dims = torch.full((B, 2), float(D), device="cuda")
    tg, _ = ot.fcos_atss_assign(boxes, nbox, dims, (D, D), C)
    P = int(tg.shape[1])
    npos = int((tg[..., 5:].amax(-1) >= 1).sum())
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *shape: torch.randn(shape, generator=g).cuda()       # noqa: E731
    cls = torch.zeros((B, P, 32), device="cuda")
    cls[..., :C] = rnd(B, P, C) - 2.0
    bf = torch.bfloat16
    d_cls = torch.zeros((B, P, 32), dtype=bf, device="cuda")
    losses = torch.zeros((B, 3), device="cuda")
    cells = B * P
    t_row, c_row = (5 + C) * 4, 32 * 4

    reg5 = torch.zeros((B, P, 8), device="cuda")
    reg5[..., :5] = rnd(B, P, 5)
    d_reg5 = torch.zeros((B, P, 32), dtype=bf, device="cuda")
    norm_p = ot.fcos_target_norm(tg, C)
    kernels = [("cvl_fcos_paper_loss", cells * (t_row + c_row + 32 + 64 + 64),
                lambda: ot.fcos_paper_loss(reg5, cls, tg, C, norm=norm_p, d_reg=d_reg5, d_cls=d_cls, losses=losses)),
               ("cvl_fcos_target_norm", cells * t_row, lambda: ot.fcos_target_norm(tg, C, out=norm_p))]
    if have_gfl:
        norm_g = ot.fcos_gfl_norm(cls, tg, C)
        for R, wide in ((16, 96), (16, 128), (7, 32)):
            ld = (4 * (R + 1) + 7) // 8 * 8
            reg = torch.zeros((B, P, ld), device="cuda")
            reg[..., :4 * (R + 1)] = rnd(B, P, 4 * (R + 1))
            d_reg = torch.zeros((B, P, wide), dtype=bf, device="cuda")
            nbytes = cells * (t_row + c_row + 2 * wide + 64) + npos * ld * 4
            kernels.append(("cvl_fcos_gfl_loss, reg_max %d, d_reg %d wide" % (R, wide), nbytes,
                            lambda reg=reg, d_reg=d_reg, R=R: ot.fcos_gfl_loss(
                                reg, cls, tg, C, R, norm=norm_g, d_reg=d_reg, d_cls=d_cls, losses=losses)))
            if wide != 128:
                box = torch.zeros((B, P, 8), device="cuda")
                kernels.append(("cvl_fcos_gfl_decode, reg_max %d" % R, cells * (ld * 4 + 32),
                                lambda reg=reg, R=R, box=box: ot.fcos_gfl_decode(reg, R, out=box)))
        kernels.append(("cvl_fcos_gfl_norm", cells * t_row + npos * c_row,
                        lambda: ot.fcos_gfl_norm(cls, tg, C, out=norm_g)))
    rows = []
    for name, nbytes, fn in kernels:
        gr = graphed(fn, args.iters)
        ms = statistics.median(passes(gr.replay, 1, args.reps, args.warmup)) / args.iters
        del gr
        rows.append((name, ms * 1000.0, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e12))
        print("%s: %.1f us, %.1f MB, %.2f TB/s" % rows[-1], flush=True)
    configs = [("atss", None, None)]
    if have_gfl:
        configs += [("gfl", 16, 96), ("gfl", 16, 128), ("gfl", 7, None)]
    steps = []
    for kind, R, npad in configs:
        kw = {} if R is None else dict(reg_max=R, reg_npad=npad)
        net = FCOSNet(C, device=torch.device("cuda", 0), seed=0, **kw)
        tr = FCOSTrainer(net, B, (D, D), use_graph=True, targets=kind)
        tr.load_batch(imgs, boxes, nbox)
        ms = passes(tr.step, args.iters, args.reps, args.warmup)
        label = "targets=\"%s\"" % kind + ("" if R is None else ", reg_max %d, reg head npad %d" % (R, net.reg_heads[0].npad))
        steps.append((label, statistics.median(ms), min(ms), max(ms)))
        print("FCOSTrainer(%s) step: %.3f ms (%.3f .. %.3f)" % steps[-1], flush=True)
        del tr, net
    lines = ["Generalized Focal Loss, %d x %d, batch %d, C = %d (P = %d cells per image, %d positive cells in the batch), "
             "%s, library %s; HIP events around a HIP graph of %d calls, median of %d passes after %d warm-up passes."
             % (D, D, B, C, P, npos, torch.cuda.get_device_name(0), os.environ.get("CVL_LIB") or "of this tree",
                args.iters, args.reps, args.warmup),
             "Command: `python tools/fcos_gfl_table.py --size %d --batch %d --iters %d --reps %d`"
             % (D, B, args.iters, args.reps), "",
             "| call | per call | bytes to move | rate |", "|---|---|---|---|"]
    lines += ["| `%s` | %.1f us | %.1f MB | %.2f TB/s |" % r for r in rows]
    lines += ["", "| whole step (two graph replays) | median | min .. max of the passes |", "|---|---|---|"]
    lines += ["| `FCOSTrainer(%s)` | %.3f ms | %.3f .. %.3f ms |" % s for s in steps]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
