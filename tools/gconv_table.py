"""Times the grouped 3x3 conv kernels (cvl_gconv3x3_fwd / dgrad / wgrad, csrc/conv_group.hip) at
ResNeXt-50's five shapes for RetinaNet 640x640, bs 8, with HIP events on the launch stream, and --
for the stride-1 shapes -- the existing dense 3x3 C -> C conv on the same map through
ops_nn.conv_igemm (forward and data gradient): that kernel does C / Cg >= 32x the MACs, so a
grouped kernel that loses to it has no reason to exist (the one bar; exit status 1 when missed).

Bytes = the algorithmic traffic: every activation operand read or written once (x and y for the
forward, dy and dx for the data gradient, x and dy for the weight gradient) plus the weights; GB/s =
bytes / time; "x floor" = time / (bytes / 6.3 TB/s, the achievable HBM rate of MI355X_MICROARCH.md),
recorded, not gated.  Each entry: warm-up launches, then the median of --reps timed windows of
--iters launches.  Prints a markdown table.
usage: gconv_table.py [--bs 8] [--iters 20] [--reps 5] [--out file.md]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd")]
import torch  # noqa: E402

from cvlite import ops_nn as nn  # noqa: E402
from cvlite.layers import Conv, ParamStore  # noqa: E402

BF16 = torch.bfloat16
HBM_GBS = 6300.0
# (H = W of the input map, C, Cg, stride): stage 1 .. 4 of ResNeXt-50 at 640 x 640
SHAPES = [(160, 128, 4, 1), (160, 256, 8, 2), (80, 256, 8, 1), (40, 512, 16, 1), (20, 1024, 32, 1)]


def time_us(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gconv_table.py times kernels: it needs the GPU")
    B = args.bs
    g = torch.Generator().manual_seed(0)
    rows, missed = [], []
    for H, C, Cg, s in SHAPES:
        Ho = (H - 1) // s + 1
        x = torch.randn((B, H, H, C), generator=g).to(BF16).cuda()
        dy = torch.randn((B, Ho, Ho, C), generator=g).to(BF16).cuda()
        w = (torch.randn((3, 3, Cg, C), generator=g) * 0.1).cuda()
        wf, wd = nn.gconv3x3_packed(C, "cuda"), nn.gconv3x3_packed(C, "cuda")
        nn.gconv3x3_pack(w, wf, wd)
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        act = (x.numel() + dy.numel()) * 2
        t = {"fwd": time_us(lambda: nn.gconv3x3_fwd(x, wf, y, Cg, s), args.iters, args.reps),
             "dgrad": time_us(lambda: nn.gconv3x3_dgrad(dy, wd, dx, Cg, s), args.iters, args.reps),
             "wgrad": time_us(lambda: nn.gconv3x3_wgrad(x, dy, dw, s), args.iters, args.reps)}
        nbytes = {"fwd": act + wf.numel() * 2, "dgrad": act + wd.numel() * 2, "wgrad": act + w.numel() * 4}
        dense = {}
        if s == 1:
            st = ParamStore()
            conv = Conv(st, "dense", 3, C, C, bias=False)
            st.finalize("cuda", 0)
            conv.pack()
            yd = torch.empty_like(x)
            fd = conv.fwd_desc(B, [nn.seg(H, H, H, H, conv.wf, None)], ld_dst=C)
            dd = conv.dgrad_desc(B, [nn.seg(H, H, H, H, conv.wd)], ld_dst=C)
            dense["fwd"] = time_us(lambda: nn.conv_igemm(fd, x, yd), args.iters, args.reps)
            dense["dgrad"] = time_us(lambda: nn.conv_igemm(dd, dy, yd), args.iters, args.reps)
        for op in ("fwd", "dgrad", "wgrad"):
            gbs = nbytes[op] / t[op] / 1e3
            floor = nbytes[op] / HBM_GBS / 1e3
            d = dense.get(op)
            if d is not None and not t[op] < d:
                missed.append((H, C, Cg, op, t[op], d))
            rows.append("| %dx%d C%d Cg%d s%d | %s | %.1f | %.1f | %.0f | %.1f | %s | %s |" % (
                H, H, C, Cg, s, op, t[op], nbytes[op] / 1e6, gbs, t[op] / floor,
                "%.1f" % d if d is not None else "-", "%.1fx" % (d / t[op]) if d is not None else "-"))
    lines = ["Grouped 3x3 conv kernels at ResNeXt-50's shapes (RetinaNet 640x640, bs %d), %s; median of %d windows "
             "of %d launches, HIP events." % (B, torch.cuda.get_device_name(0), args.reps, args.iters), "",
             "| shape | op | us | MB | GB/s | x HBM floor (6.3 TB/s) | dense 3x3 C->C us | dense / grouped |",
             "|---|---|---|---|---|---|---|---|"] + rows
    lines += ["", "The one bar (grouped forward and data gradient faster than the dense conv at every stride-1 "
              "shape): %s" % ("met" if not missed else "MISSED %s" % missed)]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    sys.exit(1 if missed else 0)


if __name__ == "__main__":
    main()
