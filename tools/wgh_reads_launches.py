"""The five halo (WH) weight-gradient launches of an FCOS 512 x 512 / bs 16 step at their real shapes,
on synthetic operands, under both step loops (default and CVL_DISPATCH=wh_reads=0; the planner reads
the key at every call, so one process runs both): one batched call per ResNet stage's 3x3 units
  c2  3 x 64->64 @ 128 x 128     c3  4 x 128->128 @ 64 x 64
  c4  6 x 256->256 @ 32 x 32     c5  3 x 512->512 @ 16 x 16
and one for the FPN output convs (fpn: 256->256 @ 64 / 32 / 16), each conv_wgrad_h_kernel<WhBatch, ..>.
Each launch (with its split reductions) is replayed 20 x inside a HIP graph and timed by events; the
two forms alternate, --reps times.  Under `rocprofv3 --pmc ...` (a run of its own, no tracing flag)
the two forms show up as two kernel names (the last template argument).  usage: wgh_reads_launches.py [--reps N]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from cvlite import ops_nn as nn  # noqa: E402
from wgx_reads_launches import timed  # noqa: E402

BF = torch.bfloat16
LAUNCHES = {"c2": [(128, 64)] * 3, "c3": [(64, 128)] * 4, "c4": [(32, 256)] * 6, "c5": [(16, 512)] * 3,
            "fpn": [(64, 256), (32, 256), (16, 256)]}


def single(gen, B, H, c):
    x = (torch.randn((B, H, H, c), generator=gen, device="cuda") * 0.5).to(BF)
    dy = (torch.randn((B, H, H, c), generator=gen, device="cuda") * 0.5).to(BF)
    w = torch.zeros((c, 9 * c), dtype=BF, device="cuda")
    d = nn.make_desc(nn.FWD, B, c, 3, 3, 1, 1, 1, c, c, c, [nn.seg(H, H, H, H, w, None)])
    return d, x, dy, torch.zeros(9 * c * c, dtype=torch.float32, device="cuda")


def launches():
    gen = torch.Generator(device="cuda").manual_seed(4)
    out = {}
    for name, probs in LAUNCHES.items():
        ps = [single(gen, 16, H, c) for H, c in probs]
        out[name] = (lambda ps: lambda: nn.conv_wgrad_batch([p[0] for p in ps], [p[1] for p in ps],
                                                           [p[2] for p in ps], [p[3] for p in ps]))(ps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    keep = os.environ.get("CVL_DISPATCH", "")
    rows = {}
    ls = launches()
    for rep in range(args.reps):
        for form in ("", "wh_reads=0"):
            os.environ["CVL_DISPATCH"] = ",".join(k for k in (keep, form) if k)
            for name, run in ls.items():
                rows.setdefault((name, form or "default"), []).append(timed(run))
    os.environ["CVL_DISPATCH"] = keep
    print("| launch | form | us per launch incl. reductions (%d runs) |" % args.reps)
    print("|---|---|---|")
    for (name, form), v in rows.items():
        print("| %s | %s | %s |" % (name, form, " / ".join("%.1f" % t for t in v)), flush=True)


if __name__ == "__main__":
    main()
