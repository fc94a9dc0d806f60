"""The X-ring weight-gradient launches of an FCOS 512 x 512 / bs 16 step at their real shapes, on
synthetic operands, under both read placements of the prefetching loop (default and
CVL_DISPATCH=wgx_reads=0; the planner reads the key at every call, so one process runs both):
  tower   grouped 3x3 256->256, 2 groups x 5 levels (64 .. 4), B 16: conv_wgrad_x_kernel<256, 32, .., WxArgs>
  b256    one batched call of the conv4_x 1x1 pairs (1024->256, 256->1024 @ 32 x 32) x 3: <256, 32, .., WxBatchArgs>
  b128    one batched call of the conv2_x 1x1 pairs (64->256, 256->64 @ 128 x 128) x 3: <128, 64, .., WxBatchArgs>
Each launch (with its split reduction) is replayed 20 x inside a HIP graph and timed by events; the
two forms alternate, --reps times.  Under `rocprofv3 --pmc ...` (a run of its own, no tracing flag)
the two forms show up as two kernel names (the last template argument).  usage: wgx_reads_launches.py [--reps N]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import wgrad_dispatch_cases as wc  # noqa: E402
from cvlite import ops_nn as nn  # noqa: E402

BF = torch.bfloat16


def single(gen, B, H, cin, cout):
    x = (torch.randn((B, H, H, cin), generator=gen, device="cuda") * 0.5).to(BF)
    dy = (torch.randn((B, H, H, cout), generator=gen, device="cuda") * 0.5).to(BF)
    w = torch.zeros((cout, cin), dtype=BF, device="cuda")
    d = nn.make_desc(nn.FWD, B, cin, 1, 1, 1, 0, 0, cout, cout, cout, [nn.seg(H, H, H, H, w, None)])
    return d, x, dy, torch.zeros(cin * cout, dtype=torch.float32, device="cuda")


def launches():
    cpu = torch.Generator(device="cpu").manual_seed(3)
    d, x, dy = wc._multi(cpu, "cuda", 16, [64, 32, 16, 8, 4], 2, 256, 256, 256, 3)
    dws = [torch.zeros(9 * 256 * 256, dtype=torch.float32, device="cuda") for _ in range(2)]
    out = {"tower": lambda: nn.conv_wgrad_grouped(d, x, dy, dws)}
    gen = torch.Generator(device="cuda").manual_seed(4)
    for name, H, a, b in (("b256", 32, 1024, 256), ("b128", 128, 64, 256)):
        ps = [single(gen, 16, H, *c) for c in ((a, b), (b, a)) * 3]
        out[name] = (lambda ps: lambda: nn.conv_wgrad_batch([p[0] for p in ps], [p[1] for p in ps],
                                                           [p[2] for p in ps], [p[3] for p in ps]))(ps)
    return out


def timed(run):
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(20):
            run()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    keep = os.environ.get("CVL_DISPATCH", "")
    rows = {}
    ls = launches()
    for rep in range(args.reps):
        for form in ("", "wgx_reads=0"):
            os.environ["CVL_DISPATCH"] = ",".join(k for k in (keep, form) if k)
            for name, run in ls.items():
                rows.setdefault((name, form or "default"), []).append(timed(run))
    os.environ["CVL_DISPATCH"] = keep
    print("| launch | form | us per launch incl. reduction (%d runs) |" % args.reps)
    print("|---|---|---|")
    for (name, form), v in rows.items():
        print("| %s | %s | %s |" % (name, form, " / ".join("%.1f" % t for t in v)), flush=True)


if __name__ == "__main__":
    main()
