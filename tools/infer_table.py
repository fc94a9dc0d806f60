"""Times the FCOS R50-FPN inference forward (train=False) at 512 x 512, batch 16, in one process:
  plain      the training graph with BN on the moving statistics (conv, bf16 z, cvl_bn_apply per unit)
  folded     forward(folded=True): the backbone's BNs folded into its convs (ResNet50.fold_bn), conv3 of
             every bottleneck through cvl_conv_igemm_res_relu with the ReLU in the persistent kernel's epilogue
  fallback   the same with CVL_DISPATCH=no_res_relu_fuse: conv3 as the beta = 1 launch + cvl_relu_
Each form is timed two ways with HIP events around --iters forwards, after --warmup passes, as the
median of --reps passes divided by --iters: launched eagerly from Python (launch gaps included: what a
caller of image_detections sees) and replayed from a HIP graph (the device time alone).  The fold itself
(one scaled pack launch + the scale / bias arithmetic) is timed separately: it runs once per weight
change, not per forward.  Nothing is fixed in advance for these numbers; the table records them.
usage: infer_table.py [--size 512] [--batch 16] [--iters 10] [--reps 5] [--out profiles/infer_fold_table.md]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402


def timed(fn, iters, reps, warmup):
    """Median over reps of (HIP-event time of iters calls) / iters, in ms."""
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
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("infer_table.py times GPU work: it needs the GPU")
    import fold_ref
    from cvlite.fcos_net import FCOSNet

    keep = os.environ.get("CVL_DISPATCH", "")
    net = FCOSNet(20, device=torch.device("cuda", 0), seed=0)
    fold_ref.randomize_bn(net.backbone.bns(), net.backbone.convs(), seed=1)
    x = torch.rand((args.batch, args.size, args.size, 3), device="cuda") * 2 - 1
    forms = [("plain", dict(), keep),
             ("folded", dict(folded=True), keep),
             ("fallback", dict(folded=True), ",".join(t for t in (keep, "no_res_relu_fuse") if t))]
    rows = []
    for name, kw, env in forms:
        os.environ["CVL_DISPATCH"] = env            # the library reads it at every plan
        fn = lambda: net.forward(x, train=False, **kw)  # noqa: E731
        eager = timed(fn, args.iters, args.reps, args.warmup)
        print("%s: eager %.3f ms per forward" % (name, eager), flush=True)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            fn()
        graph = timed(g.replay, args.iters, args.reps, args.warmup)
        del g
        rows.append((name, eager, graph))
    os.environ["CVL_DISPATCH"] = keep
    fold_ms = timed(net.fold_bn, 1, args.reps, args.warmup)
    dev = torch.cuda.get_device_name(0)
    lines = ["FCOS R50-FPN inference forward, %d x %d, batch %d, %s; HIP events around %d forwards, median of %d passes "
             "after %d warm-up passes." % (args.size, args.size, args.batch, dev, args.iters, args.reps, args.warmup),
             "Command: `python tools/infer_table.py --size %d --batch %d --iters %d --reps %d`"
             % (args.size, args.batch, args.iters, args.reps), "",
             "| form | eager launches, per forward | HIP graph replay, per forward |", "|---|---|---|"]
    what = {"plain": "plain (`train=False`: conv, z, `cvl_bn_apply` per unit)",
            "folded": "folded, conv3 fused (`relu(conv + bias + shortcut)` in the persistent kernel's epilogue)",
            "fallback": "folded, conv3 fallback (`CVL_DISPATCH=no_res_relu_fuse`: beta = 1 launch + `cvl_relu_`)"}
    for name, eager, graph in rows:
        lines.append("| %s | %.3f ms | %.3f ms |" % (what[name], eager, graph))
    p = rows[0]
    lines += ["", "folded / plain: eager %.3f, graph %.3f; fallback / plain: eager %.3f, graph %.3f"
              % (rows[1][1] / p[1], rows[1][2] / p[2], rows[2][1] / p[1], rows[2][2] / p[2]),
              "fold_bn() itself (scale / bias arithmetic + one scaled pack launch over the 52 units, once per "
              "weight change): %.3f ms" % fold_ms]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
