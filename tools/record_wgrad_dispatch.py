"""Records what the weight-gradient dispatch does, for tests/test_wgrad_dispatch_table.py (no GPU)
and tests/test_gpu_wgrad_dispatch.py: tests/data/wgrad_dispatch_table.json.

* "entries": every distinct bf16 conv_wgrad / conv_wgrad_grouped / conv_wgrad_batch call of one
  eager FCOS (512, bs 16), RetinaNet (640, bs 8) and CenterNet hourglass (512, bs 8) step, captured
  by wrapping the ops_nn functions; per CVL_DISPATCH variant the kernel of the call's last launch
  and its workspace size.  A library without the plan query (the revision the table was first
  recorded at) issues each call and reads cvl_conv_igemm_last_kernel; one with it asks the query.
* "sweep" / "sweep_batch": the workspace sizes of synthetic descriptors and batched lists under the
  same variants (host only; slab bytes are nsplit x K x n_store x 4, so equal sizes pin the split
  counts).  --sweep-only records just this half and needs no GPU.
* "bits": SHA-256 of dW of the small cases of tests/wgrad_dispatch_cases.py, one per kernel family.
usage: record_wgrad_dispatch.py [--models fcos,retinanet,centernet] [--sweep-only] [--out FILE]"""
import argparse
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from cvlite import _lib, ops_nn as nn  # noqa: E402
import wgrad_dispatch_cases as wc  # noqa: E402
from record_conv_dispatch import capture as capture_step  # noqa: E402


def capture(model, dev):
    """One eager step of `model`; {key: (descs, ngroups, xs, dys, dw sizes)} of its distinct bf16 calls."""
    orig = (nn.conv_wgrad, nn.conv_wgrad_grouped, nn.conv_wgrad_batch)
    calls = {}

    def rec(kind, descs, ngroups, xs, dys, dws):
        for d, x in zip(descs, xs):
            nn._prec(d, x)
        if any(d.prec != nn.PREC_BF16 for d in descs):
            return
        key = json.dumps([kind, ngroups, [wc.desc_to_list(d) for d in descs]])
        calls.setdefault(key, (kind, descs, ngroups, xs, dys, [t.numel() for t in dws]))

    def wgrad(desc, x, dy, dw, beta=0.0):
        rec("grouped", [desc], 1, [x], [dy], [dw])
        return orig[0](desc, x, dy, dw, beta)

    def grouped(desc, x, dy, dws, beta=0.0):
        rec("grouped", [desc], len(dws), [x], [dy], dws)
        return orig[1](desc, x, dy, dws, beta)

    def batch(descs, xs, dys, dws, beta=0.0):
        if descs:
            rec("batch", list(descs), 1, list(xs), list(dys), list(dws))
        return orig[2](descs, xs, dys, dws, beta)

    _, tr = capture_step(model, dev)          # builds the trainer and runs two steps
    nn.conv_wgrad, nn.conv_wgrad_grouped, nn.conv_wgrad_batch = wgrad, grouped, batch
    try:
        tr.step()
        torch.cuda.synchronize()
    finally:
        nn.conv_wgrad, nn.conv_wgrad_grouped, nn.conv_wgrad_batch = orig
    return calls, tr


def sizes(lib, kind, descs, ngroups):
    if kind == "batch":
        return int(lib.cvl_conv_wgrad_batch_workspace_size(wc.desc_array(descs), len(descs)))
    return int(lib.cvl_conv_wgrad_grouped_workspace_size(ctypes.byref(descs[0]), ngroups))


def last_kernel(lib, has_query, kind, descs, ngroups, xs, dys, dw_sizes):
    if has_query:
        if kind == "batch":
            st, k, l, _ = wc.batch_plan(lib, descs)
            return wc.batch_last_kernel(k, l) if not st else -st
        st, k = wc.plan(lib, descs[0], ngroups)[:2]
        return k if not st else -st
    dws = [torch.zeros(n, dtype=torch.float32, device=xs[0].device) for n in dw_sizes]
    c = dict(kind=kind, descs=descs, ngroups=ngroups, xs=xs, dys=dys, dws=dws)
    st, _, k = wc.run_case(lib, c)
    if st:
        raise RuntimeError("weight-gradient call: status %d" % st)
    return k


def pyramid(B, H, levels, stride):
    """`levels` square maps H, H/2, ... (input side) with their rows back to back: seg rows."""
    out, src, dst = [], 0, 0
    for l in range(levels):
        hs = max(H >> l, 2)
        hr = (hs + stride - 1) // stride
        out.append((hr, hs, src, dst))
        src += B * hs * hs
        dst += B * hr * hr
    return out, src, dst


def sweep_desc(B, H, cin, npad, n_store, k, stride, nseg, ngroups, relu_in):
    segs = []
    src0 = dst0 = 0
    for g in range(ngroups):
        lv, s1, d1 = pyramid(B, H, nseg // ngroups, stride)
        for hr, hs, s, t in lv:
            segs.append([hr, hr, hs, hs, src0 + s, hs * hs, dst0 + t, hr * hr, g])
        src0, dst0 = src0 + s1, dst0 + d1
    return [B, cin, k, k, stride, k // 2, k // 2, npad, n_store, npad, 0, int(relu_in), segs]


def sweep_lists():
    rnd = random.Random(0)
    chans = [(32, 32, 32), (64, 64, 64), (64, 256, 256), (128, 128, 128), (256, 256, 256), (256, 1024, 1024),
             (512, 128, 128), (1024, 256, 256), (2048, 512, 512), (256, 2048, 2048), (128, 32, 20), (256, 32, 20),
             (256, 32, 5), (96, 64, 48)]
    shapes = [(2, 16), (8, 32), (16, 32), (4, 64), (16, 16)]         # rows 512 .. 16384: below and above 1024
    groups = [(1, 1), (1, 1), (2, 1), (2, 2), (3, 3), (4, 2), (4, 4), (5, 1), (5, 5), (10, 2), (6, 3), (3, 1)]
    full = [(B, H, c, kk, g, r) for (B, H) in shapes for c in chans for kk in ((1, 1), (3, 1), (1, 2), (3, 2))
            for g in groups for r in (0, 0, 0, 1)]
    single = [sweep_desc(B, H, c[0], c[1], c[2], kk[0], kk[1], g[0], g[1], r)
              for (B, H, c, kk, g, r) in rnd.sample(full, 300)]
    probs = [(4, 32, 1, 1024, 256, 1), (4, 32, 1, 256, 1024, 1), (4, 64, 2, 512, 1024, 1), (2, 128, 1, 64, 256, 1),
             (2, 128, 1, 64, 64, 1), (8, 16, 1, 2048, 512, 1), (4, 64, 2, 256, 128, 1), (2, 32, 1, 256, 256, 3),
             (4, 16, 1, 512, 512, 3), (2, 64, 1, 128, 128, 3), (2, 128, 1, 64, 64, 3), (2, 16, 2, 256, 256, 3),
             (16, 32, 1, 128, 128, 3), (2, 16, 1, 64, 64, 1), (8, 64, 1, 256, 64, 1)]
    batches = []
    for n in [1, 2, 3, 5, 8, 12, 13, 16, 17, 24, 25, 33, 40] * 3:
        batches.append([sweep_desc(B, H, cin, (cout + 63) // 64 * 64, cout, k, st, 1, 1, 0)
                        for (B, H, st, cin, cout, k) in (rnd.choice(probs) for _ in range(n))])
    return single, batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="fcos,retinanet,centernet")
    ap.add_argument("--sweep-only", action="store_true", help="keep the file's GPU parts, record the sweep again")
    ap.add_argument("--out", default=wc.TABLE)
    args = ap.parse_args()
    lib = _lib.load()
    has_query = hasattr(lib, "cvl_conv_wgrad_plan")
    saved = os.environ.get("CVL_DISPATCH")
    table = {"entries": [], "bits": {}}
    if args.sweep_only and os.path.exists(args.out):
        with open(args.out) as f:
            table = json.load(f)

    def per_variant(fn):
        out = []
        for var in wc.VARIANTS:
            os.environ["CVL_DISPATCH"] = var
            out.append(fn())
        return out

    if not args.sweep_only:
        dev = torch.device("cuda")
        entries = {}
        for model in args.models.split(","):
            calls, tr = capture(model, dev)
            print("%s: %d distinct calls" % (model, len(calls)), flush=True)
            for key, (kind, descs, ng, xs, dys, dwn) in calls.items():
                if key in entries:
                    entries[key]["models"].append(model)
                    continue
                res = per_variant(lambda: [last_kernel(lib, has_query, kind, descs, ng, xs, dys, dwn),
                                           sizes(lib, kind, descs, ng)])
                entries[key] = {"models": [model], "kind": kind, "ngroups": ng,
                                "descs": [wc.desc_to_list(d) for d in descs], "results": res}
            del calls, tr
            torch.cuda.empty_cache()
        table["entries"] = list(entries.values())
        table["bits"] = {}
        for name in sorted(wc.CASES):
            os.environ["CVL_DISPATCH"] = wc.CASES[name][0]
            c = wc.make_case(name, dev)
            st, nb, k = wc.run_case(lib, c)
            if st:
                raise RuntimeError("case %s: status %d" % (name, st))
            table["bits"][name] = {"kernel": k, "workspace": nb, "sha256": wc.sha(c["dws"])}
            print("case %s: kernel %d, %d bytes" % (name, k, nb), flush=True)
    single, batches = sweep_lists()
    table["sweep"] = [{"ngroups": max(s[8] for s in v[-1]) + 1, "desc": v,
                       "sizes": per_variant(lambda: sizes(lib, "grouped", [wc.desc_from_list(v)],
                                                          max(s[8] for s in v[-1]) + 1))} for v in single]
    table["sweep_batch"] = []
    for b in batches:
        descs = [wc.desc_from_list(v) for v in b]
        table["sweep_batch"].append({"descs": b, "sizes": per_variant(lambda: sizes(lib, "batch", descs, 1))})
    if saved is None:
        os.environ.pop("CVL_DISPATCH", None)
    else:
        os.environ["CVL_DISPATCH"] = saved
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("{\n")
        f.write(' "variants": %s,\n "desc_columns": %s,\n "seg_columns": %s,\n "results_columns": %s,\n' % (
            json.dumps(wc.VARIANTS), json.dumps(wc.DESC_FIELDS + ["seg"]), json.dumps(wc.SEG_FIELDS),
            json.dumps(["kernel of the last launch", "workspace_size"])))
        f.write(' "bits": %s,\n' % json.dumps(table["bits"]))
        for k in ("entries", "sweep", "sweep_batch"):
            f.write(' "%s": [\n%s\n ]%s\n' % (k, ",\n".join("  " + json.dumps(e, separators=(",", ":"))
                                                           for e in table[k]), "" if k == "sweep_batch" else ","))
        f.write("}\n")
    print("wrote %s: %d entries, %d + %d sweep rows x %d variants" % (
        args.out, len(table["entries"]), len(single), len(batches), len(wc.VARIANTS)), flush=True)


if __name__ == "__main__":
    main()
