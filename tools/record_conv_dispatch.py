"""Records which kernel the forward / data-gradient conv dispatch picks for every distinct launch
of one FCOS step (512, bs 16), one RetinaNet step (640, bs 8) and one CenterNet hourglass step
(512, bs 8), under every CVL_DISPATCH variant the conv tests use, with and without a workspace:
tests/data/conv_dispatch_table.json, which tests/test_conv_dispatch_table.py checks against the
host-only plan query (cvl_conv_igemm_plan) without a GPU.

The launches are captured during one eager step (ops_nn.conv_igemm / conv_igemm_relu_mask /
conv_igemm_dgrad_bnsum / _res; the descriptors of the two BN-sums entries are recorded as the plain
data gradient they fall back to).  A library without the plan query (the revision the table was
first recorded at) issues each call once on the step's own tensors and reads
cvl_conv_igemm_last_kernel / _last_ktile; one with it asks the query and needs the GPU only for the
capture.  The two fused BN-sums forms are recorded at their smallest shapes through *fused and
last_kernel ("fused" in the table; tests/test_gpu_conv_dispatch.py repeats them).
usage: record_conv_dispatch.py [--models fcos,retinanet,centernet] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd")]
import torch  # noqa: E402

from cvlite import _lib, ops_nn as nn  # noqa: E402

# every dispatch string of tests/test_gpu_conv*.py that reaches the forward / data-gradient dispatch
VARIANTS = ["", "no_p", "no_x", "no_h", "no_l", "no_256", "p_bn=64", "p_bn=128", "p_bn=256", "p_k64=0",
            "p_wide128=0", "w256_min_k=0", "l_min_tiles=1", "l256_min_tiles=1", "l_min_tiles=1,l256_min_tiles=1,no_h",
            "no_h,no_256,l_min_tiles=1", "h_no_n32", "h_no_3stage", "h_no_wres", "h_no_sw", "l_no_sw", "x_no_sw",
            "no_h32", "x_cin32=0", "no_s2dg3", "s2dg3_min_rows=1", "ksplit_min_nk=8", "base_bk128=0"]

DESC_FIELDS = ["mode", "B", "Cin", "KH", "KW", "stride", "pad_t", "pad_l", "Npad", "n_store", "ld_dst", "dst_coff",
               "dst_f32", "relu_out", "relu_in", "beta", "nseg", "prec"]
SEG_FIELDS = ["Hr", "Wr", "Hs", "Ws", "src_base", "src_img", "dst_base", "dst_img"]


def desc_to_dict(d):
    out = {f: getattr(d, f) for f in DESC_FIELDS}
    out["seg"] = [[getattr(d.seg[i], f) for f in SEG_FIELDS] + [int(bool(d.seg[i].bias))] for i in range(d.nseg)]
    return out


def capture(model, dev):
    """One eager step of `model`; returns {key: (entry, desc, src, dst, extra)} of its distinct launches."""
    if model == "retinanet":
        from cvlite.retinanet import RetinaNet
        from cvlite.train_retinanet import RetinaTrainer, synthetic_coco_batch
        rn = RetinaNet(80, {}, anchor_sizes=[20.0, 40.0, 80.0, 160.0, 320.0])
        tr = RetinaTrainer(rn.model, rn, 8, 640, n_max=50, use_graph=False)
        tr.load_candidates(*synthetic_coco_batch(24, 640, 80, n_max=50, seed=4321, device=dev))
    elif model == "centernet":
        from cvlite.hourglass_net import HourglassNet
        from cvlite.train_centernet import CenterNetTrainer, synthetic_batch as cn_batch
        net = HourglassNet(20, device=dev, seed=0)
        tr = CenterNetTrainer(net, 8, (512, 512), sub_batch_sz=2, n_max=16, use_graph=False)
        tr.load_batch(*cn_batch(8, 512, 512, 20, n_max=16, seed=777, device=dev))
    else:
        from cvlite.fcos_net import FCOSNet
        from cvlite.train_fcos import FCOSTrainer, synthetic_batch
        net = FCOSNet(20, device=dev, seed=0)
        tr = FCOSTrainer(net, 16, (512, 512), use_graph=False)
        tr.load_batch(*synthetic_batch(16, 512, 512, 20, seed=1234, device="cuda"))
    tr.step()
    torch.cuda.synchronize()
    calls = {}
    orig = (nn.conv_igemm, nn.conv_igemm_relu_mask, nn.conv_igemm_dgrad_bnsum, nn.conv_igemm_dgrad_bnsum_res)

    def rec(entry, desc, src, dst, extra):
        nn._prec(desc, src)
        if desc.prec != nn.PREC_BF16:
            return
        stats = int(entry == "igemm" and extra is not None)
        key = json.dumps([entry, stats, desc_to_dict(desc)])
        calls.setdefault(key, (entry, desc, src, dst, extra))

    def igemm(desc, src, dst, stats=None):
        rec("igemm", desc, src, dst, stats)
        return orig[0](desc, src, dst, stats)

    def relu_mask(desc, src, dst, y):
        rec("relu_mask", desc, src, dst, y)
        return orig[1](desc, src, dst, y)

    def bnsum(desc, src, dst, *a, **kw):
        rec("igemm", desc, src, dst, None)
        return orig[2](desc, src, dst, *a, **kw)

    def bnsum_res(desc, src, dst, *a, **kw):
        rec("igemm", desc, src, dst, None)
        return orig[3](desc, src, dst, *a, **kw)

    nn.conv_igemm, nn.conv_igemm_relu_mask, nn.conv_igemm_dgrad_bnsum, nn.conv_igemm_dgrad_bnsum_res = (
        igemm, relu_mask, bnsum, bnsum_res)
    try:
        tr.step()
        torch.cuda.synchronize()
    finally:
        nn.conv_igemm, nn.conv_igemm_relu_mask, nn.conv_igemm_dgrad_bnsum, nn.conv_igemm_dgrad_bnsum_res = orig
    return calls, tr


def query(lib, desc, stats, nbytes):
    k, t = ctypes.c_int32(0), ctypes.c_int32(0)
    st = lib.cvl_conv_igemm_plan(ctypes.byref(desc), stats, nbytes, ctypes.byref(k), ctypes.byref(t))
    if st:
        raise RuntimeError("cvl_conv_igemm_plan: status %d" % st)
    return k.value, t.value


def issue(lib, entry, desc, src, dst, extra, nbytes):
    """The call itself, once; returns (kernel, ktile) of its launch."""
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device) if nbytes else None
    if entry == "relu_mask":
        st = lib.cvl_conv_igemm_relu_mask(ctypes.byref(desc), _lib.ptr(src), _lib.ptr(dst), _lib.ptr(extra),
                                          _lib.ptr(ws), nbytes, _lib.stream())
    else:
        st = lib.cvl_conv_igemm(ctypes.byref(desc), _lib.ptr(src), _lib.ptr(dst), nn.acc_ptr(extra), _lib.ptr(ws),
                                nbytes, _lib.stream())
    if st >= 1000:
        raise RuntimeError("hipError %d" % (st - 1000))
    return lib.cvl_conv_igemm_last_kernel(), lib.cvl_conv_igemm_last_ktile()


def fused_cases(dev):
    """The two fused BN-sums forms at the smallest shape each accepts: (form, run() -> fused flag)."""
    bf = torch.bfloat16
    B, H, C = 1, 16, 64
    z = torch.zeros((B, H, H, C), dtype=bf, device=dev)
    y = torch.ones((B, H, H, C), dtype=bf, device=dev)
    dy = torch.zeros((B, H, H, C), dtype=bf, device=dev)
    mr = torch.ones((B, C, 2), dtype=torch.float32, device=dev)
    ga = torch.ones(C, dtype=torch.float32, device=dev)
    be = torch.zeros(C, dtype=torch.float32, device=dev)
    w3 = torch.zeros((C, 9 * C), dtype=bf, device=dev)
    w1 = torch.zeros((C, C), dtype=bf, device=dev)
    d3 = nn.make_desc(nn.DGRAD, B, C, 3, 3, 1, 1, 1, C, C, C, [nn.seg(H, H, H, H, w3)])
    d1 = nn.make_desc(nn.DGRAD, B, C, 1, 1, 1, 0, 0, C, C, C, [nn.seg(H, H, H, H, w1)], beta=1.0)

    def run_z():
        dx = torch.zeros((B, H, H, C), dtype=bf, device=dev)
        return nn.conv_igemm_dgrad_bnsum(d3, dy, dx, z, mr, ga, be, nn.bn_acc(B, C, dev))

    def run_y():
        dx = torch.zeros((B, H, H, C), dtype=bf, device=dev)
        return nn.conv_igemm_dgrad_bnsum_res(d1, dy, dx, y, z, mr, ga, be, nn.bn_acc(B, C, dev))

    return [("z_mask", run_z), ("y_mask", run_y)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="fcos,retinanet,centernet")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "data", "conv_dispatch_table.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    lib = _lib.load()
    has_query = hasattr(lib, "cvl_conv_igemm_plan")
    saved = os.environ.get("CVL_DISPATCH")
    entries = {}
    for model in args.models.split(","):
        calls, tr = capture(model, dev)
        print("%s: %d distinct launches" % (model, len(calls)), flush=True)
        for key, (entry, desc, src, dst, extra) in calls.items():
            if key in entries:
                entries[key]["models"].append(model)
                continue
            stats = int(entry == "igemm" and extra is not None)
            results = []
            for var in VARIANTS:
                os.environ["CVL_DISPATCH"] = var
                n = int(lib.cvl_conv_igemm_workspace_size(ctypes.byref(desc)))
                row = []
                for nbytes in (n if n > 16 else 0, 0):
                    row += list(query(lib, desc, stats, nbytes) if has_query
                                else issue(lib, entry, desc, src, dst, extra, nbytes))
                results.append(row + [n])
            torch.cuda.synchronize()
            entries[key] = {"models": [model], "entry": entry, "stats": stats, "desc": desc_to_dict(desc),
                            "results": results}
        if saved is None:
            os.environ.pop("CVL_DISPATCH", None)
        else:
            os.environ["CVL_DISPATCH"] = saved
        del calls, tr
        torch.cuda.empty_cache()
    fused = []
    for form, run in fused_cases(dev):
        flag = bool(run())
        fused.append({"form": form, "fused": int(flag), "kernel": lib.cvl_conv_igemm_last_kernel()})
    torch.cuda.synchronize()
    table = {"variants": VARIANTS,
             "results_columns": ["kernel (workspace)", "ktile (workspace)", "kernel (none)", "ktile (none)",
                                 "workspace_size"],
             "seg_columns": SEG_FIELDS + ["has_bias"],
             "entries": list(entries.values()), "fused": fused}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("{\n")
        for k in ("variants", "results_columns", "seg_columns", "fused"):
            f.write(" %s: %s,\n" % (json.dumps(k), json.dumps(table[k])))
        f.write(' "entries": [\n%s\n ]\n}\n' % ",\n".join("  " + json.dumps(e) for e in table["entries"]))
    print("wrote %s: %d entries x %d variants" % (args.out, len(entries), len(VARIANTS)), flush=True)


if __name__ == "__main__":
    main()
