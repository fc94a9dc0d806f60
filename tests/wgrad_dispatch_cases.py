"""Shared by tools/record_wgrad_dispatch.py and the two weight-gradient dispatch tests: the table's
descriptor encoding, the plan queries, and the small bf16 cases (one per kernel family) whose dW
bits the table records.  Importing it needs no GPU."""
import ctypes
import hashlib
import os

import torch

from cvlite import ops_nn as nn

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "wgrad_dispatch_table.json")
DUMMY = 16      # a non-null weight address: the planner never dereferences it
BF = torch.bfloat16
# CVL_CK_WG_* (include/cvlite.h)
WG_S, WG_L128, WG_L256, WG_X, WG_SN, WG_H = 8, 9, 10, 11, 13, 15
WG_CODES = (WG_S, WG_L128, WG_L256, WG_X, WG_SN, WG_H)

# the CVL_DISPATCH strings the table is recorded under
VARIANTS = ["", "wg_no_x", "wg_no_l", "wg_no_x,wg_no_l", "wg_no_h", "wg_no_h,wg_no_x", "wg_no_pf",
            "wgb_no_h,wgb_no_256"]

DESC_FIELDS = ["B", "Cin", "KH", "KW", "stride", "pad_t", "pad_l", "Npad", "n_store", "ld_dst", "dst_coff", "relu_in"]
SEG_FIELDS = ["Hr", "Wr", "Hs", "Ws", "src_base", "src_img", "dst_base", "dst_img", "w"]


def desc_to_list(d):
    """A bf16 forward descriptor as [fields..., [segments]]; a segment's last entry numbers its weight
    tensor within the descriptor (the segments of a group share one)."""
    ws = []
    segs = []
    for i in range(d.nseg):
        q = d.seg[i]
        if q.w not in ws:
            ws.append(q.w)
        segs.append([getattr(q, f) for f in SEG_FIELDS[:-1]] + [ws.index(q.w)])
    return [getattr(d, f) for f in DESC_FIELDS] + [segs]


def desc_from_list(v):
    d = nn.ConvDesc()
    d.mode, d.prec = nn.FWD, nn.PREC_BF16
    for f, x in zip(DESC_FIELDS, v):
        setattr(d, f, x)
    d.nseg = len(v[-1])
    for i, s in enumerate(v[-1]):
        q = d.seg[i]
        q.Hr, q.Wr, q.Hs, q.Ws, q.src_base, q.src_img, q.dst_base, q.dst_img = s[:8]
        q.w = DUMMY + 16 * s[8]
    return d


def desc_array(descs):
    return (ctypes.c_void_p * len(descs))(*[ctypes.addressof(d) for d in descs])


def plan(lib, d, ngroups):
    """cvl_conv_wgrad_plan: (status, kernel, tile, nsplit, workspace) of the call's last launch."""
    k, t, s, w = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_size_t(0)
    st = lib.cvl_conv_wgrad_plan(ctypes.byref(d), ngroups, ctypes.byref(k), ctypes.byref(t), ctypes.byref(s),
                                 ctypes.byref(w))
    return st, k.value, t.value, s.value, w.value


def batch_plan(lib, descs):
    """cvl_conv_wgrad_batch_plan: (status, kernel_of, launch_of, nsplit_of), one entry per problem."""
    n = len(descs)
    k, l, s = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
    st = lib.cvl_conv_wgrad_batch_plan(desc_array(descs), n, k, l, s)
    return st, list(k), list(l), list(s)


def batch_last_kernel(kernel_of, launch_of):
    """What cvl_conv_igemm_last_kernel shows after the batched call: the kernel of its last launch."""
    return kernel_of[max(range(len(launch_of)), key=lambda i: launch_of[i])]


def sha(ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# ---- the small cases --------------------------------------------------------------------------------
# name -> (CVL_DISPATCH hooks, family the last launch runs).  The S shape is WH's own (B 2, 16x16,
# 64 -> 64, 3x3 stride 1), which WH takes first, so S runs it with wg_no_h.
CASES = {
    "s": ("wg_no_h", WG_S),
    "l": ("wg_no_x,wg_no_h", None),          # L128 or L256, as the split model decides
    "x128": ("", WG_X),
    "x_pair": ("wg_no_h", WG_X),
    "wh": ("", WG_H),
    "sn": ("", WG_SN),
    "per_group": ("", WG_X),
    "batch": ("", WG_S),                     # the last launch: the individual 3x3 stride-2 problem
}


def _rand(gen, shape, dev):
    return (torch.randn(shape, generator=gen) * 0.5).to(BF).to(dev)


def _multi(gen, dev, B, maps, ngroups, cin, npad, n_store, k, per_segment_w=False):
    """`ngroups` groups of the levels `maps` (square), rows of all segments back to back in x / dy."""
    segs, rows, ws = [], 0, []
    for g in range(ngroups):
        for h in maps:
            if per_segment_w or not ws or len(segs) % len(maps) == 0:
                ws.append(torch.zeros((npad, k * k * cin), dtype=BF, device=dev))
            segs.append(nn.seg(h, h, h, h, ws[-1], None, src_base=rows, dst_base=rows))
            rows += B * h * h
    d = nn.make_desc(nn.FWD, B, cin, k, k, 1, k // 2, k // 2, npad, n_store, npad, segs)
    x = _rand(gen, (rows, cin), dev)
    dy = _rand(gen, (rows, npad), dev)
    return d, x, dy


def make_case(name, dev="cuda"):
    """dict(kind, descs, ngroups, xs, dys, dws): inputs from a CPU generator, dW zeroed."""
    gen = torch.Generator(device="cpu").manual_seed(20 + sorted(CASES).index(name))
    f32 = torch.float32

    def single(B, H, cin, cout, k, stride=1):
        Ho = (H + stride - 1) // stride
        npad = (cout + 63) // 64 * 64
        w = torch.zeros((npad, k * k * cin), dtype=BF, device=dev)
        d = nn.make_desc(nn.FWD, B, cin, k, k, stride, k // 2, k // 2, npad, cout, cout, [nn.seg(Ho, Ho, H, H, w)])
        return d, _rand(gen, (B, H, H, cin), dev), _rand(gen, (B, Ho, Ho, cout), dev)

    if name == "batch":
        import test_gpu_wgrad_batch as wb
        probs = [wb.PROBLEMS[i] for i in (0, 4, 8, len(wb.PROBLEMS) - 1)]
        descs, xs, dys, dws = [], [], [], []
        for p in probs:
            k = p[5] if len(p) > 5 else 1
            d, x, dy = single(2, p[1], p[3], p[4], k, p[2])
            descs.append(d), xs.append(x), dys.append(dy)
            dws.append(torch.zeros(k * k * p[3] * p[4], dtype=f32, device=dev))
        return dict(kind="batch", descs=descs, ngroups=1, xs=xs, dys=dys, dws=dws)
    if name in ("s", "wh"):
        d, x, dy = single(2, 16, 64, 64, 3)
    elif name == "l":
        d, x, dy = single(4, 16, 64, 256, 3)
    elif name == "x128":
        d, x, dy = single(4, 16, 64, 64, 1)
    elif name == "x_pair":
        d, x, dy = _multi(gen, dev, 4, [16, 8], 2, 64, 256, 256, 3)
    elif name == "sn":
        d, x, dy = _multi(gen, dev, 4, [16, 8], 1, 128, 32, 20, 3, per_segment_w=True)
    elif name == "per_group":
        d, x, dy = _multi(gen, dev, 4, [16], 3, 64, 64, 64, 1)
    else:
        raise KeyError(name)
    ngroups = {"x_pair": 2, "sn": 2, "per_group": 3}.get(name, 1)
    dws = [torch.zeros(d.KH * d.KW * d.Cin * d.n_store, dtype=f32, device=dev) for _ in range(ngroups)]
    return dict(kind="grouped", descs=[d], ngroups=ngroups, xs=[x], dys=[dy], dws=dws)


def group_desc(d, ngroups, g):
    """Group g of a grouped descriptor as a one-group descriptor (what the per-group fallback runs)."""
    s = nn.ConvDesc()
    ctypes.memmove(ctypes.addressof(s), ctypes.addressof(d), ctypes.sizeof(d))
    spg = d.nseg // ngroups
    s.nseg = spg
    for i in range(spg):
        ctypes.memmove(ctypes.addressof(s.seg[i]), ctypes.addressof(d.seg[g * spg + i]), ctypes.sizeof(nn.ConvSeg))
    return s


def run_case(lib, c):
    """Issues the case's call with exactly the workspace its size function reports; returns
    (status, workspace bytes, last kernel)."""
    from cvlite import _lib
    vp = ctypes.c_void_p
    if c["kind"] == "batch":
        n = len(c["descs"])
        darr = desc_array(c["descs"])
        nb = int(lib.cvl_conv_wgrad_batch_workspace_size(darr, n))
        ws = torch.empty(nb, dtype=torch.uint8, device=c["xs"][0].device)
        st = lib.cvl_conv_wgrad_batch(darr, n, (vp * n)(*[t.data_ptr() for t in c["xs"]]),
                                      (vp * n)(*[t.data_ptr() for t in c["dys"]]),
                                      (vp * n)(*[t.data_ptr() for t in c["dws"]]), 0.0, _lib.ptr(ws), nb, _lib.stream())
    else:
        d, ng = c["descs"][0], c["ngroups"]
        nb = int(lib.cvl_conv_wgrad_grouped_workspace_size(ctypes.byref(d), ng))
        ws = torch.empty(nb, dtype=torch.uint8, device=c["xs"][0].device)
        st = lib.cvl_conv_wgrad_grouped(ctypes.byref(d), ng, _lib.ptr(c["xs"][0]), _lib.ptr(c["dys"][0]),
                                        (vp * ng)(*[t.data_ptr() for t in c["dws"]]), 0.0, _lib.ptr(ws), nb,
                                        _lib.stream())
    torch.cuda.synchronize()
    return st, nb, lib.cvl_conv_igemm_last_kernel()
