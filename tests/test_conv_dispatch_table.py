"""The forward / data-gradient conv dispatch against its recorded table (no GPU, no launch).

tests/data/conv_dispatch_table.json (tools/record_conv_dispatch.py) holds, for every distinct
forward / data-gradient launch of one FCOS (512, bs 16), RetinaNet (640, bs 8) and CenterNet
hourglass (512, bs 8) step, under every CVL_DISPATCH variant the conv tests use, with and without a
workspace: the kernel family and K-tile depth the launch ran (cvl_conv_igemm_last_kernel / _ktile
after the real call, recorded before the launch planner existed) and cvl_conv_igemm_workspace_size.
The host-only plan query must give the same answers for every entry."""
import ctypes
import json
import os

from cvlite import _lib, ops_nn as nn

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "conv_dispatch_table.json")
DUMMY = 16      # a non-null weight / bias address: the planner never dereferences it


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def desc_from_dict(e):
    d = nn.ConvDesc()
    for k, v in e.items():
        if k != "seg":
            setattr(d, k, v)
    for i, s in enumerate(e["seg"]):
        q = d.seg[i]
        q.Hr, q.Wr, q.Hs, q.Ws, q.src_base, q.src_img, q.dst_base, q.dst_img = s[:8]
        q.w = DUMMY
        q.bias = DUMMY if s[8] else None
    return d


def plan(lib, d, stats, nbytes):
    k, t = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert lib.cvl_conv_igemm_plan(ctypes.byref(d), stats, nbytes, ctypes.byref(k), ctypes.byref(t)) == 0
    return [k.value, t.value]


def test_plan_matches_recorded_dispatch(monkeypatch):
    table = load_table()
    lib = _lib.load()
    assert len(table["entries"]) >= 100 and len(table["variants"]) >= 20
    bad = []
    for n, e in enumerate(table["entries"]):
        d = desc_from_dict(e["desc"])
        assert len(e["results"]) == len(table["variants"])
        for var, rec in zip(table["variants"], e["results"]):
            monkeypatch.setenv("CVL_DISPATCH", var)
            size = int(lib.cvl_conv_igemm_workspace_size(ctypes.byref(d)))
            got = plan(lib, d, e["stats"], size if size > 16 else 0) + plan(lib, d, e["stats"], 0) + [size]
            if got != rec:
                bad.append((n, e["models"], var, rec, got))
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(table["entries"]) * len(table["variants"]), bad[:5])


def test_plan_rejects_what_the_call_rejects():
    lib = _lib.load()
    d = desc_from_dict(load_table()["entries"][0]["desc"])
    d.Cin = 24                                   # not a multiple of 32 channels
    k, t = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert lib.cvl_conv_igemm_plan(ctypes.byref(d), 0, 0, ctypes.byref(k), ctypes.byref(t)) == 1
    assert k.value == 0 and t.value == 0
