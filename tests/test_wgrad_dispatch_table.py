"""The weight-gradient dispatch against its recorded table (no GPU, no launch).

tests/data/wgrad_dispatch_table.json (tools/record_wgrad_dispatch.py) holds, under every
CVL_DISPATCH variant of the weight-gradient families, (a) for every distinct conv_wgrad /
conv_wgrad_grouped / conv_wgrad_batch call of one FCOS (512, bs 16), RetinaNet (640, bs 8) and
CenterNet hourglass (512, bs 8) step the kernel of the call's last launch
(cvl_conv_igemm_last_kernel after the real call) and its workspace size, and (b) the workspace
sizes of a few hundred synthetic descriptors and batched lists -- slab bytes are nsplit x K x
n_store x 4, so equal sizes pin the split counts -- all recorded before the launch planner
(conv_wgrad_dispatch.hip) existed.  The host-only plan queries and the size functions must give
the same answers."""
import ctypes
import json

import wgrad_dispatch_cases as wc
from cvlite import _lib


def load_table():
    with open(wc.TABLE) as f:
        return json.load(f)


def answers(lib, kind, descs, ngroups):
    """[kernel of the last launch, workspace size] from the plan queries and the size functions."""
    if kind == "batch":
        st, kern, launch, _ = wc.batch_plan(lib, descs)
        assert st == 0
        return [wc.batch_last_kernel(kern, launch),
                int(lib.cvl_conv_wgrad_batch_workspace_size(wc.desc_array(descs), len(descs)))]
    st, kern, _, _, nbytes = wc.plan(lib, descs[0], ngroups)
    assert st == 0
    size = int(lib.cvl_conv_wgrad_grouped_workspace_size(ctypes.byref(descs[0]), ngroups))
    assert nbytes == size
    return [kern, size]


def test_plan_matches_recorded_dispatch(monkeypatch):
    table = load_table()
    lib = _lib.load()
    assert table["variants"] == wc.VARIANTS
    models, codes = set(), set()
    for e in table["entries"]:
        models.update(e["models"])
        codes.update(r[0] for r in e["results"])
    assert models == {"fcos", "retinanet", "centernet"}
    assert codes == set(wc.WG_CODES)
    bad = []
    for n, e in enumerate(table["entries"]):
        descs = [wc.desc_from_list(v) for v in e["descs"]]
        assert len(e["results"]) == len(wc.VARIANTS)
        for var, rec in zip(wc.VARIANTS, e["results"]):
            monkeypatch.setenv("CVL_DISPATCH", var)
            got = answers(lib, e["kind"], descs, e["ngroups"])
            if got != rec:
                bad.append((n, e["models"], e["kind"], var, rec, got))
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(table["entries"]) * len(wc.VARIANTS), bad[:5])


def test_sizes_match_recorded_sweep(monkeypatch):
    table = load_table()
    lib = _lib.load()
    assert len(table["sweep"]) >= 200 and len(table["sweep_batch"]) >= 30
    assert any(e["ngroups"] >= 3 for e in table["sweep"])          # the per-group fallback is in it
    bad = []
    for n, e in enumerate(table["sweep"]):
        d = wc.desc_from_list(e["desc"])
        for var, rec in zip(wc.VARIANTS, e["sizes"]):
            monkeypatch.setenv("CVL_DISPATCH", var)
            got = answers(lib, "grouped", [d], e["ngroups"])[1]
            if got != rec:
                bad.append((n, var, rec, got))
    for n, e in enumerate(table["sweep_batch"]):
        descs = [wc.desc_from_list(v) for v in e["descs"]]
        for var, rec in zip(wc.VARIANTS, e["sizes"]):
            monkeypatch.setenv("CVL_DISPATCH", var)
            got = answers(lib, "batch", descs, 1)[1]
            if got != rec:
                bad.append(("batch", n, var, rec, got))
    assert not bad, "%d differ, first: %r" % (len(bad), bad[:5])


def test_plan_rejects_what_the_call_rejects():
    lib = _lib.load()
    v = next(e for e in load_table()["entries"] if e["kind"] == "grouped" and e["ngroups"] == 2)["descs"][0]

    def status(ngroups=2, **fields):
        d = wc.desc_from_list(v)
        for k, x in fields.items():
            setattr(d, k, x)
        st, kern, tile, nsplit, nbytes = wc.plan(lib, d, ngroups)
        assert st == 0 or (kern, tile, nsplit, nbytes) == (0, 0, 0, 0)
        return st

    assert status() == 0
    assert status(Cin=12) == 1                       # not a multiple of 8 channels
    assert status(ld_dst=v[wc.DESC_FIELDS.index("ld_dst")] + 4) == 1      # ld_dst % 8 != 0
    assert status(ngroups=3) == 1                    # nseg % ngroups != 0
    d = wc.desc_from_list(v)
    d.prec = 1                                       # fp32 parity mode: its own kernels
    assert wc.plan(lib, d, 2)[:2] == (0, 0)
