"""GPU side of the weight-gradient launch planner (conv_wgrad_dispatch.hip): one small bf16 call per
kernel family (tests/wgrad_dispatch_cases.py).  What cvl_conv_wgrad_plan / _batch_plan report is
what the call launches (cvl_conv_igemm_last_kernel), the workspace the size function reports is
enough (the call returns 0 with exactly that many bytes), and dW is bit for bit what the revision
before the planner wrote (SHA-256 in tests/data/wgrad_dispatch_table.json, inputs from a CPU
generator)."""
import ctypes
import json

import pytest
import torch

import wgrad_dispatch_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(wc.TABLE) as f:
        return json.load(f)["bits"]


@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_plan_equals_launch_and_bits(name, dispatch, recorded):
    from cvlite import _lib
    hooks, family = wc.CASES[name]
    if hooks:
        dispatch(*hooks.split(","))
    lib = _lib.load()
    c = wc.make_case(name)
    if c["kind"] == "batch":
        st, kern, launch, nsplit = wc.batch_plan(lib, c["descs"])
        assert st == 0
        # one 256-wide X launch, one 128-wide X launch, one WH launch, one call of its own, in launch order
        assert kern == [wc.WG_X, wc.WG_X, wc.WG_H, wc.WG_S] and launch == [1, 2, 0, 3]
        planned = wc.batch_last_kernel(kern, launch)
    else:
        st, planned, tile, nsplit, nbytes = wc.plan(lib, c["descs"][0], c["ngroups"])
        assert st == 0
        assert nbytes == int(lib.cvl_conv_wgrad_grouped_workspace_size(ctypes.byref(c["descs"][0]), c["ngroups"]))
    st, nb, launched = wc.run_case(lib, c)
    print("case", name, "plan", planned, "launch", launched, "workspace", nb, "nsplit", nsplit)
    assert st == 0
    assert launched == planned
    assert planned == family if family is not None else planned in (wc.WG_L128, wc.WG_L256)
    assert (planned, nb) == (recorded[name]["kernel"], recorded[name]["workspace"])
    assert wc.sha(c["dws"]) == recorded[name]["sha256"]


def test_per_group_fallback_runs_x_on_every_group():
    """3 groups are more than one X launch covers: each group runs as its own call, every one on X, and
    writes what a one-group call on that group's segments writes."""
    from cvlite import _lib, ops_nn as nn
    lib = _lib.load()
    c = wc.make_case("per_group")
    d = c["descs"][0]
    assert wc.run_case(lib, c)[0] == 0
    for g in range(c["ngroups"]):
        gd = wc.group_desc(d, c["ngroups"], g)
        st, kern, tile, nsplit, nbytes = wc.plan(lib, gd, 1)
        assert (st, kern, tile) == (0, wc.WG_X, 128)
        dw = torch.zeros_like(c["dws"][g])
        nn.conv_wgrad(gd, c["xs"][0], c["dys"][0], dw)
        torch.cuda.synchronize()
        assert lib.cvl_conv_igemm_last_kernel() == wc.WG_X
        assert torch.equal(dw, c["dws"][g])
