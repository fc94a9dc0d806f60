"""GPU side of the conv launch planner (conv_dispatch.hip): what cvl_conv_igemm_plan reports is what a
real call launches, the two fused BN-sums entries still fuse as recorded, and the ReLU-mask entry
rejects a call it cannot serve before it writes anything."""
import ctypes
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "conv_dispatch_table.json")
# CVL_CK_* (include/cvlite.h)
BASE, BASE_SPLITK, L64, L128, L256, X32, H64, P = 1, 2, 3, 4, 5, 7, 14, 16

# family -> (B, H, Cin, Cout, k, dispatch hooks, workspace): one small launch per family, the shapes
# and hooks of test_gpu_conv.py / test_gpu_conv_h.py.  L128 alone cannot be small: below 256
# 128-wide tiles (65,536 rows) the planner always halves the tile to 64 columns.
FAMILIES = {
    BASE: (2, 16, 64, 64, 3, ["no_l"], False),
    BASE_SPLITK: (2, 16, 64, 64, 3, ["no_l"], True),
    L64: (2, 16, 64, 64, 3, ["no_h", "l_min_tiles=1", "no_256"], True),
    L128: (16, 64, 64, 128, 1, ["no_p", "no_h"], True),
    L256: (2, 16, 64, 256, 3, ["no_h", "l_min_tiles=1", "l256_min_tiles=1", "no_x"], True),
    X32: (2, 16, 64, 256, 3, ["no_h", "l_min_tiles=1", "l256_min_tiles=1"], True),
    H64: (2, 16, 64, 64, 3, [], True),
    P: (2, 16, 64, 128, 1, [], True),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_plan_equals_launch(family, dispatch):
    from cvlite import _lib, ops_nn as nn
    B, H, Cin, Cout, k, hooks, with_ws = FAMILIES[family]
    if hooks:
        dispatch(*hooks)
    lib = _lib.load()
    x = torch.zeros((B, H, H, Cin), dtype=BF, device="cuda")
    w = torch.zeros((Cout, k * k * Cin), dtype=BF, device="cuda")
    out = torch.zeros((B, H, H, Cout), dtype=BF, device="cuda")
    d = nn.make_desc(nn.FWD, B, Cin, k, k, 1, k // 2, k // 2, Cout, Cout, Cout, [nn.seg(H, H, H, H, w)])
    n = int(lib.cvl_conv_igemm_workspace_size(ctypes.byref(d))) if with_ws else 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda") if n > 16 else None
    nbytes = n if ws is not None else 0
    kern, ktile = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert lib.cvl_conv_igemm_plan(ctypes.byref(d), 0, nbytes, ctypes.byref(kern), ctypes.byref(ktile)) == 0
    _lib.call("cvl_conv_igemm", ctypes.byref(d), _lib.ptr(x), _lib.ptr(out), None, _lib.ptr(ws), nbytes, _lib.stream())
    torch.cuda.synchronize()
    print("family", family, "plan", kern.value, ktile.value, "launch", lib.cvl_conv_igemm_last_kernel(),
          lib.cvl_conv_igemm_last_ktile())
    assert (lib.cvl_conv_igemm_last_kernel(), lib.cvl_conv_igemm_last_ktile()) == (kern.value, ktile.value)
    assert kern.value == family


def test_fused_bnsum_entries_as_recorded():
    """The z-mask form (3x3, one 16x16 image, 64 channels) and the y-mask form (1x1 64 -> 64 with the
    beta accumulate) against the record of the revision before the planner: both fuse, on the same
    kernel."""
    from cvlite import _lib, ops_nn as nn
    with open(TABLE) as f:
        recorded = {e["form"]: e for e in json.load(f)["fused"]}
    lib = _lib.load()
    B, H, C = 1, 16, 64
    z = torch.zeros((B, H, H, C), dtype=BF, device="cuda")
    y = torch.ones((B, H, H, C), dtype=BF, device="cuda")
    dy = torch.zeros((B, H, H, C), dtype=BF, device="cuda")
    mr = torch.ones((B, C, 2), dtype=torch.float32, device="cuda")
    ga = torch.ones(C, dtype=torch.float32, device="cuda")
    be = torch.zeros(C, dtype=torch.float32, device="cuda")
    w3 = torch.zeros((C, 9 * C), dtype=BF, device="cuda")
    w1 = torch.zeros((C, C), dtype=BF, device="cuda")
    d3 = nn.make_desc(nn.DGRAD, B, C, 3, 3, 1, 1, 1, C, C, C, [nn.seg(H, H, H, H, w3)])
    d1 = nn.make_desc(nn.DGRAD, B, C, 1, 1, 1, 0, 0, C, C, C, [nn.seg(H, H, H, H, w1)], beta=1.0)
    dx = torch.zeros((B, H, H, C), dtype=BF, device="cuda")
    got = {}
    fused = nn.conv_igemm_dgrad_bnsum(d3, dy, dx, z, mr, ga, be, nn.bn_acc(B, C, "cuda"))
    got["z_mask"] = (int(fused), lib.cvl_conv_igemm_last_kernel())
    fused = nn.conv_igemm_dgrad_bnsum_res(d1, dy, dx, y, z, mr, ga, be, nn.bn_acc(B, C, "cuda"))
    got["y_mask"] = (int(fused), lib.cvl_conv_igemm_last_kernel())
    torch.cuda.synchronize()
    print("fused entries", got)
    for form in ("z_mask", "y_mask"):
        assert got[form] == (recorded[form]["fused"], recorded[form]["kernel"])
        assert recorded[form]["fused"] == 1


def test_relu_mask_rejected_before_any_launch():
    """A data gradient through a ReLU that the tower kernel does not take (Npad 64) into a non-dense
    dst: the separate ReLU backward cannot serve it, so the call is CVL_EINVAL -- and dst is untouched
    (before the planner the unmasked gradient had already been written by then)."""
    from cvlite import _lib, ops_nn as nn
    lib = _lib.load()
    B, H, C = 1, 16, 64
    dy = torch.ones((B, H, H, C), dtype=BF, device="cuda")
    y = torch.ones((B, H, H, C), dtype=BF, device="cuda")
    w = torch.ones((C, 9 * C), dtype=BF, device="cuda")
    ld = 2 * C
    dst = torch.full((B, H, H, ld), -3.0, dtype=BF, device="cuda")
    sentinel = dst.clone()
    d = nn.make_desc(nn.DGRAD, B, C, 3, 3, 1, 1, 1, C, C, ld, [nn.seg(H, H, H, H, w)])
    n = int(lib.cvl_conv_igemm_workspace_size(ctypes.byref(d)))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda") if n > 16 else None
    st = lib.cvl_conv_igemm_relu_mask(ctypes.byref(d), _lib.ptr(dy), _lib.ptr(dst), _lib.ptr(y), _lib.ptr(ws),
                                      n if ws is not None else 0, _lib.stream())
    torch.cuda.synchronize()
    assert st == 1                                           # CVL_EINVAL
    assert torch.equal(dst.view(torch.int16), sentinel.view(torch.int16))
