"""Host-only checks of the grouped 3x3 conv's launch plans (cvl_gconv3x3_plan; csrc/conv_group.hip:
gc_tpw for the forward / data gradient, gw_plan for the weight gradient) -- no GPU.

  * the production geometries (RetinaNet ResNeXt-50 / 101, 640 x 640, bs 8) plan MULTI-tile: a workgroup
    walks 2 or 4 output tiles on one set of weight registers, a weight-gradient workgroup accumulates
    several pixel tiles;
  * every case of tests/test_gpu_gconv.py plans tpw = 1 and tpc = 1 -- which is why
    tests/test_gpu_gconv_plans.py exists;
  * the CVL_DISPATCH hooks gc_tpw / gw_wgs change the plan and nothing else, and the weight gradient's
    workspace size follows the one gw_plan under every hook value;
  * the query refuses what gc_ok refuses."""
import pytest

from cvlite import _lib
from cvlite import ops_nn as nn

# (B, H, W, C, Cg, stride) -> fwd / dgrad (tpw, ychunks), wgrad (tpc, nchunk); ResNeXt-50 32x4d at
# 640 x 640, bs 8: stage 1 (stride 1), stage 2 unit 1 (stride 2), stage 4 units 2.. (stride 1)
PRODUCTION_50 = [
    ((8, 160, 160, 128, 4, 1), (4, 5), (4, 5), (7, 229)),
    ((8, 160, 160, 256, 8, 2), (4, 5), (4, 5), (7, 115)),
    ((8, 20, 20, 1024, 32, 1), (1, 3), (1, 3), (2, 24)),
]
# ResNeXt-101 (32x4d as well) has the same widths, so the three above are its geometries too; what it
# adds is depth in stage 3 (23 blocks for 6).  Its twins: stage 2 units 2.., stage 3 unit 1 (stride 2),
# stage 3 units 2..23, stage 4 unit 1 (stride 2), planned by hand from gc_tpw / gw_plan
PRODUCTION_101 = [
    ((8, 80, 80, 256, 8, 1), (2, 5), (2, 5), (4, 100)),
    ((8, 80, 80, 512, 16, 2), (2, 5), (2, 5), (4, 60)),
    ((8, 40, 40, 512, 16, 1), (1, 5), (1, 5), (2, 60)),
    ((8, 40, 40, 1024, 32, 2), (2, 3), (2, 3), (3, 27)),
]
# tests/test_gpu_gconv.py CASES, its isolation test and its torch-op test
SMALL = [(2, 16, 16, 128, 4, 1), (2, 16, 16, 256, 8, 2), (1, 9, 12, 512, 16, 1), (3, 14, 11, 256, 8, 2),
         (2, 8, 8, 1024, 32, 2), (2, 5, 7, 1024, 32, 1), (1, 33, 20, 128, 4, 1), (1, 8, 8, 128, 4, 1),
         (2, 8, 8, 256, 8, 2)]
FORCED = [(2, 37, 35, 64, 4, 1), (2, 37, 35, 64, 32, 2), (1, 34, 36, 128, 8, 1), (1, 34, 36, 128, 8, 2)]


def plans(geo):
    return {k: nn.gconv3x3_plan(k, *geo) for k in ("fwd", "dgrad", "wgrad")}


def ws_size(geo):
    return int(_lib.load().cvl_gconv3x3_wgrad_workspace_size(*geo))


def _tiles(geo):
    """Destination tile grids from the kernels' tile shapes: fwd 8 (stride 2: 4) rows x 16 of y; dgrad 8
    x 16 of dx (stride 2: 8 x 32); wgrad = the forward's."""
    B, H, W, C, Cg, s = geo
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    c = lambda a, b: -(-a // b)
    fwd = (c(Wo, 16), c(Ho, 8 if s == 1 else 4))
    dgrad = (c(W, 16), c(H, 8)) if s == 1 else (c(W, 32), c(H, 8))
    return {"fwd": fwd, "dgrad": dgrad, "wgrad": fwd}


@pytest.mark.parametrize("geo,fwd,dgrad,wgrad", PRODUCTION_50 + PRODUCTION_101,
                         ids=lambda v: "x".join(map(str, v)) if len(v) == 6 else "")
def test_production_geometries_plan_multi_tile(geo, fwd, dgrad, wgrad, monkeypatch):
    monkeypatch.delenv("CVL_DISPATCH", raising=False)
    p = plans(geo)
    assert (p["fwd"]["tpw"], p["fwd"]["ychunks"]) == fwd
    assert (p["dgrad"]["tpw"], p["dgrad"]["ychunks"]) == dgrad
    assert (p["wgrad"]["tpc"], p["wgrad"]["nchunk"]) == wgrad
    assert p["wgrad"]["tpc"] > 1                                  # every production weight gradient is multi-tile
    assert p["wgrad"]["nchunk"] * (geo[3] // 32) <= 1024
    assert p["fwd"]["tpw"] > 1 or geo[1] <= 40                    # and every walk but those of the two smallest maps


@pytest.mark.parametrize("geo", SMALL, ids=lambda v: "x".join(map(str, v)))
def test_existing_gpu_cases_plan_single_tile(geo, monkeypatch):
    monkeypatch.delenv("CVL_DISPATCH", raising=False)
    p = plans(geo)
    assert p["fwd"]["tpw"] == 1 and p["dgrad"]["tpw"] == 1 and p["wgrad"]["tpc"] == 1
    for k in ("fwd", "dgrad"):
        assert p[k]["tiles_x"] * p[k]["tiles_y"] * geo[0] * (geo[3] // 32) <= 64      # workgroups


def test_fields_that_do_not_apply_are_zero(monkeypatch):
    monkeypatch.delenv("CVL_DISPATCH", raising=False)
    p = plans((2, 37, 35, 64, 4, 1))
    assert p["wgrad"]["tpw"] == 0 and p["wgrad"]["ychunks"] == 0
    for k in ("fwd", "dgrad"):
        assert p[k]["tpc"] == 0 and p[k]["nchunk"] == 0


@pytest.mark.parametrize("geo", FORCED + [g for g, _, _, _ in PRODUCTION_50], ids=lambda v: "x".join(map(str, v)))
def test_hooks_change_the_plan_and_nothing_else(geo, dispatch, monkeypatch):
    monkeypatch.delenv("CVL_DISPATCH", raising=False)
    base = plans(geo)
    tiles = _tiles(geo)
    for k in base:
        assert (base[k]["tiles_x"], base[k]["tiles_y"]) == tiles[k]
    nslab = geo[3] // 32
    ntiles = geo[0] * tiles["wgrad"][0] * tiles["wgrad"][1]
    for tpw in (1, 2, 4):
        dispatch("gc_tpw=%d" % tpw)
        p = plans(geo)
        for k in ("fwd", "dgrad"):
            assert p[k] == dict(base[k], tpw=tpw, ychunks=-(-tiles[k][1] // tpw))
        assert p["wgrad"] == base["wgrad"]                        # the other family's plan does not move
    for bad in (0, 3, 8, -1):                                     # not a legal walk: the heuristic decides
        dispatch("gc_tpw=%d" % bad)
        assert plans(geo) == base
    dispatch("gc_tpw=0")
    for wgs in (1, 2, 8, 15, 64, 1024, 4096):
        dispatch("gw_wgs=%d" % wgs)
        p = plans(geo)
        want = max(wgs // nslab, 1)
        tpc = -(-ntiles // want)
        assert p["wgrad"] == dict(base["wgrad"], tpc=tpc, nchunk=-(-ntiles // tpc))
        assert p["fwd"] == base["fwd"] and p["dgrad"] == base["dgrad"]
        assert ws_size(geo) == p["wgrad"]["nchunk"] * 9 * geo[4] * geo[3] * 4
    dispatch("gw_wgs=1024")
    assert plans(geo) == base and ws_size(geo) == base["wgrad"]["nchunk"] * 9 * geo[4] * geo[3] * 4
    monkeypatch.delenv("CVL_DISPATCH", raising=False)
    assert plans(geo) == base


def test_forced_plans_of_the_gpu_tests(dispatch, monkeypatch):
    """What tests/test_gpu_gconv_plans.py relies on: at 37 (and 34) rows every kernel has 5 tile rows and
    at least two tile columns with a ragged last one; (2, 37, 35, 64) has 30 weight-gradient tiles in
    2 slabs, and gw_wgs = 8 gives chunks of 8 tiles: 4 chunks, chunk 1 = tiles 8 .. 15 crosses from image
    0 (tiles 0 .. 14) into image 1, the last chunk has 6."""
    monkeypatch.delenv("CVL_DISPATCH", raising=False)
    for geo in FORCED:
        p = plans(geo)
        for k in p:
            assert p[k]["tiles_y"] == 5 and p[k]["tiles_x"] >= 2
        W, s = geo[2], geo[5]
        assert ((W - 1) // s + 1) % 16 != 0 and W % (16 if s == 1 else 32) != 0          # ragged last column tile
    geo = (2, 37, 35, 64, 4, 1)
    for wgs, tpc, nchunk in ((1024, 1, 30), (16, 4, 8), (8, 8, 4), (2, 30, 1), (12, 5, 6), (14, 5, 6), (10, 6, 5),
                             (9, 8, 4)):
        dispatch("gw_wgs=%d" % wgs)
        p = nn.gconv3x3_plan("wgrad", *geo)
        assert (p["tpc"], p["nchunk"]) == (tpc, nchunk), wgs
    # the smallest shapes the heuristic itself sends down the walk
    monkeypatch.delenv("CVL_DISPATCH", raising=False)
    assert plans((2, 16, 128, 2048, 32, 1))["fwd"]["tpw"] == 2
    assert plans((2, 16, 128, 2048, 32, 1))["dgrad"]["tpw"] == 2
    assert plans((2, 32, 128, 2048, 32, 1))["fwd"]["tpw"] == 4
    p = plans((8, 25, 33, 2048, 32, 2))
    assert p["fwd"]["tpw"] == 4 and p["dgrad"]["tpw"] == 4
    assert plans((8, 20, 20, 1024, 32, 1))["wgrad"]["tpc"] == 2


def test_query_rejects_what_the_kernels_reject():
    ok = (1, 8, 8, 64, 4, 1)
    assert nn.gconv3x3_plan("fwd", *ok)["tpw"] == 1
    for geo in [(1, 8, 8, 64, 2, 1), (1, 8, 8, 64, 64, 1), (1, 8, 8, 64, 4, 3), (1, 8, 8, 64, 4, 0), (1, 8, 8, 48, 4, 1),
                (0, 8, 8, 64, 4, 1), (1, 0, 8, 64, 4, 1), (1, 8, -1, 64, 4, 1), (1, 8, 8, 0, 4, 1)]:
        for kind in ("fwd", "dgrad", "wgrad"):
            with pytest.raises(_lib.CvlError):
                nn.gconv3x3_plan(kind, *geo)
        assert ws_size(geo) == 0
    with pytest.raises(_lib.CvlError):
        _lib.call("cvl_gconv3x3_plan", 3, *ok, None, None, None, None, None, None)
    _lib.call("cvl_gconv3x3_plan", 2, *ok, None, None, None, None, None, None)        # null outputs are legal
