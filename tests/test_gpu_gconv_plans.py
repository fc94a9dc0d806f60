"""The grouped 3x3 conv kernels (csrc/conv_group.hip) in the MULTI-tile plans production takes and no
other test reaches (tests/test_gconv_plan_host.py): a forward / data-gradient workgroup walking 2 or 4
output tiles on one set of weight registers with the next halo prefetched (gc_tpw), a weight-gradient
workgroup accumulating several pixel tiles, across an image boundary and with a short last chunk
(gw_plan's tpc).  The plans are forced at small maps with CVL_DISPATCH=gc_tpw / gw_wgs, and taken
unforced at the smallest shapes the heuristic itself sends down the walk; every plan is asserted
through cvl_gconv3x3_plan.

Reference, input sets and bounds: tests/gconv_ref.py (its docstring derives them).  On the EXACT set
every output must equal the reference bit for bit (torch.equal, no element left out); on the RANDOM
set every element stays under its derived bound.  Also here: walk-invariance of y and dx (tpw 2 and 4
against 1, bit for bit), BN statistics decoding to the exact sums in both accumulator modes, writes
that stay inside their buffers (C ABI between guard bytes, workspace of exactly the queried size),
and the reach of a non-finite input.  Lines starting "gconv_ratio" carry the largest error / bound per
kernel, plan and set (profiles/gconv_bounds.md)."""
import functools

import pytest
import torch

import gconv_ref as G

pytestmark = pytest.mark.gpu
BF, F64 = torch.bfloat16, torch.float64

MAPS = [(2, 37, 35), (1, 34, 36)]
CHANNELS = [(64, 4), (64, 32), (128, 8)]
GEOS = [(B, H, W, C, Cg, s) for (B, H, W) in MAPS for (C, Cg) in CHANNELS for s in (1, 2)]
TPWS = (1, 2, 4)
KINDS = ["exact", "random"]


def gid(geo):
    return "x".join(map(str, geo))


@functools.lru_cache(maxsize=None)
def case(kind, geo):
    """Inputs (CPU) and the float64 references (computed once on the device, kept on the CPU) of one
    geometry and input set, shared by every test; nobody writes to them."""
    B, H, W, C, Cg, s = geo
    inp = G.make_inputs(kind, *geo)
    x, dy, w = inp["x"].cuda(), inp["dy"].cuda(), inp["w"]
    ref = {"y": G.fwd_ref(x, w, Cg, s), "dx0": G.dgrad_ref(dy, w, Cg, s, H, W),
           "dx1": G.dgrad_ref(dy, w, Cg, s, H, W, beta=1.0, old=inp["dx_old"].cuda()),
           "dw0": G.wgrad_ref(x, dy, Cg, s),
           "dw2": G.wgrad_ref(x, dy, Cg, s, beta=2.0, old=inp["dw_old"].cuda())}
    inp["ref"] = {k: (t.cpu(), A.cpu()) for k, (t, A) in ref.items()}
    return inp


class Ops(object):
    """One case on the device: packed weights once, every launch into fresh outputs."""

    def __init__(self, inp):
        from cvlite import ops_nn as nn
        self.nn = nn
        self.inp = inp
        self.B, self.H, self.W, self.C, self.Cg, self.s = inp["geo"]
        self.Ho, self.Wo = inp["Ho"], inp["Wo"]
        self.x, self.dy = inp["x"].cuda(), inp["dy"].cuda()
        self.wf, self.wd = nn.gconv3x3_packed(self.C, "cuda"), nn.gconv3x3_packed(self.C, "cuda")
        nn.gconv3x3_pack(inp["w"].cuda(), self.wf, self.wd)

    def plan(self, kind):
        return self.nn.gconv3x3_plan(kind, self.B, self.H, self.W, self.C, self.Cg, self.s)

    def fwd(self, stats=True):
        y = torch.full((self.B, self.Ho, self.Wo, self.C), 7.0, dtype=BF, device="cuda")
        acc = self.nn.bn_acc(self.B, self.C, "cuda") if stats else None
        self.nn.gconv3x3_fwd(self.x, self.wf, y, self.Cg, self.s, acc)
        return y.cpu(), (self.nn.bn_acc_value(acc).cpu() if stats else None)

    def dgrad(self, beta):
        dx = self.inp["dx_old"].cuda().clone() if beta else torch.full((self.B, self.H, self.W, self.C), 7.0, dtype=BF,
                                                                      device="cuda")
        self.nn.gconv3x3_dgrad(self.dy, self.wd, dx, self.Cg, self.s, beta=beta)
        return dx.cpu()

    def wgrad(self, beta):
        dw = self.inp["dw_old"].cuda().clone() if beta else torch.full((3, 3, self.Cg, self.C), 7.0, device="cuda")
        self.nn.gconv3x3_wgrad(self.x, self.dy, dw, self.s, beta=beta)
        return dw.cpu()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def note(kernel, plan, kind, r):
    print("gconv_ratio kernel=%s plan=%s set=%s r=%.3g" % (kernel, plan, kind, r))


def check_out(name, kernel, plan, kind, got, ref):
    """A bf16 output against (t, A): bit equality on the exact set, the derived bound on the random one."""
    t, A = ref
    if kind == "exact":
        G.check_exact(name, got, G.expected_bf16(t))
        note(kernel, plan, kind, 0.0)
    else:
        note(kernel, plan, kind, G.check_bound(name, got, t, G.out_bound(t, A)))


def check_dw(name, plan, kind, got, ref, n, nchunk):
    t, A = ref
    if kind == "exact":
        G.check_exact(name, got, t.float())
        note("wgrad", plan, kind, 0.0)
    else:
        note("wgrad", plan, kind, G.check_bound(name, got, t, G.dw_bound(A, n, nchunk)))


# ---- forced walks at the smallest maps that have every edge -------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", GEOS, ids=gid)
def test_forced_walk_against_fp64(geo, kind, dispatch):
    """gc_tpw in {1, 2, 4} on 5 tile rows: chunks of 1 x 5, 2 + 2 + 1, 4 + 1 (the ragged last chunk, the
    prefetch of the next tile, the barrier between tiles), at least two tile columns with a ragged last
    one.  Forward with BN statistics, data gradient with beta 0 and 1, weight gradient with beta 2;
    y and dx under tpw 2 and 4 are the bits of tpw 1."""
    inp = case(kind, geo)
    op = Ops(inp)
    ref = inp["ref"]
    B, H, W, C, Cg, s = geo
    n = B * inp["Ho"] * inp["Wo"]
    first = None
    for tpw in TPWS:
        dispatch("gc_tpw=%d" % tpw)
        for k in ("fwd", "dgrad"):
            p = op.plan(k)
            assert p["tiles_y"] == 5 and p["tiles_x"] >= 2
            assert (p["tpw"], p["ychunks"]) == (tpw, {1: 5, 2: 3, 4: 2}[tpw])
        plan = "tpw%d" % tpw
        y, sv = op.fwd()
        dx0, dx1 = op.dgrad(0.0), op.dgrad(1.0)
        label = "%s %s %s" % (gid(geo), kind, plan)
        check_out(label + " y", "fwd/%d" % s, plan, kind, y, ref["y"])
        check_out(label + " dx beta=0", "dgrad/%d" % s, plan, kind, dx0, ref["dx0"])
        check_out(label + " dx beta=1", "dgrad/%d beta=1" % s, plan, kind, dx1, ref["dx1"])
        # the statistics of the stored y: (HW + 3) u sum |t| per (image, channel)
        S, bound = G.stats_ref(y)
        r = G.check_bound(label + " bn stats", sv, S, bound)
        note("fwd/%d stats" % s, plan, kind, r)
        wp = op.plan("wgrad")
        check_dw(label + " dW beta=2", "tpc%d" % wp["tpc"], kind, op.wgrad(2.0), ref["dw2"], n, wp["nchunk"])
        if first is None:
            first = (y, dx0, dx1)
        else:
            for name, a, b in zip(("y", "dx beta=0", "dx beta=1"), first, (y, dx0, dx1)):
                assert same_bits(a, b), "%s: %s under gc_tpw=%d differs from gc_tpw=1" % (label, name, tpw)


@pytest.mark.parametrize("geo", GEOS, ids=gid)
def test_forced_walk_bn_statistics_exact(geo, dispatch):
    """The statistics carried across the tiles of a walk, on the "flat" exact set: y is a multiple of
    0.5 with |y| <= 256 and, per (image, channel), sum |y| and sum y^2 stay below 2^24 units (halves,
    quarters), so every fp32 partial in any order is exact and the accumulators must decode to the
    float64 sums exactly -- in both accumulator modes, for every walk."""
    from cvlite import ops_nn as nn
    inp = case("flat", geo)
    t, _ = inp["ref"]["y"]
    want = G.expected_bf16(t)
    yd = want.to(F64)
    assert float(yd.abs().max()) <= 256 and torch.equal((2 * yd).round(), 2 * yd)
    assert float(2 * yd.abs().sum((1, 2)).max()) < 2 ** 24 and float(4 * (yd * yd).sum((1, 2)).max()) < 2 ** 24
    S, _ = G.stats_ref(want)
    assert float(S[..., 1].min()) > 0
    try:
        for on in (False, True):
            nn.set_bn_exact(on)
            op = Ops(inp)
            for tpw in TPWS:
                dispatch("gc_tpw=%d" % tpw)
                assert op.plan("fwd")["tpw"] == tpw
                y, sv = op.fwd()
                G.check_exact("%s flat tpw%d y" % (gid(geo), tpw), y, want)
                assert torch.equal(sv, S), "%s tpw%d %s: statistics differ from the exact sums by up to %g" % (
                    gid(geo), tpw, "exact bins" if on else "float64 atomics", float((sv - S).abs().max()))
    finally:
        nn.set_bn_exact(False)


# ---- weight-gradient chunks -------------------------------------------------------------------------
def _gw_plan(geo, wgs):
    """gw_plan (csrc/conv_group.hip) restated: (ntiles, tpc, nchunk)."""
    B, H, W, C, Cg, s = geo
    Ho, Wo = G.out_hw(H, W, s)
    ntiles = B * (-(-Wo // 16)) * (-(-Ho // (8 if s == 1 else 4)))
    want = max(wgs // (C // 32), 1)
    tpc = -(-ntiles // want)
    return ntiles, tpc, -(-ntiles // tpc)


def _gw_hooks(geo):
    """gw_wgs values for this map: tpc in {1, 4, 8, ntiles} and nchunk in {1, 4, 5, 7} where the tile count
    allows them (the first wgs that gives each)."""
    ntiles = _gw_plan(geo, 1024)[0]
    out = {}
    for wgs in range(1, 1025):
        _, tpc, nchunk = _gw_plan(geo, wgs)
        if (tpc in (1, 4, 8, ntiles) or nchunk in (1, 4, 5, 7)) and (tpc, nchunk) not in out.values():
            out[wgs] = (tpc, nchunk)
    return out


def test_weight_gradient_hooks_cover_the_chunkings():
    tpcs, nchunks = set(), set()
    for geo in GEOS:
        for tpc, nchunk in _gw_hooks(geo).values():
            tpcs.add(tpc)
            nchunks.add(nchunk)
    assert {1, 4, 8} <= tpcs and {1, 4, 5, 7} <= nchunks
    # (2, 37, 35, 64): 30 tiles in 2 slabs; gw_wgs=8 -> chunks of 8 tiles: chunk 1 (tiles 8 .. 15) crosses
    # from image 0 (tiles 0 .. 14) into image 1, the last chunk has 6
    assert _gw_plan((2, 37, 35, 64, 4, 1), 8) == (30, 8, 4)
    assert (8, 4) in _gw_hooks((2, 37, 35, 64, 4, 1)).values()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", GEOS, ids=gid)
def test_weight_gradient_chunks_against_fp64(geo, kind, dispatch):
    """tpc from 1 to all tiles of the launch in one workgroup: several tiles accumulated in registers, a
    chunk that crosses from one image into the next, a short last chunk, the reduce kernel's unrolled
    (nchunk >= 4) and remainder loops.  Exact set: dW is the reference's bits for every plan (hence across
    plans), beta 0 and beta 2 onto 0.25.  Random set: within bound, and the same bits on a second run."""
    inp = case(kind, geo)
    op = Ops(inp)
    B, H, W, C, Cg, s = geo
    n = B * inp["Ho"] * inp["Wo"]
    for wgs, (tpc, nchunk) in sorted(_gw_hooks(geo).items()):
        dispatch("gw_wgs=%d" % wgs)
        p = op.plan("wgrad")
        assert (p["tpc"], p["nchunk"]) == (tpc, nchunk), wgs
        label = "%s %s gw_wgs=%d tpc=%d nchunk=%d" % (gid(geo), kind, wgs, tpc, nchunk)
        dw = op.wgrad(0.0)
        check_dw(label + " dW", "tpc%d/nchunk%d" % (tpc, nchunk), kind, dw, inp["ref"]["dw0"], n, nchunk)
        if kind == "exact":
            check_dw(label + " dW beta=2", "tpc%d/nchunk%d" % (tpc, nchunk), kind, op.wgrad(2.0), inp["ref"]["dw2"], n,
                     nchunk)
        else:
            assert torch.equal(dw, op.wgrad(0.0)), label + ": not bit-identical run to run"


# ---- the heuristic's own picks ------------------------------------------------------------------------
UNFORCED = [((2, 16, 128, 2048, 32, 1), 2), ((2, 32, 128, 2048, 32, 1), 4), ((8, 25, 33, 2048, 32, 2), 4)]


@pytest.mark.parametrize("geo,tpw", UNFORCED, ids=[gid(g) for g, _ in UNFORCED])
def test_heuristic_walk_exact(geo, tpw, monkeypatch):
    """The smallest shapes gc_tpw() itself sends down the walk (>= 2048 workgroups at tpw = 1), no hook
    set; exact set, reference on the device.  (8, 25, 33) under stride 2: 4 tile rows x 2 ragged tile columns
    for both the forward (13 x 17 outputs) and the data gradient."""
    monkeypatch.delenv("CVL_DISPATCH", raising=False)
    B, H, W, C, Cg, s = geo
    inp = G.make_inputs("exact", *geo)
    op = Ops(inp)
    assert op.plan("fwd")["tpw"] == tpw and op.plan("dgrad")["tpw"] == tpw
    wp = op.plan("wgrad")
    assert wp["tpc"] > 1
    nn = op.nn
    y = torch.full((B, inp["Ho"], inp["Wo"], C), 7.0, dtype=BF, device="cuda")
    nn.gconv3x3_fwd(op.x, op.wf, y, Cg, s)
    t, _ = G.fwd_ref(op.x, inp["w"], Cg, s)
    G.check_exact("%s y" % gid(geo), y, G.expected_bf16(t))
    del t, y
    dx = torch.full((B, H, W, C), 7.0, dtype=BF, device="cuda")
    nn.gconv3x3_dgrad(op.dy, op.wd, dx, Cg, s)
    t, _ = G.dgrad_ref(op.dy, inp["w"], Cg, s, H, W)
    G.check_exact("%s dx" % gid(geo), dx, G.expected_bf16(t))
    del t, dx
    dw = torch.full((3, 3, Cg, C), 7.0, device="cuda")
    nn.gconv3x3_wgrad(op.x, op.dy, dw, s)
    t, _ = G.wgrad_ref(op.x, op.dy, Cg, s)
    G.check_exact("%s dW (tpc %d, nchunk %d)" % (gid(geo), wp["tpc"], wp["nchunk"]), dw, t.float())


def test_heuristic_weight_gradient_chunks_exact(monkeypatch):
    """Stage 4 of the production step: tpc = 2 without a hook."""
    monkeypatch.delenv("CVL_DISPATCH", raising=False)
    geo = (8, 20, 20, 1024, 32, 1)
    inp = G.make_inputs("exact", *geo)
    op = Ops(inp)
    wp = op.plan("wgrad")
    assert (wp["tpc"], wp["nchunk"]) == (2, 24)
    dw = torch.full((3, 3, 32, 1024), 7.0, device="cuda")
    op.nn.gconv3x3_wgrad(op.x, op.dy, dw, 1)
    t, _ = G.wgrad_ref(op.x, op.dy, 32, 1)
    G.check_exact("dW", dw, t.float())


# ---- writes stay in their buffers -----------------------------------------------------------------------
PAD = 208          # 16-byte aligned (the kernels' vector accesses), not a multiple of the allocator's granule


class Guarded(object):
    """`nbytes` usable bytes in the middle of a 0xA5-filled buffer."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.big = torch.full((self.n + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.ptr = self.big.data_ptr() + PAD
        assert self.ptr % 16 == 0

    def view(self, dtype, shape):
        return self.big[PAD:PAD + self.n].view(dtype).view(shape)

    def intact(self):
        return bool((self.big[:PAD] == 0xA5).all()) and bool((self.big[PAD + self.n:] == 0xA5).all())


@pytest.mark.parametrize("tpw", TPWS)
@pytest.mark.parametrize("s", [1, 2])
def test_c_entry_writes_stay_inside(s, tpw, dispatch):
    """y, dx, dW and the workspace between guard bytes on the (2, 37, 35) map, the workspace exactly
    cvl_gconv3x3_wgrad_workspace_size under the same hook (gw_wgs=8: chunks of 8 and 5 tiles); one byte
    less is refused before anything is enqueued."""
    from cvlite import _lib
    geo = (2, 37, 35, 64, 4, s)
    B, H, W, C, Cg, _ = geo
    inp = case("random", geo)
    op = Ops(inp)
    Ho, Wo = inp["Ho"], inp["Wo"]
    dispatch("gc_tpw=%d" % tpw, "gw_wgs=8")
    wp = op.plan("wgrad")
    assert wp["tpc"] > 1 and op.plan("fwd")["tpw"] == tpw
    nws = int(_lib.load().cvl_gconv3x3_wgrad_workspace_size(B, H, W, C, Cg, s))
    assert nws == wp["nchunk"] * 9 * Cg * C * 4
    y, dx, dw, ws = Guarded(B * Ho * Wo * C * 2), Guarded(B * H * W * C * 2), Guarded(9 * Cg * C * 4), Guarded(nws)
    p = lambda t_: t_.data_ptr()
    with pytest.raises(_lib.CvlError):
        _lib.call("cvl_gconv3x3_wgrad", p(op.x), p(op.dy), dw.ptr, 0.0, B, H, W, C, Cg, s, Ho, Wo, ws.ptr, nws - 1,
                  _lib.stream())
    torch.cuda.synchronize()
    for g in (dw, ws):
        assert bool((g.big == 0xA5).all())
    _lib.call("cvl_gconv3x3_fwd", p(op.x), p(op.wf), y.ptr, None, B, H, W, C, Cg, s, Ho, Wo, _lib.stream())
    _lib.call("cvl_gconv3x3_dgrad", p(op.dy), p(op.wd), dx.ptr, B, H, W, C, Cg, s, Ho, Wo, 0.0, _lib.stream())
    _lib.call("cvl_gconv3x3_wgrad", p(op.x), p(op.dy), dw.ptr, 0.0, B, H, W, C, Cg, s, Ho, Wo, ws.ptr, nws,
              _lib.stream())
    torch.cuda.synchronize()
    for name, g in (("y", y), ("dx", dx), ("dW", dw), ("workspace", ws)):
        assert g.intact(), name
    ref = inp["ref"]
    plan = "guard tpw%d" % tpw
    check_out("guard y", "fwd/%d" % s, plan, "random", y.view(BF, (B, Ho, Wo, C)).cpu(), ref["y"])
    check_out("guard dx", "dgrad/%d" % s, plan, "random", dx.view(BF, (B, H, W, C)).cpu(), ref["dx0"])
    check_dw("guard dW", "guard tpc%d" % wp["tpc"], "random", dw.view(torch.float32, (3, 3, Cg, C)).cpu(), ref["dw0"],
             B * Ho * Wo, wp["nchunk"])


# ---- the reach of a non-finite input --------------------------------------------------------------------
def _footprint(kernel, s, pos, dshape):
    """bool [Hd, Wd]: destination pixels that read source pixel `pos` (forward: y from x; dgrad: dx from dy)."""
    m = torch.zeros(dshape, dtype=torch.bool)
    py, px = pos
    for ky in range(3):
        for kx in range(3):
            if kernel == "fwd":                    # oy s - 1 + ky = py
                ny, nx = py + 1 - ky, px + 1 - kx
                if ny % s or nx % s:
                    continue
                ny, nx = ny // s, nx // s
            else:                                  # iy = oy s - 1 + ky
                ny, nx = py * s - 1 + ky, px * s - 1 + kx
            if 0 <= ny < dshape[0] and 0 <= nx < dshape[1]:
                m[ny, nx] = True
    return m


@pytest.mark.parametrize("tpw", [1, 2])
@pytest.mark.parametrize("s", [1, 2])
def test_non_finite_input_stays_local(s, tpw, dispatch):
    """One NaN, and separately one Inf, in x (forward) / dy (data gradient) at an interior, a border and
    two tile-seam positions (a seam inside a walk and one between two workgroups' chunks at tpw = 2).
    The output is the clean run's bits in every other image, in every other 32-channel slab and outside
    the 3 x 3 footprint.  Inside the footprint the planted channel's group is non-finite -- and the rest
    of its 32-channel slab may be: the kernels multiply the block-diagonal zero padding by the NaN,
    which a true grouped conv would not (grouped 3x3)."""
    geo = (2, 37, 35, 64, 4, s)
    B, H, W, C, Cg, _ = geo
    inp = case("random", geo)
    op = Ops(inp)
    dispatch("gc_tpw=%d" % tpw)
    assert op.plan("fwd")["tpw"] == tpw and op.plan("dgrad")["tpw"] == tpw
    img, ch = 1, 37                                    # image 1, slab 1, group 9
    slab = slice(32 * (ch // 32), 32 * (ch // 32) + 32)
    group = slice(Cg * (ch // Cg), Cg * (ch // Cg) + Cg)
    for kernel in ("fwd", "dgrad"):
        src = inp["x"] if kernel == "fwd" else inp["dy"]
        Hs, Ws = src.shape[1], src.shape[2]
        run = (lambda: op.fwd(stats=False)[0]) if kernel == "fwd" else (lambda: op.dgrad(0.0))
        name = "x" if kernel == "fwd" else "dy"
        keep = getattr(op, name)
        clean = run()
        assert bool(torch.isfinite(clean.float()).all())
        # destination tile rows are 8 (stride-2 forward: 4) deep, columns 16 (stride-2 dgrad: 32) wide
        if s == 1:
            seams = [(8, 16), (16, 16)]
        elif kernel == "fwd":
            seams = [(7, 31), (15, 31)]                # y rows 3 | 4 and 7 | 8, columns 15 | 16
        else:
            seams = [(4, 16), (8, 16)]                 # dx rows 7 | 8 and 15 | 16, columns 31 | 32
        for pos in [(Hs // 2 + 1, 9), (0, 0), (Hs - 1, Ws - 1)] + seams:
            fp = _footprint(kernel, s, pos, clean.shape[1:3])
            assert bool(fp.any())
            for bad in (float("nan"), float("inf")):
                planted = src.clone()
                planted[img, pos[0], pos[1], ch] = bad
                setattr(op, name, planted.cuda())
                try:
                    got = run()
                finally:
                    setattr(op, name, keep)
                label = "%s stride %d tpw %d %s at %s" % (kernel, s, tpw, bad, pos)
                assert same_bits(got[:img], clean[:img]) and same_bits(got[img + 1:], clean[img + 1:]), label
                other = torch.ones(C, dtype=torch.bool)
                other[slab] = False
                assert same_bits(got[img][..., other], clean[img][..., other]), label + ": another slab changed"
                assert same_bits(got[img][~fp], clean[img][~fp]), label + ": outside the footprint changed"
                inside = got[img][fp].float()
                assert not bool(torch.isfinite(inside[:, group]).any()), label + ": the group stayed finite"
                assert bool(torch.isfinite(inside[:, other]).all())


# ---- the launch-parity harness's grouped-conv checks ------------------------------------------------
def test_launch_parity_checks_the_grouped_conv(dispatch, monkeypatch):
    """tests/launch_parity.py wraps gconv3x3_pack / fwd / dgrad / wgrad like every other op: a walk of two
    tiles and chunks of four pass every record with no unchecked launch; a kernel whose output is off in
    one element is flagged."""
    from cvlite import ops_nn as nn
    from launch_parity import LaunchParity
    geo = (2, 37, 35, 128, 8, 2)
    B, H, W, C, Cg, s = geo
    inp = case("random", geo)
    dispatch("gc_tpw=2", "gw_wgs=16")

    def step():
        wf, wd = nn.gconv3x3_packed(C, "cuda"), nn.gconv3x3_packed(C, "cuda")
        nn.gconv3x3_pack(inp["w"].cuda(), wf, wd)
        y = torch.empty((B, inp["Ho"], inp["Wo"], C), dtype=BF, device="cuda")
        nn.gconv3x3_fwd(inp["x"].cuda(), wf, y, Cg, s, nn.bn_acc(B, C, "cuda"))
        dx = inp["dx_old"].cuda()
        nn.gconv3x3_dgrad(inp["dy"].cuda(), wd, dx, Cg, s, beta=1.0)
        dw = inp["dw_old"].cuda()
        nn.gconv3x3_wgrad(inp["x"].cuda(), inp["dy"].cuda(), dw, s, beta=2.0)

    with LaunchParity(imgs=None) as lp:
        step()
    print(lp.table())
    assert [r.what for r in lp.records] == ["w_fwd", "w_dgrad", "y", "bn_stats", "dx", "dW"]
    assert not lp.failures(), lp.table()
    assert not lp.unchecked_calls()
    orig = nn.gconv3x3_fwd

    def broken(x, wf, y, Cg_, s_, stats=None):
        orig(x, wf, y, Cg_, s_, stats)
        y[1, 18, 17, 100] += 0.25
    monkeypatch.setattr(nn, "gconv3x3_fwd", broken)
    with LaunchParity(imgs=None) as lp:
        step()
    # (the statistics no longer describe the y the harness sees either)
    assert [r.what for r in lp.failures()] == ["y", "bn_stats"], lp.table()
