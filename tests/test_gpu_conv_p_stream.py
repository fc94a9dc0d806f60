"""The cross-tile stream of the persistent 1x1 kernel (conv_igemm_p.hip, CVL_CK_P): geometry x form,
element-wise against float64.

One workgroup of P walks a contiguous chunk of 256-row tiles of one N tile; the LDS-DMA ring runs
across them, the epilogue operands of a tile (old destination chunks, z / y / bitmap bytes) are fetched
with its first K-tile and waited for by a counted vmcnt, and the BN statistics / fused BN-backward
sums stay in registers until the image changes inside the chunk.  Every case here therefore runs
SEVERAL tiles per workgroup -- forced at small sizes with CVL_DISPATCH=p_wgs=<n>, or at the default
grid with more than 256 tiles -- and asserts that from the planner's own answer
(cvl_conv_igemm_plan_grid), so a later planner change cannot silently turn a multi-tile case into a
one-tile one.  The geometries (GEOS) are uneven chunks, idle workgroups, a ragged last tile at the
end of a stream, images that straddle a chunk, grids with G % 8 != 0 (xcd_remap) and 2 / 3 / 4 N
tiles; the forms (FORMS) are every instantiation p_launch reaches plus the addressing modes; the K
depths put the number of K-tiles per tile below, at and above the ring depth D of each tile shape.
test_case_list_coverage (no GPU) holds the list to that.

Reference: out = src . W^T as a float64 matmul on the same bf16-rounded operands (the weights are
written in the packed [N][K] layout directly), independent of every cvlite kernel; rows are random and
distinct, so a swapped or shifted row shows.  The destination has guard rows in front of dst_base,
behind the last image and (some cases) between the images, and guard columns around the block; it is
filled with a sentinel (or the random `old` of an accumulating form) and every element outside the
written block must keep its bits.

Tolerances, all this project's own: bf16 results rtol 1e-2 / atol 2e-2 (test_gpu_conv_production.py,
test_gpu_conv_k64.py), the accumulating bf16 form atol 3e-2 (test_gpu_conv.py), fp32 results 1e-4, BN
statistics rtol 1e-5 / atol 1e-3 of the float64 sums of the stored output, fused sums red_err <= 1e-6
(launch_parity.py's cancellation-safe error, the bound of its bn_stats records).
test_comparison_catches_single_defects (no GPU) shows that the comparison is not vacuous."""
import collections
import ctypes

import pytest
import torch

from launch_parity import bn_affine32, red_err

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
CK_P = 16
BM = 256
FRONT, TAIL = 3, 4              # guard rows in front of dst_base / behind the last image
SENTINEL = 7.0
DEV = "cuda"

# id -> B, H, W (the GEMM grid: output pixels; dY pixels of a data gradient), N, CVL_DISPATCH hooks,
# expected (grid, N tile, tiles per chunk) of the plain forms, and the properties the case is there for:
#   multi    a busy workgroup walks >= 2 tiles            idle     workgroups without a tile
#   ragged   the last tile is partly absent            late     ... and is not the first tile of its stream
#   straddle an image boundary inside a chunk             g8       grid % 8 != 0
#   uneven   the last busy chunk is shorter
# (D on 4 workgroups: chunks 3, 3, 3, 2, so its 140-row tile is the second of its stream; the ragged tiles
# of H and I are alone in theirs.)  The z-mask fused form takes dense destination images only, so its
# cases have no rows between the images; the residual fused forms have them on the scatter (dst_up 2).
Geo = collections.namedtuple("Geo", "B H W N hooks plan chunks props big")
GEOS = collections.OrderedDict([
    ("A", Geo(4, 32, 32, 64, ("p_wgs=8",), (8, 64), [2] * 8, {"multi"}, False)),
    ("B", Geo(5, 24, 32, 64, ("p_wgs=4",), (4, 64), [4, 4, 4, 3], {"multi", "straddle", "g8", "uneven"}, False)),
    ("C", Geo(9, 16, 16, 64, ("p_wgs=8",), (8, 64), [2, 2, 2, 2, 1, 0, 0, 0], {"multi", "idle", "uneven"}, False)),
    ("D", Geo(3, 30, 30, 64, ("p_wgs=4",), (4, 64), [3, 3, 3, 2], {"multi", "ragged", "late", "g8", "uneven"}, False)),
    ("E", Geo(7, 16, 32, 192, ("p_wgs=16",), (15, 64), [3, 3, 3, 3, 2], {"multi", "g8", "uneven", "straddle"}, False)),
    ("F", Geo(5, 24, 32, 256, ("p_wgs=8", "p_bn=128"), (8, 128), [4, 4, 4, 3], {"multi", "straddle", "uneven"}, False)),
    ("G", Geo(5, 24, 32, 256, ("p_wgs=4", "p_bn=256"), (4, 256), [4, 4, 4, 3], {"multi", "straddle", "g8"}, False)),
    ("H", Geo(5, 116, 116, 64, (), (256, 64), [2] * 131 + [1] + [0] * 124, {"multi", "idle", "ragged"}, True)),
    ("I", Geo(3, 88, 88, 192, (), (255, 64), [2] * 45 + [1] + [0] * 39, {"multi", "g8", "ragged", "idle"}, True)),
    ("K", Geo(23, 24, 32, 256, ("p_bn=64",), (256, 64), [2] * 34 + [1] + [0] * 29, {"multi", "straddle", "idle"}, True)),
])

# name -> kind, needs HW % 256 == 0 (BN statistics / fused sums: a tile inside one image), fused-sums offer
Form = collections.namedtuple("Form", "kind whole offer")
FORMS = collections.OrderedDict([
    ("f1_relu_stats", Form("fwd", False, 0)),     # statistics where HW % 256 == 0, else the same launch without
    ("f2_narrow", Form("fwd", False, 0)),
    ("f3_stride2", Form("fwd", False, 0)),
    ("f4_f32", Form("fwd", False, 0)),
    ("f5_dgrad", Form("dgrad", False, 0)),
    ("f6_dgrad_beta", Form("dgrad", False, 0)),
    ("f7_dgrad_up2", Form("dgrad", False, 0)),
    ("f8_bnsum_z", Form("dgrad", True, 1)),
    ("f9_bnsum_y", Form("dgrad", True, 2)),
    ("f10_bnsum_bits", Form("dgrad", True, 3)),
])
KS = [32, 64, 96, 192, 320, 128, 160]      # 128 / 160: nk == D of the 64-deep ring / the 128-wide 32-deep one
K_REQUIRED = {32, 64, 96, 192, 320}
K_LONG = (2048, 576)                       # geometry A: vmcnt buckets 63 (both depths) / 48 and 36

Case = collections.namedtuple("Case", "geo form K var")      # var: tuple of (key, value) of the variant


def ring_depth(bn, bk):
    """D = NS - 1 of PCfg<bn, bk> (conv_igemm_p.hip), restated."""
    slot = (BM + bn) * bk * 2
    pr = 8 * 64 * 16 // (bk * 2)
    red = (2 if bn == 256 else 4) * bn * 2 * 4
    dummy = 4096 if bn < pr else 0
    return (163840 - red - dummy) // slot - 1


def cases():
    out = []
    for gi, (gid, g) in enumerate(GEOS.items()):
        whole = (g.H * g.W) % BM == 0
        for fi, (fid, f) in enumerate(FORMS.items()):
            if f.whole and not whole:
                continue
            ks = [KS[(gi + fi) % 7]]
            if f.offer:                        # these meet 7 of the 10 geometries: two depths each
                ks.append(KS[(gi + fi + 3) % 7])
            if fid == "f3_stride2" and g.big:  # (the gathered source is four times the output map)
                ks = [[32, 64, 96][gi % 3]]
            odd = gi % 2 == 1
            extra = 5 if gid in ("B", "D", "I") else 0       # dst_img > HW: rows between the images
            for K in ks:
                var = {"extra": extra}
                if fid == "f3_stride2":
                    var["odd"] = odd
                elif fid == "f4_f32":
                    # ReLU on / off x beta 0 / 1: two launches per case, the pairing alternates
                    var["pairs"] = ((1, 0.0), (0, 1.0)) if odd else ((1, 1.0), (0, 0.0))
                elif fid == "f7_dgrad_up2":
                    var["pairs"] = ((0.0, 1), (1.0, 0)) if odd else ((0.0, 0), (1.0, 1))   # (beta, odd map)
                elif fid == "f8_bnsum_z":
                    var["extra"] = 0           # the z-mask form takes dense destination images only
                    var["act_hi"] = 1.0 if gid in ("A", "E") else float("inf")
                elif f.offer:
                    var["extra"] = 0
                out.append(Case(gid, fid, K, tuple(sorted(var.items()))))
    for fid, f in FORMS.items():           # geometry A at the long depths
        for K in K_LONG:
            if K == 576 and not (f.offer or fid == "f6_dgrad_beta"):
                continue                       # (the counted wait exists in the ACC and fused-sums forms)
            var = {"extra": 0}
            if fid == "f3_stride2":
                var["odd"] = True
            elif fid == "f4_f32":
                var["pairs"] = ((1, 1.0),)
            elif fid == "f7_dgrad_up2":
                var["pairs"] = ((1.0, 1),)
            elif fid == "f8_bnsum_z":
                var["act_hi"] = float("inf")
            out.append(Case("A", fid, K, tuple(sorted(var.items()))))
    # the residual fused forms on the strided data gradient's scatter, destination images apart
    for fid in ("f9_bnsum_y", "f10_bnsum_bits"):
        out.append(Case("A", fid, 64, (("extra", 5), ("up2", 1))))
        out.append(Case("B", fid, 192, (("extra", 5), ("up2", 2))))      # odd destination map
    return out


CASES = cases()


def case_id(c):
    v = dict(c.var)
    return "%s-%s-K%d%s" % (c.geo, c.form, c.K, "-up2" if v.get("up2") else "")


def k64_settings(c):
    return (1, 0) if c.K % 64 == 0 else (1,)


# ---------------------------------------------------------------------------------------------------
# layout: everything about a launch that needs no device
# ---------------------------------------------------------------------------------------------------
class Layout(object):
    """One launch of a case: sizes, destination layout and the descriptor's arguments."""

    def __init__(self, c, relu=None, beta=None, odd=None):
        g, f, v = GEOS[c.geo], FORMS[c.form], dict(c.var)
        self.c, self.g, self.f = c, g, f
        self.B, self.H, self.W, self.N, self.K = g.B, g.H, g.W, g.N, c.K
        self.M = g.B * g.H * g.W
        self.stats = c.form == "f1_relu_stats" and (g.H * g.W) % BM == 0
        self.bias = c.form == "f1_relu_stats" or c.form == "f4_f32"
        self.relu = c.form == "f1_relu_stats" if relu is None else bool(relu)
        self.f32 = c.form == "f4_f32"
        self.beta = (1.0 if c.form in ("f6_dgrad_beta", "f9_bnsum_y", "f10_bnsum_bits") else 0.0) if beta is None else beta
        self.offer = f.offer
        self.act_hi = v.get("act_hi", float("inf"))
        self.stride = 2 if c.form == "f3_stride2" else 1
        self.up = 2 if (c.form == "f7_dgrad_up2" or v.get("up2")) else 1
        odd = (v.get("odd", False) or v.get("up2") == 2) if odd is None else odd
        s = self.stride
        self.Hs, self.Ws = (g.H * s - (1 if odd and s == 2 else 0), g.W * s - (1 if odd and s == 2 else 0))
        u = self.up
        self.Hd, self.Wd = (g.H * u - (1 if odd and u == 2 else 0), g.W * u - (1 if odd and u == 2 else 0))
        N = g.N
        if c.form == "f2_narrow":
            self.n_store, self.coff = N - 24, 8
            self.ld = self.n_store + 24
        elif self.f32:
            self.n_store, self.coff = N - 4, 4          # % 4 == 0, % 8 != 0
            self.ld = self.n_store + 12
        else:
            self.n_store, self.coff = N, 8
            self.ld = N + 16
        self.dst_img = self.Hd * self.Wd + v.get("extra", 0)
        self.rows = FRONT + g.B * self.dst_img + TAIL

    def desc(self, w, bias):
        from cvlite import ops_nn as nn
        if self.f.kind == "fwd":
            sg = nn.seg(self.H, self.W, self.Hs, self.Ws, w, bias, dst_base=FRONT, dst_img=self.dst_img)
            return nn.make_desc(nn.FWD, self.B, self.K, 1, 1, self.stride, 0, 0, self.N, self.n_store, self.ld, [sg],
                                dst_coff=self.coff, dst_f32=self.f32, relu_out=self.relu, beta=self.beta)
        sg = nn.seg(self.Hd, self.Wd, self.H, self.W, w, None, dst_base=FRONT, dst_img=self.dst_img)
        return nn.make_desc(nn.DGRAD, self.B, self.K, 1, 1, self.up, 0, 0, self.N, self.n_store, self.ld, [sg],
                            dst_coff=self.coff, beta=self.beta)

    def dst_index(self, device):
        """Destination rows of GEMM rows 0 .. M-1, and the destination rows of the gap pixels."""
        r = torch.arange(self.M, device=device, dtype=torch.int64)
        hw = self.H * self.W
        img, q = r // hw, r % hw
        y, x = q // self.W, q % self.W
        idx = FRONT + img * self.dst_img + y * self.up * self.Wd + x * self.up
        gaps = None
        if self.up != 1:
            m = torch.ones(self.rows, dtype=torch.bool, device=device)
            m[idx] = False
            m[:FRONT] = False
            m[FRONT + self.B * self.dst_img:] = False
            if self.dst_img > self.Hd * self.Wd:
                rr = (torch.arange(self.rows, device=device) - FRONT) % self.dst_img
                m &= rr < self.Hd * self.Wd
            gaps = m.nonzero().view(-1)
        return idx, gaps

    def launches(self):
        """The launches of one case: Layouts that differ in (relu, beta) or (beta, odd map)."""
        v = dict(self.c.var)
        if self.c.form == "f4_f32":
            return [Layout(self.c, relu=r, beta=b) for r, b in v["pairs"]]
        if self.c.form == "f7_dgrad_up2":
            return [Layout(self.c, beta=b, odd=bool(o)) for b, o in v["pairs"]]
        return [self]


def plan_grid(d, stats, offer):
    from cvlite import _lib
    k, t, gr, nt = (ctypes.c_int32(-1) for _ in range(4))
    st = _lib.load().cvl_conv_igemm_plan_grid(ctypes.byref(d), int(stats), int(offer), 0, ctypes.byref(k), ctypes.byref(t),
                                              ctypes.byref(gr), ctypes.byref(nt))
    assert st == 0
    return k.value, t.value, gr.value, nt.value


def chunks_of(m_tiles, npad, grid, ntile):
    """Tiles per workgroup chunk, as conv_igemm_p.hip cuts them (one entry per M chunk)."""
    ntn = npad // ntile
    nmc = grid // ntn
    mchunk = -(-m_tiles // nmc)
    return [max(0, min(mchunk, m_tiles - i * mchunk)) for i in range(nmc)]


def check_geometry(lay, plan, k64):
    """Asserts the planner's answer for this launch: P, the K-tile depth, and the geometry properties
    the case is there for, derived from the planned grid and N tile."""
    kern, ktile, grid, ntile = plan
    g = lay.g
    assert kern == CK_P, plan
    assert ktile == (64 if lay.K % 64 == 0 and k64 and ntile != 256 else 32), plan
    m_tiles = -(-lay.M // BM)
    ch = chunks_of(m_tiles, lay.N, grid, ntile)
    assert sum(ch) == m_tiles
    plain = not lay.offer or g.N == 64
    if plain:
        assert (grid, ntile) == g.plan and ch == g.chunks, (plan, ch)
    assert max(ch) >= 2, ch                                        # multi: the stream crosses tiles
    busy = [n for n in ch if n]
    props = g.props if plain else g.props & {"multi", "ragged"}
    if "idle" in props:
        assert len(busy) < len(ch), ch
    if "uneven" in props:
        assert busy[-1] < busy[0], ch
    if "ragged" in props:
        assert lay.M % BM, lay.M
    if "late" in props:
        assert busy[-1] >= 2, ch
    if "g8" in props:
        assert grid % 8, grid
    if "straddle" in props:
        per, mc = (g.H * g.W) // BM, max(ch)                       # tiles per image, per chunk
        assert (g.H * g.W) % BM == 0
        assert any(t % mc for t in range(per, m_tiles, per)) or any((i * mc) % per for i in range(1, len(busy))), ch
    return ktile, ntile


# ---------------------------------------------------------------------------------------------------
# comparison helpers (device independent)
# ---------------------------------------------------------------------------------------------------
def bits(t):
    return t.view(torch.int16) if t.dtype == BF else (t.view(torch.int32) if t.dtype == F32 else t)


def check_block(got, init, idx, c0, c1, ref, rtol, atol, gaps=None, gaps_zero=False):
    """got / init: the whole destination [rows, ld] after / before the launch.  The block (rows idx,
    columns c0:c1) against ref; the gap pixels' block columns exactly 0 (gaps_zero) or untouched;
    everything else bit-unchanged."""
    torch.testing.assert_close(got[idx, c0:c1].double(), ref, rtol=rtol, atol=atol)
    touched = torch.zeros(got.shape, dtype=torch.bool, device=got.device)
    touched[idx, c0:c1] = True
    if gaps is not None and gaps_zero:
        assert bool((got[gaps, c0:c1] == 0).all()), "gap pixels not zero"
        touched[gaps, c0:c1] = True
    same = bits(got) == bits(init)
    bad = ~(same | touched)
    assert not bool(bad.any()), "%d elements outside the block changed, first (row, col) %s" % (
        int(bad.sum()), bad.nonzero()[0].tolist())


def check_stats(val, got, idx, c0, c1, B):
    """BN statistics [B, n, 2] against the float64 sums of the stored output."""
    out = got[idx, c0:c1].double().view(B, -1, c1 - c0)
    exp = torch.stack([out.sum(1), (out * out).sum(1)], -1)
    torch.testing.assert_close(val, exp, rtol=1e-5, atol=1e-3)


def check_sums(val, got, idx, c0, c1, B, mask, xh):
    """Fused BN-backward sums [B, n, 2] against (stored dX) . mask and (stored dX) . mask . xhat."""
    n = c1 - c0
    g = got[idx, c0:c1].double().view(B, -1, n) * mask.view(B, -1, n).double()
    gx = g * xh.view(B, -1, n).double()
    ref = torch.stack([g.sum(1), gx.sum(1)], -1)
    rabs = torch.stack([g.abs().sum(1), gx.abs().sum(1)], -1)
    assert float(ref.abs().max()) > 0
    for b in range(B):
        e = red_err(val[b], ref[b], rabs[b])
        assert e <= 1e-6, "image %d: red_err %.3e" % (b, e)


def round_bf16(t):
    return t.to(BF).double()


def reference(lay, src_rows, wm, bias, old_blk):
    """float64 result of the block [M, n_store] from the GEMM's source rows [M, K] (bf16 values)."""
    r = torch.matmul(src_rows.double(), wm.double().t())[:, :lay.n_store]
    if bias is not None:
        r = r + bias[:lay.n_store].double()
    if lay.relu:
        r = r.clamp_min(0)
    if lay.f32:
        return r + lay.beta * old_blk.double() if lay.beta else r
    if lay.beta:
        return round_bf16(round_bf16(r) + lay.beta * old_blk.double())
    return r


def tolerances(lay):
    if lay.f32:
        return 1e-4, 1e-4
    return 1e-2, (3e-2 if lay.beta else 2e-2)


# ---------------------------------------------------------------------------------------------------
# CPU: the case list, the planner's geometry, the comparison
# ---------------------------------------------------------------------------------------------------
def test_case_list_coverage():
    """Every geometry meets every form it can run; every form meets the K depths and nk below, at and
    above the ring depth; the long K reaches the counted waits' upper buckets."""
    seen = collections.defaultdict(set)
    rel = collections.defaultdict(set)
    ks = collections.defaultdict(set)
    for c in CASES:
        g, f = GEOS[c.geo], FORMS[c.form]
        seen[c.form].add(c.geo)
        ks[c.form].add(c.K)
        bn = 64 if f.offer else g.plan[1]
        for on in k64_settings(c):
            bk = 64 if on and c.K % 64 == 0 and bn != 256 else 32
            nk, D = c.K // bk, ring_depth(bn, bk)
            rel[c.form].add("<" if nk < D else ("=" if nk == D else ">"))
    assert ring_depth(64, 64) == 2 and ring_depth(128, 64) == 2 and ring_depth(256, 32) == 3
    assert ring_depth(64, 32) == 6 and ring_depth(128, 32) == 5
    for fid, f in FORMS.items():
        want = {gid for gid, g in GEOS.items() if not f.whole or (g.H * g.W) % BM == 0}
        assert seen[fid] == want, (fid, want - seen[fid])
        assert ks[fid] >= K_REQUIRED | {2048}, (fid, ks[fid])
        assert rel[fid] == {"<", "=", ">"}, (fid, rel[fid])
    assert {gid for gid, g in GEOS.items() if (g.H * g.W) % BM} == {"D", "H", "I"}
    assert len({case_id(c) for c in CASES}) == len(CASES)


def test_planned_geometry_of_every_case(dispatch):
    """Host only: the planner gives every launch of every case to P with several tiles per workgroup and
    the case's own property (the GPU tests assert the same on the descriptors they run)."""
    w = torch.zeros(16, dtype=BF)
    b = torch.zeros(16)
    for c in CASES:
        for lay in Layout(c).launches():
            for on in k64_settings(c):
                keys = {h.split("=")[0] for h in lay.g.hooks}
                dispatch("p_k64=%d" % on, *([h for h in ("p_wgs=256", "p_bn=0") if h.split("=")[0] not in keys] +
                                            list(lay.g.hooks)))
                d = lay.desc(w, b if lay.bias else None)
                check_geometry(lay, plan_grid(d, lay.stats, lay.offer), on)
    # and the hook's range: at most 256 workgroups, at least 1
    lay = Layout(CASES[0])
    d = lay.desc(w, b)
    for n, grid in ((100000, 16), (0, 1), (-3, 1), (5, 5)):
        dispatch("p_wgs=%d" % n, "p_bn=0")
        assert plan_grid(d, 1, 0)[2] == grid, n


def test_comparison_catches_single_defects():
    """check_block on a correct result with one defect each: a row shifted by one pixel, one 8-channel
    chunk of one row left at its old value, one element written outside the block."""
    g = torch.Generator().manual_seed(5)
    B, HW, n, ld, c0, img = 2, 40, 16, 32, 8, 45
    rows = FRONT + B * img + TAIL
    idx = torch.cat([FRONT + b * img + torch.arange(HW) for b in range(B)])
    conv = torch.randn(B * HW, n, generator=g, dtype=F64)
    for beta in (0.0, 1.0):
        init = (torch.randn(rows, ld, generator=g) * 0.5).to(BF) if beta else torch.full((rows, ld), SENTINEL, dtype=BF)
        ref = round_bf16(round_bf16(conv) + init[idx, c0:c0 + n].double()) if beta else conv
        good = init.clone()
        good[idx, c0:c0 + n] = ref.to(BF)
        tol = dict(rtol=1e-2, atol=3e-2 if beta else 2e-2)
        check_block(good, init, idx, c0, c0 + n, ref, **tol)
        shifted = good.clone()
        shifted[idx[17]] = good[idx[18]]
        stale = good.clone()
        stale[idx[50], c0 + 8:c0 + 16] = init[idx[50], c0 + 8:c0 + 16]
        outside = []
        for r, col in ((idx[3], c0 - 1), (idx[3], c0 + n), (FRONT - 1, c0), (FRONT + HW, c0 + 2), (rows - 1, ld - 1)):
            t = good.clone()
            t[r, col] = 0.25
            outside.append(t)
        for bad in [shifted, stale] + outside:
            with pytest.raises(AssertionError):
                check_block(bad, init, idx, c0, c0 + n, ref, **tol)
    # the scatter's gap pixels: exactly zero with beta 0
    init = torch.full((rows, ld), SENTINEL, dtype=BF)
    sub = idx[::2]
    gaps = idx[1::2]
    good = init.clone()
    good[sub, c0:c0 + n] = conv[::2].to(BF)
    good[gaps, c0:c0 + n] = 0
    check_block(good, init, sub, c0, c0 + n, conv[::2], 1e-2, 2e-2, gaps=gaps, gaps_zero=True)
    bad = good.clone()
    bad[gaps[4], c0 + 3] = SENTINEL
    with pytest.raises(AssertionError):
        check_block(bad, init, sub, c0, c0 + n, conv[::2], 1e-2, 2e-2, gaps=gaps, gaps_zero=True)
    bad = good.clone()
    bad[gaps[4], c0 + 3] = 0.5
    with pytest.raises(AssertionError):
        check_block(bad, init, sub, c0, c0 + n, conv[::2], 1e-2, 2e-2, gaps=gaps, gaps_zero=False)
    # statistics and fused sums: one row's worth of error fails
    val = torch.stack([good[sub, c0:c0 + n].double().view(1, -1, n).sum(1),
                       (good[sub, c0:c0 + n].double() ** 2).view(1, -1, n).sum(1)], -1)
    check_stats(val, good, sub, c0, c0 + n, 1)
    with pytest.raises(AssertionError):
        check_stats(val + 0.05, good, sub, c0, c0 + n, 1)
    mask = torch.rand(sub.numel(), n, generator=g) > 0.5
    xh = torch.randn(sub.numel(), n, generator=g)
    gg = good[sub, c0:c0 + n].double() * mask.double()
    sums = torch.stack([gg.sum(0, keepdim=True), (gg * xh.double()).sum(0, keepdim=True)], -1)
    check_sums(sums, good, sub, c0, c0 + n, 1, mask, xh)
    off = sums.clone()
    off[0, 5, 1] += float(gg[7, 5] * xh[7, 5]) + 1e-3
    with pytest.raises(AssertionError):
        check_sums(off, good, sub, c0, c0 + n, 1, mask, xh)


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
def rnd(shape, scale, gen):
    return (torch.randn(shape, generator=gen, device=DEV, dtype=F32) * scale).to(BF)


def last_launch():
    from cvlite import _lib
    lib = _lib.load()
    return lib.cvl_conv_igemm_last_kernel(), lib.cvl_conv_igemm_last_ktile()


def run_launch(lay, on, dispatch, seed):
    from cvlite import ops_nn as nn
    dev = torch.device(DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    dispatch("p_k64=%d" % on, *lay.g.hooks)
    B, K, N = lay.B, lay.K, lay.N
    # operands: the GEMM is out[M, N] = src_rows[M, K] . wm[N, K]^T for the forward (wm: the packed forward
    # operand) and the data gradient (wm: the packed data-gradient operand) alike
    wm = rnd((N, K), K ** -0.5, g)
    bias = torch.randn(N, generator=g, device=dev) if lay.bias else None
    src = rnd((B, lay.Hs, lay.Ws, K), 1.0, g)
    src_rows = src[:, ::lay.stride, ::lay.stride][:, :lay.H, :lay.W].reshape(lay.M, K)
    dt = F32 if lay.f32 else BF
    if lay.beta:
        init = (torch.randn((lay.rows, lay.ld), generator=g, device=dev) * 0.5).to(dt)
    else:
        init = torch.full((lay.rows, lay.ld), SENTINEL, dtype=dt, device=dev)
    idx, gaps = lay.dst_index(dev)
    c0, c1 = lay.coff, lay.coff + lay.n_store
    ref = reference(lay, src_rows, wm, bias, init[idx, c0:c1])
    d = lay.desc(wm, bias)
    ktile, ntile = check_geometry(lay, plan_grid(d, lay.stats, lay.offer), on)
    dst = init.clone()
    st = sums = None
    if lay.offer:
        # z, y (and y's bitmap) are laid out as the destination; (mean, rstd) per (image, channel)
        z = rnd((lay.rows, lay.ld), 1.5, g)
        ybuf = rnd((lay.rows, lay.ld), 1.0, g)
        zb = z[idx, c0:c1].float().view(B, -1, N)
        mr = torch.stack([zb.mean(1), torch.rsqrt(zb.var(1, unbiased=False) + 1e-3)], -1).contiguous()
        gamma = torch.rand(N, generator=g, device=dev) + 0.5
        bb = torch.randn(N, generator=g, device=dev) * 0.3
        sums = nn.bn_acc(B, N, dev)
        act, xh = bn_affine32(zb, mr[:, None, :, 0], mr[:, None, :, 1], gamma, bb)
        if lay.offer == 1:
            mask = (act > 0) & (act < lay.act_hi)
            fused = nn.conv_igemm_dgrad_bnsum(d, src, dst, z, mr, gamma, bb, sums, act_hi=lay.act_hi)
        else:
            mask = ybuf[idx, c0:c1].float().view(B, -1, N) > 0
            yarg = ybuf
            if lay.offer == 3:
                # the bitmap carries the mask; the y tensor passed along says the opposite, so a launch
                # that read y instead would miss the sums
                yarg = -ybuf
                bmap = nn.attach_relu_bits(yarg)
                on8 = (ybuf.view(-1, 8).float() > 0).to(torch.int32)
                bmap.copy_((on8 << torch.arange(8, device=dev, dtype=torch.int32)).sum(-1).to(torch.uint8))
            fused = nn.conv_igemm_dgrad_bnsum_res(d, src, dst, yarg, z, mr, gamma, bb, sums)
        assert fused is True
    elif lay.stats:
        st = nn.bn_acc(B, lay.n_store, dev)
        nn.conv_igemm(d, src, dst, st)
    else:
        nn.conv_igemm(d, src, dst)
    assert last_launch() == (CK_P, ktile), last_launch()
    torch.cuda.synchronize()
    rtol, atol = tolerances(lay)
    err = (dst[idx, c0:c1].double() - ref).abs().max()
    print("%s k64=%d relu=%d beta=%g map %dx%d: ktile %d ntile %d max|err| %.3e" % (
        case_id(lay.c), on, lay.relu, lay.beta, lay.Hd, lay.Wd, ktile, ntile, float(err)))
    check_block(dst, init, idx, c0, c1, ref, rtol, atol, gaps=gaps, gaps_zero=lay.beta == 0.0)
    if st is not None:
        check_stats(nn.bn_acc_value(st), dst, idx, c0, c1, B)
    if sums is not None:
        check_sums(nn.bn_acc_value(sums), dst, idx, c0, c1, B, mask, xh)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_p_stream_against_fp64(case, dispatch):
    for li, lay in enumerate(Layout(case).launches()):
        for on in k64_settings(case):
            run_launch(lay, on, dispatch, 1000 * CASES.index(case) + 10 * li + on)
