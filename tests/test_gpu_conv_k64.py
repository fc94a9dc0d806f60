"""64-deep K-tiles (128-byte operand rows) of the persistent 1x1 kernel (conv_igemm_p.hip).

The 64-deep form multiplies the two 32-deep halves of a K-tile in k order, so its accumulation
sequence is the 32-deep form's: every case runs with CVL_DISPATCH=p_k64=1 and =0 and compares the
raw bits (outputs, BN statistics and fused BN-backward sums).  The maps below have fewer tiles than
the persistent grid, so every workgroup runs one tile; the (2, 32) map runs a second time with
CVL_DISPATCH=p_wgs=4 (2 to 8 tiles per workgroup), which holds the identity across tiles as well
(the cross-tile stream against fp64: tests/test_gpu_conv_p_stream.py).  Every case also asserts
cvl_conv_igemm_last_ktile(), so a path that is silently not taken fails: 64 where K % 64 == 0, 32
for K = 96 and with the flag off.  One forward and one data-gradient mode are checked against fp64
as well (tolerances as tests/test_gpu_conv_production.py: one bf16 rounding of the result,
rtol 1e-2 / atol 2e-2; BN statistics rtol 1e-5 of the sums of the bf16 outputs)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64

CK_P = 16


def last_kernel():
    from cvlite import _lib
    lib = _lib.load()
    code = lib.cvl_conv_igemm_last_kernel()
    return code, lib.cvl_conv_kernel_name(code).decode(), lib.cvl_conv_igemm_last_ktile()


def packs(w, npad=None, cout_pad=None):
    from cvlite import ops_nn as nn
    k, _, cin, cout = w.shape
    npad = npad or max(32, (cout + 31) // 32 * 32)
    cout_pad = cout_pad or npad
    cin_pad = (cin + 31) // 32 * 32
    wf = torch.empty((npad, k * k * cin), dtype=BF, device="cuda")
    wd = torch.empty((cin_pad, k * k * cout_pad), dtype=BF, device="cuda")
    nn.pack_conv_weights(w.float().contiguous(), k, k, cin, cout, cin, npad, wf, cin_pad, cout_pad, wd)
    return wf, wd


def rnd(shape, scale, gen):
    return (torch.randn(shape, generator=gen, device="cuda", dtype=torch.float32) * scale).to(BF)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF else t


# ---------------------------------------------------------------------------------------------
# P: the persistent 1x1 kernel
# ---------------------------------------------------------------------------------------------
P_MODES = ["fwd_stats", "fwd_s2", "fwd_f32", "dgrad", "dgrad_beta", "dgrad_up2", "bnsum", "bnsum_res"]
# B, H: one tile per image and fewer tiles than workgroups; several tiles per image; ragged (M = 192:
# one partly absent tile, no statistics)
P_MAPS = [(3, 16), (2, 32), (3, 8)]
# (B, H, p_wgs): every map on the default grid (256: one tile per workgroup at these sizes), then the
# 8-tile map on 4 workgroups
P_RUNS = [(B, H, 256) for B, H in P_MAPS] + [(2, 32, 4)]


def p_case(mode, K, N, B, H):
    """Builds the operands of one 1x1 launch (GEMM depth K, width N, B maps of H x H output rows) and
    returns run() -> tuple of result tensors, and fp64 reference of the first result (or None)."""
    from cvlite import ops_nn as nn
    g = torch.Generator(device="cuda").manual_seed(K * 1000 + N + B * 10 + H)
    ref = None
    if mode.startswith("fwd"):
        s = 2 if mode == "fwd_s2" else 1
        Hs = H * s
        x = rnd((B, Hs, Hs, K), 1.0, g)
        w = rnd((1, 1, K, N), K ** -0.5, g).to(F64)
        bias = torch.randn(N, generator=g, device="cuda")
        wf, _ = packs(w)
        f32 = mode == "fwd_f32"
        stats_on = mode == "fwd_stats" and (H * H) % 256 == 0
        d = nn.make_desc(nn.FWD, B, K, 1, 1, s, 0, 0, N, N, N, [nn.seg(H, H, Hs, Hs, wf, bias)], dst_f32=f32,
                         relu_out=not f32)
        if mode == "fwd_stats":
            ref = torch.relu(torch.matmul(x.to(F64), w[0, 0]) + bias.to(F64))

        def run():
            out = torch.full((B, H, H, N), 7.0, dtype=torch.float32 if f32 else BF, device="cuda")
            st = nn.bn_acc(B, N, "cuda") if stats_on else None
            nn.conv_igemm(d, x, out, st)
            return (out,) + ((st, nn.bn_acc_value(st)) if stats_on else ())
        return run, ref
    # data gradients: dy has K channels, dx N; the forward conv is N -> K
    w = rnd((1, 1, N, K), K ** -0.5, g).to(F64)
    _, wd = packs(w)
    dy = rnd((B, H, H, K), 0.5, g)
    up = 2 if mode == "dgrad_up2" else 1
    Hd = H * up
    beta = 1.0 if mode in ("dgrad_beta", "bnsum_res") else 0.0
    old = rnd((B, Hd, Hd, N), 0.5, g)
    d = nn.make_desc(nn.DGRAD, B, K, 1, 1, up, 0, 0, N, N, N, [nn.seg(Hd, Hd, H, H, wd)], beta=beta)
    if mode == "dgrad":
        ref = torch.matmul(dy.to(F64), w[0, 0].t())
    if mode in ("bnsum", "bnsum_res"):
        z = rnd((B, H, H, N), 1.5, g)
        y = torch.relu(rnd((B, H, H, N), 1.0, g))
        mr = torch.empty((B, N, 2), dtype=torch.float32, device="cuda")
        zf = z.double().view(B, H * H, N)
        mr[..., 0] = zf.mean(1).float()
        mr[..., 1] = torch.rsqrt(zf.var(1, unbiased=False) + 1e-3).float()
        gamma = torch.rand(N, generator=g, device="cuda") + 0.5
        bb = torch.randn(N, generator=g, device="cuda") * 0.3

    def run():
        dx = old.clone() if beta else torch.full((B, Hd, Hd, N), 7.0, dtype=BF, device="cuda")
        if mode == "bnsum":
            sums = nn.bn_acc(B, N, "cuda")
            assert nn.conv_igemm_dgrad_bnsum(d, dy, dx, z, mr, gamma, bb, sums)
            return dx, sums
        if mode == "bnsum_res":
            sums = nn.bn_acc(B, N, "cuda")
            assert nn.conv_igemm_dgrad_bnsum_res(d, dy, dx, y, z, mr, gamma, bb, sums)
            return dx, sums
        nn.conv_igemm(d, dy, dx)
        return (dx,)
    return run, ref


@pytest.mark.parametrize("N", [64, 128, 256])
@pytest.mark.parametrize("K", [64, 128, 192, 96])
@pytest.mark.parametrize("mode", P_MODES)
def test_p_k64_bit_identical_to_k32(dispatch, mode, K, N):
    """K = 64: one K-tile per tile (with p_wgs=4 the stream runs across tiles only); 128 = the ring
    depth D; 192: an odd count above D; 96: the 32-deep fallback.  N 64 / 128 / 256: the 64- and
    128-wide tiles (one and two B pieces per wave)."""
    if mode == "bnsum_res":
        dispatch("bnsum_res_min_hw=0")
    for B, H, wgs in P_RUNS:
        dispatch("p_wgs=%d" % wgs)
        if (H * H) % 256 and mode in ("bnsum", "bnsum_res"):
            continue                           # the fused sums need whole tiles per image
        run, ref = p_case(mode, K, N, B, H)
        res = []
        for on in (1, 0):
            dispatch("p_k64=%d" % on)
            r = run()
            code, name, kt = last_kernel()
            assert code == CK_P, name
            assert kt == (64 if on and K % 64 == 0 else 32), (kt, on, K)
            torch.cuda.synchronize()
            res.append(r)
        for a, b in zip(*res):
            assert torch.equal(bits(a), bits(b)), "%s K %d N %d B %d H %d wgs %d" % (mode, K, N, B, H, wgs)
        if ref is not None:
            out = res[0][0].to(F64).view(ref.shape)
            torch.testing.assert_close(out, ref, rtol=1e-2, atol=2e-2)
            if len(res[0]) == 3:               # BN statistics against the fp64 sums of the bf16 outputs
                exp = torch.stack([out.sum((1, 2)), (out * out).sum((1, 2))], -1)
                torch.testing.assert_close(res[0][2], exp, rtol=1e-5, atol=1e-3)


def test_tower_kernel_reports_32_deep(dispatch):
    """The 256 x 256 tower kernel keeps its 32-deep K-tiles (its 64-deep form did not win: DESIGN
    section 3), and the query says so for a Cin 64 launch."""
    from cvlite import ops_nn as nn
    dispatch("l_min_tiles=1", "l256_min_tiles=1", "no_h")
    B, H, C, N = 2, 16, 64, 256
    g = torch.Generator(device="cuda").manual_seed(3)
    x = rnd((B, H, H, C), 1.0, g)
    w = rnd((3, 3, C, N), (9 * C) ** -0.5, g).to(F64)
    wf, _ = packs(w)
    d = nn.make_desc(nn.FWD, B, C, 3, 3, 1, 1, 1, N, N, N, [nn.seg(H, H, H, H, wf, None)])
    out = torch.empty((B, H, H, N), dtype=BF, device="cuda")
    nn.conv_igemm(d, x, out)
    code, name, kt = last_kernel()
    assert code == 7 and kt == 32, (name, kt)
    xp = torch.nn.functional.pad(x.to(F64), (0, 0, 1, 1, 1, 1))
    ref = sum(torch.matmul(xp[:, r:r + H, s:s + H, :], w[r, s]) for r in range(3) for s in range(3))
    torch.testing.assert_close(out.to(F64), ref, rtol=1e-2, atol=2e-2)
