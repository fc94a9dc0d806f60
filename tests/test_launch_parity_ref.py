"""CPU checks of the float64 restatements the teacher-forced launch-parity harness
(tests/launch_parity.py) compares the GPU against: the explicit im2col conv forward / data
gradient / weight gradient (TF 'same' asymmetric pads, stride 2, cropped borders) against torch's
own float64 conv + autograd, and the pool / up-sample references against torch's ops."""
import torch
import torch.nn.functional as F

import launch_parity as lp


def _same(n, k, s):
    out = -(-n // s)
    return out, max((out - 1) * s + k - n, 0) // 2


def _torch_conv(x, w, s, pt, pl, Ho, Wo):
    """NHWC / OHWI float64 conv via F.conv2d with explicit asymmetric padding."""
    xn = x.permute(0, 3, 1, 2)
    KH, KW = w.shape[1], w.shape[2]
    H, W = xn.shape[2], xn.shape[3]
    pb = max(0, (Ho - 1) * s + KH - H - pt)
    pr = max(0, (Wo - 1) * s + KW - W - pl)
    y = F.conv2d(F.pad(xn, (pl, pr, pt, pb)), w.permute(0, 3, 1, 2), stride=s)
    return y[:, :, :Ho, :Wo].permute(0, 2, 3, 1)


def test_conv_restatement_vs_torch():
    g = torch.Generator().manual_seed(0)
    for (H, W, k, s, Ci, O) in [(9, 7, 3, 1, 5, 6), (10, 11, 3, 2, 4, 3), (8, 8, 1, 2, 6, 5), (13, 13, 7, 2, 3, 4),
                                (4, 4, 3, 2, 2, 2)]:
        (Ho, pt), (Wo, pl) = _same(H, k, s), _same(W, k, s)
        x = torch.randn((2, H, W, Ci), generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn((O, k, k, Ci), generator=g, dtype=torch.float64, requires_grad=True)
        y = _torch_conv(x, w, s, pt, pl, Ho, Wo)
        torch.testing.assert_close(lp.conv_fwd64(x.detach(), w.detach(), s, pt, pl, Ho, Wo), y.detach())
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        gx, gw = torch.autograd.grad(y, (x, w), dy)
        torch.testing.assert_close(lp.conv_dgrad64(dy, w.detach(), s, pt, pl, H, W), gx)
        torch.testing.assert_close(lp.conv_wgrad64(x.detach(), dy, k, k, s, pt, pl), gw.permute(1, 2, 3, 0))


def test_pool_and_upsample_restatements():
    g = torch.Generator().manual_seed(1)
    a = torch.randn((2, 9, 8, 3), generator=g).clamp_min(0).to(torch.bfloat16)
    y, arg = lp._pool3_ref(a)
    ref = F.max_pool2d(F.pad(a.float().permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    torch.testing.assert_close(y, ref)
    # argmax is the first maximum in window order; the backward routes dy there
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx = lp._pool3_bwd_ref(dy, arg, 9, 8)
    ap = F.pad(a.double().permute(0, 3, 1, 2), (1, 1, 1, 1)).requires_grad_()
    win = F.unfold(ap, 3, stride=2)
    # reference gradient: route to the first max tap, then drop the padding rows / cols
    B, C = 2, 3
    w9 = win.view(B, C, 9, -1)
    first = (w9 == w9.max(2, keepdim=True).values).double()
    first = first * (first.cumsum(2) == 1).double()
    gcols = (first * dy.permute(0, 3, 1, 2).reshape(B, C, 1, -1)).view(B, C * 9, -1)
    gpad = F.fold(gcols, (ap.shape[2], ap.shape[3]), 3, stride=2)
    torch.testing.assert_close(dx, gpad[:, :, 1:-1, 1:-1].permute(0, 2, 3, 1))
    # bilinear x2 (Keras half-pixel): out[2i] = .75 x[i] + .25 x[i-1], out[2i+1] = .75 x[i] + .25 x[i+1]
    # (edges clamped)
    p = torch.randn((1, 1, 4, 1), generator=g, dtype=torch.float64)
    up = lp._bilinear_up2(p)[0, 0, :, 0]
    x = p[0, 0, :, 0]
    xm, xp = torch.cat([x[:1], x[:-1]]), torch.cat([x[1:], x[-1:]])
    ref = torch.stack([0.75 * x + 0.25 * xm, 0.75 * x + 0.25 * xp], 1).reshape(-1)
    torch.testing.assert_close(up, ref)


def test_gconv_pack_restatement_and_decode():
    """The grouped 3x3 slab images: the restated pack written out element by element, and the master
    kernel the checks decode back from either image."""
    g = torch.Generator().manual_seed(4)
    for C, Cg in ((64, 4), (32, 32), (64, 16)):
        w = torch.randn((3, 3, Cg, C), generator=g)
        pf, pd = lp.gconv_pack_ref(w, Cg)
        pf4, pd4 = pf.view(C // 32, 9, 32, 32), pd.view(C // 32, 9, 32, 32)
        wb = w.to(torch.bfloat16).reshape(9, Cg, C)
        for slab, tap, a, b in [(0, 0, 0, 0), (C // 32 - 1, 5, 9, 10), (0, 8, 31, 28), (0, 3, 4, 3), (0, 2, 17, 30)]:
            same = a // Cg == b // Cg
            # forward [out a][in b]; data gradient [out = input channel a][in = output channel b], tap flipped
            assert float(pf4[slab, tap, a, b]) == (float(wb[tap, b % Cg, slab * 32 + a]) if same else 0.0)
            assert float(pd4[slab, tap, a, b]) == (float(wb[8 - tap, a % Cg, slab * 32 + b]) if same else 0.0)
        assert int((pf4 != 0).sum()) <= 9 * C * Cg
        want = w.to(torch.bfloat16).float()
        assert torch.equal(lp.gconv_w_from_fwd(pf, C, Cg), want)
        assert torch.equal(lp.gconv_w_from_dgrad(pd, C, Cg), want)


def test_gconv_checks_pass_a_correct_launch_and_flag_a_wrong_one():
    """check_gconv_fwd / dgrad / wgrad on the CPU with a stand-in launch that writes the float64 conv2d
    result (rounded as the kernel stores it): all records pass; one element off by a bf16 step, or one
    weight-gradient entry off by 1e-3 of its scale, fails."""
    import gconv_ref as G
    from cvlite import ops_nn
    for (B, H, W, C, Cg, s) in [(2, 9, 7, 64, 4, 1), (3, 8, 10, 32, 32, 2)]:
        inp = G.make_inputs("random", B, H, W, C, Cg, s, seed=5)
        x, w, dy = inp["x"], inp["w"], inp["dy"]
        pf, pd = lp.gconv_pack_ref(w, Cg)
        xd = x.double().permute(0, 3, 1, 2).requires_grad_()
        wd = w.to(torch.bfloat16).double().requires_grad_()
        y64 = F.conv2d(F.pad(xd, (1, 1, 1, 1)), wd.permute(3, 2, 0, 1), None, s, groups=C // Cg)
        gx, gw = torch.autograd.grad(y64, (xd, wd), dy.double().permute(0, 3, 1, 2))
        y64, gx = y64.detach().permute(0, 2, 3, 1), gx.permute(0, 2, 3, 1)
        for wrong in (False, True):
            p = lp.LaunchParity(imgs=2)
            p.nn = ops_nn

            def fwd(x_, wf_, y_, Cg_, s_, stats_):
                y_.copy_(y64.to(torch.bfloat16))
                if wrong:
                    y_[B - 1, 2, 3, 5] = (y_[B - 1, 2, 3, 5].float() * (1 + 2.0 ** -6) + 1e-3).to(torch.bfloat16)

            def dgrad(dy_, wd_, dx_, Cg_, s_, beta=0.0):
                dx_.copy_((gx + beta * dx_.double()).to(torch.bfloat16))
                if wrong:
                    dx_[0, H - 1, W - 1, C - 1] = 0.0

            def wgrad(x_, dy_, dw_, s_, beta=0.0):
                dw_.copy_((gw + beta * dw_.double()).float())
                if wrong:
                    dw_[2, 2, Cg - 1, C - 1] += 1e-3 * float(gw.abs().mean())

            lp.check_gconv_fwd(p, "gconv3x3_fwd", fwd, x, pf, torch.empty(y64.shape, dtype=torch.bfloat16), Cg, s)
            lp.check_gconv_dgrad(p, "gconv3x3_dgrad", dgrad, dy, pd, inp["dx_old"].clone(), Cg, s, beta=1.0)
            lp.check_gconv_wgrad(p, "gconv3x3_wgrad", wgrad, x, dy, inp["dw_old"].clone(), s, beta=2.0)
            assert [r.what for r in p.records] == ["y", "dx", "dW"]
            if wrong:
                assert len(p.failures()) == 3, p.table()
            else:
                assert not p.failures(), p.table()
                assert all(0 < r.err <= 1 for r in p.records)


def test_bn_affine_mask_is_fma_exact():
    g = torch.Generator().manual_seed(2)
    z = torch.randn(4096, generator=g).to(torch.bfloat16)
    m, rs, ga, be = torch.tensor(0.1), torch.tensor(1.7), torch.tensor(0.9), torch.tensor(-0.05)
    a, xh = lp.bn_affine32(z, m, rs, ga, be)
    exact = ga.double() * ((z.float() - m) * rs).double() + be.double()
    assert torch.equal(a > 0, exact > 0)


def test_row_err_sees_one_row_where_rel_l2_does_not():
    """The worst-row criterion of the conv destinations: bf16 rounding stays below 2^-8 (two roundings:
    2^-7), all-zero rows do not divide by nothing, and ONE wrong row of a large block -- which moves
    the whole-tensor rel-L2 by far less than its tolerance -- scores above 1."""
    g = torch.Generator().manual_seed(3)
    ref = torch.randn((100000, 64), generator=g, dtype=torch.float64)
    ref[100:200] = 0                                   # all-zero rows (the gap pixels of a strided data gradient)
    ref[300] *= 1e-6                                   # a row far below the typical size
    got = ref.to(torch.bfloat16)
    assert lp.row_err(got, ref) <= 2.0 ** -8
    old = torch.randn(ref.shape, generator=g, dtype=torch.float64).to(torch.bfloat16)
    acc = (ref.to(torch.bfloat16).double() + old.double()).to(torch.bfloat16)
    assert lp.row_err(acc, ref + old.double()) <= 2.0 ** -7
    for bad_row in (got[4001].clone(), old[7], torch.zeros(64, dtype=torch.bfloat16)):
        bad = got.clone()
        bad[4000] = bad_row                            # a row one pixel off / left at its old value / unwritten
        assert lp.rel_l2(bad, ref) < lp.TOL_BF16
        assert lp.row_err(bad, ref) > 0.9
    bad = got.clone()
    bad[150, 3] = 0.5                                  # a store into a row that must stay zero
    assert lp.row_err(bad, ref) > lp.TOL_BF16
    assert lp.row_err(torch.zeros(4, 8), torch.zeros(4, 8)) == 0.0
