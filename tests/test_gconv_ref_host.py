"""CPU self-test of tests/gconv_ref.py: the nine-einsum float64 reference of the grouped 3x3 conv
(forward, data gradient, weight gradient, with beta) against F.conv2d(groups=...) autograd in float64;
the absolute companions against the same on absolute values; and the exact set's promises -- every
value a float32 number, bf16 ties present where the docstring says they are."""
import pytest
import torch
import torch.nn.functional as F

import gconv_ref as G

F64 = torch.float64
# Cg in {4, 32}, strides 1 and 2, odd and even H and W (stride 2 on an even map drops the last row / column
# of x from every window's centre: Ho = H / 2)
CASES = [(2, 7, 6, 64, 4, 1), (2, 7, 6, 64, 4, 2), (1, 6, 9, 64, 32, 1), (1, 6, 9, 64, 32, 2),
         (2, 8, 8, 32, 4, 2), (1, 5, 5, 64, 32, 2), (1, 4, 7, 32, 32, 1)]


def _torch_ref(x, w, dy, Cg, s):
    xd = x.to(F64).permute(0, 3, 1, 2).requires_grad_()
    wd = w.to(G.BF).to(F64).requires_grad_()
    y = F.conv2d(F.pad(xd, (1, 1, 1, 1)), wd.permute(3, 2, 0, 1), None, s, groups=x.shape[3] // Cg)
    gx, gw = torch.autograd.grad(y, (xd, wd), dy.to(F64).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), gx.permute(0, 2, 3, 1), gw


@pytest.mark.parametrize("kind", ["random", "exact"])
@pytest.mark.parametrize("B,H,W,C,Cg,s", CASES)
def test_reference_vs_conv2d_autograd(B, H, W, C, Cg, s, kind):
    inp = G.make_inputs(kind, B, H, W, C, Cg, s, seed=1)
    x, w, dy = inp["x"], inp["w"], inp["dy"]
    y, gx, gw = _torch_ref(x, w, dy, Cg, s)
    assert tuple(y.shape[1:3]) == (inp["Ho"], inp["Wo"])
    ya, gxa, gwa = _torch_ref(x.abs(), w.abs(), dy.abs(), Cg, s)
    t, A = G.fwd_ref(x, w, Cg, s)
    torch.testing.assert_close(t, y, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(A, ya, rtol=1e-13, atol=1e-13)
    t, A = G.dgrad_ref(dy, w, Cg, s, H, W)
    torch.testing.assert_close(t, gx, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(A, gxa, rtol=1e-13, atol=1e-13)
    old = inp["dx_old"]
    t, A = G.dgrad_ref(dy, w, Cg, s, H, W, beta=1.0, old=old)
    torch.testing.assert_close(t, gx + old.to(F64), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(A, gxa + old.to(F64).abs(), rtol=1e-13, atol=1e-13)
    # the gradient w.r.t. the (bf16-valued) kernel: x and dy do not depend on the weights' rounding
    t, A = G.wgrad_ref(x, dy, Cg, s)
    torch.testing.assert_close(t, gw, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(A, gwa, rtol=1e-13, atol=1e-13)
    t, A = G.wgrad_ref(x, dy, Cg, s, beta=2.0, old=inp["dw_old"])
    torch.testing.assert_close(t, gw + 2.0 * inp["dw_old"].to(F64), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(A, gwa + 2.0 * inp["dw_old"].to(F64).abs(), rtol=1e-13, atol=1e-13)
    assert bool((A >= t.abs() - 1e-12).all())


def test_bounds_see_a_dropped_border_tap_and_truncation():
    """What the 4e-3 rel-L2 of test_gpu_gconv.py hides and the per-element bound does not: the centre tap
    dropped in one 8-channel store at one border pixel, and truncation in place of round-to-nearest-even."""
    B, H, W, C, Cg, s = 2, 16, 16, 160, 4, 1
    inp = G.make_inputs("random", B, H, W, C, Cg, s, seed=2)
    t, A = G.fwd_ref(inp["x"], inp["w"], Cg, s)
    good = t.float().to(G.BF)
    assert G.check_bound("y", good, t, G.out_bound(t, A)) <= 1.0
    x2 = inp["x"].clone()
    x2[0, 15, 15, :8] = 0
    bad = good.clone()
    bad[0, 15, 15, :8] = G.fwd_ref(x2, inp["w"], Cg, s)[0][0, 15, 15, :8].float().to(G.BF)
    rel = float((bad.double() - t).norm() / t.norm())
    print("dropped tap: rel-L2 %.2e" % rel)
    assert rel < 4e-3
    with pytest.raises(AssertionError):
        G.check_bound("y", bad, t, G.out_bound(t, A))
    trunc = (t.float().view(torch.int32) & ~0xffff).view(torch.float32).to(G.BF)     # truncation for RNE
    assert float((trunc.double() - t).norm() / t.norm()) < 4e-3
    with pytest.raises(AssertionError):
        G.check_bound("y", trunc, t, G.out_bound(t, A))


@pytest.mark.parametrize("kind", ["exact", "flat"])
@pytest.mark.parametrize("B,H,W,C,Cg,s", [(2, 37, 35, 64, 32, 1), (2, 37, 35, 64, 32, 2), (1, 34, 36, 64, 4, 1),
                                          (1, 34, 36, 128, 8, 2)])
def test_exact_set_is_exact(B, H, W, C, Cg, s, kind):
    inp = G.make_inputs(kind, B, H, W, C, Cg, s)
    assert torch.equal(inp["w"].to(G.BF).float(), inp["w"]), "the pack would round the master weights"
    assert 2 * (9 * 32 * 2 * 1 + 4) < 2 ** 24 and B * inp["Ho"] * inp["Wo"] * 4 < 2 ** 24
    for t, _ in (G.fwd_ref(inp["x"], inp["w"], Cg, s),
                 G.dgrad_ref(inp["dy"], inp["w"], Cg, s, H, W, beta=1.0, old=inp["dx_old"])):
        assert torch.equal((2 * t).round(), 2 * t) and float(t.abs().max()) <= 580
        G.expected_bf16(t)
    t, _ = G.wgrad_ref(inp["x"], inp["dy"], Cg, s, beta=2.0, old=inp["dw_old"])
    assert torch.equal((2 * t).round(), 2 * t) and float(t.abs().max()) < 2 ** 15
    assert torch.equal(t.float().to(F64), t)
    assert bool(((t - 0.5) == (t - 0.5).round()).all()), "beta = 2 onto 0.25 leaves an integer + 0.5"


@pytest.mark.parametrize("s", [1, 2])
def test_exact_set_contains_bf16_ties(s):
    """Cg = 32 on the (2, 37, 35) map: stores that round, ties among them, for y and dx at both
    strides; Cg = 4 never rounds (|t| <= 72 + 4 < 128)."""
    B, H, W, C = 2, 37, 35, 64
    inp = G.make_inputs("exact", B, H, W, C, 32, s)
    ty, _ = G.fwd_ref(inp["x"], inp["w"], 32, s)
    tx, _ = G.dgrad_ref(inp["dy"], inp["w"], 32, s, H, W)
    for name, t in (("y", ty), ("dx", tx)):
        rounded = int((G.expected_bf16(t).to(F64) != t).sum())
        ties = G.count_ties(t)
        print("stride %d %s: %d of %d stores round, %d ties, both signs %s" % (
            s, name, rounded, t.numel(), ties, bool((t > 0).any() and (t < 0).any())))
        assert rounded > 1000 and ties > 100
        assert bool((t > 128).any()) and bool((t < -128).any())
    # round-to-nearest-even differs from round-half-away and from truncation on this data
    up = ((ty.float().view(torch.int32) + 0x8000) & ~0xffff).view(torch.float32).to(G.BF)
    assert not torch.equal(up, G.expected_bf16(ty))
    inp4 = G.make_inputs("exact", B, H, W, C, 4, s)
    t4, _ = G.fwd_ref(inp4["x"], inp4["w"], 4, s)
    assert G.count_ties(t4) == 0 and torch.equal(G.expected_bf16(t4).to(F64), t4)


def test_count_ties_on_known_values():
    t = torch.tensor([128.5, 129.0, 129.5, -257.0, -258.0, 3.0, 0.0, 64.5, 1025.0, 1028.0], dtype=F64)
    # spacing 1 in [128, 256): halves tie; 2 in [256, 512): odd integers tie; 8 in [1024, 2048): 1028 ties
    assert G.count_ties(t) == 4
