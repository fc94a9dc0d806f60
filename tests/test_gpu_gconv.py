"""ResNeXt-50 / 101 backbones (RetinaNet/retinanet_module.py:53-66) on the GPU.

  * cvl_gconv3x3_fwd / dgrad / wgrad vs float64 torch (groups = C / Cg) on the same bf16 operands:
    bf16 outputs within 4e-3 rel-L2 (one bf16 rounding is ~1.1e-3 rms), the fp32 weight gradient
    within 1e-4 -- the bounds test_gpu_mobilenet.py uses for the depthwise family; dgrad with beta = 1
    onto 0.5, wgrad with beta = 2 onto 0.25; the fused BN statistics vs the kernel's own output;
  * group isolation and run-to-run bit-identity of the weight gradient;
  * the bn_data kernels vs float64, and d beta vs float64 autograd through pad(3) + conv 7x7/2;
  * torch.ops.cvlite.group_conv3x3_nhwc forward and autograd;
  * the ResNeXt-50 backbone (taps and every parameter gradient) vs the float64 restatement
    (tests/resnext_ref.py) with and without emulated bf16 storage;
  * RetinaNet(backbone_model="resnext50") under RetinaTrainer: two captured steps, bit-identical
    across two trainers; resnext101 builds and runs a forward.
"""
import pytest
import torch
import torch.nn.functional as F

import resnext_ref as rr
from oracle import model_ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

CASES = [(2, 16, 16, 128, 4, 1), (2, 16, 16, 256, 8, 2), (1, 9, 12, 512, 16, 1),
         (3, 14, 11, 256, 8, 2),         # odd width under stride 2
         (2, 8, 8, 1024, 32, 2), (2, 5, 7, 1024, 32, 1),
         (1, 33, 20, 128, 4, 1)]         # rows that straddle the kernels' 8-row tiles


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _operands(B, H, W, C, Cg, s, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g).to(BF16)
    w = torch.randn(3, 3, Cg, C, generator=g) * 0.3
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    dy = torch.randn(B, Ho, Wo, C, generator=g).to(BF16)
    return x, w, dy, Ho, Wo


def _packs(nn, w):
    C = int(w.shape[3])
    wf, wd = nn.gconv3x3_packed(C, "cuda"), nn.gconv3x3_packed(C, "cuda")
    nn.gconv3x3_pack(w.cuda(), wf, wd)
    return wf, wd


def _ref(x, w, s, Cg):
    """float64 torch on the bf16-rounded weights (the kernels multiply bf16 operands)."""
    xd = x.double().permute(0, 3, 1, 2).requires_grad_()
    wd = w.to(BF16).double().requires_grad_()
    y = F.conv2d(F.pad(xd, (1, 1, 1, 1)), wd.permute(3, 2, 0, 1), None, s, groups=x.shape[3] // Cg)
    return xd, wd, y


@pytest.mark.parametrize("B,H,W,C,Cg,s", CASES)
def test_gconv_fwd_dgrad_wgrad_vs_fp64(B, H, W, C, Cg, s):
    from cvlite import ops_nn as nn
    x, w, dy, Ho, Wo = _operands(B, H, W, C, Cg, s, C + Cg + s)
    wf, wd_img = _packs(nn, w)
    y = torch.empty((B, Ho, Wo, C), dtype=BF16, device="cuda")
    stats = nn.bn_acc(B, C, "cuda")
    nn.gconv3x3_fwd(x.cuda(), wf, y, Cg, s, stats)
    xd, wd, ref = _ref(x, w, s, Cg)
    assert ref.shape[2:] == (Ho, Wo)
    e_y = rel(y.permute(0, 3, 1, 2), ref.detach())
    ref.backward(dy.double().permute(0, 3, 1, 2))
    dx = torch.full((B, H, W, C), 0.5, dtype=BF16, device="cuda")
    nn.gconv3x3_dgrad(dy.cuda(), wd_img, dx, Cg, s, beta=1.0)
    e_dx = rel(dx.permute(0, 3, 1, 2), xd.grad + 0.5)
    dw = torch.full((3, 3, Cg, C), 0.25, device="cuda")
    nn.gconv3x3_wgrad(x.cuda(), dy.cuda(), dw, s, beta=2.0)
    e_dw = rel(dw, wd.grad + 0.5)
    # fused BN statistics: (sum, sumsq) per image and channel of the rounded outputs; the kernel adds
    # fp32 lane partials of at most a few hundred terms (each add rounds by <= 2^-24 of sum |y|)
    sv = nn.bn_acc_value(stats).cpu()
    yd = y.double().cpu()
    s1, s2 = yd.sum((1, 2)), (yd * yd).sum((1, 2))
    e_s1 = float(((sv[..., 0] - s1).abs() / yd.abs().sum((1, 2)).clamp(min=1e-30)).max())
    e_s2 = float(((sv[..., 1] - s2).abs() / s2.clamp(min=1e-30)).max())
    print("fwd %.2e dgrad %.2e wgrad %.2e stats %.1e %.1e" % (e_y, e_dx, e_dw, e_s1, e_s2))
    assert e_y < 4e-3
    assert e_dx < 4e-3
    assert e_dw < 1e-4
    assert e_s1 < 1e-5 and e_s2 < 1e-5


def test_gconv_rejects_other_geometries():
    from cvlite import _lib
    from cvlite import ops_nn as nn
    wf = nn.gconv3x3_packed(64, "cuda")
    x = torch.zeros((1, 8, 8, 64), dtype=BF16, device="cuda")
    y = torch.zeros((1, 8, 8, 64), dtype=BF16, device="cuda")
    with pytest.raises(_lib.CvlError):
        nn.gconv3x3_fwd(x, wf, y, 2, 1)                       # Cg = 2
    with pytest.raises(_lib.CvlError):
        nn.gconv3x3_fwd(x, wf, y, 4, 3)                       # stride 3
    with pytest.raises(_lib.CvlError):
        nn.gconv3x3_fwd(x, wf, y[:, :7], 4, 1)                # Ho != (H - 1) / stride + 1
    x48 = torch.zeros((1, 8, 8, 48), dtype=BF16, device="cuda")
    with pytest.raises(_lib.CvlError):
        nn.gconv3x3_dgrad(x48, wf, torch.zeros_like(x48), 4, 1)   # C % 32


def test_gconv_group_isolation_and_wgrad_reproducible():
    from cvlite import ops_nn as nn
    B, H, W, C, Cg, s = 1, 8, 8, 128, 4, 1
    x, w, dy, Ho, Wo = _operands(B, H, W, C, Cg, s, 77)
    wf, wd_img = _packs(nn, w)
    grp = 13
    lo, hi = grp * Cg, (grp + 1) * Cg
    other = torch.ones(C, dtype=torch.bool)
    other[lo:hi] = False

    def fwd(t):
        y = torch.empty((B, Ho, Wo, C), dtype=BF16, device="cuda")
        nn.gconv3x3_fwd(t.cuda(), wf, y, Cg, s)
        return y.cpu()

    def dgrad(t):
        dx = torch.empty((B, H, W, C), dtype=BF16, device="cuda")
        nn.gconv3x3_dgrad(t.cuda(), wd_img, dx, Cg, s)
        return dx.cpu()

    for op, t in ((fwd, x), (dgrad, dy)):
        t2 = t.clone()
        t2[..., lo:hi] = (t2[..., lo:hi].float() * -1.5 + 0.25).to(BF16)
        a, b = op(t), op(t2)
        assert torch.equal(a[..., other], b[..., other]), "another group's channels changed"
        assert not torch.equal(a[..., lo:hi], b[..., lo:hi])
    dws = []
    for _ in range(2):
        dw = torch.empty((3, 3, Cg, C), device="cuda")
        nn.gconv3x3_wgrad(x.cuda(), dy.cuda(), dw, s)
        dws.append(dw.cpu())
    assert torch.isfinite(dws[0]).all()
    assert torch.equal(dws[0], dws[1]), "the weight gradient is not bit-identical run to run"


def test_bn_data_forward_vs_fp64():
    from cvlite import ops_nn as nn
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 12, 10
    img = torch.randn(B, H, W, 3, generator=g) * torch.tensor([0.5, 2.0, 1.0]) + torch.tensor([0.3, -1.0, 4.0])
    beta = torch.tensor([0.25, -0.5, 1.5])
    mr = torch.empty((B, 3, 2), device="cuda")
    rm, rv = torch.zeros(3, device="cuda"), torch.ones(3, device="cuda")
    nn.bn_data_stats(img.cuda(), mr, rm, rv, 2e-5, 0.99)
    out = torch.empty((B, H, W, 3), device="cuda")
    nn.bn_data_apply(img.cuda(), mr, beta.cuda(), out)
    d = img.double()
    m = d.mean((1, 2), keepdim=True)
    v = ((d - m) ** 2).mean((1, 2), keepdim=True)
    ref = (d - m) / torch.sqrt(v + 2e-5) + beta.double()
    # fp32 arithmetic on float64 statistics: a few fp32 roundings of values of magnitude <= ~6
    assert rel(out, ref) < 1e-6
    assert rel(mr[..., 0], m.reshape(B, 3)) < 1e-6 and rel(mr[..., 1], 1 / torch.sqrt(v + 2e-5).reshape(B, 3)) < 1e-6
    # moving statistics: the images in order, unbiased variance (as the library's other BNs)
    erm, erv = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    n = H * W
    for b in range(B):
        erm = erm * 0.99 + m[b].reshape(3) * 0.01
        erv = erv * 0.99 + v[b].reshape(3) * n / (n - 1) * 0.01
    assert rel(rm, erm) < 1e-5 and rel(rv, erv) < 1e-5


def test_bn_data_beta_gradient_vs_fp64_autograd():
    """d bn_data/beta for a given dz0 (resnext.bn_data_beta_grad: an all-ones cvl_stem_wgrad, then the
    contraction with the bf16 kernel the forward multiplies) vs float64 autograd through pad(3) +
    conv 7x7/2, on an image small enough that border taps matter."""
    from cvlite.resnext import bn_data_beta_grad
    g = torch.Generator().manual_seed(8)
    B, H, W = 2, 20, 18
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    w = torch.randn(7, 7, 3, 64, generator=g) * 0.1
    dz = torch.randn(B, Ho, Wo, 64, generator=g).to(BF16)
    got = bn_data_beta_grad(w.cuda(), dz.cuda(), torch.ones((B, H, W, 3), device="cuda"))
    beta = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    xn = torch.zeros((B, 3, H, W), dtype=torch.float64) + beta.view(1, 3, 1, 1)
    z = F.conv2d(F.pad(xn, (3, 3, 3, 3)), w.to(BF16).double().permute(3, 2, 0, 1), None, 2)
    (gb,) = torch.autograd.grad((z * dz.double().permute(0, 3, 1, 2)).sum(), beta)
    # interior-only sums would be wrong here: most taps of a 10 x 9 output map touch the border
    full = (w.to(BF16).double() * dz.double().sum((0, 1, 2))).sum((0, 1, 3))
    assert rel(full, gb) > 1e-2
    assert rel(got, gb) < 1e-4


def test_group_conv3x3_nhwc_op_forward_and_autograd():
    import cvlite.torch_ops  # noqa: F401
    B, H, W, C, Cg, s = 2, 8, 8, 256, 8, 2
    x, w, dy, Ho, Wo = _operands(B, H, W, C, Cg, s, 21)
    xg = x.cuda().requires_grad_()
    wg = w.cuda().requires_grad_()
    y = torch.ops.cvlite.group_conv3x3_nhwc(xg, wg, s)
    assert y.dtype == BF16 and tuple(y.shape) == (B, Ho, Wo, C)
    gx, gw = torch.autograd.grad(y, (xg, wg), dy.cuda())
    xd, wd, ref = _ref(x, w, s, Cg)
    ref.backward(dy.double().permute(0, 3, 1, 2))
    assert rel(y.permute(0, 3, 1, 2), ref.detach()) < 4e-3
    assert rel(gx.permute(0, 3, 1, 2), xd.grad) < 4e-3
    assert gw.dtype == torch.float32 and rel(gw, wd.grad) < 1e-4


SEED = 3


def test_resnext50_backbone_vs_restatement():
    """Taps and every backbone parameter gradient of ResNeXt-50 (B = 2, 128 x 128, bn3 / sc_bn gammas
    damped: resnext_ref.DAMP) for loss = sum <tap, cotangent>, vs the float64 restatement with bf16
    storage emulated; bounds relative to the restatement's own bf16-vs-fp32 divergence."""
    from cvlite.retina_net import RetinaNetNet
    net = RetinaNetNet(8, backbone_model="resnext50", seed=SEED)
    assert type(net.backbone).__name__ == "ResNeXt"
    for k in net.store.offsets:
        if k.endswith(("_bn3/gamma", "_sc_bn/gamma")):
            net.store.p(k).mul_(rr.DAMP)
    net.pack()
    params = {k: v for k, v in net.store.state_dict().items() if k.startswith(rr.BACKBONE_PREFIXES)}
    x, cots = rr.backbone_case(SEED)
    taps, saved = net.backbone.forward(x.cuda(), True)
    assert [tuple(t.shape) for t, _, _ in taps] == [tuple(c.shape) for c in cots]
    net.store.grad.zero_()
    net.backbone.backward([c.to(BF16).cuda() for c in cots], saved)
    torch.cuda.synchronize()
    with model_ref.emulate_bf16():
        t16, g16 = rr.loss_and_grads(params, x, cots)
    t32, g32 = rr.loss_and_grads(params, x, cots)
    for i, (t, _, _) in enumerate(taps):
        e, own = rel(t, t16[i]), rel(t16[i], t32[i])
        print("tap C%d: %.4f | bf16 restatement vs fp32: %.4f" % (i + 3, e, own))
        assert float(t.float().min()) < 0, "taps are pre-ReLU"
        assert e < max(2e-2, 1.5 * own)
    names = rr.compared(g32)
    excess = []
    for k in names:
        e_gpu, e_emu = rel(net.store.g(k), g32[k]), rel(g16[k], g32[k])
        excess.append((e_gpu - (2.0 * e_emu + 0.1), e_gpu, e_emu, k))
    excess.sort(reverse=True)
    print("compared %d of %d; worst (excess, gpu, bf16 restatement, tensor):" % (len(names), len(g32)), excess[:4])
    print("bn_data/beta:", [e for e in excess if e[3] == "bn_data/beta"])
    assert len(g32) == 160 and len(names) >= 120
    assert "bn_data/beta" in names
    for s in range(1, 5):
        assert any(k.startswith("stage%d_" % s) and k.endswith("gconv/kernel") for k in names)
    assert excess[0][0] <= 0, excess[:4]


def _trainer(name, B, D, C=8):
    from cvlite.retinanet import RetinaNet
    from cvlite.train_retinanet import RetinaTrainer, synthetic_coco_batch
    rn = RetinaNet(C, {}, anchor_sizes=[20.0, 40.0, 80.0, 160.0, 320.0], backbone_model=name)
    net = rn.model
    tr = RetinaTrainer(net, rn, B, D, n_max=16)
    tr.load_candidates(*synthetic_coco_batch(3 * B, D, C, n_max=16, seed=3, device="cuda"))
    return net, tr


def test_retinanet_resnext50_trains_and_is_bit_reproducible():
    flats = []
    for _ in range(2):
        net, tr = _trainer("resnext50", 2, 256)
        assert type(net.backbone).__name__ == "ResNeXt"
        w0 = net.store.flat.clone()
        for _ in range(2):
            losses = tr.step()
        torch.cuda.synchronize()
        assert torch.isfinite(losses).all() and float(losses.sum()) > 0
        assert torch.isfinite(net.store.flat).all()
        assert not torch.equal(w0, net.store.flat)
        gk = net.store.p("stage2_unit1_gconv/kernel")
        assert not torch.equal(gk, w0[net.store.offsets["stage2_unit1_gconv/kernel"][0]:][:gk.numel()].view_as(gk))
        assert float(net.backbone.stem.bn_data.run_var.sub(1).abs().max()) > 0       # moving statistics moved
        flats.append(net.store.flat.clone())
        del net, tr
    assert torch.equal(flats[0], flats[1]), "two trainers from one seed diverge"


def test_retinanet_resnext101_builds_and_forwards():
    from cvlite.retina_net import RetinaNetNet
    net = RetinaNetNet(8, backbone_model="resnext101", seed=0)
    assert sum(len(s) for s in net.backbone.stages) == 33
    x = torch.rand((2, 128, 128, 3), device="cuda") * 2 - 1
    reg, cls = net.forward(x, train=True)
    reg_e, cls_e = net.forward(x, train=False)                 # inference: the moving statistics
    torch.cuda.synchronize()
    for r, c in ((reg, cls), (reg_e, cls_e)):                  # (the pitch pads past 4A / AC are never written)
        assert torch.isfinite(r[..., :4 * net.A]).all() and torch.isfinite(c[..., :net.A * net.C]).all()
