"""Inference with BatchNorm folded into the ResNet convs (ConvBN.fold / ResNet50.fold_bn /
forward(train=False, folded=True)), on the GPU: the scaled weight pack, the in-place ReLU, the
residual conv entry relu(conv + bias + old) in its fused and two-launch forms, folded bottlenecks,
the whole backbone and detector against the float64 inference restatement of tests/fold_ref.py, the
staleness rule, the refusals and the drivers' fold_bn argument.

Every BatchNorm here is non-trivial (fold_ref.randomize_bn): a fresh model's BN is the identity.

Tolerances.
* Scaled pack, cvl_relu_, fused against two-launch residual conv: bit-exact (one fp32 multiply then
  the same rounding; ReLU of a bf16 value is exact).
* The residual conv against float64 on the same bf16 operands: the project's own tolerance for the
  accumulating bf16 form, rtol 1e-2 / atol 3e-2 (tests/test_gpu_conv.py).
* A folded bottleneck against float64: three chained bf16 convs.  A bf16 rounding is a relative error
  of at most 2^-9 (rms 2^-9 / sqrt(3) = 1.1e-3); per conv the rounded weights and the rounded input add
  in quadrature to 1.6e-3 of the result's rms, its stored output adds 1.1e-3, conv3 stores twice:
  about 2e-3 per conv, 4e-3 over the chain (the BN scale leaves relative errors as they are, ReLU and
  the shortcut add do not amplify).  Bounds: relative L2 error <= 1e-2 (2.5 x that estimate), and
  element-wise |err| <= 2e-2 |ref| + 5e-2 rms(ref) (more than ten of those standard deviations, the
  relative term covering the final rounding of large values).
* Whole backbone / detector: e_fold <= 1.5 * e_plain, both relative L2 errors against float64, e_plain
  of the existing train=False path: the folded path drops the bf16 rounding of z and adds one rounding
  of the scaled weights, the same order of error; the 0.5 is slack for the seed."""
import ctypes

import numpy as np
import pytest
import torch

import fold_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
CK_P = 16
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _last_kernel():
    from cvlite import _lib
    return int(_lib.load().cvl_conv_igemm_last_kernel())


# ---- scaled pack --------------------------------------------------------------------------------------
PACK_CASES = [(1, 64, 256, 64, 256), (3, 64, 64, 64, 64), (1, 32, 40, 32, 64)]     # k, Cin, Cout, Cin_k, Npad


def test_scaled_pack_matches_pack_of_premultiplied_weights():
    from cvlite import ops_nn as nn
    g = torch.Generator().manual_seed(0)
    entries, refs = [], []
    for k, cin, cout, cin_k, npad in PACK_CASES:
        w = torch.randn((k, k, cin, cout), generator=g).to(DEV)
        s = (torch.rand(cout, generator=g) + 0.5).to(DEV)
        ref = torch.full((npad, k * k * cin_k), 7.0, dtype=BF, device=DEV)
        nn.pack_conv_weights((w * s).contiguous(), k, k, cin, cout, cin_k, npad, ref)      # fp32 product on the host side
        got = torch.full((npad, k * k * cin_k), 7.0, dtype=BF, device=DEV)
        entries.append((w, s, k * k, cin, cout, cin_k, npad, got))
        refs.append(ref)
    nn.ScaledPackPlan(entries, DEV).run()             # the three items in one launch
    for (k, cin, cout, cin_k, npad), e, ref in zip(PACK_CASES, entries, refs):
        got = e[-1]
        assert torch.equal(_bits(got), _bits(ref)), (k, cin, cout)
        assert not bool(got[cout:].any()), "padding rows are zero"
        assert bool((got[:cout] != 0).any())


# ---- in-place ReLU --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 37, 70001])
def test_relu_inplace_exact(k):
    from cvlite import ops_nn as nn
    n = 8 * k + 3
    g = torch.Generator().manual_seed(k)
    x0 = torch.randn(n + 9, generator=g).to(BF)
    x0[:2] = torch.tensor([-0.0, 0.0])
    x0 = x0.to(DEV)
    for off in (0, 1):                                  # 16-byte aligned / 2 bytes off the 16-byte grid
        buf = x0.clone()
        nn.relu_(buf[off:off + n])
        ref = x0.clone()
        ref[off:off + n] = torch.relu(x0[off:off + n])
        assert torch.equal(buf.float(), ref.float()), (k, off)
        assert torch.equal(_bits(buf[off + n:]), _bits(x0[off + n:])) and torch.equal(_bits(buf[:off]), _bits(x0[:off]))
        assert not bool((_bits(buf[off:off + n]) < 0).any())          # no sign bit left (-0 -> +0)


# ---- the residual conv entry ------------------------------------------------------------------------------
# id -> B, H, W, Cin, Cout, CVL_DISPATCH hooks, expected (N tile, K tile) of the persistent kernel, tiles
# per workgroup the case is there for
RES_CASES = {
    "n128_k64": (2, 16, 16, 64, 256, (), (128, 64), 1),
    "n64": (2, 16, 16, 1024, 256, (), (64, 64), 1),
    "k32": (2, 16, 16, 96, 128, (), (128, 32), 1),
    "ragged_span": (3, 10, 10, 64, 256, (), (128, 64), 1),
    "multi_tile": (2, 16, 16, 64, 256, ("p_wgs=2",), (128, 64), 2),
}


def _res_problem(B, H, W, cin, cout, seed):
    from cvlite import ops_nn as nn
    g = torch.Generator().manual_seed(seed)
    src = torch.randn((B, H, W, cin), generator=g).to(BF).to(DEV)
    wp = (torch.randn((cout, cin), generator=g) / cin ** 0.5).to(BF).to(DEV)         # packed [N][K] directly
    bias = (torch.randn(cout, generator=g) * 0.5).to(DEV)
    old = torch.randn((B, H, W, cout), generator=g).to(BF).to(DEV)
    d = nn.make_desc(nn.FWD, B, cin, 1, 1, 1, 0, 0, cout, cout, cout, [nn.seg(H, W, H, W, wp, bias)], beta=1.0)
    conv = src.double().reshape(-1, cin) @ wp.double().t() + bias.double()
    ref = torch.relu(conv + old.double().reshape(-1, cout))
    # `old` has both signs: ReLU before the add is a different function
    assert float((ref - (torch.relu(conv) + old.double().reshape(-1, cout))).abs().max()) > 0.5
    return d, src, old, ref.reshape(B, H, W, cout)


@pytest.mark.parametrize("case", list(RES_CASES))
def test_res_relu_entry_matches_float64_and_two_launch_form(case, dispatch):
    from cvlite import _lib, ops_nn as nn
    B, H, W, cin, cout, hooks, (ntile, ktile), tiles_per_wg = RES_CASES[case]
    if hooks:
        dispatch(*hooks)
    d, src, old, ref = _res_problem(B, H, W, cin, cout, seed=len(case))
    # the form the case is there for, from the planner's own answer
    k, t, grid, nt = (ctypes.c_int32(-1) for _ in range(4))
    assert _lib.load().cvl_conv_igemm_plan_grid(ctypes.byref(d), 0, 0, 0, ctypes.byref(k), ctypes.byref(t),
                                                ctypes.byref(grid), ctypes.byref(nt)) == 0
    assert (k.value, nt.value, t.value) == (CK_P, ntile, ktile)
    m_tiles = -(-B * H * W // 256)
    assert -(-m_tiles // (grid.value // (cout // ntile))) == tiles_per_wg
    if case == "ragged_span":
        assert (B * H * W) % 256 and (H * W) % 256            # part-filled last tile, tiles spanning images
    assert nn.conv_igemm_res_relu_plan(d) == (CK_P, 1)
    fused = old.clone()
    nn.conv_igemm_res_relu(d, src, fused)
    assert _last_kernel() == CK_P
    torch.testing.assert_close(fused.double(), ref, rtol=1e-2, atol=3e-2)
    dispatch("no_res_relu_fuse")
    assert nn.conv_igemm_res_relu_plan(d) == (CK_P, 0)
    two = old.clone()
    nn.conv_igemm_res_relu(d, src, two)
    assert torch.equal(_bits(fused), _bits(two))


def test_res_relu_entry_other_kernel_family(dispatch):
    """Without the persistent kernel the beta = 1 launch of another family + the ReLU pass."""
    from cvlite import ops_nn as nn
    d, src, old, ref = _res_problem(2, 16, 16, 64, 256, seed=11)
    dispatch("no_p")
    kernel, fused = nn.conv_igemm_res_relu_plan(d)
    assert fused == 0 and kernel not in (0, CK_P)
    out = old.clone()
    nn.conv_igemm_res_relu(d, src, out)
    assert _last_kernel() == kernel
    torch.testing.assert_close(out.double(), ref, rtol=1e-2, atol=3e-2)


# ---- bottlenecks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cin,stride", [("identity", 256, 1), ("projection_s1", 64, 1), ("projection_s2", 256, 2)])
def test_folded_bottleneck_matches_float64(kind, cin, stride):
    from cvlite.layers import FoldPlan, ParamStore
    from cvlite.resnet import Bottleneck
    B, H, W, f = 2, 16, 16, 64
    st = ParamStore()
    blk = Bottleneck(st, "blk", cin, f, stride, kind != "identity")
    st.finalize(torch.device(DEV), seed=5)
    for u in blk.units():
        u.bn.init_buffers(DEV)
    fold_ref.randomize_bn([u.bn for u in blk.units()], [u.conv for u in blk.units()], seed=6)
    FoldPlan(blk.units()).run()
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn((B, H, W, cin), generator=g).to(BF).to(DEV)
    x = x0.clone()
    y, Ho, Wo = blk.forward_folded(x, B, H, W)
    assert (Ho, Wo) == (H // stride, W // stride) and tuple(y.shape) == (B, Ho, Wo, 4 * f)
    if kind == "identity":
        assert y.data_ptr() == x.data_ptr()               # formed in its input buffer
    else:
        assert y.data_ptr() != x.data_ptr() and torch.equal(_bits(x), _bits(x0))     # the input only read
    p = fold_ref.params64(st, [u.bn for u in blk.units()])
    ref = fold_ref.bottleneck(x0.cpu().double().permute(0, 3, 1, 2), p, "blk", stride, kind != "identity")
    ref = ref.permute(0, 2, 3, 1)
    got = y.cpu().double()
    rms = float(ref.pow(2).mean().sqrt())
    err = fold_ref.rel_l2(got, ref)
    print("bottleneck %s: rel L2 %.3e, max |err| / rms %.3e" % (kind, err, float((got - ref).abs().max()) / rms))
    assert err <= 1e-2
    torch.testing.assert_close(got, ref, rtol=2e-2, atol=5e-2 * rms)


# ---- whole backbone and detector ---------------------------------------------------------------------------
C = 20


@pytest.fixture(scope="module")
def fcos_case():
    """One FCOSNet with non-trivial BNs, its float64 parameters, and the float64 references (computed
    once, shared, left unchanged): backbone taps at 2 x 64 x 64, head outputs at 2 x 128 x 128."""
    from cvlite.fcos_net import FCOSNet
    net = FCOSNet(C, device=torch.device(DEV), seed=0)
    fold_ref.randomize_bn(net.backbone.bns(), net.backbone.convs(), seed=1)
    p = fold_ref.params64(net.store, net.backbone.bns())
    g = torch.Generator().manual_seed(2)
    x64 = torch.rand((2, 64, 64, 3), generator=g) * 2 - 1
    x128 = torch.rand((2, 128, 128, 3), generator=g) * 2 - 1
    with torch.no_grad():
        taps = [t.permute(0, 2, 3, 1) for t in fold_ref.resnet50_taps(x64.double().permute(0, 3, 1, 2), p)]
        reg, cls = fold_ref.fcos_heads(x128.double().permute(0, 3, 1, 2), p, C)
    return dict(net=net, x64=x64.to(DEV), x128=x128.to(DEV), taps=taps, reg=reg, cls=cls)


def test_folded_backbone_error_against_float64(fcos_case):
    bb = fcos_case["net"].backbone
    plain, _ = bb.forward(fcos_case["x64"], train=False)
    plain = [t[0].clone() for t in plain]
    folded, saved = bb.forward(fcos_case["x64"], train=False, folded=True)
    assert saved is None and bb.fold_fresh
    for name, a, b, ref in zip(("C3", "C4", "C5"), plain, folded, fcos_case["taps"]):
        assert tuple(b[0].shape) == tuple(ref.shape)
        e_plain, e_fold = fold_ref.rel_l2(a, ref), fold_ref.rel_l2(b[0], ref)
        print("backbone 2x64x64 %s: e_plain %.3e  e_fold %.3e" % (name, e_plain, e_fold))
        assert 0 < e_plain < 0.2, "the yardstick itself is off (a broken restatement makes the ratio vacuous)"
        assert e_fold <= 1.5 * e_plain, (name, e_plain, e_fold)


def test_folded_detector_error_against_float64(fcos_case):
    net = fcos_case["net"]
    reg_p, cls_p = (t.clone() for t in net.forward(fcos_case["x128"], train=False))
    reg_f, cls_f = net.forward(fcos_case["x128"], train=False, folded=True)
    for name, a, b, ref, n in (("reg", reg_p, reg_f, fcos_case["reg"], 5), ("cls", cls_p, cls_f, fcos_case["cls"], C)):
        assert tuple(b.shape) == tuple(a.shape)
        e_plain, e_fold = fold_ref.rel_l2(a[..., :n], ref), fold_ref.rel_l2(b[..., :n], ref)
        print("FCOS 2x128x128 %s: e_plain %.3e  e_fold %.3e" % (name, e_plain, e_fold))
        assert 0 < e_plain < 0.2, "the yardstick itself is off (a broken restatement makes the ratio vacuous)"
        assert e_fold <= 1.5 * e_plain, (name, e_plain, e_fold)


def test_folded_forward_runs_no_bn_pass(fcos_case, monkeypatch):
    from cvlite import ops_nn as nn

    def boom(*a, **k):
        raise AssertionError("bn_apply ran in a folded forward")
    monkeypatch.setattr(nn, "bn_apply", boom)
    with pytest.raises(AssertionError):
        fcos_case["net"].forward(fcos_case["x128"], train=False)         # the plain path does run it
    reg, cls = fcos_case["net"].forward(fcos_case["x128"], train=False, folded=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(reg).all()) and bool(torch.isfinite(cls).all())


def test_folded_forward_is_inference_only(fcos_case):
    with pytest.raises(ValueError):
        fcos_case["net"].forward(fcos_case["x128"], train=True, folded=True)


def test_fold_goes_stale_with_pack_and_disturbs_nothing():
    from cvlite.fcos_net import FCOSNet
    net = FCOSNet(C, device=torch.device(DEV), seed=3)
    bb = net.backbone
    fold_ref.randomize_bn(bb.bns(), bb.convs(), seed=4)
    x = (torch.rand((2, 64, 64, 3), generator=torch.Generator().manual_seed(5)) * 2 - 1).to(DEV)
    c5 = lambda **kw: bb.forward(x, train=False, **kw)[0][2][0].clone()  # noqa: E731
    r0 = c5()                                            # before any fold
    assert not bb.fold_fresh
    f1 = c5(folded=True)
    assert bb.fold_fresh
    assert torch.equal(_bits(c5()), _bits(r0))             # the fold leaves the plain path alone
    ws = [b.c3.conv.w for b in bb.stages[3]]
    for w in ws:
        w.mul_(4.0)                                      # exact in fp32, undone below
    net.pack()
    assert not bb.fold_fresh
    f2 = c5(folded=True)                                 # folds again first
    assert bb.fold_fresh
    r2 = c5()
    moved, follows = fold_ref.rel_l2(f1, r2), fold_ref.rel_l2(f2, r2)
    print("staleness: stale fold vs new plain %.3e, fresh fold vs new plain %.3e" % (moved, follows))
    # two bf16 paths of the same map differ by their rounding only: about 50 chained convs at 2e-3 each
    # (the module docstring) are sqrt(50) * 2e-3 = 1.4e-2 against float64, two such paths 2e-2 apart; the
    # bound is 2.5 x that.  Conv5's residual branches times four move C5 by far more.
    assert follows <= 5e-2 and moved >= 4 * follows
    for w in ws:
        w.mul_(0.25)
    net.pack()
    assert torch.equal(_bits(c5()), _bits(r0))
    assert torch.equal(_bits(c5(folded=True)), _bits(f1))


# ---- refusals ---------------------------------------------------------------------------------------------
def test_fold_bn_refusals():
    from cvlite.fcos_net import FCOSNet
    from cvlite.retina_net import RetinaNetNet
    x = torch.zeros((1, 128, 128, 3), device=DEV)
    for net in (FCOSNet(3, backbone_model="mobilenetv2"), RetinaNetNet(3, backbone_model="resnext50"),
                FCOSNet(3, precision="fp32")):
        with pytest.raises(NotImplementedError):
            net.fold_bn()
        with pytest.raises(NotImplementedError):
            net.forward(x, train=False, folded=True)


# ---- drivers -----------------------------------------------------------------------------------------------
def _samples(n, S, nc):
    rng = np.random.default_rng(8)
    out = []
    for _ in range(n):
        k = int(rng.integers(1, 4))
        hw = rng.uniform(0.2, 0.8, (k, 2))
        c = rng.uniform(hw / 2, 1 - hw / 2)
        out.append(dict(image=rng.uniform(-1, 1, (S, S, 3)).astype(np.float32),
                        bbox=np.concatenate([c, hw], 1).astype(np.float32), label=rng.integers(0, nc, k)))
    return out


def test_drivers_take_fold_bn(fcos_case):
    from cvlite.evaluate import evaluate_fcos, evaluate_retinanet
    from cvlite.infer_fcos import image_detections
    from cvlite.retinanet import RetinaNet
    net = fcos_case["net"]
    samples = _samples(2, 128, C)
    x = np.stack([s["image"] for s in samples])
    det = image_detections(x, net, C, cls_thresh=0.0101, max_total_size=40, fold_bn=True)
    assert tuple(det.nmsed_boxes.shape) == (2, 40, 4) and tuple(det.nmsed_scores.shape) == (2, 40)
    assert tuple(det.nmsed_classes.shape) == (2, 40) and tuple(det.valid_detections.shape) == (2,)
    assert net.backbone.fold_fresh
    res = evaluate_fcos(net, samples, C, batch_size=2, cls_thresh=0.0101, max_total_size=40, fold_bn=True)
    assert "mAP" in res and "ap" in res
    retina = RetinaNet(3, {}, anchor_sizes=[20.0, 40.0, 80.0, 160.0, 320.0])
    fold_ref.randomize_bn(retina.model.backbone.bns(), retina.model.backbone.convs(), seed=9)
    rows = retina.image_detections(x[:1], cls_thresh=0.0101, fold_bn=True)
    assert rows.ndim == 2 and rows.shape[1] == 6 and retina.model.backbone.fold_fresh
    res = evaluate_retinanet(retina, _samples(2, 128, 3), batch_size=2, cls_thresh=0.0101, fold_bn=True)
    assert "mAP" in res


def test_centernet_s8_folded_forward_tracks_plain():
    """The ResNet-101 stride-8 CenterNet takes the same argument: its folded forward is the plain
    train=False forward up to the two paths' bf16 rounding (the bound of the staleness test: two paths
    within sqrt(n convs) * 2e-3 of float64 each -- 104 backbone convs here, 2.9e-2 apart in quadrature,
    bound 2.5 x that), and a MobileNetV2 one refuses."""
    from cvlite.centernet_s8_net import CenterNetS8Net
    net = CenterNetS8Net(3, n_scales=2, seed=4)
    fold_ref.randomize_bn(net.backbone.bns(), net.backbone.convs(), seed=10)
    x = (torch.rand((1, 128, 128, 3), generator=torch.Generator().manual_seed(11)) * 2 - 1).to(DEV)
    plain = [t.clone() for t in net.forward(x, train=False)]
    folded = net.forward(x, train=False, folded=True)
    assert net.backbone.fold_fresh
    for name, a, b in zip(("reg", "cls"), plain, folded):
        e = fold_ref.rel_l2(b, a)
        print("CenterNet s8 1x128x128 %s: folded vs plain rel L2 %.3e" % (name, e))
        assert e <= 7.2e-2
    with pytest.raises(NotImplementedError):
        CenterNetS8Net(3, n_scales=2, backbone_model="mobilenetv2").forward(x, train=False, folded=True)
