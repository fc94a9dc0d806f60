"""The FCOS papers' recipe on the GPU (csrc/fcos_paper.hip and everything above it) against the
restatement tests/fcos_paper_ref.py: assignment bit-exact, target norm, fused loss + gradients within
the tolerances of the existing fused loss (tests/test_gpu_targets_loss.py: rtol 2e-5 on the sums,
rtol 1e-4 / atol 1e-6 on fp32 gradients), the torch ops, the trainer and the clamped inference."""
import functools

import numpy as np
import pytest
import torch

import fcos_paper_ref as ref

pytestmark = pytest.mark.gpu

PAD = ref.PAD
f32 = np.float32


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _gpu_assign(boxes, nbox, dims, C, bounds, radius, pad=PAD):
    from cvlite import ops_targets as ot
    b, n, d = _dev(np.asarray(boxes, f32), np.asarray(nbox, np.int32), np.asarray(dims, f32))
    tg, nt = ot.fcos_paper_assign(b, n, d, pad, C, bounds=bounds, center_radius=radius)
    return tg.cpu().numpy(), nt.cpu().numpy()


# ---- assignment ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 20])
@pytest.mark.parametrize("radius", [1.5, 0.0])
@pytest.mark.parametrize("family", ["A", "B"])
def test_assign_bit_exact(family, radius, C):
    """B = 3 images (scene seeds 2, 3, 5: all five levels in family A) with nbox 8, 0 and 5; P = 1022 is
    no multiple of the 256-cell tile and the maps are not square."""
    sc = [ref.scene(s, family, C) for s in (2, 3, 5)]
    boxes = np.stack([s[0] for s in sc])
    dims = np.stack([s[1] for s in sc])
    nbox = [8, 0, 5]
    want_t, want_n, _ = ref.paper_assign(boxes, nbox, dims, PAD, C, bounds=sc[0][2], center_radius=radius)
    assert want_n[0].sum() > 0 and want_n[1].sum() == 0 and want_n[2].sum() > 0
    got_t, got_n = _gpu_assign(boxes, nbox, dims, C, sc[0][2], radius)
    assert got_t.shape == (3, 1022, 5 + C)
    np.testing.assert_array_equal(got_n, want_n)
    np.testing.assert_array_equal(got_t, want_t)


def test_assign_all_seeds_and_narrow_tile():
    """Every scene seed of both families at C = 3, and C = 60, whose rows need the 128-cell tile."""
    for family in "AB":
        sc = [ref.scene(s, family, 3) for s in range(8)]
        boxes, dims = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
        want_t, want_n, _ = ref.paper_assign(boxes, [8] * 8, dims, PAD, 3, bounds=sc[0][2])
        got_t, got_n = _gpu_assign(boxes, [8] * 8, dims, 3, sc[0][2], 1.5)
        np.testing.assert_array_equal(got_n, want_n)
        np.testing.assert_array_equal(got_t, want_t)
    boxes, dim, bounds = ref.scene(0, "B", 60)
    want_t, want_n, _ = ref.paper_assign(boxes[None], [8], dim[None], PAD, 60, bounds=bounds)
    got_t, got_n = _gpu_assign(boxes[None], [8], dim[None], 60, bounds, 1.5)
    np.testing.assert_array_equal(got_n, want_n)
    np.testing.assert_array_equal(got_t, want_t)


@pytest.mark.parametrize("radius", [1.5, 0.0])
def test_assign_edge_cases(radius):
    """Labels outside [0, C), nbox > n_max, a box partly outside the image, two equal-area boxes over
    the same cells, img_dim smaller than the pad."""
    C = 3
    H, W = 250.0, 181.0
    px = lambda y, x, h, w, c: [y / H, x / W, h / H, w / W, c]   # noqa: E731
    boxes = np.array([
        [px(100, 90, 80, 60, 1), px(110, 80, 60, 80, 2),          # equal areas, overlapping
         px(100, 90, 120, 100, 3), px(100, 90, 30, 30, -1),       # labels C and -1: skipped
         px(10, 170, 90, 70, 0), px(240, 20, 50, 50, 2)],         # partly outside the image
        [px(60, 60, 100, 100, 0), px(60, 60, 50, 200, 1), px(200, 100, 64, 64, 2),
         px(125, 90, 240, 170, 1), px(30, 30, 20, 20, 0), px(128, 96, 12, 12, 2)]], f32)
    dims = np.array([[H, W], [H, W]], f32)
    nbox = [6, 9]                                                  # 9 > n_max = 6: clamped
    assert boxes[0, 0, 2] * f32(H) * (boxes[0, 0, 3] * f32(W)) == boxes[0, 1, 2] * f32(H) * (boxes[0, 1, 3] * f32(W))
    want_t, want_n, ncand = ref.paper_assign(boxes, nbox, dims, PAD, C, center_radius=radius)
    assert (ncand >= 2).any() and want_n.sum() > 0
    got_t, got_n = _gpu_assign(boxes, nbox, dims, C, ref.PAPER_BOUNDS, radius)
    np.testing.assert_array_equal(got_n, want_n)
    np.testing.assert_array_equal(got_t, want_t)


# ---- target norm -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 20])
def test_target_norm(C):
    from cvlite import ops_targets as ot
    _, _, tg = ref.loss_inputs(C, 8, 32, seeds=(0, 1, 4))
    tg[1] = 0                                                       # an image without positives
    got = ot.fcos_target_norm(_dev(tg)[0], C).cpu().numpy()
    want = ref.target_norm(tg, C)
    assert want[0, 0] > 0 and want[1, 0] == 0
    np.testing.assert_array_equal(got[:, 0], want[:, 0])
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=1e-6)


# ---- loss --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_case(C, ld_reg, ld_cls, use_norm):
    """Inputs (numpy) and the float64 restatement's losses and gradients, computed once per case."""
    reg, cls, tg = ref.loss_inputs(C, ld_reg, ld_cls)
    norm = ref.target_norm(tg, C).astype(f32) if use_norm else None
    r = torch.tensor(reg, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(cls, dtype=torch.float64, requires_grad=True)
    L = ref.paper_loss(r, c, tg, C, norm=norm)
    L.sum().backward()
    g_reg, g_cls = r.grad.numpy().copy(), c.grad.numpy().copy()
    assert not g_reg[..., 5:].any() and not g_cls[..., C:].any()
    return reg, cls, tg, norm, L.detach().numpy(), g_reg, g_cls


def _run_loss(reg, cls, tg, norm, C, gdt=torch.float32, ld_dreg=None, ld_dcls=None, grad_scale=1.0):
    from cvlite import ops_targets as ot
    B, P = tg.shape[:2]
    r, c, t = _dev(reg, cls, tg)
    n = None if norm is None else _dev(norm)[0]
    d_reg = torch.full((B, P, ld_dreg or reg.shape[2]), 7.0, dtype=gdt, device="cuda")
    d_cls = torch.full((B, P, ld_dcls or cls.shape[2]), 7.0, dtype=gdt, device="cuda")
    losses, d_reg, d_cls = ot.fcos_paper_loss(r, c, t, C, norm=n, grad_scale=grad_scale, grad_dtype=gdt,
                                              d_reg=d_reg, d_cls=d_cls)
    return losses, d_reg, d_cls


@pytest.mark.parametrize("use_norm", [True, False])
@pytest.mark.parametrize("ld_cls", ["c8", 32])
@pytest.mark.parametrize("ld_reg", [8, 32])
@pytest.mark.parametrize("C", [3, 20])
def test_loss_matches_float64_restatement(C, ld_reg, ld_cls, use_norm):
    ld_cls = (C + 7) // 8 * 8 if ld_cls == "c8" else ld_cls
    reg, cls, tg, norm, want, g_reg, g_cls = _loss_case(C, ld_reg, ld_cls, use_norm)
    pos = tg[..., 5:].max(-1) >= 1
    neg_share = float((reg[..., :4][pos] < 0).mean())
    assert 0.15 < neg_share < 0.4, neg_share
    losses, d_reg, d_cls = _run_loss(reg, cls, tg, norm, C)
    np.testing.assert_allclose(losses.cpu().numpy(), want, rtol=2e-5)
    np.testing.assert_allclose(d_reg.cpu().numpy(), g_reg, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(d_cls.cpu().numpy(), g_cls, rtol=1e-4, atol=1e-6)
    assert not d_reg[..., 5:].any() and not d_cls[..., C:].any()          # padding columns zero
    # two runs are bit-identical
    again = _run_loss(reg, cls, tg, norm, C)
    for x, y in zip((losses, d_reg, d_cls), again):
        assert torch.equal(x, y)


@pytest.mark.parametrize("C", [40, 80])
def test_loss_narrow_tiles(C, dispatch):
    """C = 40 / 80: the LDS rows fit 128 / 64 cells per block.  Against the restatement, and the
    gradients against the row form's (their block sums differ in order, their cells do not)."""
    ld_cls = (C + 7) // 8 * 8
    reg, cls, tg, norm, want, g_reg, g_cls = _loss_case(C, 8, ld_cls, True)
    losses, d_reg, d_cls = _run_loss(reg, cls, tg, norm, C)
    np.testing.assert_allclose(losses.cpu().numpy(), want, rtol=2e-5)
    np.testing.assert_allclose(d_reg.cpu().numpy(), g_reg, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(d_cls.cpu().numpy(), g_cls, rtol=1e-4, atol=1e-6)
    dispatch("loss_rows=1")
    _, r_reg, r_cls = _run_loss(reg, cls, tg, norm, C)
    assert torch.equal(d_reg, r_reg) and torch.equal(d_cls, r_cls)


@pytest.mark.parametrize("C", [3, 20])
def test_loss_bf16_gradients_are_rounded_fp32(C):
    """bf16 gradient outputs (the trainer's layout: d_reg 32 wide off an 8-wide reg) equal the fp32
    outputs rounded to bf16, bit for bit; padding columns zero."""
    reg, cls, tg, norm, _, _, _ = _loss_case(C, 8, 32, True)
    l32, r32, c32 = _run_loss(reg, cls, tg, norm, C, ld_dreg=32, grad_scale=0.37)
    l16, r16, c16 = _run_loss(reg, cls, tg, norm, C, gdt=torch.bfloat16, ld_dreg=32, grad_scale=0.37)
    assert torch.equal(l32, l16)
    assert torch.equal(r16, r32.to(torch.bfloat16)) and torch.equal(c16, c32.to(torch.bfloat16))
    assert not r16[..., 5:].any() and not c16[..., C:].any() and bool(r16[..., :5].any())


def test_loss_image_without_positives():
    C = 3
    reg, cls, tg, _, _, _, _ = _loss_case(C, 8, 8, True)
    tg = tg.copy()
    tg[1] = 0
    norm = ref.target_norm(tg, C).astype(f32)
    assert norm[1].tolist() == [0.0, 0.0]
    losses, d_reg, d_cls = _run_loss(reg, cls, tg, norm, C)
    L = losses.cpu().numpy()
    assert L[1, 1] == 0 and L[1, 2] == 0 and L[1, 0] > 0 and L[0, 1] > 0
    assert torch.isfinite(d_reg).all() and torch.isfinite(d_cls).all() and not d_reg[1].any()
    want = ref.paper_loss(torch.tensor(reg, dtype=torch.float64), torch.tensor(cls, dtype=torch.float64), tg, C,
                          norm=norm).numpy()
    np.testing.assert_allclose(L, want, rtol=2e-5)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [3, 20])
def test_loss_lds_form_bit_identical_to_row_form(dispatch, C, gdt):
    """The LDS-staged kernel against the row-pointer kernel (CVL_DISPATCH=loss_rows): the same per-cell
    arithmetic and sum order at 256-cell tiles, so losses and both gradients match bit for bit."""
    reg, cls, tg, norm, _, _, _ = _loss_case(C, 8, 32, True)
    outs = []
    for rows in ("1", "0"):
        dispatch("loss_rows=" + rows)
        outs.append(_run_loss(reg, cls, tg, norm, C, gdt=gdt, ld_dreg=32, grad_scale=0.37))
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y), float((x.double() - y.double()).abs().max())


# ---- torch ops ---------------------------------------------------------------------------------------
def test_torch_ops_forward_and_backward():
    import cvlite.torch_ops  # noqa: F401
    C = 3
    sc = [ref.scene(s, "B", C) for s in (0, 1)]
    boxes, dims = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
    b, n, d = _dev(boxes, np.array([8, 8], np.int32), dims)
    tg, nt = torch.ops.cvlite.fcos_paper_assign(b, n, d, PAD[0], PAD[1], C, 1.5)
    reg, cls, tg_ref, norm_ref, _, _, _ = _loss_case(C, 8, 8, True)
    np.testing.assert_array_equal(tg.cpu().numpy(), tg_ref)
    norm = torch.ops.cvlite.fcos_target_norm(tg, C)
    np.testing.assert_allclose(norm.cpu().numpy(), norm_ref, rtol=1e-6)
    w = torch.tensor([[0.7, 1.3, 0.4], [1.1, 0.2, 2.0]], dtype=torch.float64)
    r64 = torch.tensor(reg, dtype=torch.float64, requires_grad=True)
    c64 = torch.tensor(cls, dtype=torch.float64, requires_grad=True)
    L64 = ref.paper_loss(r64, c64, tg_ref, C, norm=norm.cpu().numpy())
    (L64 * w).sum().backward()
    r = torch.tensor(reg, device="cuda", requires_grad=True)
    c = torch.tensor(cls, device="cuda", requires_grad=True)
    L = torch.ops.cvlite.fcos_paper_loss(r, c, tg, norm, C)
    np.testing.assert_allclose(L.detach().cpu().numpy(), L64.detach().numpy(), rtol=2e-5)
    (L * w.float().cuda()).sum().backward()
    np.testing.assert_allclose(r.grad.cpu().numpy(), r64.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(c.grad.cpu().numpy(), c64.grad.numpy(), rtol=1e-4, atol=1e-6)


# ---- trainer -------------------------------------------------------------------------------------------
TC, TB, TD = 3, 2, 128


def _batch():
    from cvlite.train_fcos import synthetic_batch
    return synthetic_batch(TB, TD, TD, TC, seed=7)


@pytest.fixture
def bn_exact():
    """BatchNorm statistics in integer bins: identical by construction from run to run."""
    from cvlite import ops_nn as nn
    nn.set_bn_exact(True)
    yield
    nn.set_bn_exact(False)


def test_trainer_eager_step_equals_ops_by_hand(bn_exact):
    from cvlite import ops_targets as ot
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer
    imgs, boxes, nbox = _batch()
    net = FCOSNet(TC, seed=1)
    tr = FCOSTrainer(net, TB, (TD, TD), use_graph=False, targets="paper")
    tr.load_batch(imgs, boxes, nbox)
    tr.run_fwd_bwd()
    torch.cuda.synchronize()
    assert int(tr.ntgt.sum()) > 0 and float(tr.norm[:, 0].sum()) == float(tr.ntgt.sum())

    net2 = FCOSNet(TC, seed=1)
    dims = torch.full((TB, 2), float(TD), device="cuda")
    tg, nt = ot.fcos_paper_assign(tr.boxes, nbox, dims, (TD, TD), TC)
    norm = ot.fcos_target_norm(tg, TC)
    reg, cls = net2.forward(imgs)
    d_reg = torch.zeros((TB, tg.shape[1], 32), dtype=net2.store.act, device="cuda")
    d_cls = torch.zeros((TB, tg.shape[1], net2.cls_ld), dtype=net2.store.act, device="cuda")
    losses, _, _ = ot.fcos_paper_loss(reg, cls, tg, TC, norm=norm, d_reg=d_reg, d_cls=d_cls)
    net2.backward(d_reg, d_cls)
    torch.cuda.synchronize()
    assert torch.equal(tr.targets, tg) and torch.equal(tr.ntgt, nt) and torch.equal(tr.norm, norm)
    assert torch.equal(tr.losses, losses) and float(losses.sum()) > 0
    assert torch.equal(net.store.grad, net2.store.grad) and bool(net.store.grad.any())


def test_trainer_graph_replay_equals_eager_and_loss_falls(bn_exact):
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer
    imgs, boxes, nbox = _batch()
    res = {}
    for graph in (False, True):
        net = FCOSNet(TC, seed=1)
        tr = FCOSTrainer(net, TB, (TD, TD), use_graph=graph, targets="paper", init_lr=1e-3)
        tr.load_batch(imgs, boxes, nbox)
        tr.step()
        torch.cuda.synchronize()
        res[graph] = (net.store.flat.clone(), tr.losses.clone())
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][0], res[False][0])
    first = float(res[True][1].sum())
    for _ in range(29):                      # the graph trainer goes on, on the same batch
        tr.step()
    torch.cuda.synchronize()
    last = float(tr.losses.sum())
    print("paper recipe: total loss step 1 %.5f, step 30 %.5f" % (first, last))
    assert np.isfinite(last) and last < first


def test_trainer_rejects_centre_network_and_unknown_recipe():
    from cvlite.train_fcos import FCOSTrainer, JitterFCOSTrainer, train

    class Centre(object):
        cen_heads = ()
        C = 3
    with pytest.raises(ValueError):
        FCOSTrainer(Centre(), 2, (128, 128), targets="paper")
    with pytest.raises(ValueError):
        JitterFCOSTrainer(Centre(), 2, targets="paper")
    with pytest.raises(ValueError):
        train([{"image": np.zeros((128, 128, 3), f32), "bbox": np.zeros((0, 4), f32), "label": []}] * 2, [],
              Centre(), 2, None, None, None, 0, 1, recipe="papers")


def test_jitter_trainer_paper_two_sizes():
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import JitterFCOSTrainer, synthetic_batch
    net = FCOSNet(TC, seed=0)
    jt = JitterFCOSTrainer(net, 2, use_graph=False, targets="paper", center_radius=1.5)
    a, boxes, nbox = synthetic_batch(2, 128, 128, TC, seed=3)
    b, _, _ = synthetic_batch(1, 256, 256, TC, seed=4)
    dims = np.array([[128, 128], [256, 256]], f32)
    losses = jt.step([a[0], b[0]], boxes, nbox, dims)
    torch.cuda.synchronize()
    assert sorted(jt.buckets) == [(128, 1), (256, 1)]
    assert all(t.target_kind == "paper" for t in jt.buckets.values())
    assert torch.isfinite(losses).all() and float(losses.sum()) > 0
    for k, pad in enumerate((128, 256)):      # positive cells per level, as the restatement counts them
        _, cnt, _ = ref.paper_assign(boxes[k:k + 1].cpu().numpy(), nbox[k:k + 1].cpu().numpy(), dims[k:k + 1],
                                     (pad, pad), TC)
        np.testing.assert_array_equal(jt.ntgt[k].cpu().numpy(), cnt[0])


# ---- inference -----------------------------------------------------------------------------------------
def test_detect_clamp_reg():
    from cvlite.infer_fcos import detect_from_outputs
    C, B = 3, 2
    shapes = ref.level_shapes(PAD)
    P = sum(h * w for h, w in shapes)
    g = torch.Generator().manual_seed(5)
    reg = (torch.randn(B, P, 8, generator=g) * 2 + 1).cuda()
    cls = (torch.randn(B, P, 32, generator=g) * 2 - 1).cuda()
    assert bool((reg[..., :4] < 0).any())
    keep = reg.clone()
    kw = dict(cls_thresh=0.3)
    clamped = detect_from_outputs(reg, cls, shapes, C, clamp_reg=True, **kw)
    assert torch.equal(reg, keep)                                   # the clamp works on a copy
    pre = reg.clone()
    pre[..., :4] = pre[..., :4].clamp(min=0)
    by_hand = detect_from_outputs(pre, cls, shapes, C, **kw)
    default = detect_from_outputs(reg, cls, shapes, C, **kw)
    off = detect_from_outputs(reg, cls, shapes, C, clamp_reg=False, **kw)
    assert int(default.valid_detections.min()) > 0
    differs = False
    for x, y, z, u in zip(clamped, by_hand, default, off):
        assert torch.equal(x, y) and torch.equal(z, u)
        differs = differs or not torch.equal(x, z)
    assert differs                                                  # the default does not clamp
