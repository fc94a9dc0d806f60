"""ATSS for RetinaNet on the GPU (csrc/retina_atss.hip and everything above it) against the restatement
tests/retina_atss_ref.py: targets, counts, candidates, IoUs and thresholds bit for bit; edge cases;
determinism; invalid arguments; the loss against float64 autograd (the tolerances of
tests/test_gpu_fcos_paper.py: rtol 2e-5 on the sums, rtol 1e-4 / atol 1e-6 on fp32 gradients); the round
trip through decode_detections; the trainer."""
import functools

import numpy as np
import pytest
import torch

import retina_atss_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
SEEDS = tuple(range(8))


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _gpu_assign(boxes, nbox, dims, pad, C, adims=None, candidates=True, **kw):
    from cvlite import ops_targets as ot
    adims = ref.default_anchor_dims() if adims is None else adims
    b, n, d, ad = _dev(np.asarray(boxes, f32), np.asarray(nbox, np.int32), np.asarray(dims, f32), np.asarray(adims, f32))
    out = ot.retina_atss_assign(b, n, d, pad, ad, C, return_candidates=candidates, **kw)
    return [t.cpu().numpy() for t in out]


@functools.lru_cache(maxsize=None)
def _want(pad, C, n_box, topk):
    """The restatement's result for the 8-scene batch, computed once and shared."""
    boxes, dims = ref.scene_batch(SEEDS, pad, C, n_box)
    return ref.atss_assign(boxes, [n_box] * len(boxes), dims, pad, C, topk=topk)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check(got, want):
    """targets, num_targets[, cand_idx, cand_iou, cand_thr] as bits against the restatement's."""
    names = ("targets", "num_targets", "cand_idx", "cand_iou", "cand_thr")
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=name)


def _both(boxes, nbox, dims, pad, C, want, **kw):
    _check(_gpu_assign(boxes, nbox, dims, pad, C, **kw), want)
    plain = _gpu_assign(boxes, nbox, dims, pad, C, candidates=False, **kw)
    assert len(plain) == 2
    _check(plain, want)


# ---- bit-exact against the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 80])
def test_assign_bit_exact_pad128(C):
    """pad 128 (P = 341), 4 boxes, seeds 0..7 as one batch."""
    boxes, dims = ref.scene_batch(SEEDS, 128, C, 4)
    want = _want(128, C, 4, 9)
    assert want[0].shape == (8, 341, 9, 8) and (want[1].sum(1) > 0).all()
    _both(boxes, [4] * 8, dims, 128, C, want)


def test_assign_bit_exact_pad256():
    """pad 256: P = 1364 is no multiple of the 64-cell tile; 8 boxes, seeds 0..7 as one batch."""
    boxes, dims = ref.scene_batch(SEEDS, 256, 80, 8)
    want = _want(256, 80, 8, 9)
    assert want[0].shape == (8, 1364, 9, 8) and (want[1].sum(1) > 0).all()
    _both(boxes, [8] * 8, dims, 256, 80, want)


@pytest.mark.parametrize("topk", [1, 9, 27, 81])
def test_assign_bit_exact_24_boxes(topk):
    """24 boxes: contested anchors; topk below A, equal to A, 3 and 9 cells per level."""
    boxes, dims = ref.scene_batch(SEEDS, 256, 20, 24)
    want = _want(256, 20, 24, topk)
    if topk >= 9:
        assert ((want[5] >= 2).sum(1) > 0).all()
    _both(boxes, [24] * 8, dims, 256, 20, want, topk=topk)


def test_assign_bit_exact_three_anchors_topk4():
    """A = 3 with topk 4: one full cell and the first anchor of the next."""
    adims = ref.default_anchor_dims()[:, [0, 4, 8]].copy()
    boxes, dims = ref.scene_batch(SEEDS, 256, 5, 8)
    want = ref.atss_assign(boxes, [8] * 8, dims, 256, 5, anchor_dims=adims, topk=4)
    assert want[0].shape == (8, 1364, 3, 8) and want[1].sum() > 0
    _both(boxes, [8] * 8, dims, 256, 5, want, adims=adims, topk=4)


def _px(rows, n_max, dim):
    H, W = dim
    out = np.zeros((n_max, 5), f32)
    for k, (y, x, h, w, c) in enumerate(rows):
        out[k] = [y / H, x / W, h / H, w / W, c]
    return out


def test_assign_edge_cases():
    """One batch: nbox 0, > n_max and negative; labels -1, C and NaN; zero, negative and NaN sizes; a NaN
    centre; a centre exactly on an anchor centre of every level; duplicated boxes; boxes outside the image,
    one of them so far that the window check must send the selection to the whole level; img_dim below
    the pad.  All outputs finite."""
    C, n_max, pad = 3, 8, 256
    nan = float("nan")
    dim = (250.0, 181.0)
    imgs = [
        [(128, 128, 100, 80, 1), (128, 128, 100, 80, 0), (64, 64, 40, 40, 2), (8, 8, 12, 12, 0),     # on anchors, duplicates
         (128, 96, 100, 80, -1), (128, 96, 100, 80, 3), (100, 90, 0, 60, 1), (100, 90, -50, 60, 1)],
        [(128, 96, nan, 80, 1), (128, 96, 100, 80, nan), (nan, 96, 100, 80, 1), (-60, 300, 40, 40, 1),
         (-10, 96, 60, 60, 2), (1e9, 96, 50, 50, 1), (128, -1e6, 3e6, 3e6, 0), (200, 100, 64, 64, 2)],
        [(60, 60, 100, 100, 0)] * 8,                                                                  # nbox 0
        [(60, 60, 100, 100, 0), (60, 60, 50, 120, 1), (200, 100, 64, 64, 2), (125, 90, 240, 170, 1),
         (30, 30, 20, 20, 0), (128, 96, 12, 12, 2), (90, 40, 30, 70, 1), (180, 150, 70, 30, 0)],     # nbox 11 > n_max
        [(60, 60, 100, 100, 0)] * 8,                                                                  # nbox -3
    ]
    boxes = np.stack([_px(rows, n_max, dim) for rows in imgs])
    dims = np.array([dim] * len(imgs), f32)
    nbox = [8, 8, 0, 11, -3]
    want = ref.atss_assign(boxes, nbox, dims, pad, C)
    tg, cnt, idx, iou, thr, npair, owner = want
    assert cnt[0].sum() > 0 and cnt[1].sum() > 0 and cnt[3].sum() > 0 and not cnt[2].any() and not cnt[4].any()
    assert (npair[0] == 2).any() and (idx[0, 4:] == -1).all() and (idx[1, :2] == -1).all()
    assert idx[1, 2, :9].tolist() == list(range(9))                     # the NaN centre: index order
    assert (idx[1, 5, :9] >= 0).all() and (owner[1] == 6).any()         # the far box has candidates
    got = _gpu_assign(boxes, nbox, dims, pad, C)
    assert all(np.isfinite(g).all() for g in got)
    _check(got, want)
    _check(_gpu_assign(boxes, nbox, dims, pad, C, candidates=False), want)


def test_assign_large_levels_and_far_centres():
    """A 384 pad: level 0 has 48 x 48 = 2304 cells, more than a lane's register cache holds, so the
    whole-level selection that a rejected window falls back to recomputes its keys every round.  Far and
    NaN centres take that path on every level; the ordinary boxes beside them take the window.  topk 144
    is the largest allowed (16 cells per level, 720 candidate slots)."""
    pad, C = 384, 4
    dim = (380.0, 300.0)
    nan = float("nan")
    rows = [(190, 150, 200, 150, 1), (1e9, 96, 50, 50, 1), (128, -1e6, 3e6, 3e6, 0), (nan, 96, 100, 80, 2),
            (256, 192, 64, 64, 3), (3e38, 3e38, 10, 10, 0), (40, 250, 60, 50, 2), (-2e5, -2e5, 5e5, 5e5, 3)]
    boxes = _px(rows, 8, dim)[None]
    dims = np.array([dim], f32)
    for topk in (9, 144):
        want = ref.atss_assign(boxes, [8], dims, pad, C, topk=topk)
        assert want[0].shape == (1, 3069, 9, 8) and want[1].sum() > 0
        assert want[2][0, 3, :topk].tolist() == list(range(topk))         # the NaN centre: index order
        assert len(set(want[6][want[6] >= 0].tolist())) >= 3
        got = _gpu_assign(boxes, [8], dims, pad, C, topk=topk)
        assert np.isfinite(got[0]).all()
        _check(got, want)


def test_assign_is_deterministic():
    from cvlite import ops_targets as ot
    boxes, dims = ref.scene_batch(SEEDS, 256, 20, 24)
    b, n, d, ad = _dev(boxes, np.full(8, 24, np.int32), dims, ref.default_anchor_dims())
    tg0, nt0 = ot.retina_atss_assign(b, n, d, 256, ad, 20, topk=27)
    tg1, nt1 = ot.retina_atss_assign(b, n, d, 256, ad, 20, topk=27)
    assert int(nt0.sum()) > 0
    assert torch.equal(tg0.view(torch.int32), tg1.view(torch.int32)) and torch.equal(nt0, nt1)


def test_invalid_arguments_leave_outputs_untouched():
    from cvlite import _lib
    from cvlite import ops_targets as ot
    boxes, dims = ref.scene_batch((0,), 128, 3, 4)
    b, n, d, ad = _dev(boxes, np.array([4], np.int32), dims, ref.default_anchor_dims())
    out = torch.full((1, 341, 9, 8), 7.0, device="cuda")
    nt = torch.full((1, 5), 7, dtype=torch.int32, device="cuda")
    bad = [dict(topk=0), dict(topk=145), dict(pad=200), dict(pad=0), dict(C=0), dict(C=257)]
    for kw in bad:
        a = dict(pad=128, C=3, topk=9)
        a.update(kw)
        bufs = dict(out=out, num_targets=nt) if a["pad"] == 128 else {}     # another pad is another P
        with pytest.raises(_lib.CvlError):
            ot.retina_atss_assign(b, n, d, a["pad"], ad, a["C"], topk=a["topk"], **bufs)
    for A, topk in ((17, 9), (3, 49)):                 # too many anchors; ceil(topk / A) = 17 cells
        wide = torch.ones((5, A, 2), device="cuda") * 32
        o = torch.full((1, 341, A, 8), 7.0, device="cuda")
        with pytest.raises(_lib.CvlError):
            ot.retina_atss_assign(b, n, d, 128, wide, 3, topk=topk, out=o, num_targets=nt)
        assert bool((o == 7.0).all())
    big = torch.zeros((1, 257, 5), device="cuda")
    with pytest.raises(_lib.CvlError):
        ot.retina_atss_assign(big, n, d, 128, ad, 3, out=out, num_targets=nt)
    # a short workspace, through the C entry itself
    need = int(_lib.load().cvl_retina_atss_workspace_size(1, 341, 9))
    assert need == 341 * 9 * 8 and int(_lib.load().cvl_retina_atss_workspace_size(0, 341, 9)) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    st = (_lib.ctypes.c_int32 * 5)(*ref.STRIDES)
    args = lambda nbytes: (_lib.ptr(b), _lib.ptr(n), _lib.ptr(d), 1, 4, 128, 3, _lib.ptr(ad), 9,   # noqa: E731
                           _lib.ctypes.cast(st, _lib.c_void_p), 9, _lib.ptr(out), _lib.ptr(nt), None, None, None,
                           _lib.ptr(ws), nbytes, _lib.stream())
    with pytest.raises(_lib.CvlError):
        _lib.call("cvl_retina_atss_assign", *args(need - 8))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((nt == 7).all())
    _lib.call("cvl_retina_atss_assign", *args(need))                  # the same call with enough room runs
    torch.cuda.synchronize()
    assert int(nt.sum()) > 0 and not bool((out == 7.0).any())
    # the loss: leading dimensions too small, a bad dtype code is unreachable from Python; poison stays
    reg = torch.zeros((1, 341, 40), device="cuda")
    cls = torch.zeros((1, 341, 32), device="cuda")
    losses = torch.full((1, 2), 7.0, device="cuda")
    with pytest.raises(_lib.CvlError):
        ot.retina_atss_loss(reg[..., :32].contiguous(), cls, out, nt, 9, 3, losses=losses)
    with pytest.raises(_lib.CvlError):
        ot.retina_atss_loss(reg, cls[..., :24].contiguous(), out, nt, 9, 3, losses=losses)
    with pytest.raises(_lib.CvlError):
        ot.retina_atss_loss(reg, cls, out, nt, 9, 3, gamma=-1.0, losses=losses)
    torch.cuda.synchronize()
    assert bool((losses == 7.0).all())


# ---- the loss ---------------------------------------------------------------------------------------------
def _bf16_bits(t):
    return t.view(torch.int16).cpu().numpy()


@pytest.mark.parametrize("C,ld_reg,ld_cls", [(3, 37, 29), (3, 40, 32), (20, 40, 184)],
                         ids=["scalar", "reg4", "reg4-cls4"])
def test_loss_against_float64_autograd(C, ld_reg, ld_cls):
    """The 8-scene batch's targets (image 5 emptied: N = 1, it trains on its negatives) and random
    outputs.  Leading dimensions that take the one-channel and the four-channel forms."""
    from cvlite import ops_targets as ot
    A, pad = 9, 256
    boxes, dims = ref.scene_batch(SEEDS, pad, C, 8)
    nbox = np.full(8, 8, np.int32)
    nbox[5] = 0
    tg, nt = ref.atss_assign(boxes, nbox, dims, pad, C)[:2]
    assert nt[5].sum() == 0 and (np.delete(nt.sum(1), 5) > 0).all()
    B, P = tg.shape[:2]
    rng = np.random.default_rng(11)
    reg = rng.normal(0, 1, (B, P, ld_reg)).astype(f32)
    reg[..., :4 * A] += tg[..., :4].reshape(B, P, 4 * A)
    cls = (rng.normal(0, 2, (B, P, ld_cls)) - 2).astype(f32)
    w = np.array([1, 1, 0, 1, 1, 1, 0, 1], f32)
    gs = 0.7
    r64 = torch.tensor(reg, dtype=torch.float64, requires_grad=True)
    c64 = torch.tensor(cls, dtype=torch.float64, requires_grad=True)
    L64 = ref.atss_loss(r64, c64, tg, nt, A, C, img_weight=w)
    (L64.sum() * gs).backward()
    assert float(L64.detach()[5, 0]) > 0 and float(L64.detach()[5, 1]) == 0 and float(L64.detach()[0, 1]) > 0

    r, c, t, n, wd = _dev(reg, cls, tg, nt, w)
    poison = 7.0
    d_reg = torch.full((B, P, ld_reg), poison, device="cuda")
    d_cls = torch.full((B, P, ld_cls), poison, device="cuda")
    L = ot.retina_atss_loss(r, c, t, n, A, C, img_weight=wd, grad_scale=gs, d_reg=d_reg, d_cls=d_cls)
    print("losses", L.cpu().numpy().tolist(), "float64", L64.detach().numpy().tolist())
    np.testing.assert_allclose(L.cpu().numpy(), L64.detach().numpy(), rtol=2e-5)
    np.testing.assert_allclose(d_reg[..., :4 * A].cpu().numpy(), r64.grad.numpy()[..., :4 * A], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(d_cls[..., :A * C].cpu().numpy(), c64.grad.numpy()[..., :A * C], rtol=1e-4, atol=1e-6)
    assert bool((d_reg[..., 4 * A:] == poison).all()) and bool((d_cls[..., A * C:] == poison).all())
    assert bool((d_reg[2][..., :4 * A] == 0).all()) and bool((d_cls[6][..., :A * C] == 0).all())     # weight 0
    # bf16 gradients: the same fp32 values, rounded
    b_reg = torch.full((B, P, ld_reg), poison, device="cuda", dtype=torch.bfloat16)
    b_cls = torch.full((B, P, ld_cls), poison, device="cuda", dtype=torch.bfloat16)
    Lb = ot.retina_atss_loss(r, c, t, n, A, C, img_weight=wd, grad_scale=gs, d_reg=b_reg, d_cls=b_cls)
    assert torch.equal(Lb, L)
    np.testing.assert_array_equal(_bf16_bits(b_reg), _bf16_bits(d_reg.to(torch.bfloat16)))
    np.testing.assert_array_equal(_bf16_bits(b_cls), _bf16_bits(d_cls.to(torch.bfloat16)))
    # forward only, and no weights: image 2's loss appears
    L1 = ot.retina_atss_loss(r, c, t, n, A, C)
    np.testing.assert_allclose(L1.cpu().numpy(), ref.atss_loss(r64, c64, tg, nt, A, C).detach().numpy(), rtol=2e-5)
    # the box slots of a non-positive anchor are never read
    tp = tg.copy()
    tp[..., :4][tp[..., 4] < 0] = np.nan
    p_reg, p_cls = torch.zeros_like(d_reg), torch.zeros_like(d_cls)
    q_reg, q_cls = torch.zeros_like(d_reg), torch.zeros_like(d_cls)
    Lq = ot.retina_atss_loss(r, c, t, n, A, C, img_weight=wd, grad_scale=gs, d_reg=q_reg, d_cls=q_cls)
    Lp = ot.retina_atss_loss(r, c, _dev(tp)[0], n, A, C, img_weight=wd, grad_scale=gs, d_reg=p_reg, d_cls=p_cls)
    assert torch.equal(Lp, Lq) and torch.equal(p_reg, q_reg) and torch.equal(p_cls, q_cls)
    assert torch.equal(Lq, L)                                                              # run to run


def test_torch_ops_match_and_differentiate():
    import cvlite.torch_ops  # noqa: F401
    from cvlite import ops_targets as ot
    C, A, pad = 3, 9, 128
    boxes, dims = ref.scene_batch((0, 1), pad, C, 4)
    b, n, d, ad = _dev(boxes, np.array([4, 4], np.int32), dims, ref.default_anchor_dims())
    tg, nt = torch.ops.cvlite.retina_atss_assign(b, n, d, pad, ad, C, 9)
    tg2, nt2 = ot.retina_atss_assign(b, n, d, pad, ad, C)
    assert torch.equal(tg, tg2) and torch.equal(nt, nt2) and tuple(tg.shape) == (2, 341, A, 8)
    rng = np.random.default_rng(3)
    reg = rng.normal(0, 1, (2, 341, 40)).astype(f32)
    cls = (rng.normal(0, 2, (2, 341, 32)) - 2).astype(f32)
    w = torch.tensor([[0.7, 1.3], [1.1, 0.2]], dtype=torch.float64)
    r64 = torch.tensor(reg, dtype=torch.float64, requires_grad=True)
    c64 = torch.tensor(cls, dtype=torch.float64, requires_grad=True)
    L64 = ref.atss_loss(r64, c64, tg.cpu().numpy(), nt.cpu().numpy(), A, C)
    (L64 * w).sum().backward()
    r = torch.tensor(reg, device="cuda", requires_grad=True)
    c = torch.tensor(cls, device="cuda", requires_grad=True)
    L = torch.ops.cvlite.retina_atss_loss(r, c, tg, nt, None, A, C)
    np.testing.assert_allclose(L.detach().cpu().numpy(), L64.detach().numpy(), rtol=2e-5)
    (L * w.float().cuda()).sum().backward()
    np.testing.assert_allclose(r.grad.cpu().numpy(), r64.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(c.grad.cpu().numpy(), c64.grad.numpy(), rtol=1e-4, atol=1e-6)


# ---- round trip ----------------------------------------------------------------------------------------------
def test_targets_decode_back_to_the_boxes():
    """The targets' box slots as the box outputs and a large logit at the label: decode_detections
    returns every winning gt box's corners within 1e-3 px (about 30 fp32 ulps at 256 px)."""
    from cvlite.retinanet import RetinaNet
    C, A, pad, n_box = 20, 9, 256, 8
    rn = RetinaNet(C, {})
    np.testing.assert_array_equal(np.array(rn.anchor_boxes, f32), ref.default_anchor_dims())
    boxes, dims = ref.scene_batch((0, 1), pad, C, n_box)
    b, n, d = _dev(boxes, np.array([n_box] * 2, np.int32), dims)
    tg, nt = rn.format_data_atss(b, n, d, pad)
    want = ref.atss_assign(boxes, [n_box] * 2, dims, pad, C)
    np.testing.assert_array_equal(tg.cpu().numpy(), want[0])
    B, P = tg.shape[:2]
    reg = tg[..., :4].reshape(B, P, 4 * A).contiguous()
    cls = torch.full((B, P, A * C), -10.0, device="cuda")
    label = tg[..., 4].reshape(B, P * A)
    rows = torch.nonzero(label >= 0)
    cls.view(B, P * A, C)[rows[:, 0], rows[:, 1], label[rows[:, 0], rows[:, 1]].long()] = 10.0
    shapes = [(pad // s, pad // s) for s in ref.STRIDES]
    dets = rn.decode_detections(reg, cls, shapes, iou_thresh=1.0, cls_thresh=0.5)
    for k in range(B):
        gt = boxes[k]
        yc, xc, h, w = (gt[:, j] * pad for j in range(4))
        corners = np.stack([yc - h / 2, xc - w / 2, yc + h / 2, xc + w / 2], 1)
        owners = set(want[6][k][want[6][k] >= 0].tolist())
        assert len(dets[k]) == int(want[1][k].sum()) and len(owners) == n_box
        err = np.abs(dets[k][:, None, :4] - corners[None]).max(2)          # [detections, boxes]
        hit = err.argmin(1)
        print("image %d: %d detections, worst corner error %.3g px" % (k, len(dets[k]), err.min(1).max()))
        assert err.min(1).max() < 1e-3
        assert set(hit.tolist()) == owners
        np.testing.assert_array_equal(dets[k][:, 5], gt[hit, 4])


# ---- trainer -----------------------------------------------------------------------------------------------
TC, TB, TD = 3, 2, 128


@pytest.fixture
def bn_exact():
    """BatchNorm statistics in integer bins: identical by construction from run to run."""
    from cvlite import ops_nn as nn
    nn.set_bn_exact(True)
    yield
    nn.set_bn_exact(False)


def _trainer(candidates, graph, seed=1, **kw):
    from cvlite.retina_net import RetinaNetNet
    from cvlite.retinanet import RetinaNet
    from cvlite.train_retinanet import RetinaTrainer, synthetic_coco_batch
    rn = RetinaNet(TC, {})
    net = RetinaNetNet(TC, seed=seed)
    tr = RetinaTrainer(net, rn, TB, TD, n_max=16, candidates=candidates, use_graph=graph, targets="atss", **kw)
    tr.load_candidates(*synthetic_coco_batch(candidates * TB, TD, TC, n_max=16, seed=7))
    return net, tr


@pytest.mark.parametrize("candidates", [1, 3])
def test_trainer_graph_equals_eager_and_losses_match_the_restatement(bn_exact, candidates):
    res = {}
    for graph in (True, False):
        net, tr = _trainer(candidates, graph)
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        res[graph] = (net.store.flat.clone(), tr.losses.clone())
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][0], res[False][0])
    # the eager trainer's last forward: its losses are the restated loss on its outputs and targets
    assert tuple(tr.cand_targets.shape) == (candidates * TB, tr.P * tr.A, 8) and tuple(tr.ntgt.shape) == (TB, 5)
    assert float(tr.img_w.sum()) == TB and int(tr.ntgt.sum()) > 0
    np.testing.assert_array_equal(tr.cand_counts.cpu().numpy(), tr.cand_ntgt.sum(1).cpu().numpy())
    sel = tr.sel.cpu().numpy()
    want = ref.atss_assign(tr.cand_boxes.cpu().numpy()[sel], tr.cand_nbox.cpu().numpy()[sel],
                           tr.cand_dim.cpu().numpy()[sel], TD, TC)
    np.testing.assert_array_equal(tr.targets.cpu().numpy().reshape(want[0].shape), want[0])
    np.testing.assert_array_equal(tr.ntgt.cpu().numpy(), want[1])
    reg, cls = (t.detach().double().cpu() for t in tr.outputs)
    L64 = ref.atss_loss(reg, cls, want[0], want[1], tr.A, TC, img_weight=tr.img_w.cpu().numpy())
    print("trainer losses", tr.losses.cpu().numpy().tolist(), "restated", L64.numpy().tolist())
    np.testing.assert_allclose(tr.losses.cpu().numpy(), L64.numpy(), rtol=2e-5)


def test_trainer_loss_falls_on_a_fixed_batch(bn_exact):
    net, tr = _trainer(3, True)
    hist = []
    for _ in range(30):
        tr.step()
        hist.append(tr.losses.sum().clone())
    torch.cuda.synchronize()
    hist = [float(h) for h in hist]
    first, last = float(np.mean(hist[:3])), float(np.mean(hist[20:]))
    print("retina atss recipe: mean total loss steps 1..3 %.5f, steps 21..30 %.5f" % (first, last))
    assert np.isfinite(hist).all() and last < first


def test_reference_mode_is_untouched_and_bad_strings_raise(monkeypatch):
    from cvlite import ops_targets as ot
    from cvlite.retina_net import RetinaNetNet
    from cvlite.retinanet import RetinaNet
    from cvlite.train_retinanet import RetinaTrainer, synthetic_coco_batch
    RC = 4          # one-hot rows of 4 + 4 floats: the 16-byte row rule of cvl_gather_rows holds at P = 341
    rn = RetinaNet(RC, {}, anchor_sizes=[20.0, 40.0, 80.0, 160.0, 320.0])
    net = RetinaNetNet(RC, seed=1)
    with pytest.raises(ValueError):
        RetinaTrainer(net, rn, TB, TD, targets="paper")
    tr = RetinaTrainer(net, rn, TB, TD, n_max=16, use_graph=False)
    assert tr.target_kind == "reference" and not hasattr(tr, "ntgt") and not hasattr(tr, "cand_ntgt")
    assert tuple(tr.cand_targets.shape) == (3 * TB, tr.A * tr.P, 4 + RC)
    assert tuple(tr.targets.shape) == (TB, tr.A * tr.P, 4 + RC) and tuple(tr.cand_counts.shape) == (3 * TB,)
    calls = []
    for name in ("retina_assign", "retina_loss", "retina_atss_assign", "retina_atss_loss"):
        real = getattr(ot, name)
        monkeypatch.setattr(ot, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    tr.load_candidates(*synthetic_coco_batch(3 * TB, TD, RC, n_max=16, seed=7))
    tr.step()
    torch.cuda.synchronize()
    assert calls == ["retina_assign", "retina_loss"] and torch.isfinite(tr.losses).all()
