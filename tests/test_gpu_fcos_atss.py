"""The ATSS assignment on the GPU (csrc/fcos_atss.hip and everything above it) against the restatement
tests/fcos_atss_ref.py: targets, counts, candidates, IoUs and thresholds bit for bit; edge cases;
determinism; invalid arguments; the torch op with fcos_paper_loss on its targets (the tolerances of
tests/test_gpu_fcos_paper.py: rtol 2e-5 on the sums, rtol 1e-4 / atol 1e-6 on fp32 gradients); the
trainer."""
import functools

import numpy as np
import pytest
import torch

import fcos_atss_ref as ref

pytestmark = pytest.mark.gpu

PAD = ref.PAD
f32 = np.float32


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _gpu_assign(boxes, nbox, dims, C, candidates=True, pad=PAD, **kw):
    from cvlite import ops_targets as ot
    b, n, d = _dev(np.asarray(boxes, f32), np.asarray(nbox, np.int32), np.asarray(dims, f32))
    out = ot.fcos_atss_assign(b, n, d, pad, C, return_candidates=candidates, **kw)
    return [t.cpu().numpy() for t in out]


@functools.lru_cache(maxsize=None)
def _scene_batch(families, seeds, C, n_box):
    sc = [ref.scene(s, f, C, n_box=n_box, n_max=n_box) for f in families for s in seeds]
    return np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])


@functools.lru_cache(maxsize=None)
def _want(families, seeds, C, n_box, topk, scale):
    """The restatement's result for a batch of scenes, computed once and shared."""
    boxes, dims = _scene_batch(families, seeds, C, n_box)
    return ref.atss_assign(boxes, [n_box] * len(boxes), dims, PAD, C, topk=topk, anchor_scale=scale)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check(got, want):
    """targets, num_targets[, cand_cells, cand_iou, cand_thr] as bits against the restatement's."""
    names = ("targets", "num_targets", "cand_cells", "cand_iou", "cand_thr")
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=name)


# ---- bit-exact against the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 20])
@pytest.mark.parametrize("family", ["A", "B"])
def test_assign_bit_exact_scenes(family, C):
    """Seeds 0..7 as one batch of 8 at the default anchor_scale 8; P = 1022 is no multiple of the
    256-cell tile and the maps are not square.  With and without the optional outputs."""
    boxes, dims = _scene_batch(family, tuple(range(8)), C, 8)
    want = _want(family, tuple(range(8)), C, 8, 9, 8.0)
    assert (want[1].sum(1) > 0).all()
    got = _gpu_assign(boxes, [8] * 8, dims, C)
    assert got[0].shape == (8, 1022, 5 + C)
    _check(got, want)
    plain = _gpu_assign(boxes, [8] * 8, dims, C, candidates=False)
    assert len(plain) == 2
    _check(plain, want)


@pytest.mark.parametrize("topk", [1, 9, 16])
def test_assign_bit_exact_24_boxes(topk):
    """The 24-box scenes, seeds 0..3, at anchor_scale 2: positives on every level and contested cells."""
    boxes, dims = _scene_batch("A", (0, 1, 2, 3), 20, 24)
    want = _want("A", (0, 1, 2, 3), 20, 24, topk, 2.0)
    if topk == 9:
        assert (want[1][:2] > 0).all() and (want[5] >= 2).sum() >= 20
    _check(_gpu_assign(boxes, [24] * 4, dims, 20, topk=topk, anchor_scale=2.0), want)
    _check(_gpu_assign(boxes, [24] * 4, dims, 20, candidates=False, topk=topk, anchor_scale=2.0), want)


def _px(rows, n_max, dim):
    H, W = dim
    out = np.zeros((n_max, 5), f32)
    for k, (y, x, h, w, c) in enumerate(rows):
        out[k] = [y / H, x / W, h / H, w / W, c]
    return out


def test_assign_edge_cases():
    """One batch: nbox 0, > n_max and negative; labels -1 and C; zero and negative height; NaN size, label
    and centre; centres exactly on grid corners; duplicated boxes; boxes outside the image, one of them
    so far that the window check must send the selection to the whole level; img_dim below the pad."""
    C, n_max = 3, 8
    nan = float("nan")
    dim = (250.0, 181.0)
    imgs = [
        [(128, 96, 100, 80, 1), (128, 96, 100, 80, 0), (64, 64, 40, 40, 2), (8, 8, 12, 12, 0),       # corners, duplicates
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
    want = ref.atss_assign(boxes, nbox, dims, PAD, C)
    tg, cnt, cells, _, thr, npair, owner = want
    assert cnt[0].sum() > 0 and cnt[1].sum() > 0 and cnt[3].sum() > 0 and not cnt[2].any() and not cnt[4].any()
    assert (npair[0] == 2).any() and (cells[0, 4:] == -1).all() and (cells[1, :2] == -1).all()
    assert cells[1, 2, :9].tolist() == list(range(9)) and np.isfinite(tg).all()
    assert (cells[1, 5, :9] >= 0).all() and (owner[1] == 6).any()
    _check(_gpu_assign(boxes, nbox, dims, C), want)
    _check(_gpu_assign(boxes, nbox, dims, C, candidates=False), want)


def test_assign_256_boxes_and_narrow_tile():
    """n_max = 256 with 256 valid small boxes on a 6 px lattice with jitter, so the contest sees many
    boxes per cell; and C = 80, whose rows need the 128-cell tile."""
    rng = np.random.default_rng(5)
    H, W = float(PAD[0]), float(PAD[1])
    rows = [(40 + 6 * (k // 16) + rng.uniform(-2, 2), 30 + 6 * (k % 16) + rng.uniform(-2, 2),
             rng.uniform(18, 40), rng.uniform(18, 40), int(rng.integers(0, 5))) for k in range(256)]
    boxes = _px(rows, 256, (H, W))[None]
    dims = np.array([[H, W]], f32)
    want = ref.atss_assign(boxes, [256], dims, PAD, 5, anchor_scale=4.0)
    assert want[5].max() >= 4 and (want[5] >= 2).sum() >= 50
    _check(_gpu_assign(boxes, [256], dims, 5, anchor_scale=4.0), want)
    b80, d80 = _scene_batch("B", (0, 1), 80, 8)
    _check(_gpu_assign(b80, [8, 8], d80, 80), _want("B", (0, 1), 80, 8, 9, 8.0))


def test_assign_large_levels_and_far_centres():
    """A 512 x 384 pad: level 0 has 64 x 48 = 3072 cells, more than a lane's register cache holds, so the
    whole-level selection that a rejected window falls back to recomputes its keys every round.  Far and
    NaN centres take that path on every level; the ordinary boxes beside them take the window."""
    pad, C = (512, 384), 4
    dim = (500.0, 380.0)
    nan = float("nan")
    rows = [(250, 190, 200, 150, 1), (1e9, 96, 50, 50, 1), (128, -1e6, 3e6, 3e6, 0), (nan, 96, 100, 80, 2),
            (256, 192, 64, 64, 3), (3e38, 3e38, 10, 10, 0), (40, 350, 60, 50, 2), (-2e5, -2e5, 5e5, 5e5, 3)]
    boxes = _px(rows, 8, dim)[None]
    dims = np.array([dim], f32)
    for topk in (9, 16):
        want = ref.atss_assign(boxes, [8], dims, pad, C, topk=topk)
        assert want[1].sum() > 0 and want[2][0, 3, :topk].tolist() == list(range(topk))
        assert len(set(want[6][want[6] >= 0].tolist())) >= 4
        _check(_gpu_assign(boxes, [8], dims, C, pad=pad, topk=topk), want)


def test_assign_is_deterministic():
    """20 calls on the 24-box batch: 20 bit-identical results (targets and counts)."""
    from cvlite import ops_targets as ot
    boxes, dims = _scene_batch("A", (0, 1, 2, 3), 20, 24)
    b, n, d = _dev(boxes, np.full(4, 24, np.int32), dims)
    first = None
    for _ in range(20):
        tg, nt = ot.fcos_atss_assign(b, n, d, PAD, 20, anchor_scale=2.0)
        if first is None:
            first = (tg.clone(), nt.clone())
            assert int(nt.sum()) > 0
        else:
            assert torch.equal(tg.view(torch.int32), first[0].view(torch.int32)) and torch.equal(nt, first[1])


def test_invalid_arguments_leave_targets_untouched():
    from cvlite import _lib
    from cvlite import ops_targets as ot
    boxes, dims = _scene_batch("A", (0,), 3, 8)
    b, n, d = _dev(boxes, np.array([8], np.int32), dims)
    out = torch.full((1, 1022, 8), 7.0, device="cuda")
    nt = torch.full((1, 5), 7, dtype=torch.int32, device="cuda")
    for kw in (dict(topk=0), dict(topk=17), dict(anchor_scale=0.0), dict(anchor_scale=-1.0)):
        with pytest.raises(_lib.CvlError):
            ot.fcos_atss_assign(b, n, d, PAD, 3, out=out, num_targets=nt, **kw)
    big = torch.zeros((1, 257, 5), device="cuda")
    with pytest.raises(_lib.CvlError):
        ot.fcos_atss_assign(big, n, d, PAD, 3, out=out, num_targets=nt)
    # a short workspace, through the C entry itself
    need = int(_lib.load().cvl_fcos_atss_workspace_size(1, 1022))
    assert need == 1022 * 8 and int(_lib.load().cvl_fcos_atss_workspace_size(0, 1022)) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    st = (_lib.ctypes.c_int32 * 5)(*ref.STRIDES)
    args = lambda nbytes: (_lib.ptr(b), _lib.ptr(n), _lib.ptr(d), 1, 8, PAD[0], PAD[1], 3,   # noqa: E731
                           _lib.ctypes.cast(st, _lib.c_void_p), 9, 8.0, _lib.ptr(out), _lib.ptr(nt), None, None, None,
                           _lib.ptr(ws), nbytes, _lib.stream())
    with pytest.raises(_lib.CvlError):
        _lib.call("cvl_fcos_atss_assign", *args(need - 8))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((nt == 7).all())
    _lib.call("cvl_fcos_atss_assign", *args(need))                    # the same call with enough room runs
    torch.cuda.synchronize()
    assert int(nt.sum()) > 0 and not bool((out == 7.0).any())


# ---- torch op --------------------------------------------------------------------------------------------
def test_torch_op_and_paper_loss_on_its_targets():
    import cvlite.torch_ops  # noqa: F401
    from cvlite import ops_targets as ot
    from fcos_paper_ref import paper_loss, target_norm
    C = 3
    boxes, dims = _scene_batch("B", (0, 1), C, 8)
    b, n, d = _dev(boxes, np.array([8, 8], np.int32), dims)
    tg, nt = torch.ops.cvlite.fcos_atss_assign(b, n, d, PAD[0], PAD[1], C, 9, 8.0)
    tg2, nt2 = ot.fcos_atss_assign(b, n, d, PAD, C)
    assert torch.equal(tg, tg2) and torch.equal(nt, nt2)
    want = _want("B", (0, 1), C, 8, 9, 8.0)
    np.testing.assert_array_equal(tg.cpu().numpy(), want[0])
    tg_ref = want[0]
    norm = torch.ops.cvlite.fcos_target_norm(tg, C)
    np.testing.assert_allclose(norm.cpu().numpy(), target_norm(tg_ref, C), rtol=1e-6)
    rng = np.random.default_rng(11)
    B, P = tg_ref.shape[:2]
    reg = rng.normal(0, 1, (B, P, 8)).astype(f32)
    reg[..., :4] = tg_ref[..., :4] + rng.normal(0, 0.5, (B, P, 4)).astype(f32)
    cls = (rng.normal(0, 2, (B, P, 8)) - 2).astype(f32)
    w = torch.tensor([[0.7, 1.3, 0.4], [1.1, 0.2, 2.0]], dtype=torch.float64)
    r64 = torch.tensor(reg, dtype=torch.float64, requires_grad=True)
    c64 = torch.tensor(cls, dtype=torch.float64, requires_grad=True)
    L64 = paper_loss(r64, c64, tg_ref, C, norm=norm.cpu().numpy())
    (L64 * w).sum().backward()
    r = torch.tensor(reg, device="cuda", requires_grad=True)
    c = torch.tensor(cls, device="cuda", requires_grad=True)
    L = torch.ops.cvlite.fcos_paper_loss(r, c, tg, norm, C)
    assert float(L64.detach()[:, 1].min()) > 0
    np.testing.assert_allclose(L.detach().cpu().numpy(), L64.detach().numpy(), rtol=2e-5)
    (L * w.float().cuda()).sum().backward()
    np.testing.assert_allclose(r.grad.cpu().numpy(), r64.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(c.grad.cpu().numpy(), c64.grad.numpy(), rtol=1e-4, atol=1e-6)


# ---- trainer -----------------------------------------------------------------------------------------------
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
    tr = FCOSTrainer(net, TB, (TD, TD), use_graph=False, targets="atss")
    tr.load_batch(imgs, boxes, nbox)
    tr.run_fwd_bwd()
    torch.cuda.synchronize()
    assert int(tr.ntgt.sum()) > 0 and float(tr.norm[:, 0].sum()) == float(tr.ntgt.sum())

    net2 = FCOSNet(TC, seed=1)
    dims = torch.full((TB, 2), float(TD), device="cuda")
    tg, nt = ot.fcos_atss_assign(tr.boxes, nbox, dims, (TD, TD), TC)
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
    # the keywords reach the kernel: another topk gives other targets
    tr1 = FCOSTrainer(FCOSNet(TC, seed=1), TB, (TD, TD), use_graph=False, targets="atss", atss_topk=1, atss_scale=4.0)
    tr1.load_batch(imgs, boxes, nbox)
    tr1.run_fwd_bwd()
    tg1, _ = ot.fcos_atss_assign(tr.boxes, nbox, dims, (TD, TD), TC, topk=1, anchor_scale=4.0)
    torch.cuda.synchronize()
    assert torch.equal(tr1.targets, tg1) and not torch.equal(tg1, tg)


def test_trainer_graph_replay_equals_eager_and_loss_falls(bn_exact):
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer
    imgs, boxes, nbox = _batch()
    res = {}
    for graph in (False, True):
        net = FCOSNet(TC, seed=1)
        tr = FCOSTrainer(net, TB, (TD, TD), use_graph=graph, targets="atss", init_lr=1e-3)
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
    print("atss recipe: total loss step 1 %.5f, step 30 %.5f" % (first, last))
    assert np.isfinite(last) and last < first


def test_trainer_rejects_centre_network():
    from cvlite.train_fcos import FCOSTrainer, JitterFCOSTrainer, train

    class Centre(object):
        cen_heads = ()
        C = 3
    with pytest.raises(ValueError):
        FCOSTrainer(Centre(), 2, (128, 128), targets="atss")
    with pytest.raises(ValueError):
        JitterFCOSTrainer(Centre(), 2, targets="atss")
    with pytest.raises(ValueError):
        train([{"image": np.zeros((128, 128, 3), f32), "bbox": np.zeros((0, 4), f32), "label": []}] * 2, [],
              Centre(), 2, None, None, None, 0, 1, recipe="atss")


def test_jitter_trainer_atss_two_sizes():
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import JitterFCOSTrainer, synthetic_batch
    net = FCOSNet(TC, seed=0)
    jt = JitterFCOSTrainer(net, 2, use_graph=False, targets="atss", atss_topk=7, atss_scale=6.0)
    a, boxes, nbox = synthetic_batch(2, 128, 128, TC, seed=3)
    b, _, _ = synthetic_batch(1, 256, 256, TC, seed=4)
    dims = np.array([[128, 128], [256, 256]], f32)
    losses = jt.step([a[0], b[0]], boxes, nbox, dims)
    torch.cuda.synchronize()
    assert sorted(jt.buckets) == [(128, 1), (256, 1)]
    assert all(t.target_kind == "atss" and t.atss_topk == 7 and t.atss_scale == 6.0 for t in jt.buckets.values())
    assert torch.isfinite(losses).all() and float(losses.sum()) > 0
    for k, pad in enumerate((128, 256)):      # positive cells per level, as the restatement counts them
        cnt = ref.atss_assign(boxes[k:k + 1].cpu().numpy(), nbox[k:k + 1].cpu().numpy(), dims[k:k + 1], (pad, pad),
                              TC, topk=7, anchor_scale=6.0)[1]
        assert cnt.sum() > 0
        np.testing.assert_array_equal(jt.ntgt[k].cpu().numpy(), cnt[0])


def test_train_atss_reaches_the_evaluation_hook_clamped(monkeypatch, tmp_path):
    """train(recipe="atss") builds an "atss" trainer with its keywords and calls the evaluation hook with
    clamp_reg=True (a stub stands in for evaluate_fcos)."""
    import cvlite.evaluate as ev
    from cvlite.fcos_net import FCOSNet
    from cvlite import train_fcos
    seen, made = [], []

    def stub(net, data, C, **kw):
        seen.append(kw)
        return {"mAP": 0.0}
    monkeypatch.setattr(ev, "evaluate_fcos", stub)
    real = train_fcos.FCOSTrainer

    class Spy(real):
        def __init__(self, *a, **kw):
            made.append(kw)
            real.__init__(self, *a, **kw)
    monkeypatch.setattr(train_fcos, "FCOSTrainer", Spy)
    rng = np.random.default_rng(0)
    samples = [{"image": rng.uniform(-1, 1, (128, 128, 3)).astype(f32),
                "bbox": np.array([[0.5, 0.5, 0.4, 0.3]], f32), "label": [1]} for _ in range(2)]
    net = FCOSNet(TC, seed=0)
    train_fcos.train(samples, [], net, 2, None, None, None, 0, 1, weight_decay=0.0, eval_data=samples, eval_every=1,
                     recipe="atss", atss_topk=5, atss_scale=4.0, save_loss_file=str(tmp_path / "loss.csv"))
    assert len(seen) == 1 and seen[0]["clamp_reg"] is True
    assert made[0]["targets"] == "atss" and made[0]["atss_topk"] == 5 and made[0]["atss_scale"] == 4.0
