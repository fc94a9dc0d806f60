"""The task-aligned assignment and its loss on the GPU (csrc/fcos_tal.hip and everything above it) against
the restatement tests/fcos_tal_ref.py.  Assignment: the selected cells per box and rank, the winners per
cell, num_targets, the (t, b, l, r) and one-hot columns equal exactly (the committed scenes are decided:
float64 names every selection and winner with a margin of 1e-3, far above fp32's error); the IoUs within
rtol 2e-5, the project's fused-loss bound; the metric, slot 4 and the boxes' best metric within rtol 1e-4
(six fp32 factors of u, an expf and a float64 quotient rounded once).  Loss: rtol 2e-5 on the per-image
sums, rtol 1e-4 / atol 1e-6 on every fp32 gradient element (tests/test_gpu_fcos_paper.py's bounds).  All
kernel cases run B 3 on PAD (256, 192): P = 1022 cells, no multiple of any tile; the staging case runs
on (640, 640): P = 8525 cells, more than the 6144 keys a workgroup stages.

The trainer cases run at 128 x 128, bs 2, the geometry of the ATSS trainer tests."""
import functools

import numpy as np
import pytest
import torch

import fcos_tal_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
B = 3
P = sum(h * w for h, w in ref.level_shapes(ref.PAD))


def _dev(*arrs):
    return [torch.tensor(np.asarray(a)).cuda() for a in arrs]           # (a copy: the cached cases are read-only)


def _ld_cls(C):
    return (C + 7) // 8 * 8 + 8                                          # always padded


@functools.lru_cache(maxsize=None)
def _scene(C, cfg, pad=ref.PAD):
    """The committed scene of a configuration and the restatement's result on it (computed once)."""
    topk, clamp, alpha, beta = cfg
    seed = ref.SEEDS[(C,) + cfg] if pad == ref.PAD else ref.BIG_SEED
    sc = ref.scene(seed, C, ld_cls=_ld_cls(C), pad=pad)
    want = ref.scene_assign(sc, topk=topk, clamp=bool(clamp), alpha=alpha, beta=beta)
    assert ref.decided_result(want, topk)
    for a in list(sc.values()) + list(want.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc, want


def _gpu_assign(sc, cfg, candidates=True, out=None, **over):
    from cvlite import ops_targets as ot
    topk, clamp, alpha, beta = cfg
    b, n, d, dist, cls = _dev(sc["boxes"], sc["nbox"], sc["dims"], sc["dist"], sc["cls"])
    kw = dict(topk=topk, alpha=alpha, beta=beta, clamp=bool(clamp), return_candidates=candidates, out=out)
    kw.update(over)
    res = ot.fcos_tal_assign(b, n, d, sc["pad"], sc["C"], kw.pop("dist", dist), kw.pop("cls", cls), **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in res]


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want)), initial=0.0))


def _check_assign(got, want, C, tag):
    tg, cnt, cells, metric, iou, bmax = got
    np.testing.assert_array_equal(cells, want["cand_cells"], err_msg="selected cells per box and rank")
    pos = tg[..., 5:].max(-1) >= 1
    np.testing.assert_array_equal(pos, want["owner"] >= 0, err_msg="won cells")
    np.testing.assert_array_equal(cnt, want["counts"])
    np.testing.assert_array_equal(tg[..., :4], want["targets"][..., :4])
    np.testing.assert_array_equal(tg[..., 5:], want["targets"][..., 5:])     # the winner's one-hot class
    print("%s: max rel err cand_iou %.2e, box max_u %.2e, cand_metric %.2e, slot 4 %.2e, box max_m %.2e"
          % (tag, _rel(iou, want["cand_iou"]), _rel(bmax[..., 1], want["box_max"][..., 1]),
             _rel(metric, want["cand_metric"]), _rel(tg[..., 4], want["that"]),
             _rel(bmax[..., 0], want["box_max"][..., 0])))
    np.testing.assert_allclose(iou, want["cand_iou"], rtol=2e-5, atol=0)
    np.testing.assert_allclose(bmax[..., 1], want["box_max"][..., 1], rtol=2e-5, atol=0)
    np.testing.assert_allclose(metric, want["cand_metric"], rtol=1e-4, atol=0)
    np.testing.assert_allclose(tg[..., 4], want["that"], rtol=1e-4, atol=0)
    np.testing.assert_allclose(bmax[..., 0], want["box_max"][..., 0], rtol=1e-4, atol=0)
    assert not tg[~pos].any() and (metric[cells < 0] == 0).all() and (iou[cells < 0] == 0).all()


# ---- the assignment ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ref.CONFIGS, ids=lambda c: "k%d-clamp%d-a%g-b%g" % c)
@pytest.mark.parametrize("C", [1, 20, 80])
def test_assign_against_the_restatement(C, cfg):
    sc, want = _scene(C, cfg)
    assert sc["dist"].shape == (B, P, 8) and sc["cls"].shape == (B, P, _ld_cls(C))
    assert want["counts"][:2].sum(1).min() > 0 and not want["counts"][2].any()
    got = _gpu_assign(sc, cfg)
    assert got[0].shape == (B, P, 5 + C) and got[2].shape == (B, ref.N_MAX, cfg[0])
    _check_assign(got, want, C, "C %d %r" % (C, cfg))
    plain = _gpu_assign(sc, cfg, candidates=False)                # the optional outputs change nothing
    assert len(plain) == 2
    np.testing.assert_array_equal(plain[0].view(np.uint32), got[0].view(np.uint32))
    np.testing.assert_array_equal(plain[1], got[1])


def test_whole_pad_box_beyond_the_staged_keys():
    """(640, 640): P = 8525 cells, every one inside the whole-pad box and nearly every one a candidate --
    more than the 6144 keys a workgroup stages, so that box's rounds recompute their keys; the other boxes
    of the same launch are staged."""
    cfg = (13, 1, 1.0, 6.0)
    sc, want = _scene(20, cfg, pad=ref.BIG_PAD)
    assert sc["dist"].shape[1] == 8525 and want["metrics"][0].size > 6144
    assert all(m.size <= 6144 for m in want["metrics"][1:])
    got = _gpu_assign(sc, cfg)
    _check_assign(got, want, 20, "P 8525")


def test_two_runs_are_bit_identical():
    cfg = (13, 1, 1.0, 6.0)
    for C, pad in ((20, ref.PAD), (20, ref.BIG_PAD)):
        sc, _ = _scene(C, cfg, pad=pad)
        a, b = _gpu_assign(sc, cfg), _gpu_assign(sc, cfg)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("clamp", [1, 0])
def test_nan_predictions_outside_every_box_change_nothing(clamp):
    cfg = (13, clamp, 1.0, 6.0)
    sc, want = _scene(20, cfg)
    out = ~want["inside"]
    assert out[1].sum() > 100 and out[2].all()
    dist, cls = sc["dist"].copy(), sc["cls"].copy()
    dist[out] = np.nan
    cls[out] = np.nan
    good = _gpu_assign(sc, cfg)
    bad = _gpu_assign(sc, cfg, dist=_dev(dist)[0], cls=_dev(cls)[0])
    for x, y in zip(good, bad):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.isfinite(bad[0]).all()


def test_invalid_arguments_leave_the_targets_untouched():
    from cvlite import _lib
    cfg = (13, 1, 1.0, 6.0)
    C = 20
    sc, _ = _scene(C, cfg)
    out = torch.full((B, P, 5 + C), float("nan"), device="cuda")
    nt = torch.full((B, 5), -7, dtype=torch.int32, device="cuda")
    dist, cls = _dev(sc["dist"], sc["cls"])
    bad = [dict(topk=0), dict(topk=33), dict(topk=-1), dict(alpha=-0.5), dict(beta=-1.0), dict(alpha=float("nan")),
           dict(beta=float("nan")), dict(dist=dist[..., :3].contiguous()), dict(cls=cls[..., :C - 1].contiguous())]
    for kw in bad:
        with pytest.raises(_lib.CvlError):
            _gpu_assign(sc, cfg, out=out, num_targets=nt, **kw)
    big = dict(sc, boxes=np.zeros((B, 257, 5), f32))                  # n_max beyond 256
    with pytest.raises(_lib.CvlError):
        _gpu_assign(big, cfg, out=out, num_targets=nt)
    # a short workspace, through the C entry itself
    lib = _lib.load()
    need = int(lib.cvl_fcos_tal_workspace_size(B, P, ref.N_MAX))
    assert need == B * P * 8 + B * ref.N_MAX * 32 * 12 + B * ref.N_MAX * 8
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    bx, nb, dm = _dev(sc["boxes"], sc["nbox"], sc["dims"])
    st = (_lib.ctypes.c_int32 * 5)(*ref.STRIDES)
    args = lambda nbytes: (_lib.ptr(bx), _lib.ptr(nb), _lib.ptr(dm), B, ref.N_MAX, 256, 192, C,  # noqa: E731
                           _lib.ctypes.cast(st, _lib.c_void_p), _lib.ptr(dist), 8, 1, _lib.ptr(cls), _ld_cls(C), 13,
                           1.0, 6.0, _lib.ptr(out), _lib.ptr(nt), None, None, None, None, _lib.ptr(ws), nbytes,
                           _lib.stream())
    with pytest.raises(_lib.CvlError):
        _lib.call("cvl_fcos_tal_assign", *args(need - 8))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((nt == -7).all())
    _lib.call("cvl_fcos_tal_assign", *args(need))                     # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and not bool((nt == -7).any())


# ---- the loss ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_case(C, with_norm, grad_scale, qfl_beta=2.0, w_box=2.0):
    """Head outputs of the committed scene, the restatement's targets on them, the fp32 norm both sides
    read, and the float64 losses and gradients (computed once)."""
    sc, res = _scene(C, (13, 1, 1.0, 6.0))
    tg = res["targets"]
    norm = ref.target_norm(tg, C) if with_norm else None
    want = ref.tal_loss_reference(sc["dist"], sc["cls"], tg, C, norm=norm, grad_scale=grad_scale, qfl_beta=qfl_beta,
                                  w_box=w_box)
    for a in want:
        a.setflags(write=False)
    return dict(reg=sc["dist"], cls=sc["cls"], targets=tg), norm, want


def _run_loss(inp, norm, C, gdt=torch.float32, ld_dreg=None, with_grad=True, **kw):
    from cvlite import ops_targets as ot
    reg, cls, tg = _dev(inp["reg"], inp["cls"], inp["targets"])
    nm = None if norm is None else _dev(norm)[0]
    d_reg = d_cls = None
    if with_grad:        # pre-filled: every element has to be written
        d_reg = torch.full((B, P, ld_dreg or reg.shape[2]), float("nan"), dtype=gdt, device="cuda")
        d_cls = torch.full((B, P, cls.shape[2]), float("nan"), dtype=gdt, device="cuda")
    out = ot.fcos_tal_loss(reg, cls, tg, C, norm=nm, with_grad=with_grad, d_reg=d_reg, d_cls=d_cls, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("with_norm", [True, False])
@pytest.mark.parametrize("C", [1, 20, 80])
def test_loss_and_gradients_against_float64(C, with_norm):
    inp, norm, (L, g_reg, g_cls) = _loss_case(C, with_norm, 0.37)
    losses, d_reg, d_cls = [t.cpu().numpy() for t in _run_loss(inp, norm, C, grad_scale=0.37)]
    print("C %d norm %s: losses max rel err %.2e; d_reg max abs err %.2e, d_cls %.2e"
          % (C, with_norm, _rel(losses, L), np.abs(d_reg - g_reg).max(), np.abs(d_cls - g_cls).max()))
    assert (L[:2, :2] > 0).all() and L[2, 0] > 0 and L[2, 1] == 0 and not L[:, 2].any()
    if with_norm:
        assert (norm[:2, 1] > 1).all()                     # the divisor is the sum of slot 4, not its floor
    np.testing.assert_allclose(losses, L, rtol=2e-5)
    assert d_reg.shape == g_reg.shape == (B, P, 8) and d_cls.shape == g_cls.shape
    np.testing.assert_allclose(d_reg, g_reg, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(d_cls, g_cls, rtol=1e-4, atol=1e-6)
    pos = inp["targets"][..., 5:].max(-1) >= 1
    assert not d_reg[~pos].any() and not d_reg[..., 4:].any() and not d_cls[..., C:].any()
    assert np.abs(d_reg[pos]).max() > 1e-4 and np.abs(d_cls).max() > 1e-4


def test_target_norm_of_the_aligned_targets():
    from cvlite import ops_targets as ot
    inp, norm, _ = _loss_case(20, True, 0.37)
    got = ot.fcos_target_norm(_dev(inp["targets"])[0], 20).cpu().numpy()
    np.testing.assert_array_equal(got[:, 0], norm[:, 0])
    np.testing.assert_allclose(got[:, 1], norm[:, 1], rtol=1e-6)


@pytest.mark.parametrize("kw", [dict(beta=1.5), dict(beta=0.0, box_weight=1.0), dict(box_weight=0.5)])
def test_loss_keywords_reach_the_kernel(kw):
    C = 20
    rk = dict(qfl_beta=kw.get("beta", 2.0), w_box=kw.get("box_weight", 2.0))
    inp, norm, (L, g_reg, g_cls) = _loss_case(C, True, 1.0, **rk)
    losses, d_reg, d_cls = _run_loss(inp, norm, C, **kw)
    np.testing.assert_allclose(losses.cpu().numpy(), L, rtol=2e-5)
    np.testing.assert_allclose(d_reg.cpu().numpy(), g_reg, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(d_cls.cpu().numpy(), g_cls, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("C", [1, 20, 80])
def test_loss_bf16_gradients_are_rounded_fp32(C):
    """bf16 gradient outputs in the trainer's layout (d_reg 32 wide off the 8-wide reg) equal the fp32
    outputs rounded to bf16, bit for bit; padding zero."""
    inp, norm, _ = _loss_case(C, True, 0.37)
    l32, r32, c32 = _run_loss(inp, norm, C, ld_dreg=32, grad_scale=0.37)
    l16, r16, c16 = _run_loss(inp, norm, C, gdt=torch.bfloat16, ld_dreg=32, grad_scale=0.37)
    assert torch.equal(l32, l16)
    assert torch.equal(r16, r32.to(torch.bfloat16)) and torch.equal(c16, c32.to(torch.bfloat16))
    assert not r16[..., 4:].any() and not c16[..., C:].any() and bool(r16[..., :4].any())


def test_forward_only_and_two_runs():
    C = 20
    inp, norm, _ = _loss_case(C, True, 0.37)
    a = _run_loss(inp, norm, C, grad_scale=0.37)
    b = _run_loss(inp, norm, C, grad_scale=0.37)
    fwd, none_r, none_c = _run_loss(inp, norm, C, with_grad=False, grad_scale=0.37)
    assert none_r is None and none_c is None
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert torch.equal(fwd, a[0])


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 20, 80])
def test_lds_form_bit_identical_to_row_form(dispatch, C, gdt):
    """The LDS-staged kernel (256-cell tiles at C 1 and 20, 64-cell tiles at C 80) against the row-pointer
    kernel on the same tiles (CVL_DISPATCH=loss_rows): one fp32 sequence per cell and one sum order."""
    inp, norm, _ = _loss_case(C, True, 0.37)
    outs = []
    for rows in ("1", "0"):
        dispatch("loss_rows=" + rows)
        outs.append(_run_loss(inp, norm, C, gdt=gdt, grad_scale=0.37))
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y), float((x.double() - y.double()).abs().max())
    # gradient rows that take no 16-byte stores (5 fp32 columns) run the row form by themselves
    if gdt == torch.float32:
        losses, d_reg, _ = _run_loss(inp, norm, C, ld_dreg=5, grad_scale=0.37)
        assert torch.equal(losses, outs[0][0]) and torch.equal(d_reg, outs[0][1][..., :5])


def test_non_positive_cells_never_read_their_box_rows(dispatch):
    C = 20
    inp, norm, _ = _loss_case(C, True, 0.37)
    pos = inp["targets"][..., 5:].max(-1) >= 1
    poisoned = dict(inp, reg=inp["reg"].copy())
    poisoned["reg"][~pos] = np.nan
    poisoned["reg"][..., 4:] = np.nan                       # nor the centerness column of any cell
    for rows in ("0", "1"):
        dispatch("loss_rows=" + rows)
        for x, y in zip(_run_loss(inp, norm, C), _run_loss(poisoned, norm, C)):
            assert torch.isfinite(x).all() and torch.equal(x, y)


def test_loss_invalid_arguments_leave_outputs_untouched():
    from cvlite import _lib
    from cvlite import ops_targets as ot
    C = 20
    inp, norm, _ = _loss_case(C, True, 0.37)
    reg, cls, tg, nm = _dev(inp["reg"], inp["cls"], inp["targets"], norm)
    losses = torch.full((B, 3), 7.0, device="cuda")
    d_reg = torch.full((B, P, 8), 7.0, device="cuda")
    d_cls = torch.full((B, P, cls.shape[2]), 7.0, device="cuda")
    run = lambda r=reg, c=cls, dr=d_reg, dc=d_cls, **kw: ot.fcos_tal_loss(   # noqa: E731
        r, c, tg, C, norm=nm, d_reg=dr, d_cls=dc, losses=losses, **kw)
    bad = [dict(beta=-1.0), dict(beta=float("nan")), dict(r=reg[..., :4].contiguous()),
           dict(c=cls[..., :C - 1].contiguous()), dict(dr=torch.full((B, P, 4), 7.0, device="cuda")),
           dict(dc=torch.full((B, P, C - 1), 7.0, device="cuda"))]
    for kw in bad:
        with pytest.raises(_lib.CvlError):
            run(**kw)
        for t in (kw.get("dr"), kw.get("dc")):
            assert t is None or bool((t == 7.0).all())
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (losses, d_reg, d_cls))
    run()
    torch.cuda.synchronize()
    assert not any(bool((t == 7.0).any()) for t in (losses, d_reg, d_cls))


def test_torch_ops_match_ops_targets_with_autograd():
    """torch.ops.cvlite.fcos_tal_assign / fcos_tal_loss: the targets and losses of ops_targets, and
    autograd gradients = the kernel's gradient rows scaled by the upstream per-image, per-term weights."""
    import cvlite.torch_ops  # noqa: F401
    from cvlite import ops_targets as ot
    C, cfg = 20, (13, 1, 1.0, 6.0)
    sc, _ = _scene(C, cfg)
    bx, nb, dm, dist, cls = _dev(sc["boxes"], sc["nbox"], sc["dims"], sc["dist"], sc["cls"])
    tg0, nt0 = ot.fcos_tal_assign(bx, nb, dm, ref.PAD, C, dist, cls)
    tg, nt = torch.ops.cvlite.fcos_tal_assign(bx, nb, dm, ref.PAD[0], ref.PAD[1], C, dist, cls)
    assert torch.equal(tg, tg0) and torch.equal(nt, nt0)
    tg5, _ = torch.ops.cvlite.fcos_tal_assign(bx, nb, dm, ref.PAD[0], ref.PAD[1], C, dist, cls, 5, 0.5, 2.0, False)
    tg5_0, _ = ot.fcos_tal_assign(bx, nb, dm, ref.PAD, C, dist, cls, topk=5, alpha=0.5, beta=2.0, clamp=False)
    assert torch.equal(tg5, tg5_0) and not torch.equal(tg5, tg)
    nm = torch.ops.cvlite.fcos_target_norm(tg, C)
    L0, g_reg, g_cls = ot.fcos_tal_loss(dist, cls, tg, C, norm=nm, beta=1.5, box_weight=1.0)
    r = dist.clone().requires_grad_(True)
    c = cls.clone().requires_grad_(True)
    L = torch.ops.cvlite.fcos_tal_loss(r, c, tg, nm, C, 1.5, 1.0)
    assert torch.equal(L.detach(), L0)
    w = torch.tensor([[0.5, 2.0, 9.0], [1.0, 0.25, 9.0], [3.0, 1.0, 9.0]], device="cuda")
    (L * w).sum().backward()
    assert torch.equal(r.grad, g_reg * w[:, 1].view(-1, 1, 1)) and not r.grad[..., 4:].any()
    assert torch.equal(c.grad[..., :C], g_cls[..., :C] * w[:, 0].view(-1, 1, 1)) and not c.grad[..., C:].any()
    assert bool(r.grad.any()) and bool(c.grad.any())


# ---- trainer ---------------------------------------------------------------------------------------------------
TC, TB, TD = 3, 2, 128
# beta 2 in the place of 6: near its initialisation the network predicts boxes of a fraction of a pixel, whose
# IoU to the sixth power leaves fp32's range
TOPK, BETA = 5, 2.0


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


def _sets_decided(res, topk, margin=1e-3):
    """What the targets buffer depends on: per box the SET of selected cells (the gap between the last
    selected and the first unselected metric), the contests, and no metric near fp32's zero."""
    for m in res["metrics"]:
        if m.size and m.min() < ref.TINY:
            return False
        if m.size > topk and not m[topk - 1] - m[topk] > margin * m[topk - 1]:
            return False
    return all(u[0] - u[1] > margin * u[0] for u in res["contests"])


def _check_targets_against_restatement(tr, boxes, nbox, topk):
    reg, cls = [t.cpu().numpy() for t in tr.outputs]
    dims = np.full((TB, 2), float(TD), f32)
    res = ref.tal_assign(boxes.cpu().numpy(), nbox.cpu().numpy(), dims, (TD, TD), TC, reg, cls, topk=topk, beta=BETA)
    assert _sets_decided(res, topk), "this step's head outputs leave a selection to fp32's last bits"
    tg = tr.targets.cpu().numpy()
    np.testing.assert_array_equal(tg[..., :4], res["targets"][..., :4])
    np.testing.assert_array_equal(tg[..., 5:], res["targets"][..., 5:])
    np.testing.assert_allclose(tg[..., 4], res["that"], rtol=1e-4, atol=0)
    np.testing.assert_array_equal(tr.ntgt.cpu().numpy(), res["counts"])
    return res


def test_trainer_graph_replay_equals_eager(bn_exact):
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer
    imgs, boxes, nbox = _batch()
    out = {}
    for graph in (False, True):
        net = FCOSNet(TC, seed=1)
        tr = FCOSTrainer(net, TB, (TD, TD), use_graph=graph, targets="tal", tal_topk=TOPK, tal_beta=BETA, init_lr=1e-3)
        assert tuple(tr.d_reg.shape) == (TB, tr.P, 32) and tr.norm is not None and not tr.tal_warm
        tr.load_batch(imgs, boxes, nbox)
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        out[graph] = (net.store.flat.clone(), tr.losses.clone(), tr.targets.clone())
    for x, y in zip(out[True], out[False]):
        assert torch.equal(x, y)
    losses = out[True][1]
    assert torch.isfinite(losses).all() and bool((losses[:, 0] > 0).all()) and not losses[:, 2].any()
    res = _check_targets_against_restatement(tr, boxes, nbox, TOPK)
    assert res["counts"].sum() > 0 and bool((losses[:, 1] > 0).all())
    # the head's centerness column got no gradient
    assert not tr.d_reg[..., 4:].any() and bool(tr.d_reg[..., :4].any())


def test_trainer_warmup_is_atss_then_one_recapture(bn_exact):
    """tal_warmup = 2: steps 1-2 are an FCOSTrainer whose assignment is ATSS under the same norm and loss
    (a "tal" trainer that never leaves its warm-up); step 3 assigns from the head outputs; the graphs are
    captured twice in all."""
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer
    imgs, boxes, nbox = _batch()
    nets = [FCOSNet(TC, seed=1), FCOSNet(TC, seed=1)]
    tr = FCOSTrainer(nets[0], TB, (TD, TD), targets="tal", tal_topk=TOPK, tal_beta=BETA, tal_warmup=2, atss_topk=7,
                     init_lr=1e-3)
    atss = FCOSTrainer(nets[1], TB, (TD, TD), targets="tal", tal_topk=TOPK, tal_beta=BETA, tal_warmup=10 ** 6,
                       atss_topk=7, init_lr=1e-3)
    captures = []
    real = tr.capture
    tr.capture = lambda: (captures.append(tr.tal_steps), real())[1]
    for t in (tr, atss):
        t.load_batch(imgs, boxes, nbox)
    assert tr.tal_warm and atss.tal_warm
    for step in (1, 2):
        tr.step()
        atss.step()
        torch.cuda.synchronize()
        assert tr.tal_warm and torch.equal(tr.losses, atss.losses) and torch.equal(tr.targets, atss.targets)
        assert torch.equal(nets[0].store.flat, nets[1].store.flat)
    # the warm-up targets are cvl_fcos_atss_assign's, centerness in slot 4
    from cvlite import ops_targets as ot
    dims = torch.full((TB, 2), float(TD), device="cuda")
    tg_atss, _ = ot.fcos_atss_assign(tr.boxes, tr.nbox, dims, (TD, TD), TC, topk=7)
    assert torch.equal(tr.targets, tg_atss) and int(tr.ntgt.sum()) > 0
    tr.step()
    atss.step()
    torch.cuda.synchronize()
    assert not tr.tal_warm and atss.tal_warm
    assert not torch.equal(tr.targets, atss.targets) and torch.equal(atss.targets, tg_atss)
    _check_targets_against_restatement(tr, boxes, nbox, TOPK)
    tr.step()
    torch.cuda.synchronize()
    assert captures == [1, 3] and torch.isfinite(tr.losses).all()


def test_jitter_trainer_switches_all_buckets_together():
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import JitterFCOSTrainer, synthetic_batch
    net = FCOSNet(TC, seed=0)
    jt = JitterFCOSTrainer(net, 2, use_graph=False, targets="tal", tal_topk=TOPK, tal_beta=BETA, tal_box_weight=1.5,
                           tal_warmup=1)
    a, boxes, nbox = synthetic_batch(2, 128, 128, TC, seed=3)
    b, _, _ = synthetic_batch(1, 256, 256, TC, seed=4)
    dims = np.array([[128, 128], [256, 256]], f32)
    w0 = net.store.flat.clone()
    jt.step([a[0], b[0]], boxes, nbox, dims)
    torch.cuda.synchronize()
    assert sorted(jt.buckets) == [(128, 1), (256, 1)] and jt.tal_warm
    assert all(t.target_kind == "tal" and t.tal_warm and t.tal == (TOPK, 1.0, BETA, 1.5) for t in jt.buckets.values())
    losses = jt.step([a[0], b[0]], boxes, nbox, dims)
    torch.cuda.synchronize()
    assert not jt.tal_warm and not any(t.tal_warm for t in jt.buckets.values())
    assert torch.isfinite(losses).all() and bool((losses[:, 0] > 0).all())
    assert torch.isfinite(net.store.flat).all() and not torch.equal(w0, net.store.flat)


def test_train_tal_reaches_the_evaluation_hook(monkeypatch, tmp_path, capsys):
    """train(recipe="tal") builds a "tal" trainer with its keywords, and its evaluation hook runs
    evaluate_fcos on the trained network with the box outputs clamped and the class score alone."""
    from cvlite import evaluate, train_fcos
    from cvlite.fcos_net import FCOSNet
    seen, made = [], []
    real_eval = evaluate.evaluate_fcos

    def spy_eval(*a, **kw):
        seen.append(kw)
        res = real_eval(*a, **kw)
        seen.append(res)
        return res
    monkeypatch.setattr(evaluate, "evaluate_fcos", spy_eval)
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
    train_fcos.train(samples, [], net, 2, None, None, None, 0, 2, weight_decay=0.0, eval_data=samples, eval_every=2,
                     recipe="tal", atss_topk=5, tal_topk=7, tal_alpha=0.5, tal_beta=4.0, tal_box_weight=1.5,
                     tal_warmup=1, save_loss_file=str(tmp_path / "loss.csv"))
    assert "Eval mAP:" in capsys.readouterr().out
    assert len(seen) == 2 and seen[0]["clamp_reg"] is True and seen[0]["center"] is False
    assert np.isfinite(seen[1]["mAP"])
    kw = made[0]
    assert kw["targets"] == "tal" and kw["atss_topk"] == 5 and kw["tal_topk"] == 7 and kw["tal_alpha"] == 0.5
    assert kw["tal_beta"] == 4.0 and kw["tal_box_weight"] == 1.5 and kw["tal_warmup"] == 1


def test_default_recipe_never_enters_the_tal_path(monkeypatch):
    """A default step calls no task-aligned op and counts no warm-up."""
    from cvlite import ops_targets as ot
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer

    def boom(*a, **kw):
        raise AssertionError("the default recipe entered the task-aligned path")
    for name in ("fcos_tal_assign", "fcos_tal_loss"):
        monkeypatch.setattr(ot, name, boom)
    imgs, boxes, nbox = _batch()
    tr = FCOSTrainer(FCOSNet(TC, seed=1), TB, (TD, TD), use_graph=False)
    assert tr.norm is None and not tr.tal_warm
    tr.load_batch(imgs, boxes, nbox)
    tr.step()
    torch.cuda.synchronize()
    assert torch.isfinite(tr.losses).all() and not tr.tal_warm
