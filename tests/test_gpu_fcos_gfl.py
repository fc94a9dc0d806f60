"""Generalized Focal Loss on the GPU (csrc/fcos_gfl.hip and everything above it) against the float64
restatement tests/fcos_gfl_ref.py.  The tolerances are the existing fused loss's (tests/
test_gpu_fcos_paper.py): rtol 2e-5 on the per-image sums, rtol 1e-4 / atol 1e-6 on every fp32 gradient
element, rtol 1e-6 on the norm's sum.  All kernel cases run B 3 on PAD (256, 192): P = 1022 cells, no
multiple of any tile.

The trainer cases run at 128 x 128, bs 2, the geometry of the ATSS trainer tests: cvl_fcos_atss_assign
takes no padded size below the largest stride (a 64 x 64 image has no cell at stride 128)."""
import functools

import numpy as np
import pytest
import torch

import fcos_gfl_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
B, P = 3, ref.P_CELLS


def _dev(*arrs):
    return [torch.tensor(np.asarray(a)).cuda() for a in arrs]           # (a copy: the cached cases are read-only)


@functools.lru_cache(maxsize=None)
def _case(C, R, ld_reg, ld_cls, with_norm, grad_scale):
    """Inputs, the fp32 norm both sides read, and the float64 losses and gradients (computed once)."""
    inp = ref.make_inputs(C, R, seed=1000 * C + R, ld_reg=ld_reg, ld_cls=ld_cls)
    norm = ref.gfl_norm(inp["cls"], inp["targets"], C).astype(f32) if with_norm else None
    want = ref.gfl_reference(inp, C, R, norm=norm, grad_scale=grad_scale)
    for a in (inp["reg"], inp["cls"], inp["targets"]) + want:
        a.setflags(write=False)
    return inp, norm, want


def _run(inp, norm, C, R, gdt=torch.float32, ld_dreg=None, ld_dcls=None, with_grad=True, fill=float("nan"), **kw):
    from cvlite import ops_targets as ot
    reg, cls, tg = _dev(inp["reg"], inp["cls"], inp["targets"])
    nm = None if norm is None else _dev(norm)[0]
    d_reg = d_cls = None
    if with_grad:        # pre-filled: every element has to be written
        d_reg = torch.full((B, P, ld_dreg or reg.shape[2]), fill, dtype=gdt, device="cuda")
        d_cls = torch.full((B, P, ld_dcls or cls.shape[2]), fill, dtype=gdt, device="cuda")
    out = ot.fcos_gfl_loss(reg, cls, tg, C, R, norm=nm, with_grad=with_grad, d_reg=d_reg, d_cls=d_cls, **kw)
    torch.cuda.synchronize()
    return out


# (C, R, ld_reg (None: exactly 4 (R + 1)), ld_cls (None: round_up(C, 8)), norm, grad_scale); C 80 / R 16 has
# rows too wide for the 256- and the 128-cell tile
LOSS_CASES = [(20, 16, None, None, True, 1.0), (20, 16, 96, 32, False, 0.37),
              (3, 7, None, None, True, 0.37), (3, 7, 96, 32, False, 1.0),
              (1, 1, None, None, True, 1.0), (1, 1, 96, 32, False, 0.37),
              (80, 16, None, None, True, 0.37), (80, 16, 96, None, False, 1.0)]


@pytest.mark.parametrize("C,R,ld_reg,ld_cls,with_norm,gs", LOSS_CASES)
def test_loss_and_gradients_against_float64(C, R, ld_reg, ld_cls, with_norm, gs):
    ld_reg = 4 * (R + 1) if ld_reg is None else ld_reg
    inp, norm, (L, g_reg, g_cls) = _case(C, R, ld_reg, ld_cls, with_norm, gs)
    losses, d_reg, d_cls = _run(inp, norm, C, R, grad_scale=gs)
    losses, d_reg, d_cls = losses.cpu().numpy(), d_reg.cpu().numpy(), d_cls.cpu().numpy()
    print("C %d R %d: losses max rel err %.2e; d_reg max abs err %.2e, d_cls %.2e"
          % (C, R, np.abs(losses / np.where(L == 0, 1, L) - (L != 0)).max(), np.abs(d_reg - g_reg).max(),
             np.abs(d_cls - g_cls).max()))
    assert (L[:2] > 0).all() and not L[2, 1:].any()
    np.testing.assert_allclose(losses, L, rtol=2e-5)
    assert d_reg.shape == g_reg.shape == (B, P, ld_reg) and d_cls.shape == g_cls.shape
    np.testing.assert_allclose(d_reg, g_reg, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(d_cls, g_cls, rtol=1e-4, atol=1e-6)
    pos = ref.positives(inp["targets"], C).numpy()
    assert not d_reg[~pos].any() and not d_reg[..., 4 * (R + 1):].any() and not d_cls[..., C:].any()
    assert np.abs(d_reg[pos]).max() > 1e-4 and np.abs(d_cls).max() > 1e-4


@pytest.mark.parametrize("kw", [dict(beta=1.5), dict(beta=0.0, box_weight=1.0, dfl_weight=1.0),
                                dict(beta=2.0, box_weight=0.5, dfl_weight=0.0)])
def test_loss_keywords_reach_the_kernel(kw):
    C, R = 3, 7
    inp, norm, _ = _case(C, R, 32, None, True, 1.0)
    rk = dict(beta=kw["beta"], w_box=kw.get("box_weight", 2.0), w_dfl=kw.get("dfl_weight", 0.25))
    L, g_reg, g_cls = ref.gfl_reference(inp, C, R, norm=norm, **rk)
    losses, d_reg, d_cls = _run(inp, norm, C, R, **kw)
    np.testing.assert_allclose(losses.cpu().numpy(), L, rtol=2e-5)
    np.testing.assert_allclose(d_reg.cpu().numpy(), g_reg, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(d_cls.cpu().numpy(), g_cls, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("C,R", [(3, 7), (20, 16)])
def test_loss_bf16_gradients_are_rounded_fp32(C, R):
    """bf16 gradient outputs in the trainer's layout (d_reg as wide as the head's padding, off a
    round_up(4 (R + 1), 8)-wide reg) equal the fp32 outputs rounded to bf16, bit for bit; padding zero."""
    NB = 4 * (R + 1)
    inp, norm, _ = _case(C, R, (NB + 7) // 8 * 8, 32, True, 1.0)
    wide = 32 if NB <= 32 else 128
    l32, r32, c32 = _run(inp, norm, C, R, ld_dreg=wide, grad_scale=0.37)
    l16, r16, c16 = _run(inp, norm, C, R, gdt=torch.bfloat16, ld_dreg=wide, grad_scale=0.37)
    assert torch.equal(l32, l16)
    assert torch.equal(r16, r32.to(torch.bfloat16)) and torch.equal(c16, c32.to(torch.bfloat16))
    assert not r16[..., NB:].any() and not c16[..., C:].any() and bool(r16[..., :NB].any())


def test_forward_only_and_two_runs():
    C, R = 20, 16
    inp, norm, _ = _case(C, R, 68, None, True, 1.0)
    a = _run(inp, norm, C, R)
    b = _run(inp, norm, C, R)
    fwd, none_r, none_c = _run(inp, norm, C, R, with_grad=False)
    assert none_r is None and none_c is None
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert torch.equal(fwd, a[0])


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,R", [(3, 7), (20, 16), (80, 16)])
def test_lds_form_bit_identical_to_row_form(dispatch, C, R, gdt):
    """The LDS-staged kernel (256- / 128- / 64-cell tiles here) against the row-pointer kernel on the
    same tiles (CVL_DISPATCH=loss_rows): one fp32 sequence per cell and one sum order."""
    inp, norm, _ = _case(C, R, 96, None, True, 1.0)
    outs = []
    for rows in ("1", "0"):
        dispatch("loss_rows=" + rows)
        outs.append(_run(inp, norm, C, R, gdt=gdt, grad_scale=0.37))
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y), float((x.double() - y.double()).abs().max())
    # gradient rows that take no 16-byte stores (68 bf16 columns) run the row form by themselves
    if gdt == torch.bfloat16 and R == 16:
        inp68, norm68, (L, g_reg, _) = _case(C, R, 68, None, True, 1.0)
        losses, d_reg, _ = _run(inp68, norm68, C, R, gdt=gdt)
        np.testing.assert_allclose(losses.cpu().numpy(), L, rtol=2e-5)
        np.testing.assert_allclose(d_reg.float().cpu().numpy(), g_reg, rtol=1e-2, atol=1e-6)


def test_non_positive_cells_never_read_their_box_rows(dispatch):
    C, R = 20, 16
    inp, norm, _ = _case(C, R, 96, None, True, 1.0)
    pos = ref.positives(inp["targets"], C).numpy()
    poisoned = dict(inp)
    poisoned["reg"] = inp["reg"].copy()
    poisoned["reg"][~pos] = np.nan
    for rows in ("0", "1"):
        dispatch("loss_rows=" + rows)
        for x, y in zip(_run(inp, norm, C, R), _run(poisoned, norm, C, R)):
            assert torch.isfinite(x).all() and torch.equal(x, y)


def test_invalid_arguments_leave_outputs_untouched():
    from cvlite import _lib
    from cvlite import ops_targets as ot
    C, R = 3, 7
    inp, norm, _ = _case(C, R, 32, None, True, 1.0)
    reg, cls, tg, nm = _dev(inp["reg"], inp["cls"], inp["targets"], norm)
    losses = torch.full((B, 3), 7.0, device="cuda")
    d_reg = torch.full((B, P, 32), 7.0, device="cuda")
    d_cls = torch.full((B, P, 8), 7.0, device="cuda")
    run = lambda r=reg, c=cls, R_=R, dr=d_reg, dc=d_cls, **kw: ot.fcos_gfl_loss(   # noqa: E731
        r, c, tg, C, R_, norm=nm, d_reg=dr, d_cls=dc, losses=losses, **kw)
    bad = [dict(R_=0), dict(R_=17), dict(R_=-1), dict(beta=-1.0), dict(beta=float("nan")),
           dict(R_=8),                                              # 36 logits in 32 columns
           dict(dr=torch.full((B, P, 28), 7.0, device="cuda")),     # gradient rows too narrow
           dict(dc=torch.full((B, P, 2), 7.0, device="cuda")),
           dict(c=cls[..., :2].contiguous())]
    for kw in bad:
        with pytest.raises(_lib.CvlError):
            run(**kw)
        for t in (kw.get("dr"), kw.get("dc")):
            assert t is None or bool((t == 7.0).all())
    lib = _lib.load()
    need = int(lib.cvl_fcos_gfl_loss_workspace_size(B, P))
    assert need == B * 16 * 3 * 8 and int(lib.cvl_fcos_gfl_loss_workspace_size(0, P)) == 0
    assert int(lib.cvl_fcos_gfl_norm_workspace_size(B, P)) == B * 4 * 2 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    args = lambda nbytes, dt=0: (_lib.ptr(reg), 32, _lib.ptr(cls), 8, _lib.ptr(tg), _lib.ptr(nm), B, P, C, R, 1.0,  # noqa: E731
                                 2.0, 2.0, 0.25, _lib.ptr(losses), _lib.ptr(d_reg), 32, dt, _lib.ptr(d_cls), 8, 0,
                                 _lib.ptr(ws), nbytes, _lib.stream())
    for a in (args(need - 8), args(need, dt=2)):                   # a short workspace, an unknown dtype
        with pytest.raises(_lib.CvlError):
            _lib.call("cvl_fcos_gfl_loss", *a)
    nrm = torch.full((B, 2), 7.0, device="cuda")
    with pytest.raises(_lib.CvlError):
        ot.fcos_gfl_norm(cls[..., :2].contiguous(), tg, C, out=nrm)
    out = torch.full((B, P, 8), 7.0, device="cuda")
    for kw in (dict(reg_max=0), dict(reg_max=17), dict(reg_max=8)):
        with pytest.raises(_lib.CvlError):
            ot.fcos_gfl_decode(reg, out=out, **kw)
    with pytest.raises(_lib.CvlError):
        ot.fcos_gfl_decode(reg, R, out=torch.full((B, P, 4), 7.0, device="cuda"))
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (losses, d_reg, d_cls, nrm, out))
    _lib.call("cvl_fcos_gfl_loss", *args(need))                    # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert not bool((losses == 7.0).any()) and not bool((d_reg == 7.0).any()) and not bool((d_cls == 7.0).any())


@pytest.mark.parametrize("C,R,ld_cls", [(20, 16, None), (3, 7, 32), (1, 1, None), (80, 16, None)])
def test_norm(C, R, ld_cls):
    from cvlite import ops_targets as ot
    inp, _, _ = _case(C, R, 4 * (R + 1), ld_cls, False, 1.0)
    cls, tg = _dev(inp["cls"], inp["targets"])
    got = ot.fcos_gfl_norm(cls, tg, C).cpu().numpy()
    again = ot.fcos_gfl_norm(cls, tg, C).cpu().numpy()
    want = ref.gfl_norm(inp["cls"], inp["targets"], C)
    assert want[2].tolist() == [0.0, 0.0] and (want[:2, 0] > 50).all()
    np.testing.assert_array_equal(got[:, 0], want[:, 0])
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=1e-6)
    np.testing.assert_array_equal(got, again)


@pytest.mark.parametrize("R,ld_reg,ld_out", [(16, 68, 8), (16, 96, 16), (7, 32, 8), (1, 8, 12)])
def test_decode_against_float64(R, ld_reg, ld_out):
    from cvlite import ops_targets as ot
    rng = np.random.default_rng(R)
    NB = 4 * (R + 1)
    reg = np.full((B, P, ld_reg), np.nan, f32)
    reg[..., :NB] = np.clip(rng.normal(0, 8, (B, P, NB)), -30, 30)
    reg[0, :40, :NB] = rng.choice([-60.0, 60.0], (40, NB))
    reg[1, :40, :NB] = 0.0                                      # uniform: d = R / 2
    out = torch.full((B, P, ld_out), float("nan"), device="cuda")
    got = ot.fcos_gfl_decode(_dev(reg)[0], R, out=out).cpu().numpy()
    want = ref.gfl_decode(reg, R).numpy()
    err = np.abs(got[..., :4] - want)
    print("decode R %d: max abs err %.2e, max rel err %.2e" % (R, err.max(), (err / np.maximum(want, 1e-30)).max()))
    np.testing.assert_allclose(got[..., :4], want, rtol=1e-5, atol=1e-6)
    assert not got[..., 4:].any() and (got[..., :4] >= 0).all() and (got[..., :4] <= R * (1 + 1e-6)).all()
    np.testing.assert_array_equal(got[1, :40, :4], np.full((40, 4), R / 2, f32))
    if ld_out == 8:
        np.testing.assert_array_equal(ot.fcos_gfl_decode(_dev(reg)[0], R).cpu().numpy(), got)


def test_decode_is_the_expectation_the_loss_uses():
    """q of the loss is the IoU of the decoded box: with the decode's distances as targets, q = 1 and the
    box term is zero up to rounding."""
    from cvlite import ops_targets as ot
    C, R = 3, 7
    inp, _, _ = _case(C, R, 32, None, False, 1.0)
    reg, cls = _dev(inp["reg"], inp["cls"])
    d = ot.fcos_gfl_decode(reg, R)
    tg = _dev(inp["targets"])[0].clone()
    tg[..., :4] = torch.where(tg[..., 5:].amax(-1, keepdim=True) >= 1, d[..., :4], tg[..., :4])
    losses, _, _ = ot.fcos_gfl_loss(reg, cls, tg, C, R, with_grad=False)
    assert float(losses[:, 1].abs().max()) < 1e-4 and float(losses[:, 2].min()) >= 0


# ---- torch ops ---------------------------------------------------------------------------------------------
def test_torch_ops_forward_and_backward():
    import cvlite.torch_ops  # noqa: F401
    C, R = 3, 7
    inp, norm, _ = _case(C, R, 32, None, True, 1.0)
    w = torch.tensor([[0.7, 1.3, 0.4], [1.1, 0.2, 2.0], [0.5, 0.6, 0.9]], dtype=torch.float64)
    r64 = torch.tensor(np.nan_to_num(inp["reg"]), dtype=torch.float64, requires_grad=True)
    c64 = torch.tensor(np.nan_to_num(inp["cls"]), dtype=torch.float64, requires_grad=True)
    L64 = ref.gfl_loss(r64, c64, inp["targets"], C, R, norm=norm)
    (L64 * w).sum().backward()
    tg = _dev(inp["targets"])[0]
    r = torch.tensor(inp["reg"], device="cuda", requires_grad=True)
    c = torch.tensor(inp["cls"], device="cuda", requires_grad=True)
    nm = torch.ops.cvlite.fcos_gfl_norm(c.detach(), tg, C)
    np.testing.assert_array_equal(nm.cpu().numpy(), norm)
    L = torch.ops.cvlite.fcos_gfl_loss(r, c, tg, nm, C, R)
    np.testing.assert_allclose(L.detach().cpu().numpy(), L64.detach().numpy(), rtol=2e-5)
    (L * w.float().cuda()).sum().backward()
    np.testing.assert_allclose(r.grad.cpu().numpy(), r64.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(c.grad.cpu().numpy(), c64.grad.numpy(), rtol=1e-4, atol=1e-6)
    d = torch.ops.cvlite.fcos_gfl_decode(r.detach(), R)
    np.testing.assert_allclose(d[..., :4].cpu().numpy(), ref.gfl_decode(inp["reg"], R).numpy(), rtol=1e-5, atol=1e-6)


# ---- network and trainer -----------------------------------------------------------------------------------
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


@pytest.mark.parametrize("R", [7, 16])
def test_trainer_eager_step_equals_ops_by_hand(bn_exact, R):
    from cvlite import ops_targets as ot
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer
    imgs, boxes, nbox = _batch()
    net = FCOSNet(TC, seed=1, reg_max=R)
    NB = 4 * (R + 1)
    assert net.reg_max == R and net.reg_ld == (NB + 7) // 8 * 8 and net.reg_heads[0].cout == NB
    kw = dict(gfl_beta=1.5, gfl_box_weight=1.0, gfl_dfl_weight=0.5, atss_topk=7)
    tr = FCOSTrainer(net, TB, (TD, TD), use_graph=False, targets="gfl", **kw)
    wide = net.reg_heads[0].cout_pad
    assert tuple(tr.d_reg.shape) == (TB, tr.P, wide) and wide % 32 == 0 and wide >= NB
    tr.load_batch(imgs, boxes, nbox)
    tr.run_fwd_bwd()
    torch.cuda.synchronize()
    assert int(tr.ntgt.sum()) > 0 and float(tr.norm[:, 0].sum()) == float(tr.ntgt.sum())

    net2 = FCOSNet(TC, seed=1, reg_max=R)
    dims = torch.full((TB, 2), float(TD), device="cuda")
    tg, nt = ot.fcos_atss_assign(tr.boxes, nbox, dims, (TD, TD), TC, topk=7)
    reg, cls = net2.forward(imgs)
    assert tuple(reg.shape) == (TB, tr.P, net.reg_ld) and not reg[..., NB:].any()
    norm = ot.fcos_gfl_norm(cls, tg, TC)
    d_reg = torch.zeros((TB, tg.shape[1], wide), dtype=net2.store.act, device="cuda")
    d_cls = torch.zeros((TB, tg.shape[1], net2.cls_ld), dtype=net2.store.act, device="cuda")
    losses, _, _ = ot.fcos_gfl_loss(reg, cls, tg, TC, R, norm=norm, d_reg=d_reg, d_cls=d_cls, beta=1.5, box_weight=1.0,
                                    dfl_weight=0.5)
    net2.backward(d_reg, d_cls)
    torch.cuda.synchronize()
    assert torch.equal(tr.targets, tg) and torch.equal(tr.ntgt, nt) and torch.equal(tr.norm, norm)
    assert torch.equal(tr.losses, losses) and bool((losses[:, 0] > 0).all()) and bool((losses.sum(0) > 0).all())
    assert torch.equal(net.store.grad, net2.store.grad) and bool(net.store.grad.any())
    assert bool(net.reg_heads[0].dw.any()) and bool(net.reg_heads[0].db.any())
    # the losses are the restatement's on these head outputs
    want = ref.gfl_loss(reg.double().cpu(), cls.double().cpu(), tg.cpu().numpy(), TC, R, norm=norm.cpu().numpy(),
                        beta=1.5, w_box=1.0, w_dfl=0.5).numpy()
    np.testing.assert_allclose(losses.cpu().numpy(), want, rtol=2e-5)


@pytest.mark.parametrize("R", [7, 16])
def test_trainer_graph_replay_equals_eager_and_loss_falls(bn_exact, R):
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer
    imgs, boxes, nbox = _batch()
    res = {}
    for graph in (False, True):
        net = FCOSNet(TC, seed=1, reg_max=R)
        tr = FCOSTrainer(net, TB, (TD, TD), use_graph=graph, targets="gfl", init_lr=1e-3)
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
    print("gfl recipe, reg_max %d: total loss step 1 %.5f, step 30 %.5f" % (R, first, last))
    assert np.isfinite(last) and last < first


def test_wrong_network_recipe_pairs_raise():
    from cvlite.fcos_net import FCOSNet
    from cvlite.fcos_center_net import FCOSCenterNet
    from cvlite.train_fcos import FCOSTrainer, JitterFCOSTrainer, train
    from cvlite import infer_fcos
    plain, gfl = FCOSNet(TC, seed=0), FCOSNet(TC, seed=0, reg_max=7)
    sample = {"image": np.zeros((128, 128, 3), f32), "bbox": np.zeros((0, 4), f32), "label": []}
    with pytest.raises(ValueError, match="reg_max"):
        FCOSTrainer(plain, 2, (128, 128), targets="gfl")
    with pytest.raises(ValueError, match="reg_max"):
        JitterFCOSTrainer(plain, 2, targets="gfl")
    with pytest.raises(ValueError, match="reg_max"):
        train([sample] * 2, [], plain, 2, None, None, None, 0, 1, recipe="gfl")
    for kind in ("fcos", "paper", "atss", "center"):
        with pytest.raises(ValueError, match="gfl"):
            FCOSTrainer(gfl, 2, (128, 128), targets=kind)
    with pytest.raises(ValueError, match="gfl"):
        JitterFCOSTrainer(gfl, 2, targets="atss")
    for recipe in ("reference", "paper", "atss"):
        with pytest.raises(ValueError, match="gfl"):
            train([sample] * 2, [], gfl, 2, None, None, None, 0, 1, recipe=recipe)
    with pytest.raises(TypeError):
        FCOSCenterNet(TC, reg_max=7)
    x = torch.zeros((1, 128, 128, 3), device="cuda")
    with pytest.raises(ValueError, match="center"):
        infer_fcos.image_detections(x, gfl, TC, center=True)


def test_checkpoint_round_trip_and_head_mismatch(tmp_path):
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import load_checkpoint, save_checkpoint
    a, b, plain = FCOSNet(TC, seed=1, reg_max=7), FCOSNet(TC, seed=2, reg_max=7), FCOSNet(TC, seed=3)
    save_checkpoint(str(tmp_path / "gfl"), a, None, 5)
    assert not torch.equal(a.store.flat, b.store.flat)
    assert load_checkpoint(str(tmp_path / "gfl.pt"), b) == 5
    assert torch.equal(a.store.flat, b.store.flat) and torch.equal(a.reg_heads[2].wf, b.reg_heads[2].wf)
    save_checkpoint(str(tmp_path / "plain"), plain, None, 1)
    with pytest.raises(ValueError, match="5 outputs.*32.*reg_max"):
        load_checkpoint(str(tmp_path / "plain.pt"), b)
    with pytest.raises(ValueError, match="reg_max"):
        load_checkpoint(str(tmp_path / "gfl.pt"), plain)
    assert torch.equal(a.store.flat, b.store.flat)


def test_jitter_trainer_gfl_two_sizes():
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import JitterFCOSTrainer, synthetic_batch
    net = FCOSNet(TC, seed=0, reg_max=7)
    jt = JitterFCOSTrainer(net, 2, use_graph=False, targets="gfl", atss_topk=7, gfl_dfl_weight=0.5)
    a, boxes, nbox = synthetic_batch(2, 128, 128, TC, seed=3)
    b, _, _ = synthetic_batch(1, 256, 256, TC, seed=4)
    dims = np.array([[128, 128], [256, 256]], f32)
    w0 = net.store.flat.clone()
    losses = jt.step([a[0], b[0]], boxes, nbox, dims)
    torch.cuda.synchronize()
    assert sorted(jt.buckets) == [(128, 1), (256, 1)]
    assert all(t.target_kind == "gfl" and t.atss_topk == 7 and t.gfl == (2.0, 2.0, 0.5) for t in jt.buckets.values())
    assert torch.isfinite(losses).all() and bool((losses.sum(0) > 0).all()) and int(jt.ntgt.sum()) > 0
    assert torch.isfinite(net.store.flat).all() and not torch.equal(w0, net.store.flat)


@pytest.mark.parametrize("R", [7, 16])
def test_image_detections_decode_the_distributions(R):
    """image_detections on a GFL network = cvl_fcos_detect (center = 0) on the float64-decoded distances."""
    from cvlite import infer_fcos
    from cvlite.fcos_net import FCOSNet
    net = FCOSNet(TC, seed=4, reg_max=R)
    g = torch.Generator(device="cpu").manual_seed(2)
    x = (torch.rand((2, 128, 192, 3), generator=g) * 2 - 1).cuda()
    det = infer_fcos.image_detections(x, net, TC, cls_thresh=0.005)
    reg, cls = net.forward(x, train=False)
    shapes, _, _ = net.layout(2, 128, 192)
    box = torch.zeros(tuple(reg.shape[:2]) + (8,), device="cuda")
    box[..., :4] = ref.gfl_decode(reg.cpu(), R).float().cuda()
    want = infer_fcos.detect_from_outputs(box, cls, shapes, TC, cls_thresh=0.005)
    torch.cuda.synchronize()
    assert int(det.valid_detections.min()) > 0
    assert torch.equal(det.valid_detections, want.valid_detections)
    assert torch.equal(det.nmsed_scores, want.nmsed_scores) and torch.equal(det.nmsed_classes, want.nmsed_classes)
    np.testing.assert_allclose(det.nmsed_boxes.cpu().numpy(), want.nmsed_boxes.cpu().numpy(), rtol=1e-5, atol=1e-5)
    folded = infer_fcos.image_detections(x, net, TC, cls_thresh=0.005, fold_bn=True)
    assert int(folded.valid_detections.min()) > 0


def test_train_gfl_reaches_the_evaluation_hook(monkeypatch, tmp_path, capsys):
    """train(recipe="gfl") builds a "gfl" trainer with its keywords, and its evaluation hook detects
    through the distribution decode."""
    from cvlite import infer_fcos, train_fcos
    from cvlite.fcos_net import FCOSNet
    seen, made = [], []
    real_detect = infer_fcos.detect_from_outputs

    def spy_detect(reg, *a, **kw):
        seen.append((tuple(reg.shape), kw.get("reg_max")))
        return real_detect(reg, *a, **kw)
    monkeypatch.setattr(infer_fcos, "detect_from_outputs", spy_detect)
    real = train_fcos.FCOSTrainer

    class Spy(real):
        def __init__(self, *a, **kw):
            made.append(kw)
            real.__init__(self, *a, **kw)
    monkeypatch.setattr(train_fcos, "FCOSTrainer", Spy)
    rng = np.random.default_rng(0)
    samples = [{"image": rng.uniform(-1, 1, (128, 128, 3)).astype(f32),
                "bbox": np.array([[0.5, 0.5, 0.4, 0.3]], f32), "label": [1]} for _ in range(2)]
    net = FCOSNet(TC, seed=0, reg_max=7)
    train_fcos.train(samples, [], net, 2, None, None, None, 0, 1, weight_decay=0.0, eval_data=samples, eval_every=1,
                     recipe="gfl", atss_topk=5, gfl_beta=1.0, gfl_box_weight=1.5, gfl_dfl_weight=0.5,
                     save_loss_file=str(tmp_path / "loss.csv"))
    assert "Eval mAP:" in capsys.readouterr().out
    assert len(seen) == 1 and seen[0] == ((2, 341, 32), 7)
    assert made[0]["targets"] == "gfl" and made[0]["atss_topk"] == 5 and made[0]["gfl_beta"] == 1.0
    assert made[0]["gfl_box_weight"] == 1.5 and made[0]["gfl_dfl_weight"] == 0.5


def test_default_network_step_never_enters_the_gfl_path(bn_exact, monkeypatch):
    """FCOSNet without reg_max keeps its 5-output head and 32-wide gradient rows, and a default step is
    the existing ops called by hand, bit for bit, with every GFL op made to fail."""
    from cvlite import ops_targets as ot
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import FCOSTrainer

    def boom(*a, **kw):
        raise AssertionError("the default recipe entered the GFL path")
    for name in ("fcos_gfl_norm", "fcos_gfl_loss", "fcos_gfl_decode"):
        monkeypatch.setattr(ot, name, boom)
    imgs, boxes, nbox = _batch()
    net = FCOSNet(TC, seed=1)
    assert net.reg_max is None and net.reg_ld == 8 and net.reg_heads[0].cout == 5 and net.reg_heads[0].cout_pad == 32
    assert tuple(net.reg_heads[0].w.shape) == (3, 3, 256, 5)
    tr = FCOSTrainer(net, TB, (TD, TD), use_graph=False)
    assert tuple(tr.d_reg.shape) == (TB, tr.P, 32) and tr.norm is None
    tr.load_batch(imgs, boxes, nbox)
    tr.run_fwd_bwd()
    net2 = FCOSNet(TC, seed=1)
    dims = torch.full((TB, 2), float(TD), device="cuda")
    tg, nt = ot.fcos_assign(tr.boxes, nbox, dims, (TD, TD), TC)
    reg, cls = net2.forward(imgs)
    d_reg = torch.zeros((TB, tg.shape[1], 32), dtype=net2.store.act, device="cuda")
    d_cls = torch.zeros((TB, tg.shape[1], net2.cls_ld), dtype=net2.store.act, device="cuda")
    losses, _, _ = ot.fcos_loss(reg, cls, tg, TC, d_reg=d_reg, d_cls=d_cls)
    net2.backward(d_reg, d_cls)
    torch.cuda.synchronize()
    assert torch.equal(tr.outputs[0], reg) and torch.equal(tr.outputs[1], cls) and tuple(reg.shape)[2] == 8
    assert torch.equal(tr.losses, losses) and torch.equal(net.store.grad, net2.store.grad)
