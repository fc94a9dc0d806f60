"""The Gaussian CenterNet recipe on the GPU (csrc/centernet_gauss.hip) against the restatement of
centernet_gauss_ref.py: the assign and the norm, the fused loss, the trainer, the peak-decode evaluation.

Bounds.  Assign: box channels, the exact zeros and the exact ones to the bit; every other heat value within
rtol 4e-6 of the float64 value -- the exponent's magnitude stays below 9 (2 r^2 * 18 / (2r+1)^2 < 9), its
three fp32 roundings (sigma, 2 sigma^2, the quotient) move it by at most 3 * 2^-24 * 9 = 1.6e-6, expf adds
an ulp or two: about 1.8e-6 in all, doubled.  Loss: rtol 2e-5 on the per-image sums and rtol 1e-4 / atol
1e-6 on every gradient element, the bounds of test_gpu_fcos_gfl.py; the kernel's gradient is bf16, so an
element passes when it is the bf16 rounding of some value inside that interval (rounding is monotonic: it
lies between the roundings of the interval's ends)."""
import numpy as np
import pytest
import torch

import centernet_gauss_ref as ref

pytestmark = pytest.mark.gpu

SEEDS = tuple(range(8))
GEOMS = [(128, 128, 4), (128, 96, 4), (120, 100, 4), (128, 128, 8)]     # maps 32x32, 32x24, 30x25, 16x16


def _dev(*arrays):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]       # a copy: the scenes are read-only


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- assign and norm ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_h,pad_w,stride", GEOMS)
@pytest.mark.parametrize("C", [1, 3, 20, 80])
@pytest.mark.parametrize("n_box", [4, 24])
def test_assign_matches_restatement(pad_h, pad_w, stride, C, n_box):
    from cvlite import ops_targets as ot
    (boxes, nbox, dims), want = ref.scene_targets(SEEDS, pad_h, pad_w, C, n_box, stride)
    b, n, d = _dev(boxes, nbox, dims)
    t = ot.centernet_gauss_assign(b, n, d, (pad_h, pad_w), C, stride=stride)
    assert tuple(t.shape) == (8, pad_h // stride, pad_w // stride, 4 + C) and t.dtype == torch.float32
    got = t.cpu().numpy()
    assert np.array_equal(_bits(got[..., :4]), _bits(want[..., :4]))
    gh, wh = got[..., 4:].astype(np.float64), want[..., 4:]
    assert np.array_equal(gh == 0.0, wh == 0.0) and np.array_equal(gh == 1.0, wh == 1.0)
    mid = (wh != 0.0) & (wh != 1.0)
    err = float(np.max(np.abs(gh[mid] - wh[mid]) / wh[mid])) if mid.any() else 0.0
    print("heat max rel err %.3e over %d values (%dx%d s%d C%d n%d)" % (err, int(mid.sum()), pad_h, pad_w, stride,
                                                                       C, n_box))
    assert err <= 4e-6
    npos = ot.centernet_gauss_norm(t, C)
    assert npos.dtype == torch.int32 and np.array_equal(npos.cpu().numpy(), ref.npos_ref(want, C))
    assert int(npos[-1]) == 0 and int(npos[:-1].min()) >= 1
    # run to run
    t2 = ot.centernet_gauss_assign(b, n, d, (pad_h, pad_w), C, stride=stride)
    assert torch.equal(t.view(torch.int32), t2.view(torch.int32))
    assert torch.equal(npos, ot.centernet_gauss_norm(t2, C))


@pytest.mark.parametrize("pad,stride", [(128, 4), (128, 8)])
@pytest.mark.parametrize("C,n_box", [(3, 24), (20, 4)])
def test_assign_square_pad_equals_reference_assign(pad, stride, C, n_box):
    """Square pad, square images, labels in range: the box channels and the positions of the exact ones are
    cvl_centernet_assign's, bit for bit."""
    from cvlite import ops_targets as ot
    boxes, nbox, dims = ref.scene_batch(SEEDS, pad, pad, C, n_box, stride)
    boxes = boxes.copy()
    lab = boxes[..., 4]
    lab[(lab < 0) | (lab >= C)] = 0.0
    assert np.array_equal(dims[:, 0], dims[:, 1])
    b, n, d = _dev(boxes, nbox, dims)
    new = ot.centernet_gauss_assign(b, n, d, (pad, pad), C, stride=stride)
    old = ot.centernet_assign(b, n, d, (pad, pad), C, stride=stride)
    assert torch.equal(new[..., :4].contiguous().view(torch.int32), old[..., :4].contiguous().view(torch.int32))
    assert torch.equal(new[..., 4:] == 1.0, old[..., 4:] == 1.0) and int((old[..., 4:] == 1.0).sum()) > 8
    assert torch.equal(ot.centernet_gauss_norm(new, C), ot.centernet_gauss_norm(old, C))


def test_norm_on_any_map_and_odd_sizes():
    """The count on maps that are not the assign's: odd P * (4 + C) (no 16-byte loads), ones in the box
    channels (not counted), values next to 1."""
    from cvlite import ops_targets as ot
    g = torch.Generator().manual_seed(5)
    for B, P, C in ((3, 750, 3), (2, 1023, 1), (2, 333, 20), (1, 1024, 80)):
        t = torch.rand((B, P, 4 + C), generator=g)
        t[torch.rand((B, P, 4 + C), generator=g) < 0.03] = 1.0
        t[..., :4][torch.rand((B, P, 4), generator=g) < 0.2] = 1.0
        t[0, 0, 4] = float(np.nextafter(np.float32(1), np.float32(0)))
        t[0, 1, 4] = float(np.nextafter(np.float32(1), np.float32(2)))
        t[-1] = t[-1].clamp(max=0.5)
        want = (t[..., 4:] == 1.0).sum((1, 2)).to(torch.int32)
        got = ot.centernet_gauss_norm(t.cuda(), C)
        assert torch.equal(got.cpu(), want) and int(want[-1]) == 0


def test_invalid_arguments_return_the_error_code():
    from cvlite import _lib
    from cvlite import ops_targets as ot
    dims = torch.full((1, 2), 64.0, device="cuda")
    nbox = torch.ones((1,), dtype=torch.int32, device="cuda")
    boxes = torch.zeros((1, 4, 5), device="cuda")
    out = torch.full((1, 16, 16, 7), 7.0, device="cuda")
    bad = [dict(boxes=torch.zeros((1, 257, 5), device="cuda")), dict(C=257), dict(min_overlap=0.0),
           dict(min_overlap=1.0)]
    for kw in bad:
        with pytest.raises(_lib.CvlError, match="invalid argument"):
            ot.centernet_gauss_assign(kw.get("boxes", boxes), nbox, dims, kw.get("pad", (64, 64)), kw.get("C", 3),
                                      stride=kw.get("stride", 4), min_overlap=kw.get("min_overlap", 0.7),
                                      out=out if "C" not in kw else torch.zeros((1, 16, 16, 261), device="cuda"))
    assert bool((out == 7.0).all())                                  # nothing was written
    lib = _lib.load()
    t = torch.zeros((1, 256, 7), device="cuda")
    npos = torch.zeros((1,), dtype=torch.int32, device="cuda")
    st = _lib.stream()
    for pad_h, stride in ((64, 0), (64, -4), (64, 128), (2, 4)):        # no stride, or a map without a row
        assert lib.cvl_centernet_gauss_assign(_lib.ptr(boxes), _lib.ptr(nbox), _lib.ptr(dims), 1, 4, pad_h, 64, 3,
                                              stride, 0.7, _lib.ptr(out), st) != 0
    assert bool((out == 7.0).all())
    assert lib.cvl_centernet_gauss_norm(_lib.ptr(t), 1, 0, 3, _lib.ptr(npos), st) != 0
    assert lib.cvl_centernet_gauss_norm(_lib.ptr(t), 1, 256, 3, None, st) != 0
    pred = torch.zeros((1, 256, 8), device="cuda")
    d = torch.zeros((1, 256, 8), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.CvlError, match="invalid argument"):
        ot.centernet_gauss_loss(pred, torch.zeros((1, 256, 4 + 5), device="cuda"), npos, 5, d_pred=d)   # ld < 4 + C
    with pytest.raises(_lib.CvlError, match="invalid argument"):
        ot.centernet_gauss_loss(pred, t, npos, 3, alpha=-1.0, d_pred=d)
    with pytest.raises(_lib.CvlError, match="invalid argument"):
        ot.centernet_gauss_loss(pred, t, npos, 3, beta=-0.5, d_pred=d)


# ---- loss ----------------------------------------------------------------------------------------------
LOSS_SEEDS = (0, 1, 2)
LOSS_CASES = [(1, 32, 32), (3, 96, 32), (20, 32, 32), (80, 96, 96)]      # C, ld_pred, ld_d


def _loss_inputs(pad_h, pad_w, C, ld_pred):
    """targets of a 3-image scene (the last image all negative) as fp32, predictions with logits up to +-30
    and box errors on both sides of zero, exact equality included."""
    _, t64 = ref.scene_targets(LOSS_SEEDS, pad_h, pad_w, C, 24, 4)
    t = torch.from_numpy(t64.astype(np.float32)).view(3, -1, 4 + C)
    assert np.array_equal((t64[..., 4:] == 1.0), (t.view(t64.shape)[..., 4:] == 1.0).numpy())
    B, P = 3, t.shape[1]
    g = torch.Generator().manual_seed(1000 + C + pad_w)
    pred = torch.randn((B, P, ld_pred), generator=g)
    x = torch.randn((B, P, C), generator=g) * 3.0
    wide = torch.rand((B, P, C), generator=g) < 0.1
    x = torch.where(wide, torch.rand((B, P, C), generator=g) * 60.0 - 30.0, x)
    x[0, 0, 0], x[0, 1, 0] = 30.0, -30.0
    steps = torch.tensor([-1.5, -0.25, 0.0, 0.0, 0.25, 0.75])
    e = steps[torch.randint(0, len(steps), (B, P, 4), generator=g)]
    pred[..., :4] = t[..., :4] + e
    pred[..., 4:4 + C] = x
    return pred.contiguous(), t.contiguous()


def _bf16_interval_ok(got_bf16, want64, rtol=1e-4, atol=1e-6):
    """got is the bf16 rounding of a value within atol + rtol |want| of want."""
    w = torch.as_tensor(want64, dtype=torch.float64)
    tol = atol + rtol * w.abs()
    lo = (w - tol).to(torch.float32).to(torch.bfloat16).double()
    hi = (w + tol).to(torch.float32).to(torch.bfloat16).double()
    g = got_bf16.double().cpu()
    return (g >= lo) & (g <= hi)


@pytest.mark.parametrize("pad_h,pad_w", [(128, 128), (120, 100)])         # P = 1024 and 750
@pytest.mark.parametrize("C,ld_pred,ld_d", LOSS_CASES)
def test_loss_matches_float64(pad_h, pad_w, C, ld_pred, ld_d):
    from cvlite import ops_targets as ot
    pred, t = _loss_inputs(pad_h, pad_w, C, ld_pred)
    B, P = 3, t.shape[1]
    assert P == (pad_h // 4) * (pad_w // 4)
    pd, td = pred.cuda(), t.cuda()
    npos = ot.centernet_gauss_norm(td, C)
    want_n = ref.npos_ref(t.numpy(), C)
    assert np.array_equal(npos.cpu().numpy(), want_n) and want_n[-1] == 0 and want_n[:2].min() >= 1
    cs, rs = 2.5, 0.75
    d = torch.full((B, P, ld_d), 3.0, dtype=torch.bfloat16, device="cuda")
    losses, _ = ot.centernet_gauss_loss(pd, td, npos, C, cls_scale=cs, reg_scale=rs, d_pred=d)
    L, G = ref.loss_and_grad64(pred, t, want_n, C, cls_scale=cs, reg_scale=rs)
    got = losses.cpu().numpy()
    print("losses", got.tolist(), "rel err", (np.abs(got - L) / np.maximum(np.abs(L), 1e-300)).max())
    np.testing.assert_allclose(got, L, rtol=2e-5)
    assert got[2, 1] == 0.0 and got[2, 0] > 0.0                    # the all-negative image: class term only
    ok = _bf16_interval_ok(d[..., :4 + C], G[..., :4 + C])
    assert bool(ok.all()), "%d gradient elements outside rtol 1e-4 / atol 1e-6" % int((~ok).sum())
    assert not d[..., 4 + C:].any()                                 # padding channels
    # the L1 gradient: +-reg_scale / N by selection, exactly zero at equality and off the centres
    cell = (t[..., 4:] == 1.0).any(-1)
    dbox = d[..., :4].float().cpu()
    assert not dbox[~cell].any() and bool((dbox[cell][pred[..., :4][cell] == t[..., :4][cell]] == 0).all())
    assert int((dbox != 0).sum()) > 0
    # run to run, and the 16-byte form against the element form is covered by test_loss_element_form
    d2 = torch.empty_like(d)
    l2, _ = ot.centernet_gauss_loss(pd, td, npos, C, cls_scale=cs, reg_scale=rs, d_pred=d2)
    assert torch.equal(l2.view(torch.int32), losses.view(torch.int32)) and torch.equal(d2.view(torch.int16),
                                                                                     d.view(torch.int16))
    # NaN box predictions off the centres change nothing
    poisoned = pd.clone()
    poisoned[..., :4][~cell.cuda()] = float("nan")
    d3 = torch.empty_like(d)
    l3, _ = ot.centernet_gauss_loss(poisoned, td, npos, C, cls_scale=cs, reg_scale=rs, d_pred=d3)
    assert torch.equal(l3.view(torch.int32), losses.view(torch.int32)) and torch.equal(d3.view(torch.int16),
                                                                                     d.view(torch.int16))


@pytest.mark.parametrize("C,ld_pred,ld_d", [(3, 7, 7), (20, 25, 28), (2, 8, 12)])
def test_loss_element_form(C, ld_pred, ld_d):
    """Rows that take no 16-byte accesses (odd pitches) run the element form: same bounds; and with pitches
    that allow both, the forced element form equals the 16-byte form bit for bit in the gradient."""
    from cvlite import ops_targets as ot
    pred, t = _loss_inputs(120, 100, C, ld_pred)
    pd, td = pred.cuda(), t.cuda()
    npos = ot.centernet_gauss_norm(td, C)
    d = torch.full((3, 750, ld_d), 3.0, dtype=torch.bfloat16, device="cuda")
    losses, _ = ot.centernet_gauss_loss(pd, td, npos, C, d_pred=d)
    L, G = ref.loss_and_grad64(pred, t, npos.cpu().numpy(), C)
    np.testing.assert_allclose(losses.cpu().numpy(), L, rtol=2e-5)
    assert bool(_bf16_interval_ok(d[..., :4 + C], G[..., :4 + C]).all()) and not d[..., 4 + C:].any()


def test_loss_forced_element_form_equals_vector_form(dispatch):
    from cvlite import ops_targets as ot
    C = 20
    pred, t = _loss_inputs(120, 100, C, 32)
    pd, td = pred.cuda(), t.cuda()
    npos = ot.centernet_gauss_norm(td, C)
    lv, dv = ot.centernet_gauss_loss(pd, td, npos, C, alpha=1.5, beta=3.0)
    dispatch("loss_rows")
    le, de = ot.centernet_gauss_loss(pd, td, npos, C, alpha=1.5, beta=3.0)
    assert torch.equal(dv.view(torch.int16), de.view(torch.int16))
    np.testing.assert_allclose(lv.cpu().numpy(), le.cpu().numpy(), rtol=1e-6)
    # other exponents go through powf: the same float64 bounds
    L, G = ref.loss_and_grad64(pred, t, npos.cpu().numpy(), C, alpha=1.5, beta=3.0)
    np.testing.assert_allclose(lv.cpu().numpy(), L, rtol=2e-5)
    assert bool(_bf16_interval_ok(dv[..., :4 + C], G[..., :4 + C]).all())


def test_torch_op_autograd_equals_direct_call():
    import cvlite.torch_ops  # noqa: F401
    from cvlite import ops_targets as ot
    C = 3
    (boxes, nbox, dims), _ = ref.scene_targets(LOSS_SEEDS, 128, 128, C, 24, 4)
    b, n, dm = _dev(boxes, nbox, dims)
    t, npos = torch.ops.cvlite.centernet_gauss_assign(b, n, dm, 128, 128, C, 4, 0.7)
    assert torch.equal(t, ot.centernet_gauss_assign(b, n, dm, (128, 128), C, stride=4))
    assert torch.equal(npos, ot.centernet_gauss_norm(t, C))
    pred, _ = _loss_inputs(128, 128, C, 32)
    p = pred.view(3, 32, 32, 32).cuda().requires_grad_(True)
    L = torch.ops.cvlite.centernet_gauss_loss(p, t, npos, C, 2.0, 4.0)
    d = torch.empty((3, 1024, 32), dtype=torch.bfloat16, device="cuda")
    direct, _ = ot.centernet_gauss_loss(p.detach().view(3, 1024, 32), t.view(3, 1024, 4 + C), npos, C, d_pred=d)
    assert torch.equal(L, direct)
    L.sum().backward()
    assert p.grad.shape == p.shape and torch.equal(p.grad.view(3, 1024, 32), d.float())
    # per-term, per-image upstream gradients scale the two channel groups
    p.grad = None
    w = torch.tensor([[2.0, 0.5], [1.0, 0.0], [0.0, 4.0]], device="cuda")
    (torch.ops.cvlite.centernet_gauss_loss(p, t, npos, C) * w).sum().backward()
    want = d.float().clone()
    want[..., :4] *= w[:, 1].view(3, 1, 1)
    want[..., 4:] *= w[:, 0].view(3, 1, 1)
    assert torch.equal(p.grad.view(3, 1024, 32), want)


# ---- trainer -------------------------------------------------------------------------------------------
TC, TB, TD = 20, 2, 128


@pytest.fixture
def bn_exact():
    """BatchNorm statistics in integer bins: identical by construction from run to run."""
    from cvlite import ops_nn as nn
    nn.set_bn_exact(True)
    yield
    nn.set_bn_exact(False)


def _net(seed=3):
    from cvlite.hourglass_net import HourglassNet
    return HourglassNet(TC, seed=seed)


def _batch():
    from cvlite.train_centernet import synthetic_batch
    return synthetic_batch(TB, TD, TD, TC, n_max=8, seed=21)


def test_trainer_graph_replay_equals_eager(bn_exact):
    from cvlite.train_centernet import CenterNetTrainer
    imgs, boxes, nbox = _batch()
    res = {}
    for graph in (False, True):
        net = _net()
        tr = CenterNetTrainer(net, TB, (TD, TD), sub_batch_sz=2, n_max=8, use_graph=graph, targets="gaussian")
        steps = []
        for _ in range(3):
            tr.load_batch(imgs, boxes, nbox)
            steps.append(tr.step().clone())
        torch.cuda.synchronize()
        res[graph] = (torch.stack(steps), net.store.flat.clone(), tr.npos.clone(), tr.targets.clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    losses, _, npos, tg = res[True]
    assert torch.isfinite(losses).all() and bool((losses > 0).all())
    assert bool((npos.cpu() >= 1).all()) and bool((npos.cpu() <= nbox.cpu()).all())   # at most one centre per box
    want = ref.assign_gather(boxes.cpu().numpy(), nbox.cpu().numpy(), np.full((TB, 2), float(TD), np.float32),
                             (TD, TD), TC, 4)
    assert np.array_equal(_bits(tg.cpu().numpy()[..., :4]), _bits(want[..., :4]))
    assert np.array_equal(tg.cpu().numpy()[..., 4:] == 1.0, want[..., 4:] == 1.0)


def test_trainer_class_loss_falls():
    from cvlite.train_centernet import CenterNetTrainer
    imgs, boxes, nbox = _batch()
    tr = CenterNetTrainer(_net(), TB, (TD, TD), sub_batch_sz=2, n_max=8, targets="gaussian")
    hist = []
    for _ in range(8):
        tr.load_batch(imgs, boxes, nbox)
        hist.append(tr.step().double().sum(0).cpu().numpy().copy())
    hist = np.array(hist)
    print("gaussian recipe, (cls, reg) summed over the batch, steps 1..8:", hist.tolist())
    assert np.isfinite(hist).all() and hist[-1, 0] < hist[0, 0]


def test_trainer_load_targets_equals_load_batch(bn_exact):
    from cvlite import centernet_hourglass as ch
    from cvlite.train_centernet import CenterNetTrainer
    imgs, boxes, nbox = _batch()
    a = CenterNetTrainer(_net(), TB, (TD, TD), sub_batch_sz=2, n_max=8, targets="gaussian")
    a.load_batch(imgs, boxes, nbox)
    la = a.step().clone()
    maps = []
    for b in range(TB):
        m, n = ch.format_data_gaussian(boxes[b, :int(nbox[b])].cpu().numpy(), [TD, TD], TC, img_pad=[TD, TD], stride=4)
        assert n == int(nbox[b]) and m.shape == (TD // 4, TD // 4, 4 + TC)
        maps.append(m)
    maps = torch.from_numpy(np.stack(maps)).cuda()
    assert torch.equal(maps, a.targets)
    c = CenterNetTrainer(_net(), TB, (TD, TD), sub_batch_sz=2, n_max=8, targets="gaussian")
    c.load_targets(imgs, maps)
    lc = c.step().clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lc) and torch.equal(a.npos, c.npos)
    # the drop-in train_step with recipe="gaussian" runs the same step (its own trainer, cached by recipe)
    net = _net()
    cls, reg = ch.train_step(net, 2, imgs, maps, None, recipe="gaussian")
    assert cls == pytest.approx(float(la[:, 0].double().sum()) / TB, rel=1e-6)
    assert reg == pytest.approx(float(la[:, 1].double().sum()) / TB, rel=1e-6)
    assert [k[-1] for k in net._trainers] == ["gaussian"]


def test_default_recipe_step_is_the_reference_ops_by_hand(bn_exact, monkeypatch):
    """The default trainer never enters the new path, and its first step's losses are the existing ops called
    by hand, bit for bit."""
    from cvlite import ops_targets as ot
    from cvlite.train_centernet import CenterNetTrainer

    def boom(*a, **kw):
        raise AssertionError("the default recipe entered the gaussian path")
    for name in ("centernet_gauss_assign", "centernet_gauss_norm", "centernet_gauss_loss"):
        monkeypatch.setattr(ot, name, boom)
    imgs, boxes, nbox = _batch()
    net = _net()
    tr = CenterNetTrainer(net, TB, (TD, TD), sub_batch_sz=2, n_max=8, use_graph=False)
    assert tr.recipe == "reference" and not hasattr(tr, "npos")
    tr.load_batch(imgs, boxes, nbox)
    got = tr.step().clone()
    net2 = _net()
    dims = torch.full((TB, 2), float(TD), device="cuda")
    tg = ot.centernet_assign(tr.boxes, nbox, dims, (TD, TD), TC, stride=4)
    out = net2.forward(imgs, group=2)
    want, _ = ot.centernet_loss(out.view(TB, -1, out.shape[-1]), tg.view(TB, -1, 4 + TC), TC, 2.5, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(tg, tr.targets) and torch.equal(got, want)


# ---- evaluation ----------------------------------------------------------------------------------------
class _MapModel(object):
    """Stands in for a trained network: returns hand-made prediction maps, batch by batch."""

    def __init__(self, maps, batch):
        self.maps, self.batch, self.calls = maps, batch, 0

    def __call__(self, x, training=False):
        i0 = self.calls * self.batch
        self.calls += 1
        out = torch.full((self.batch,) + tuple(self.maps.shape[1:]), -12.0, device="cuda")
        out[..., :4] = 0.0
        n = max(0, min(self.batch, self.maps.shape[0] - i0))
        out[:n] = self.maps[i0:i0 + n]
        return out


def _eval_samples(rng, n, S, C):
    out = []
    for _ in range(n):
        k = int(rng.integers(1, 4))
        hw = rng.uniform(0.2, 0.6, (k, 2))
        c = rng.uniform(hw / 2, 1 - hw / 2)
        out.append(dict(image=np.zeros((S, S, 3), np.float32), bbox=np.concatenate([c, hw], 1).astype(np.float32),
                        label=rng.integers(0, C, k), difficult=np.zeros(k, np.uint8)))
    return out


def test_evaluate_centernet_peak_and_nms_paths():
    from cvlite import centernet_hourglass as ch
    from cvlite import ops_targets as ot
    from cvlite.evaluate import MAX_T, Evaluator, evaluate_centernet, gt_from_labels
    C, S, K = 3, 128, 50
    samples = _eval_samples(np.random.default_rng(9), 3, S, C)
    # prediction maps from the Gaussian targets themselves: logit of 0.9 * heat (floor 1e-5), the box
    # channels of the centres, and one spurious low peak per image
    maps, gts = [], []
    for s in samples:
        n = len(s["label"])
        bx = np.concatenate([s["bbox"], np.asarray(s["label"], np.float32)[:, None]], 1)
        m, _ = ch.format_data_gaussian(bx, [S, S], C, img_pad=[S, S], stride=4)
        p = np.clip(0.9 * m[..., 4:].astype(np.float64), 1e-5, None)
        m = m.copy()
        m[..., 4:] = np.log(p / (1 - p))
        m[1, 1, 4] = 0.0                                                        # p = 0.5, a false positive
        m[1, 1, :4] = 1.5
        maps.append(m)
        gtb, gtl, _ = gt_from_labels(bx[None], [n], (S, S))
        gts.append(np.concatenate([gtb[0].numpy()[:n], gtl[0].numpy()[:n, None].astype(np.float32),
                                   np.zeros((n, 1), np.float32)], 1))
    maps = torch.from_numpy(np.stack(maps).astype(np.float32)).cuda()
    for protocol in ("voc12", "coco"):
        got = evaluate_centernet(_MapModel(maps, 2), samples, C, batch_size=2, protocol=protocol, decode="peak", K=K,
                                 thresh=0.3)
        dets = ch.peak_detections(maps, thresh=0.3, K=K, downsample=4, num_classes=C)
        assert min(len(d) for d in dets) >= 2
        ev = Evaluator(C, protocol)
        ev.add_rows([d[:MAX_T] for d in dets], gts, fmt="yxyx")
        hand = ev.result()
        assert got["ap"].tobytes() == hand["ap"].tobytes()
        np.testing.assert_equal(got["mAP"], hand["mAP"])
        np.testing.assert_array_equal(got["npos"], hand["npos"])
        assert float(got["mAP"]) > 0.5, "the decoded centres must match their boxes"
        # the default path: decode_detections per image (threshold + NMS), as before
        old = evaluate_centernet(_MapModel(maps, 2), samples, C, batch_size=2, protocol=protocol, thresh=0.3)
        ev = Evaluator(C, protocol)
        rows = [ch.decode_detections(maps[b], thresh=0.3, downsample=4, img_rows=S, img_cols=S)[1][:MAX_T]
                for b in range(3)]
        ev.add_rows(rows, gts, fmt="xyxy")
        hand = ev.result()
        assert old["ap"].tobytes() == hand["ap"].tobytes()
        np.testing.assert_equal(old["mAP"], hand["mAP"])
