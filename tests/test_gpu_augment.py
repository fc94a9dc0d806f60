"""GPU parity of the batched augmentation kernel (csrc/augment.hip, cvlite/augment.py): every image of every
batch bit for bit the staged numpy restatement tests/augment_ref.py (the same fp32 operation sequence),
the identity against the existing per-image kernel, both store paths, the padding, the torch op and the
FCOS training hook."""
import numpy as np
import pytest
import torch

import augment_ref as ar

pytestmark = pytest.mark.gpu

f32 = np.float32
FILL = (123.675, 116.28, 103.53)


def _source(h, w, u8, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return img if u8 else img.astype(f32) + rng.uniform(0, 1, img.shape).astype(f32)


@pytest.fixture(scope="module")
def sources():
    """The batch of the geometric tests: 37x53 uint8, 53x37 fp32, 64x64 uint8, 20x91 fp32 (H x W)."""
    return [_source(37, 53, True, 1), _source(53, 37, False, 2), _source(64, 64, True, 3), _source(20, 91, False, 4)]


def _check(outs, srcs, plans):
    for o, s, p in zip(outs, srcs, plans):
        np.testing.assert_array_equal(o.cpu().numpy(), ar.augment_plan(s, p))


def test_identity_equals_the_per_image_kernel():
    """Three sources, three padded sizes (64x96, 96x64, 64x64) in one launch: each output is
    preprocess_image's, bit for bit."""
    from cvlite import augment as ag
    from cvlite.data_preprocess import preprocess_image
    srcs = [_source(37, 53, True, 5), _source(64, 48, False, 6), _source(50, 50, True, 7)]
    flips = [False, True, False]
    kw = dict(min_side=64.0, max_side=1333.0, stride=32.0, equal_dims=False)
    plans = [ag.plan_geometry(s.shape[0], s.shape[1], flip=f, **kw) for s, f in zip(srcs, flips)]
    assert [(p.ph, p.pw) for p in plans] == [(64, 96), (96, 64), (64, 64)]
    outs, stacked = ag.run_plans(srcs, plans)
    assert stacked is None
    for o, s, f, p in zip(outs, srcs, flips, plans):
        ref, new_shape, _ = preprocess_image(s, None, 64.0, 1333.0, 32.0, False, flip=f)
        np.testing.assert_array_equal(new_shape, p.new_shape)
        assert torch.equal(o, ref)
    _check(outs, srcs, plans)


def _everything_plans():
    from cvlite import augment as ag
    col = [ag.colour_affine(brightness=-20.0, contrast=1.3, saturation=1.6, hue=25.0, perm=(2, 0, 1)),
           ag.colour_affine(brightness=31.0, contrast=0.6, saturation=0.5, hue=-18.0, perm=(1, 0, 2), contrast_first=False),
           ag.colour_affine(saturation=1.5, hue=170.0),
           ag.colour_affine(brightness=5.0, contrast=1.5, perm=(2, 1, 0))]
    assert all((m < 0).any() for m, _ in col[:3])
    geo = [  # source flush against the canvas' top-left corner, a crop across the source / fill seam, upscale > 2
           dict(canvas=(80, 100, 0, 0), crop=(20, 30, 40, 50), flip=True, out_hw=(90, 110), pad_hw=(96, 112)),
           # source in the canvas' interior, a 1 x N crop
           dict(canvas=(70, 60, 10, 15), crop=(30, 5, 1, 40), flip=False, out_hw=(7, 33), pad_hw=(8, 36)),
           # no zoom-out, an N x 1 crop, an odd padded row (the scalar store path)
           dict(canvas=None, crop=(3, 17, 50, 1), flip=True, out_hw=(21, 5), pad_hw=(24, 7)),
           # source flush against the canvas' bottom-right corner, downscale > 2
           dict(canvas=(50, 200, 30, 109), crop=(0, 0, 50, 200), flip=False, out_hw=(16, 64), pad_hw=(32, 64))]
    hw = [(37, 53), (53, 37), (64, 64), (20, 91)]
    return [ag.plan_geometry(h, w, m=m, t=t, fill=FILL, **g) for (h, w), (m, t), g in zip(hw, col, geo)]


def test_everything_on(sources):
    from cvlite import augment as ag
    plans = _everything_plans()
    outs, _ = ag.run_plans(sources, plans)
    _check(outs, sources, plans)
    # the seam is really inside the first crop: the reference holds both source-derived and fill-derived rows
    p = plans[0]
    flat = ar.apply_affine_f32(np.array(FILL, f32), p.m, p.t) / f32(127.5) - f32(1.0)
    ref = ar.augment_plan(sources[0], p)
    assert np.array_equal(ref[p.oh - 1, 0], flat) and not np.array_equal(ref[0, p.ow - 1], flat)


@pytest.fixture(scope="module")
def fixed_cases(sources):
    """Fixed mode, S = 45 (odd rows: the scalar store path) and S = 64 (the 16-byte path): the default
    policy's seeded plans and their references, shared by the tests below."""
    from cvlite import augment as ag
    boxes = [np.array([[0.1, 0.2, 0.6, 0.9], [0.5, 0.4, 0.95, 0.8]], f32), np.array([[0.2, 0.1, 0.9, 0.7]], f32),
             np.zeros((0, 4), f32), np.array([[0.3, 0.1, 0.8, 0.9]], f32)]
    labels = [[3, 1], [2], [], [0]]
    cases = {}
    for S in (45, 64):
        rng = np.random.default_rng(100 + S)
        plans = [ag.plan_image(s.shape[:2], b, l, ag.AugmentPolicy(), rng, size=S) for s, b, l in zip(sources, boxes, labels)]
        cases[S] = (plans, [ar.augment_plan(s, p) for s, p in zip(sources, plans)])
    return boxes, labels, cases


@pytest.mark.parametrize("S", [45, 64])
def test_fixed_mode_into_slots(sources, fixed_cases, S):
    from cvlite import augment as ag
    boxes, labels, cases = fixed_cases
    plans, refs = cases[S]
    B = len(sources)
    buf = torch.full((B + 2, S, S, 3), 7.0, device="cuda")
    dev = [torch.from_numpy(s).cuda() for s in sources]
    outs, bx, nb, dims = ag.augment_batch(dev, boxes, labels, ag.AugmentPolicy(), np.random.default_rng(100 + S), size=S,
                                          out=[buf[1 + k] for k in range(B)])
    assert (buf[1].data_ptr() % 16 == 0) == (S == 64)
    got = buf.cpu().numpy()
    assert (got[0] == 7.0).all() and (got[B + 1] == 7.0).all()             # the neighbouring slots are untouched
    for k in range(B):
        assert outs[k].data_ptr() == buf[1 + k].data_ptr()
        np.testing.assert_array_equal(got[1 + k], refs[k])
        np.testing.assert_array_equal(bx[k, :nb[k], :4], plans[k].boxes)
        assert bx[k, :nb[k], 4].tolist() == plans[k].labels.tolist() and not bx[k, nb[k]:].any()
    assert nb.tolist() == [len(p.boxes) for p in plans] and bx.shape == (B, 16, 5) and nb.dtype == np.int32
    np.testing.assert_array_equal(dims, np.full((B, 2), S, f32))
    # without `out`: the stacked tensor
    st, _, _, _ = ag.augment_batch(dev, boxes, labels, ag.AugmentPolicy(), np.random.default_rng(100 + S), size=S)
    assert tuple(st.shape) == (B, S, S, 3)
    np.testing.assert_array_equal(st.cpu().numpy(), np.stack(refs))


def test_padding_is_exactly_zero(sources):
    """oh < ph and ow < pw over a destination prefilled with NaN, through the 16-byte path, the scalar path
    of an odd row, and the scalar path of a destination that is not 16-byte aligned."""
    from cvlite import augment as ag
    m, t = ag.colour_affine(brightness=12.0, saturation=0.7)
    plans = [ag.plan_geometry(37, 53, canvas=(45, 60, 4, 6), crop=(2, 3, 40, 50), m=m, t=t, fill=FILL, out_hw=(30, 41),
                              pad_hw=(32, 64)),
             ag.plan_geometry(53, 37, flip=True, m=m, t=t, out_hw=(50, 30), pad_hw=(51, 33)),
             ag.plan_geometry(64, 64, crop=(10, 10, 40, 40), m=m, t=t, out_hw=(20, 20), pad_hw=(32, 32))]
    flat = torch.full((1 + 32 * 32 * 3,), float("nan"), device="cuda")
    outs = [torch.full((32, 64, 3), float("nan"), device="cuda"), torch.full((51, 33, 3), float("nan"), device="cuda"),
            flat[1:].view(32, 32, 3)]
    assert outs[0].data_ptr() % 16 == 0 and outs[2].data_ptr() % 16 == 4
    ag.run_plans(sources[:3], plans, out=outs)
    _check(outs, sources[:3], plans)
    for o, p in zip(outs, plans):
        g = o.cpu().numpy()
        assert not np.isnan(g).any() and not g[p.oh:].any() and not g[:, p.ow:].any() and g[:p.oh, :p.ow].any()
    assert torch.isnan(flat[0])


@pytest.mark.parametrize("S", [45, 64])
def test_torch_op_equals_fixed_mode(sources, fixed_cases, S):
    import cvlite.torch_ops  # noqa: F401
    from cvlite import augment as ag
    plans, refs = fixed_cases[2][S]
    dev = [torch.from_numpy(s).cuda() for s in sources]
    out = torch.ops.cvlite.augment_images(dev, ag.plan_table(plans), S, S)
    assert tuple(out.shape) == (len(sources), S, S, 3) and out.dtype == torch.float32
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack(refs))
    with pytest.raises(ValueError):
        torch.ops.cvlite.augment_images(dev, ag.plan_table(plans), S + 1, S)


def test_raw_batch_into_the_jitter_trainer():
    """train_fcos._raw_batch with two raw samples (decoded arrays) into JitterFCOSTrainer.step: the identity
    policy is today's path bit for bit (images, boxes, dims, per-image losses); the default policy trains."""
    from cvlite import augment as ag
    from cvlite.fcos_net import FCOSNet
    from cvlite.train_fcos import JitterFCOSTrainer, _raw_batch
    C = 20
    data = [dict(image=_source(90, 120, True, 8), objects=dict(bbox=np.array([[0.1, 0.2, 0.6, 0.9], [0.5, 0.3, 0.9, 0.8]], f32),
                                                                label=np.array([3, 7])),
                 l_jitter=100, u_jitter=128, min_side=128.0, max_side=128.0),
            dict(image=_source(120, 100, True, 9), objects=dict(bbox=np.array([[0.2, 0.1, 0.8, 0.7]], f32),
                                                                 label=np.array([11])),
                 l_jitter=100, u_jitter=128, min_side=128.0, max_side=128.0)]
    dev = torch.device("cuda", 0)
    res = []
    for policy in (None, ag.AugmentPolicy.identity()):
        rng = np.random.default_rng(5)
        imgs, bx, nb, dims = _raw_batch(data, [0, 1], rng, augment=policy)
        tr = JitterFCOSTrainer(FCOSNet(C, device=dev, seed=0), 2, use_graph=False)
        losses = tr.step(imgs, bx, nb, dims).clone()
        res.append((imgs, bx, nb, dims, losses, rng.bit_generator.state))
    a, b = res
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and len(a[0]) == len(b[0]) == 2
    for x, y in zip(a[1:4], b[1:4]):
        np.testing.assert_array_equal(x, y)
        assert x.dtype == y.dtype and x.shape == y.shape
    assert torch.equal(a[4], b[4]) and torch.isfinite(a[4]).all() and a[5] == b[5]
    # the default policy: two more steps on the second trainer; the counts are the planner's
    pol = ag.AugmentPolicy()
    rng, twin = np.random.default_rng(6), np.random.default_rng(6)
    for _ in range(2):
        imgs, bx, nb, dims = _raw_batch(data, [1, 0], rng, augment=pol)
        plans = [ag.plan_image(s["image"].shape[:2], s["objects"]["bbox"], s["objects"]["label"], pol, twin,
                               jitter=[s["l_jitter"], s["u_jitter"]], min_side=s["min_side"], max_side=s["max_side"])
                 for s in (data[1], data[0])]
        assert nb.tolist() == [len(p.boxes) for p in plans] and min(nb) >= 1
        assert [tuple(i.shape) for i in imgs] == [(p.ph, p.pw, 3) for p in plans]
        np.testing.assert_array_equal(dims, np.stack([p.new_shape for p in plans]))
        losses = tr.step(imgs, bx, nb, dims)
        assert torch.isfinite(losses).all() and float(losses.sum()) > 0
