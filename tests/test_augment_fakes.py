"""The library export and loader entries of cvl_augment_batch, the fake (shape-only) implementation of
torch.ops.cvlite.augment_images, and the argument checks and defaults of the augmentation hook that need
no device (CPU)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch


def test_library_export_and_signature():
    from cvlite import _lib
    from cvlite import augment as ag
    lib = _lib.load()
    assert hasattr(lib, "cvl_augment_batch")
    assert "cvl_augment_batch" in _lib.SIGNATURES and "cvl_augment_batch" in _lib.NEWER
    assert len(_lib.SIGNATURES["cvl_augment_batch"][1]) == 4
    assert ag.DESC.itemsize == 144 and ag.DESC.fields["m"][1] == 80 and ag.DESC.fields["fill"][1] == 128


def test_entry_checks_its_arguments_before_any_launch():
    """CVL_EINVAL (status 1) comes from the host-side checks, ahead of the launch: no device is touched."""
    from cvlite import _lib
    from cvlite import augment as ag
    lib = _lib.load()
    good = ag.plan_table([ag.plan_geometry(37, 53, canvas=(60, 80, 3, 5), crop=(1, 2, 40, 50), out_hw=(20, 30),
                                           pad_hw=(32, 32))]).numpy().view(ag.DESC).reshape(1)
    good["src"], good["dst"] = 4096, 8192            # never dereferenced: every case below is refused

    def status(B=1, **kw):
        t = good.copy()
        for k, v in kw.items():
            t[k] = v
        return lib.cvl_augment_batch(ctypes.c_void_p(t.ctypes.data), ctypes.c_void_p(4096), B, None)

    assert status(B=0) == 1 and status(B=4097) == 1
    assert status(src=0) == 1 and status(dst=0) == 1
    assert status(oy=24) == 1 and status(ox=28) == 1 and status(oy=-1) == 1          # the source leaves the canvas
    assert status(y0=21) == 1 and status(x0=31) == 1 and status(x0=-1) == 1          # the crop leaves the canvas
    assert status(hh=0) == 1 and status(ww=0) == 1
    assert status(oh=33) == 1 and status(ow=33) == 1 and status(oh=0) == 1           # oh <= ph, ow <= pw
    assert status(flip=2) == 1 and status(src_u8=2) == 1
    assert status(ph=65536, pw=65536) == 1
    assert lib.cvl_augment_batch(None, ctypes.c_void_p(4096), 1, None) == 1
    assert lib.cvl_augment_batch(ctypes.c_void_p(good.ctypes.data), None, 1, None) == 1


def test_augment_images_fake_gives_the_shape():
    import cvlite.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        images = [torch.empty((37, 53, 3), dtype=torch.uint8, device="cuda"),
                  torch.empty((64, 48, 3), dtype=torch.float32, device="cuda"),
                  torch.empty((50, 50, 3), dtype=torch.uint8, device="cuda")]
        table = torch.empty((3, 144), dtype=torch.uint8)
        for ph, pw in ((45, 45), (64, 64), (128, 96)):
            out = torch.ops.cvlite.augment_images(images, table, ph, pw)
            assert tuple(out.shape) == (3, ph, pw, 3) and out.dtype == torch.float32 and out.device.type == "cuda"


def test_plan_table_layout():
    from cvlite import augment as ag
    m = np.arange(9, dtype=np.float32).reshape(3, 3)
    p = ag.plan_geometry(37, 53, canvas=(60, 80, 3, 5), crop=(1, 2, 40, 50), flip=True, m=m, t=[1, 2, 3],
                         fill=[4, 5, 6], out_hw=(20, 30), pad_hw=(32, 48))
    t = ag.plan_table([p, p])
    assert tuple(t.shape) == (2, 144) and t.dtype == torch.uint8
    d = t.numpy().view(ag.DESC).reshape(2)[1]
    assert [int(d[k]) for k in ("src", "dst", "src_u8", "H", "W", "ch", "cw", "oy", "ox", "y0", "x0", "hh", "ww", "flip",
                                "oh", "ow", "ph", "pw", "reserved")] == \
        [0, 0, 0, 37, 53, 60, 80, 3, 5, 1, 2, 40, 50, 1, 20, 30, 32, 48, 0]
    assert d["m"].tolist() == list(range(9)) and d["t"].tolist() == [1, 2, 3] and d["fill"].tolist() == [4, 5, 6]


def test_no_cpu_fallback():
    from cvlite import _lib
    from cvlite import augment as ag
    if not torch.cuda.is_available():           # a missing device is an error, never a host computation
        with pytest.raises(_lib.CvlError):
            ag.run_plans([np.zeros((8, 8, 3), np.uint8)], [ag.plan_geometry(8, 8, size=8)])
    with pytest.raises(ValueError):
        ag.run_plans([], [])
    with pytest.raises(ValueError):
        ag.augment_batch([np.zeros((8, 8, 3), np.uint8)], [np.zeros((0, 4))], [[]], None, np.random.default_rng(0))


def test_hook_keywords_default_to_none():
    from cvlite import train_fcos
    assert inspect.signature(train_fcos.train).parameters["augment"].default is None
    p = inspect.signature(train_fcos._raw_batch).parameters
    assert p["augment"].default is None and list(p) == ["train_data", "idx", "rng", "jpeg_decode", "augment"]


class _Net(object):
    C = 3
    device = "cpu"


def test_train_rejects_augment_for_preprocessed_samples():
    from cvlite import train_fcos
    from cvlite.augment import AugmentPolicy
    pre = [dict(image=np.zeros((128, 128, 3), np.float32), bbox=np.zeros((1, 4), np.float32), label=np.zeros(1))] * 4
    with pytest.raises(ValueError, match="raw samples"):
        train_fcos.train(pre, [], _Net(), 2, None, "", None, 0, 1, augment=AugmentPolicy())
    raw = [dict(image=np.zeros((37, 53, 3), np.uint8), objects=dict(bbox=np.zeros((1, 4), np.float32), label=[0]),
                l_jitter=60, u_jitter=70, min_side=64.0, max_side=128.0)] * 4
    with pytest.raises(ValueError, match="AugmentPolicy"):
        train_fcos.train(raw, [], _Net(), 2, None, "", None, 0, 1, augment="default")


def test_bad_policies_raise():
    from cvlite.augment import AugmentPolicy
    for kw in (dict(contrast=(1.5, 0.5)), dict(saturation=(2.0, 1.0)), dict(expand=(4.0, 1.0)), dict(expand=(0.5, 2.0)),
               dict(min_crop=0.0), dict(min_crop=1.5), dict(min_crop=-0.3), dict(flip=1.5), dict(photo_prob=-0.1),
               dict(expand_prob=2.0), dict(brightness=-1.0), dict(hue=-3.0), dict(min_ious=(0.5, 1.0)),
               dict(min_ious=(0.0,)), dict(fill=(1.0, 2.0)), dict(contrast=(-0.5, 1.0))):
        with pytest.raises(ValueError):
            AugmentPolicy(**kw)
    p = AugmentPolicy()
    assert (p.flip, p.brightness, p.contrast, p.saturation, p.hue, p.swap_channels, p.photo_prob) == \
        (0.5, 32.0, (0.5, 1.5), (0.5, 1.5), 18.0, True, 0.5)
    assert (p.expand, p.expand_prob, p.fill, p.min_ious, p.min_crop) == \
        ((1.0, 4.0), 0.5, (123.675, 116.28, 103.53), (0.1, 0.3, 0.5, 0.7, 0.9), 0.3)
    i = AugmentPolicy.identity()
    assert i.flip == 0.5 and i.brightness == 0.0 and i.contrast is None and i.saturation is None and i.hue == 0.0
    assert not i.swap_channels and i.expand is None and i.min_ious is None
    AugmentPolicy(min_crop=1.0)
