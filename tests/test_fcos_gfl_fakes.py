"""The fake (shape-only) implementations of the Generalized Focal Loss torch ops, and the argument
checks of FCOSNet, FCOSTrainer, JitterFCOSTrainer and train that need no device (CPU)."""
import numpy as np
import pytest
import torch


def test_gfl_op_fakes_give_the_shapes():
    import cvlite.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        tg = torch.empty((2, 1022, 8), device="cuda")
        cls = torch.empty((2, 1022, 32), device="cuda")
        for R, ld in ((7, 32), (16, 72), (16, 96)):
            reg = torch.empty((2, 1022, ld), device="cuda")
            norm = torch.ops.cvlite.fcos_gfl_norm(cls, tg, 3)
            assert tuple(norm.shape) == (2, 2) and norm.dtype == torch.float32
            losses = torch.ops.cvlite.fcos_gfl_loss(reg, cls, tg, norm, 3, R)
            assert tuple(losses.shape) == (2, 3) and losses.dtype == torch.float32
            losses = torch.ops.cvlite.fcos_gfl_loss(reg, cls, tg, None, 3, R, 1.5, 1.0, 0.5)
            assert tuple(losses.shape) == (2, 3)
            d = torch.ops.cvlite.fcos_gfl_decode(reg, R)
            assert tuple(d.shape) == (2, 1022, 8) and d.dtype == torch.float32


def test_library_exports_and_signatures():
    from cvlite import _lib
    lib = _lib.load()
    names = ["cvl_fcos_gfl_norm_workspace_size", "cvl_fcos_gfl_norm", "cvl_fcos_gfl_loss_workspace_size",
             "cvl_fcos_gfl_loss", "cvl_fcos_gfl_decode"]
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and n in _lib.NEWER
    assert len(_lib.SIGNATURES["cvl_fcos_gfl_loss"][1]) == 24
    # the workspace sizes are host arithmetic: 64-cell tiles x 3 sums, 256-cell tiles x 2 sums, float64
    assert int(lib.cvl_fcos_gfl_loss_workspace_size(16, 5456)) == 16 * 86 * 3 * 8
    assert int(lib.cvl_fcos_gfl_norm_workspace_size(16, 5456)) == 16 * 22 * 2 * 8
    assert int(lib.cvl_fcos_gfl_loss_workspace_size(0, 10)) == 0 and int(lib.cvl_fcos_gfl_norm_workspace_size(1, 0)) == 0


def test_ops_refuse_host_tensors():
    """No CPU fallback: the ops raise on host tensors (and without a GPU) instead of computing."""
    from cvlite import _lib
    from cvlite import ops_targets as ot
    reg, cls, tg = torch.zeros((1, 4, 32)), torch.zeros((1, 4, 8)), torch.zeros((1, 4, 8))
    with pytest.raises(_lib.CvlError):
        ot.fcos_gfl_norm(cls, tg, 3)
    with pytest.raises(_lib.CvlError):
        ot.fcos_gfl_loss(reg, cls, tg, 3, 7)
    with pytest.raises(_lib.CvlError):
        ot.fcos_gfl_decode(reg, 7)


def test_fcosnet_reg_max_arguments():
    from cvlite.fcos_net import FCOSNet
    from cvlite.fcos_center_net import FCOSCenterNet
    from cvlite.retina_net import RetinaNetNet
    for bad in (0, 17, -1, 2.5, "7", True):
        with pytest.raises((ValueError, TypeError)):
            FCOSNet(3, device="cpu", reg_max=bad)
    assert FCOSNet.check_reg_max(None) is None and FCOSNet.check_reg_max(16) == 16 and FCOSNet.check_reg_max(1) == 1
    with pytest.raises(TypeError):
        FCOSCenterNet(3, reg_max=7)
    with pytest.raises(TypeError):
        RetinaNetNet(3, reg_max=7)


def test_parameter_layouts():
    """The default network's parameters are what they were (the 5-output head); reg_max changes the reg
    heads' last dimension and nothing else."""
    from cvlite.fcos_net import FCOSNet
    plain = FCOSNet.param_dict(3)
    assert FCOSNet.reg_max is None
    for l in range(1, 6):
        assert tuple(plain["reg_output_%d/kernel" % l].shape) == (3, 3, 256, 5)
        assert tuple(plain["reg_output_%d/bias" % l].shape) == (5,)
    for R in (7, 16):
        gfl = FCOSNet.param_dict(3, reg_max=R)
        n = 4 * (R + 1)
        assert list(gfl) == list(plain)
        for k in plain:
            if k.startswith("reg_output_"):
                assert tuple(gfl[k].shape)[-1] == n and tuple(gfl[k].shape)[:-1] == tuple(plain[k].shape)[:-1]
            else:
                assert tuple(gfl[k].shape) == tuple(plain[k].shape), k
        # Conv's default initialisation: glorot-uniform kernel, zero bias
        w = gfl["reg_output_3/kernel"]
        lim = float(np.sqrt(6.0 / (9 * 256 + 9 * n)))
        assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.9 * lim and not gfl["reg_output_3/bias"].any()
    assert FCOSNet.reg_max is None                      # param_dict left the class as it was


class _Plain(object):
    C = 3
    reg_max = None


class _Gfl(object):
    C = 3
    reg_max = 7


class _Centre(object):
    C = 3
    cen_heads = ()


def test_recipe_argument_errors():
    """The network / recipe pairs that cannot train raise before any device work."""
    from cvlite.train_fcos import FCOSTrainer, JitterFCOSTrainer, check_recipe, train
    sample = {"image": np.zeros((128, 128, 3), np.float32), "bbox": np.zeros((0, 4), np.float32), "label": []}
    with pytest.raises(ValueError, match="reg_max"):
        FCOSTrainer(_Plain(), 2, (128, 128), targets="gfl")
    with pytest.raises(ValueError, match="centre"):
        FCOSTrainer(_Centre(), 2, (128, 128), targets="gfl")
    with pytest.raises(ValueError, match="reg_max"):
        JitterFCOSTrainer(_Plain(), 2, targets="gfl", gfl_beta=1.0)
    with pytest.raises(ValueError, match="reg_max"):
        train([sample] * 2, [], _Plain(), 2, None, None, None, 0, 1, recipe="gfl")
    for kind in ("fcos", "center", "center_v1", "paper", "atss"):
        with pytest.raises(ValueError, match="gfl"):
            FCOSTrainer(_Gfl(), 2, (128, 128), targets=kind)
        with pytest.raises(ValueError, match="gfl"):
            JitterFCOSTrainer(_Gfl(), 2, targets=kind)
    for recipe in ("reference", "paper", "atss"):
        with pytest.raises(ValueError, match="gfl"):
            train([sample] * 2, [], _Gfl(), 2, None, None, None, 0, 1, recipe=recipe)
    with pytest.raises(ValueError):
        FCOSTrainer(_Plain(), 2, (128, 128), targets="gfocal")
    with pytest.raises(ValueError, match="recipe"):
        train([sample] * 2, [], _Gfl(), 2, None, None, None, 0, 1, recipe="gfocal")
    check_recipe(_Gfl(), "gfl")
    for kind in ("fcos", "paper", "atss"):
        check_recipe(_Plain(), kind)


def test_checkpoint_head_mismatch_message():
    """A 5-output checkpoint into a GFL network (and the reverse) fails on the layout check with a message
    that names the box head, before anything is copied."""
    from cvlite import checkpoint as ck

    class Store(object):
        def __init__(self, n):
            self.offsets = {"cls_layer_1/kernel": (0, 9 * 256 * 256, (3, 3, 256, 256)),
                            "reg_output_1/kernel": (9 * 256 * 256, 9 * 256 * n, (3, 3, 256, n))}

    class Net(object):
        def __init__(self, n, reg_max):
            self.store, self.reg_max = Store(n), reg_max
    old = {"names": [[k, o, n] for k, (o, n, _) in Store(5).offsets.items()]}
    with pytest.raises(ValueError, match="5 outputs.*68.*reg_max=16"):
        ck.load_net_state(Net(68, 16), old)
    new = {"names": [[k, o, n] for k, (o, n, _) in Store(32).offsets.items()]}
    with pytest.raises(ValueError, match="32 outputs.*has 5"):
        ck.load_net_state(Net(5, None), new)
