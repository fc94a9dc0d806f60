"""The fake (shape-only) implementations of the Gaussian CenterNet torch ops, the library's exports, and
the argument checks and defaults of CenterNetTrainer, train_step and evaluate_centernet that need no
device (CPU)."""
import inspect

import numpy as np
import pytest
import torch


def test_gauss_op_fakes_give_the_shapes():
    import cvlite.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        boxes = torch.empty((2, 6, 5), device="cuda")
        nbox = torch.empty((2,), dtype=torch.int32, device="cuda")
        dims = torch.empty((2, 2), device="cuda")
        for (ph, pw, s, C, ld) in ((128, 128, 4, 3, 32), (128, 96, 4, 20, 32), (120, 100, 8, 80, 96)):
            t, npos = torch.ops.cvlite.centernet_gauss_assign(boxes, nbox, dims, ph, pw, C, s, 0.7)
            assert tuple(t.shape) == (2, ph // s, pw // s, 4 + C) and t.dtype == torch.float32
            assert tuple(npos.shape) == (2,) and npos.dtype == torch.int32
            pred = torch.empty((2, ph // s, pw // s, ld), device="cuda")
            losses = torch.ops.cvlite.centernet_gauss_loss(pred, t, npos, C)
            assert tuple(losses.shape) == (2, 2) and losses.dtype == torch.float32
            losses = torch.ops.cvlite.centernet_gauss_loss(pred.view(2, -1, ld), t.view(2, -1, 4 + C), npos, C, 1.5, 3.0)
            assert tuple(losses.shape) == (2, 2)
        t, _ = torch.ops.cvlite.centernet_gauss_assign(boxes, nbox, dims, 64, 64, 3)     # stride 4, overlap 0.7
        assert tuple(t.shape) == (2, 16, 16, 7)


def test_library_exports_and_signatures():
    from cvlite import _lib
    lib = _lib.load()
    names = ["cvl_centernet_gauss_assign", "cvl_centernet_gauss_norm", "cvl_centernet_gauss_loss_workspace_size",
             "cvl_centernet_gauss_loss"]
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and n in _lib.NEWER
    assert len(_lib.SIGNATURES["cvl_centernet_gauss_assign"][1]) == 12
    assert len(_lib.SIGNATURES["cvl_centernet_gauss_norm"][1]) == 6
    assert len(_lib.SIGNATURES["cvl_centernet_gauss_loss"][1]) == 16
    # host arithmetic: 32-cell tiles (the smallest) x 2 sums, float64
    assert int(lib.cvl_centernet_gauss_loss_workspace_size(8, 16384)) == 8 * 512 * 2 * 8
    assert int(lib.cvl_centernet_gauss_loss_workspace_size(3, 750)) == 3 * 24 * 2 * 8
    assert int(lib.cvl_centernet_gauss_loss_workspace_size(0, 10)) == 0
    assert int(lib.cvl_centernet_gauss_loss_workspace_size(1, 0)) == 0


def test_ops_refuse_host_tensors():
    """No CPU fallback: the ops raise on host tensors (and without a GPU) instead of computing."""
    from cvlite import _lib
    from cvlite import ops_targets as ot
    boxes, nbox, dims = torch.zeros((1, 2, 5)), torch.zeros((1,), dtype=torch.int32), torch.zeros((1, 2))
    t, pred, npos = torch.zeros((1, 16, 7)), torch.zeros((1, 16, 8)), torch.zeros((1,), dtype=torch.int32)
    with pytest.raises(_lib.CvlError):
        ot.centernet_gauss_assign(boxes, nbox, dims, (16, 16), 3)
    with pytest.raises(_lib.CvlError):
        ot.centernet_gauss_norm(t, 3)
    with pytest.raises(_lib.CvlError):
        ot.centernet_gauss_loss(pred, t, npos, 3)


class _Net(object):
    C = 3


def test_bad_recipe_names_raise_before_device_work():
    from cvlite.train_centernet import CenterNetTrainer
    from cvlite.centernet_hourglass import train_step
    from cvlite.evaluate import evaluate_centernet
    for bad in ("gauss", "paper", "", None, 1):
        with pytest.raises(ValueError, match="targets"):
            CenterNetTrainer(_Net(), 2, (128, 128), targets=bad)
        with pytest.raises(ValueError, match="recipe"):
            train_step(_Net(), 2, np.zeros((2, 128, 128, 3), np.float32), np.zeros((2, 32, 32, 7), np.float32), None,
                       recipe=bad)
    for bad in ("max", "soft-nms", "", None):
        with pytest.raises(ValueError, match="decode"):
            evaluate_centernet(_Net(), [], 3, decode=bad)


def test_signature_defaults():
    from cvlite.train_centernet import CenterNetTrainer
    from cvlite.centernet_hourglass import format_data_gaussian, train_step
    from cvlite.evaluate import evaluate_centernet
    from cvlite import ops_targets as ot
    p = inspect.signature(CenterNetTrainer.__init__).parameters
    assert p["targets"].default == "reference" and p["min_overlap"].default == 0.7
    assert p["focal_alpha"].default == 2.0 and p["focal_beta"].default == 4.0
    assert p["cls_lambda"].default == 2.5 and p["reg_lambda"].default == 1.0
    assert inspect.signature(train_step).parameters["recipe"].default == "reference"
    p = inspect.signature(evaluate_centernet).parameters
    assert p["decode"].default == "nms" and p["K"].default == 100
    p = inspect.signature(format_data_gaussian).parameters
    assert list(p) == ["gt_labels", "img_dim", "num_classes", "img_pad", "stride", "min_overlap"]
    assert p["img_pad"].default is None and p["stride"].default == 8 and p["min_overlap"].default == 0.7
    p = inspect.signature(ot.centernet_gauss_loss).parameters
    assert p["alpha"].default == 2.0 and p["beta"].default == 4.0
    assert inspect.signature(ot.centernet_gauss_assign).parameters["min_overlap"].default == 0.7
