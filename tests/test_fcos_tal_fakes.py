"""The fake (shape-only) implementations of the task-aligned torch ops, the library's exports, and the
argument checks of FCOSTrainer, JitterFCOSTrainer, check_recipe and train for "tal" that need no device
(CPU)."""
import numpy as np
import pytest
import torch


def test_tal_op_fakes_give_the_shapes():
    import cvlite.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        boxes = torch.empty((2, 16, 5), device="cuda")
        nbox = torch.empty((2,), device="cuda", dtype=torch.int32)
        dims = torch.empty((2, 2), device="cuda")
        reg = torch.empty((2, 1022, 8), device="cuda")
        for C, ld in ((1, 8), (20, 32), (80, 80)):
            cls = torch.empty((2, 1022, ld), device="cuda")
            tg, nt = torch.ops.cvlite.fcos_tal_assign(boxes, nbox, dims, 256, 192, C, reg, cls)
            assert tuple(tg.shape) == (2, 1022, 5 + C) and tg.dtype == torch.float32
            assert tuple(nt.shape) == (2, 5) and nt.dtype == torch.int32
            tg, nt = torch.ops.cvlite.fcos_tal_assign(boxes, nbox, dims, 256, 192, C, reg, cls, 32, 0.5, 2.0, False)
            assert tuple(tg.shape) == (2, 1022, 5 + C)
            norm = torch.ops.cvlite.fcos_target_norm(tg, C)
            losses = torch.ops.cvlite.fcos_tal_loss(reg, cls, tg, norm, C)
            assert tuple(losses.shape) == (2, 3) and losses.dtype == torch.float32
            losses = torch.ops.cvlite.fcos_tal_loss(reg, cls, tg, None, C, 1.5, 1.0)
            assert tuple(losses.shape) == (2, 3)


def test_library_exports_and_signatures():
    from cvlite import _lib
    lib = _lib.load()
    for n in ("cvl_fcos_tal_workspace_size", "cvl_fcos_tal_assign", "cvl_fcos_tal_loss"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES and n in _lib.NEWER
    assert len(_lib.SIGNATURES["cvl_fcos_tal_assign"][1]) == 26
    assert _lib.SIGNATURES["cvl_fcos_tal_loss"] == _lib.SIGNATURES["cvl_fcos_paper_loss"]
    # host arithmetic: one 64-bit key per cell, (cell, metric, IoU) for 32 ranks per box, two maxima per box
    assert int(lib.cvl_fcos_tal_workspace_size(16, 5456, 16)) == 16 * 5456 * 8 + 16 * 16 * 32 * 12 + 16 * 16 * 8
    assert int(lib.cvl_fcos_tal_workspace_size(0, 10, 4)) == 0 and int(lib.cvl_fcos_tal_workspace_size(1, 10, 0)) == 0


def test_ops_refuse_host_tensors():
    """No CPU fallback: the ops raise on host tensors (and without a GPU) instead of computing."""
    from cvlite import _lib
    from cvlite import ops_targets as ot
    reg, cls, tg = torch.zeros((1, 1022, 8)), torch.zeros((1, 1022, 8)), torch.zeros((1, 1022, 8))
    boxes, nbox, dims = torch.zeros((1, 4, 5)), torch.zeros((1,), dtype=torch.int32), torch.zeros((1, 2))
    with pytest.raises(_lib.CvlError):
        ot.fcos_tal_assign(boxes, nbox, dims, (256, 192), 3, reg, cls)
    with pytest.raises(_lib.CvlError):
        ot.fcos_tal_loss(reg, cls, tg, 3)


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
    """ "tal" is a recipe; it needs the plain FCOS network (no centre variant, no reg_max), and its
    options are checked before any device work."""
    from cvlite.train_fcos import TARGET_KINDS, FCOSTrainer, JitterFCOSTrainer, check_recipe, train
    sample = {"image": np.zeros((128, 128, 3), np.float32), "bbox": np.zeros((0, 4), np.float32), "label": []}
    assert "tal" in TARGET_KINDS
    check_recipe(_Plain(), "tal")
    with pytest.raises(ValueError, match="centre"):
        check_recipe(_Centre(), "tal")
    with pytest.raises(ValueError, match="gfl"):
        check_recipe(_Gfl(), "tal")
    with pytest.raises(ValueError, match="centre"):
        FCOSTrainer(_Centre(), 2, (128, 128), targets="tal")
    with pytest.raises(ValueError, match="gfl"):
        FCOSTrainer(_Gfl(), 2, (128, 128), targets="tal")
    with pytest.raises(ValueError, match="gfl"):
        JitterFCOSTrainer(_Gfl(), 2, targets="tal", tal_warmup=3)
    with pytest.raises(ValueError, match="centre"):
        train([sample] * 2, [], _Centre(), 2, None, None, None, 0, 1, recipe="tal")
    with pytest.raises(ValueError, match="gfl"):
        train([sample] * 2, [], _Gfl(), 2, None, None, None, 0, 1, recipe="tal", tal_topk=9)
    for kw in (dict(tal_topk=0), dict(tal_topk=33), dict(tal_alpha=-1.0), dict(tal_beta=float("nan")),
               dict(tal_warmup=-1)):
        with pytest.raises(ValueError, match="tal_"):
            FCOSTrainer(_Plain(), 2, (128, 128), targets="tal", **kw)
    with pytest.raises(ValueError, match="tal_warmup"):
        JitterFCOSTrainer(_Plain(), 2, targets="tal", tal_warmup=-2)
    with pytest.raises(ValueError, match="recipe"):
        train([sample] * 2, [], _Plain(), 2, None, None, None, 0, 1, recipe="toood")
    with pytest.raises(ValueError, match="'tal'"):
        FCOSTrainer(_Plain(), 2, (128, 128), targets="toood")
