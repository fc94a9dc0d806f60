"""The fake (shape-only) implementations of the FCOS papers' torch ops, and the argument checks of the
Python surface that need no device (CPU)."""
import pytest
import torch


def test_paper_ops_fakes_give_the_shapes():
    import cvlite.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        boxes = torch.empty((2, 8, 5), device="cuda")
        nbox = torch.empty((2,), dtype=torch.int32, device="cuda")
        dims = torch.empty((2, 2), device="cuda")
        tg, nt = torch.ops.cvlite.fcos_paper_assign(boxes, nbox, dims, 256, 192, 3, 1.5)
        assert tuple(tg.shape) == (2, 1022, 8) and tg.dtype == torch.float32
        assert tuple(nt.shape) == (2, 5) and nt.dtype == torch.int32
        norm = torch.ops.cvlite.fcos_target_norm(tg, 3)
        assert tuple(norm.shape) == (2, 2) and norm.dtype == torch.float32
        reg, cls = torch.empty((2, 1022, 8), device="cuda"), torch.empty((2, 1022, 32), device="cuda")
        for nm in (norm, None):
            losses = torch.ops.cvlite.fcos_paper_loss(reg, cls, tg, nm, 3)
            assert tuple(losses.shape) == (2, 3) and losses.dtype == torch.float32


def test_paper_recipe_argument_errors():
    """targets="paper" on a centre network and an unknown recipe raise before any device work; the centre
    variants' loss flags are no keywords of fcos_paper_loss."""
    from cvlite import ops_targets as ot
    from cvlite.train_fcos import FCOSTrainer, JitterFCOSTrainer, train

    class Centre(object):
        cen_heads = ()
        C = 3
    with pytest.raises(ValueError):
        FCOSTrainer(Centre(), 2, (128, 128), targets="paper")
    with pytest.raises(ValueError):
        JitterFCOSTrainer(Centre(), 2, targets="paper")
    with pytest.raises(ValueError):
        FCOSTrainer(Centre(), 2, (128, 128), targets="papers")
    sample = {"image": torch.zeros((128, 128, 3)).numpy(), "bbox": torch.zeros((0, 4)).numpy(), "label": []}
    with pytest.raises(ValueError):
        train([sample] * 2, [], Centre(), 2, None, None, None, 0, 1, recipe="papers")
    t = torch.zeros((1, 4, 8))
    for flag in ("cen_in_cls", "reg_sigmoid", "float_mask"):
        with pytest.raises(TypeError):
            ot.fcos_paper_loss(t, t, t, 3, **{flag: True})
    assert ot.FCOS_PAPER_BOUNDS == (64.0, 128.0, 256.0, 512.0)
