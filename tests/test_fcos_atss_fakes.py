"""The fake (shape-only) implementation of the ATSS torch op, and the argument checks of the Python
surface that need no device (CPU)."""
import pytest
import torch


def test_atss_op_fake_gives_the_shapes():
    import cvlite.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        boxes = torch.empty((2, 8, 5), device="cuda")
        nbox = torch.empty((2,), dtype=torch.int32, device="cuda")
        dims = torch.empty((2, 2), device="cuda")
        tg, nt = torch.ops.cvlite.fcos_atss_assign(boxes, nbox, dims, 256, 192, 3, 9, 8.0)
        assert tuple(tg.shape) == (2, 1022, 8) and tg.dtype == torch.float32
        assert tuple(nt.shape) == (2, 5) and nt.dtype == torch.int32
        norm = torch.ops.cvlite.fcos_target_norm(tg, 3)
        reg, cls = torch.empty((2, 1022, 8), device="cuda"), torch.empty((2, 1022, 32), device="cuda")
        losses = torch.ops.cvlite.fcos_paper_loss(reg, cls, tg, norm, 3)
        assert tuple(losses.shape) == (2, 3) and losses.dtype == torch.float32


def test_atss_recipe_argument_errors():
    """targets="atss" on a centre network raises before any device work, in both trainers and train()."""
    from cvlite.train_fcos import FCOSTrainer, JitterFCOSTrainer, train

    class Centre(object):
        cen_heads = ()
        C = 3
    with pytest.raises(ValueError):
        FCOSTrainer(Centre(), 2, (128, 128), targets="atss")
    with pytest.raises(ValueError):
        JitterFCOSTrainer(Centre(), 2, targets="atss", atss_topk=5)
    sample = {"image": torch.zeros((128, 128, 3)).numpy(), "bbox": torch.zeros((0, 4)).numpy(), "label": []}
    with pytest.raises(ValueError):
        train([sample] * 2, [], Centre(), 2, None, None, None, 0, 1, recipe="atss")
