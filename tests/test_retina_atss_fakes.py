"""The fake (shape-only) implementations of the RetinaNet ATSS torch ops, and the argument checks of the
Python surface that need no device (CPU)."""
import pytest
import torch


def test_retina_atss_op_fakes_give_the_shapes():
    import cvlite.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        boxes = torch.empty((2, 8, 5), device="cuda")
        nbox = torch.empty((2,), dtype=torch.int32, device="cuda")
        dims = torch.empty((2, 2), device="cuda")
        adims = torch.empty((5, 9, 2), device="cuda")
        tg, nt = torch.ops.cvlite.retina_atss_assign(boxes, nbox, dims, 256, adims, 3, 9)
        assert tuple(tg.shape) == (2, 1364, 9, 8) and tg.dtype == torch.float32
        assert tuple(nt.shape) == (2, 5) and nt.dtype == torch.int32
        tg3, _ = torch.ops.cvlite.retina_atss_assign(boxes, nbox, dims, 128, adims[:, :3], 80, 4)
        assert tuple(tg3.shape) == (2, 341, 3, 8)
        reg, cls = torch.empty((2, 1364, 40), device="cuda"), torch.empty((2, 1364, 32), device="cuda")
        losses = torch.ops.cvlite.retina_atss_loss(reg, cls, tg, nt, None, 9, 3)
        assert tuple(losses.shape) == (2, 2) and losses.dtype == torch.float32
        w = torch.empty((2,), device="cuda")
        losses = torch.ops.cvlite.retina_atss_loss(reg, cls, tg, nt, w, 9, 3, 0.25, 2.0)
        assert tuple(losses.shape) == (2, 2)


def test_retina_atss_recipe_argument_errors():
    """Anything other than "reference" / "atss" raises before any device work, in the trainer and train()."""
    from cvlite import train_retinanet as tr
    assert tr.TARGET_KINDS == ("reference", "atss")
    sample = {"image": torch.zeros((128, 128, 3)).numpy(), "bbox": torch.zeros((0, 4)).numpy(), "label": []}
    with pytest.raises(ValueError):
        tr.train([sample] * 6, [], None, 2, None, None, None, 0, 1, recipe="paper")
    import inspect
    sig = inspect.signature(tr.RetinaTrainer.__init__).parameters
    assert sig["targets"].default == "reference" and sig["atss_topk"].default == 9
    sig = inspect.signature(tr.train).parameters
    assert sig["recipe"].default == "reference" and sig["atss_topk"].default == 9
