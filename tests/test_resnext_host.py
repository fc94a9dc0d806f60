"""ResNeXt-50 / 101 backbones (RetinaNet/retinanet_module.py:53-66), host side: the parameter set
RetinaNetNet builds for them, and the float64 restatement (tests/resnext_ref.py) the GPU tests
compare against."""
import pytest
import torch

import resnext_ref as rr

SEED = 3


def _backbone(sd):
    return {k: v for k, v in sd.items() if k.startswith(rr.BACKBONE_PREFIXES)}


@pytest.fixture(scope="module")
def params50():
    from cvlite.retina_net import RetinaNetNet
    return RetinaNetNet.param_dict(8, seed=SEED, backbone_model="resnext50")


@pytest.mark.parametrize("name,count,tensors", [("resnext50", 22979907, 160), ("resnext101", 42128707, 313)])
def test_param_dict_builds_with_the_stated_counts(name, count, tensors):
    from cvlite.retina_net import RetinaNetNet
    bb = _backbone(RetinaNetNet.param_dict(8, backbone_model=name))
    assert sum(v.numel() for v in bb.values()) == count
    assert len(bb) == tensors
    assert tuple(bb["stage1_unit1_gconv/kernel"].shape) == (3, 3, 4, 128)
    assert tuple(bb["stage4_unit3_gconv/kernel"].shape) == (3, 3, 32, 1024)
    assert not [k for k in bb if k.endswith("/bias")]
    assert tuple(bb["bn_data/beta"].shape) == (3,) and "bn_data/gamma" not in bb
    assert RetinaNetNet.backbone_kind(name) == name


def test_grouped_kernel_init_is_glorot_per_group(params50):
    w = params50["stage2_unit1_gconv/kernel"]               # Cg = 8: limit sqrt(6 / (72 + 72))
    lim = (6.0 / (2 * 9 * 8)) ** 0.5
    assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.95 * lim


def test_other_detectors_keep_their_backbone_mapping():
    from cvlite.fpn_det import FPNDetector
    assert FPNDetector.backbone_kind("resnext50") == "mobilenetv2"          # fcos.py:29-41: no ResNeXt branch


def test_restatement_tap_shapes_and_pre_relu_taps(params50):
    p = {k: v.double() for k, v in _backbone(params50).items()}
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2 - 1
    with torch.no_grad():
        taps, nexts = rr.resnext(x, p, with_inputs=True)
    assert [tuple(t.permute(0, 2, 3, 1).shape) for t in taps] == [(2, 8, 8, 512), (2, 4, 4, 1024), (2, 2, 2, 2048)]
    for t, h in zip(taps, nexts):
        assert float(t.min()) < 0, "a tap is the pre-ReLU sum"
        assert float(h.min()) >= 0, "the next stage reads ReLU(a)"
        assert torch.equal(h, torch.relu(t))


def test_restatement_alone_leaves_enough_tensors_to_compare(params50):
    """The GPU whole-backbone test (test_gpu_gconv.py) skips tensors whose fp32-restatement gradient
    norm is below 1e-3 of the largest; which ones depends only on the restatement, so the floor of 120
    compared tensors (of 160) is checked here, without a GPU."""
    p = rr.damp({k: v.clone() for k, v in _backbone(params50).items()})
    x, cots = rr.backbone_case(SEED)
    _, g32 = rr.loss_and_grads(p, x, cots)
    names = rr.compared(g32)
    assert len(g32) == 160 and len(names) >= 120, len(names)
    assert "bn_data/beta" in names
    for s in range(1, 5):
        assert any(k.startswith("stage%d_" % s) and k.endswith("gconv/kernel") for k in names)
