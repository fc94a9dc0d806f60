"""BN folding for inference, the host side (no GPU): the launch plan of the residual conv
(cvl_conv_igemm_res_relu_plan) for every conv3 of ResNet-50, and the fold arithmetic of a ConvBN unit
against a numpy float64 restatement (tests/fold_ref.py)."""
import numpy as np
import pytest
import torch

from cvlite import ops_nn as nn, resnet
from cvlite.layers import ConvBN, ParamStore, same_pad

from fold_ref import fold_scale_shift, randomize_bn

CK_P = 16


def conv3_descs(H, B):
    """The conv3 (1x1, filters -> 4 * filters, accumulating into the shortcut) descriptor of every
    bottleneck of ResNet-50 at an H x H input, batch B, from the network's own tables."""
    dummy = torch.zeros(8)                     # the planner never dereferences weights or bias
    h, _ = same_pad(H, 7, 2)                   # conv1 (7x7 / 2 after ZeroPadding2D(3): the same size)
    h = (h + 2 - 3) // 2 + 1                   # pool1
    out = []
    for (f, _, stride), nb in zip(resnet.ResNet50.STACKS, resnet.DEPTHS["resnet50"]):
        h, _ = same_pad(h, 1, stride)
        for bi in range(nb):
            d = nn.make_desc(nn.FWD, B, f, 1, 1, 1, 0, 0, 4 * f, 4 * f, 4 * f, [nn.seg(h, h, h, h, dummy, dummy)],
                             beta=1.0)
            out.append(("%dx%d %d->%d block %d" % (h, h, f, 4 * f, bi + 1), d))
    assert len(out) == 16
    return out


@pytest.mark.parametrize("H,B", [(512, 16), (640, 8)], ids=["fcos512_bs16", "retinanet640_bs8"])
def test_res_relu_plan_resnet50_conv3(H, B, dispatch):
    descs = conv3_descs(H, B)
    for name, d in descs:
        assert nn.conv_igemm_res_relu_plan(d) == (CK_P, 1), name
    for hook in ("no_res_relu_fuse", "no_p"):
        dispatch(hook)
        for name, d in descs:
            kernel, fused = nn.conv_igemm_res_relu_plan(d)
            assert fused == 0 and kernel > 0, (hook, name, kernel)
            assert (kernel == CK_P) == (hook == "no_res_relu_fuse"), (hook, name, kernel)
        dispatch(hook + "=0")


def test_res_relu_plan_rejects_other_forms():
    from cvlite import _lib
    _, d = conv3_descs(512, 16)[0]
    for field, value in (("beta", 0.0), ("relu_out", 1), ("dst_f32", 1), ("mode", nn.DGRAD), ("prec", nn.PREC_F32)):
        keep = getattr(d, field)
        setattr(d, field, value)
        with pytest.raises(_lib.CvlError):
            nn.conv_igemm_res_relu_plan(d)
        setattr(d, field, keep)
    assert nn.conv_igemm_res_relu_plan(d) == (CK_P, 1)
    # a plan without the fused epilogue needs a dense destination for the separate ReLU pass
    d.ld_dst += 8
    assert nn.conv_igemm_res_relu_plan(d) == (CK_P, 1)


def test_res_relu_fallback_needs_dense_destination(dispatch):
    from cvlite import _lib
    _, d = conv3_descs(512, 16)[0]
    d.ld_dst += 8
    dispatch("no_res_relu_fuse")
    with pytest.raises(_lib.CvlError):
        nn.conv_igemm_res_relu_plan(d)


@pytest.mark.parametrize("bias", [True, False])
def test_fold_scale_shift_matches_float64(bias):
    st = ParamStore()
    units = [ConvBN(st, "a", 1, 32, 40, bias=bias), ConvBN(st, "b", 3, 40, 72, bias=bias, eps=1e-3)]
    st.finalize("cpu", 0)
    for u in units:
        u.bn.init_buffers("cpu")
    randomize_bn([u.bn for u in units], [u.conv for u in units], seed=3)
    for u in units:
        s, b = u.fold_params()
        assert s.dtype == torch.float32 and b.dtype == torch.float32 and s.shape == (u.bn.c,)
        rs, rb = fold_scale_shift(u.bn.gamma.numpy(), u.bn.beta.numpy(), u.bn.run_mean.numpy(), u.bn.run_var.numpy(),
                                  u.bn.eps, u.conv.b.numpy() if bias else None)
        np.testing.assert_allclose(s.numpy(), rs, rtol=1e-6, atol=0)
        np.testing.assert_allclose(b.numpy(), rb, rtol=1e-6, atol=0)
        assert np.abs(rs - 1).max() > 0.1 and np.abs(rb).max() > 0.1        # a non-trivial BN


def test_fold_refuses_fp32_parity_store():
    st = ParamStore()
    st.act = torch.float32
    u = ConvBN(st, "a", 1, 32, 32)
    st.finalize("cpu", 0)
    u.bn.init_buffers("cpu")
    with pytest.raises(NotImplementedError):
        u.fold_params()
