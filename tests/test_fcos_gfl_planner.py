"""The conv launch planners accept the Generalized Focal Loss box head (host only: no device memory, no
launch): the forward, data-gradient and grouped weight-gradient descriptors FCOSNet builds for its
4 (reg_max + 1)-output reg heads, with the padding the network actually uses, at the training geometry
(512 x 512, bs 16) and a small one (64 x 64, bs 2)."""
import ctypes

import pytest
import torch

from wgrad_dispatch_cases import WG_CODES, plan as wgrad_plan

FPN_C = 256
FWD_CODES = (1, 2, 3, 4, 5, 7, 14, 16)         # CVL_CK_* of the forward / data-gradient families


def _heads(R):
    """The reg heads as FCOSNet(reg_max=R) builds them (no device: the planners read no weights)."""
    from cvlite.fcos_net import FCOSNet
    from cvlite.layers import ParamStore
    net = FCOSNet.__new__(FCOSNet)
    net.reg_max = R
    net._build_heads(ParamStore(), 3)
    for h in net.reg_heads:
        h.wf = h.wd = torch.zeros(16)
    net.reg_ld = 8 if R is None else (4 * (R + 1) + 7) // 8 * 8
    return net


def _igemm_plan(lib, d):
    k, t = ctypes.c_int32(-1), ctypes.c_int32(-1)
    nbytes = int(lib.cvl_conv_igemm_workspace_size(ctypes.byref(d)))
    st = lib.cvl_conv_igemm_plan(ctypes.byref(d), 0, nbytes, ctypes.byref(k), ctypes.byref(t))
    return st, k.value, t.value


@pytest.mark.parametrize("size,B", [(512, 16), (64, 2)])
@pytest.mark.parametrize("R", [7, 16])
def test_planners_take_the_gfl_reg_head(R, size, B):
    from cvlite import _lib, ops_nn as nn
    lib = _lib.load()
    net = _heads(R)
    heads = net.reg_heads
    n = 4 * (R + 1)
    assert heads[0].cout == n and heads[0].npad % 32 == 0 and heads[0].npad >= n
    assert heads[0].cout_pad == heads[0].npad and net.reg_ld >= n and net.reg_ld % 8 == 0
    shapes, off, P = net.layout(B, size, size)
    # forward (FCOSNet._heads_forward): fp32 rows of reg_ld columns in the loss layout
    segs = [nn.seg(h, w, h, w, heads[l].wf, None, src_base=B * off[l], src_img=h * w, dst_base=off[l], dst_img=P)
            for l, (h, w) in enumerate(shapes)]
    d = heads[0].fwd_desc(B, segs, ld_dst=net.reg_ld, dst_f32=True, n_store=n)
    d.prec = nn.PREC_BF16
    st, k, _ = _igemm_plan(lib, d)
    assert st == 0 and k in FWD_CODES, (st, k)
    names = [lib.cvl_conv_kernel_name(k)]
    # data gradient (FCOSNet._heads_backward): bf16 gradient rows cout_pad wide
    segs = [nn.seg(h, w, h, w, heads[l].wd, None, src_base=off[l], src_img=P, dst_base=B * off[l], dst_img=h * w)
            for l, (h, w) in enumerate(shapes)]
    d = heads[0].dgrad_desc(B, segs, ld_dst=FPN_C)
    d.prec = nn.PREC_BF16
    st, k, _ = _igemm_plan(lib, d)
    assert st == 0 and k in FWD_CODES, (st, k)
    names.append(lib.cvl_conv_kernel_name(k))
    # weight gradient: one group per level
    segs = [nn.seg(h, w, h, w, heads[l].wf, None, src_base=B * off[l], src_img=h * w, dst_base=off[l], dst_img=P)
            for l, (h, w) in enumerate(shapes)]
    d = heads[0].fwd_desc(B, segs, ld_dst=heads[0].cout_pad, npad=heads[0].cout_pad)
    d.prec = nn.PREC_BF16
    st, k, tile, nsplit, ws = wgrad_plan(lib, d, len(shapes))
    assert st == 0 and k in WG_CODES and tile > 0 and nsplit >= 1, (st, k, tile, nsplit)
    names.append(lib.cvl_conv_kernel_name(k))
    print("reg_max %d, %d x %d bs %d, npad %d: %s; wgrad tile %d nsplit %d workspace %d"
          % (R, size, size, B, heads[0].npad, names, tile, nsplit, ws))


def test_default_head_is_unchanged():
    net = _heads(None)
    assert [h.cout for h in net.reg_heads] == [5] * 5 and net.reg_heads[0].npad == 32
