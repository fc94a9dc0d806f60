"""Restatement of the ResNeXt-50 / 101 (32x4d) backbone of cvlite/resnext.py in plain torch (any
float dtype; the tests run it in float64), for the ResNeXt tests.  Built on oracle/model_ref's conv,
bn and bf16 storage-point helpers (q / qw, model_ref.emulate_bf16); the grouped 3x3 is
F.conv2d(groups=32) on the (3, 3, Cg, f) kernel in the TF / torch grouped layout.

Third-party architecture (classification_models' ResNeXt, post-activation blocks), restated, not
pinned to that package: see the module docstring of cvlite/resnext.py.
"""
import torch
import torch.nn.functional as F

from oracle.model_ref import bn, conv, q, qw

EPS = 2e-5
BACKBONE_PREFIXES = ("bn_data", "conv0", "bn0", "stage")


def depths(p):
    out = []
    for st in range(1, 5):
        n = 0
        while "stage%d_unit%d_conv1/kernel" % (st, n + 1) in p:
            n += 1
        out.append(n)
    return tuple(out)


def gconv(x, p, name, stride):
    """ZeroPadding(1) + grouped 3x3 valid, 32 groups; bf16 storage points as model_ref.conv."""
    w = p[name + "/kernel"]                       # (3, 3, Cg, f)
    return q(F.conv2d(F.pad(q(x), (1, 1, 1, 1)), qw(w).permute(3, 2, 0, 1), None, stride, groups=32))


def bn_data(x, p):
    """BatchNormalization(scale=False), training-mode statistics per image; fp32 result."""
    m = x.mean(dim=(2, 3), keepdim=True)
    v = ((x - m) ** 2).mean(dim=(2, 3), keepdim=True)
    return (x - m) / torch.sqrt(v + EPS) + p["bn_data/beta"].view(1, -1, 1, 1)


def resnext(x, p, with_inputs=False):
    """x NCHW.  Returns the taps [C3, C4, C5] = the pre-ReLU sums of the last blocks of stages 2..4
    (NCHW); with_inputs: also the inputs ReLU(a) the following stages read."""
    h = conv(bn_data(x, p), p, "conv0", 2, pad=3, bias=False)
    h = q(F.relu(bn(h, p, "bn0", EPS)))
    h = F.max_pool2d(F.pad(h, (1, 1, 1, 1)), 3, 2)
    taps, nexts = [], []
    for si, nb in enumerate(depths(p)):
        for bi in range(nb):
            n = "stage%d_unit%d" % (si + 1, bi + 1)
            s = (1 if si == 0 else 2) if bi == 0 else 1
            sc = q(bn(conv(h, p, n + "_sc", s, bias=False), p, n + "_sc_bn", EPS)) if bi == 0 else h
            y = q(F.relu(bn(conv(h, p, n + "_conv1", 1, bias=False), p, n + "_bn1", EPS)))
            y = q(F.relu(bn(gconv(y, p, n + "_gconv", s), p, n + "_bn2", EPS)))
            a = bn(conv(y, p, n + "_conv3", 1, bias=False), p, n + "_bn3", EPS) + sc
            if si >= 1 and bi == nb - 1:
                a = q(a)
                taps.append(a)
                h = F.relu(a)
                nexts.append(h)
            else:
                h = q(F.relu(a))
    return (taps, nexts) if with_inputs else taps


def loss_and_grads(params, x_nhwc, cots, dtype=torch.float64):
    """loss = sum over taps of <tap, cotangent> (cots NHWC); returns (taps NHWC, {name: grad}) for
    the backbone parameters."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items() if k.startswith(BACKBONE_PREFIXES)}
    taps = resnext(x_nhwc.to(dtype).permute(0, 3, 1, 2), p)
    loss = sum((t * c.to(dtype).permute(0, 3, 1, 2)).sum() for t, c in zip(taps, cots))
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    return [t.detach().permute(0, 2, 3, 1) for t in taps], dict(zip(names, [g.detach() for g in grads]))


# With the project's usual x0.25 the restatement's own gradients span too wide a range: conv0/kernel's
# norm (it grows with every residual branch the gradient crosses on its way back) leaves only 108 of
# the 160 tensors above 1e-3 of the largest (104 at x0.5, 113 at x0.125, 120 at x0.0625, 123 at x0.03125,
# seeds 3 and 5 alike).  The whole-backbone comparison wants at least 120, so it damps by 1/32.
DAMP = 0.03125


def damp(params, factor=DAMP):
    """bn3 / sc_bn gammas x factor (the project's practice for random-init residual graphs)."""
    for k, v in params.items():
        if k.endswith(("_bn3/gamma", "_sc_bn/gamma")):
            v.mul_(factor)
    return params


def backbone_case(seed=3, B=2, D=128):
    """The whole-backbone comparison's inputs: (image NHWC fp32, tap cotangents NHWC, bf16-exact)."""
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.rand((B, D, D, 3), generator=g) * 2 - 1
    cots = [torch.randn((B, D // s, D // s, c), generator=g).to(torch.bfloat16).float()
            for s, c in ((8, 512), (16, 1024), (32, 2048))]
    return x, cots


def compared(g32):
    """Names whose fp32-restatement gradient norm is at least 1e-3 of the largest."""
    big = max(float(v.norm()) for v in g32.values())
    return [k for k, v in g32.items() if float(v.norm()) >= 1e-3 * big]
