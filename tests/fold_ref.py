"""float64 restatement of the inference (training=False) graph the BN-folding tests compare against,
written from the Keras layer definitions on torch CPU ops; independent of every cvlite kernel.

  Conv2D            HWIO kernel, 'same' padding as TensorFlow lays it out (the extra pixel goes
                    bottom / right), or ZeroPadding2D(p) + 'valid'
  BatchNormalization(training=False)
                    y = gamma * (x - moving_mean) / sqrt(moving_variance + epsilon) + beta
  ResNet v1 bottleneck (keras.applications.resnet block1)
                    shortcut = BN(Conv1x1/s(x)) if conv_shortcut else x
                    y = ReLU(BN(Conv1x1/s(x))); y = ReLU(BN(Conv3x3(y))); y = BN(Conv1x1(y))
                    out = ReLU(shortcut + y)
  ResNet50          ZeroPadding2D(3), Conv7x7/2, BN, ReLU, ZeroPadding2D(1), MaxPool3x3/2, the stacks;
                    taps conv3_block4_out / conv4_block6_out / conv5_block3_out
  FCOS              the FPN, towers and heads of cvlite.fpn_det / cvlite.fcos_net (their docstrings)

Everything is NCHW float64 inside; parameters come as a dict of Keras names -> tensors (ParamStore
names plus <bn>/moving_mean and <bn>/moving_variance).  randomize_bn gives the BatchNorms and conv
biases non-trivial values: a fresh model's BN is the identity map and shows nothing."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def randomize_bn(bns, convs, seed=0):
    """gamma ~ U(0.5, 1.5), beta ~ N(0, 0.2), moving_mean ~ N(0, 0.5), moving_var ~ U(0.5, 2) for every
    BatchNorm of `bns`; bias ~ N(0, 0.1) for every conv of `convs` that has one.  In place, on the
    tensors' own device, from a host generator."""
    g = torch.Generator().manual_seed(seed)
    for bn in bns:
        c = bn.c
        bn.gamma.copy_(torch.rand(c, generator=g) + 0.5)
        bn.beta.copy_(torch.randn(c, generator=g) * 0.2)
        bn.run_mean.copy_(torch.randn(c, generator=g) * 0.5)
        bn.run_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.5)
    for cv in convs:
        if cv.has_bias:
            cv.b.copy_(torch.randn(cv.cout, generator=g) * 0.1)


def params64(store, bns):
    """Keras-named float64 host parameters of a ParamStore plus the BatchNorms' moving statistics."""
    p = {k: v.to(F64) for k, v in store.state_dict().items()}
    for bn in bns:
        p[bn.name + "/moving_mean"] = bn.run_mean.detach().cpu().to(F64)
        p[bn.name + "/moving_variance"] = bn.run_var.detach().cpu().to(F64)
    return p


def fold_scale_shift(gamma, beta, mean, var, eps, bias=None):
    """numpy float64: s = gamma / sqrt(var + eps), b' = (bias - mean) * s + beta, rounded once to fp32."""
    gamma, beta, mean, var = (np.asarray(t, np.float64) for t in (gamma, beta, mean, var))
    b = np.zeros_like(gamma) if bias is None else np.asarray(bias, np.float64)
    s = gamma / np.sqrt(var + np.float64(eps))
    return s.astype(np.float32), ((b - mean) * s + beta).astype(np.float32)


def _same(n, k, s):
    total = max((-(-n // s) - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def conv(x, p, name, stride=1, pad="same", bias=True):
    w = p[name + "/kernel"]
    k = w.shape[0]
    if pad == "same":
        (pt, pb), (pl, pr) = _same(x.shape[2], k, stride), _same(x.shape[3], k, stride)
    else:
        pt = pb = pl = pr = int(pad)
    x = F.pad(x, (pl, pr, pt, pb))
    return F.conv2d(x, w.permute(3, 2, 0, 1), p[name + "/bias"] if bias and (name + "/bias") in p else None, stride)


def bn_eval(x, p, name, eps=1.001e-5):
    v = lambda k: p[name + "/" + k].view(1, -1, 1, 1)  # noqa: E731
    return v("gamma") * (x - v("moving_mean")) / torch.sqrt(v("moving_variance") + eps) + v("beta")


def bottleneck(x, p, name, stride, conv_shortcut):
    sc = bn_eval(conv(x, p, name + "_0_conv", stride), p, name + "_0_bn") if conv_shortcut else x
    y = F.relu(bn_eval(conv(x, p, name + "_1_conv", stride), p, name + "_1_bn"))
    y = F.relu(bn_eval(conv(y, p, name + "_2_conv"), p, name + "_2_bn"))
    y = bn_eval(conv(y, p, name + "_3_conv"), p, name + "_3_bn")
    return F.relu(sc + y)


def resnet50_taps(x, p, blocks=(3, 4, 6, 3)):
    """x NCHW float64 -> [C3, C4, C5]."""
    h = F.relu(bn_eval(conv(x, p, "conv1_conv", 2, pad=3), p, "conv1_bn"))
    h = F.max_pool2d(F.pad(h, (1, 1, 1, 1)), 3, 2)
    taps = []
    for si, (nb, stride) in enumerate(zip(blocks, (1, 2, 2, 2))):
        for bi in range(nb):
            h = bottleneck(h, p, "conv%d_block%d" % (si + 2, bi + 1), stride if bi == 0 else 1, bi == 0)
        taps.append(h)
    return taps[1:]


def fcos_heads(x, p, num_classes):
    """x NCHW float64 -> (reg [B, P, 5], cls [B, P, C]), cells level-major (P3 .. P7), as FCOSNet."""
    c3, c4, c5 = resnet50_taps(x, p)
    l3, l4, l5 = conv(c3, p, "c3_1x1"), conv(c4, p, "c4_1x1"), conv(c5, p, "c5_1x1")
    up = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)  # noqa: E731
    p6 = conv(c5, p, "c6_3x3", 2)
    levels = [conv(l3 + up(l4), p, "c3_3x3"), conv(l4 + up(l5), p, "c4_3x3"), conv(l5, p, "c5_3x3"), p6,
              conv(F.relu(p6), p, "c7_3x3", 2)]
    regs, clss = [], []
    B = x.shape[0]
    for l, f in enumerate(levels):
        c = r = f
        for i in range(4):
            c = conv(c, p, "cls_layer_%d" % (i + 1), bias=False)
            r = conv(r, p, "reg_layer_%d" % (i + 1), bias=False)
        c = conv(F.relu(c), p, "logits_output_%d" % (l + 1))
        r = conv(F.relu(r), p, "reg_output_%d" % (l + 1))
        clss.append(c.permute(0, 2, 3, 1).reshape(B, -1, num_classes))
        regs.append(r.permute(0, 2, 3, 1).reshape(B, -1, 5))
    return torch.cat(regs, 1), torch.cat(clss, 1)


def rel_l2(got, ref):
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    return float((got - ref).norm() / ref.norm())
