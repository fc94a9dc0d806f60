"""ResNeXt-50 / ResNeXt-101 (32x4d) backbones (the `backbone_model="resnext50" | "resnext101"`
branch of RetinaNet/retinanet_module.py:53-66), explicit forward/backward on the cvlite kernels.

The reference takes these graphs from the third-party `classification_models` package
(`Classifiers.get("resnext50")(include_top=False, input_shape=[None, None, 3])`).  That package is
not a dependency of cvlite: the architecture is restated here (as resnet.py and mobilenet_v2.py
restate Keras), not pinned to the package -- importing one of its checkpoints is out of scope
(its 32 per-group Keras sublayers carry auto-generated names).

Structure (post-activation blocks, no conv bias, every BN eps 2e-5 / momentum 0.99, training-mode
statistics per image as everywhere in cvlite):
  stem    bn_data (BatchNormalization(scale=False) on the fp32 image: beta only) -> ZeroPadding(3)
          -> conv0 7x7/2, 64 -> bn0 -> ReLU -> ZeroPadding(1) -> MaxPool 3x3/2
  stages  s = 0..3, filters f = 128 * 2^s, blocks (3, 4, 6, 3) / (3, 4, 23, 3), every block outputs
          2f channels; the first block of a stage is a projection block (stride 1 in stage 0, 2 after)
  block   stage{s+1}_unit{b+1}: _conv1 1x1 cin -> f, _bn1, ReLU; grouped 3x3 (ZeroPadding(1) + valid,
          the block's stride, 32 groups of Cg = f / 32 channels) f -> f, _bn2, ReLU; _conv3 1x1 f -> 2f,
          _bn3; projection blocks: _sc 1x1 cin -> 2f with the block's stride on the block input,
          _sc_bn; a = bn3 + shortcut; output ReLU(a)
  taps    the reference taps the Add layers: C3 / C4 / C5 are the pre-ReLU sums `a` of the last
          blocks of stages 1 / 2 / 3 (512 / 1024 / 2048 channels at strides 8 / 16 / 32); the next
          stage reads ReLU(a), so in backward da = d_tap + d_out * (a > 0).

The grouped conv is ONE parameter `stage{S}_unit{B}_gconv/kernel` of shape (3, 3, Cg, f) (the TF /
torch grouped layout: output channel o belongs to group o // Cg), initialised glorot_uniform per
Keras sublayer (fan_in = fan_out = 9 Cg).

MI355X mapping: 1x1 convs on the MFMA implicit-GEMM kernels with the BN statistics fused into
their epilogue (layers.ConvBN, the plain two-pass BN backward); the grouped 3x3 on
cvl_gconv3x3_* (csrc/conv_group.hip); bn_data on cvl_bn_data_*; the stem conv, pool and their
backward on the ResNet stem kernels.  bf16 only (no fp32 parity mode).

Known cost: bn_data/beta is trained and conv0's zero padding comes after the BN, so
d beta_c = sum_{ky,kx,co} w[ky,kx,c,co] * R[ky,kx,co] with R the sum of dz0 over the output pixels whose
tap lands inside the image; R comes from one extra cvl_stem_wgrad launch on an all-ones image.
"""
import torch

from . import ops_nn as nn
from .layers import BF16, BatchNorm, Conv, ConvBN, StatsArena, constant, glorot_uniform, wgrad_batch
from .resnet import FUSE_POOL_BWD, STEM_K, STEM_KP, Stem

BN_EPS, BN_MOM = 2e-5, 0.99
GROUPS = 32
DEPTHS = {"resnext50": (3, 4, 6, 3), "resnext101": (3, 4, 23, 3)}
TAP_CHANNELS = (512, 1024, 2048)


class DataBN(object):
    """BatchNormalization(scale=False) on the fp32 image: beta [3] and the moving statistics."""

    def __init__(self, store, name):
        self.name, self.c, self.eps, self.momentum = name, 3, BN_EPS, BN_MOM
        self.gname = None
        self.bname = store.add(name + "/beta", (3,), constant(0.0))
        self.store = store
        self.run_mean = self.run_var = None

    def init_buffers(self, device):
        self.run_mean = torch.zeros(3, dtype=torch.float32, device=device)
        self.run_var = torch.ones(3, dtype=torch.float32, device=device)

    @property
    def beta(self):
        return self.store.p(self.bname)

    def forward(self, x, train):
        B = x.shape[0]
        mr = torch.empty((B, 3, 2), dtype=torch.float32, device=x.device)
        if train:
            nn.bn_data_stats(x, mr, self.run_mean, self.run_var, self.eps, self.momentum)
        else:
            mr[:, :, 0] = self.run_mean
            mr[:, :, 1] = torch.rsqrt(self.run_var + self.eps)
        out = torch.empty_like(x)
        nn.bn_data_apply(x, mr, self.beta, out)
        return out


def bn_data_beta_grad(w, dz, ones):
    """d bn_data/beta [3] from dz0 = the gradient of conv0's output: conv0's zero padding comes after the
    BN, so d beta_c = sum_{ky,kx,co} w[ky,kx,c,co] * R[ky,kx,co], R = the sum of dz0 over the output
    pixels whose tap (ky, kx) lands inside the image = the stem weight gradient of an all-ones image
    (`ones`, the image's shape).  w: the fp32 master kernel [7,7,3,64]; the forward multiplies its
    bf16 rounding, so that is what the contraction uses."""
    r = torch.empty((192, 64), dtype=torch.float32, device=dz.device)    # rows ky*24 + kx*3 + c
    nn.stem_wgrad(ones, dz, r)
    nn.wgrad_flush()                                 # r is read right away (deferred reductions)
    rv = r.view(8, 24, 64)[:7, :21].reshape(7, 7, 3, 64)
    return (w.to(BF16).float() * rv).sum((0, 1, 3))


class XStem(Stem):
    """bn_data -> conv0 (7x7/2 after ZeroPadding(3), no bias) -> bn0 -> ReLU -> pool, on the ResNet
    stem kernels (cvl_stem_conv7x7s2 takes a null bias)."""

    def __init__(self, store):
        self.bn_data = DataBN(store, "bn_data")
        self.conv = Conv(store, "conv0", STEM_K, 3, 64, stride=2, pad=3, bias=False, dgrad=False, cin_k=STEM_KP)
        self.bn = BatchNorm(store, "bn0", 64, eps=BN_EPS, momentum=BN_MOM)
        self._ones = None

    def forward(self, x, train=True, arena=None):
        return Stem.forward(self, self.bn_data.forward(x, train), train, arena)

    def backward(self, dp, saved):
        A, z, y, mr, arg, B, Ho, Wo = saved
        dz = torch.empty_like(z)
        st = self.bn.store
        dy = torch.empty_like(z)
        if FUSE_POOL_BWD:
            nn.maxpool3x3s2_backward_bn_relu(dp, arg, z, mr, self.bn.gamma, self.bn.beta, dy, dz, st.g(self.bn.gname),
                                             st.g(self.bn.bname))
        else:
            nn.maxpool3x3s2_backward(dp, arg, dy)
            nn.bn_backward_relu(dy, z, mr, self.bn.gamma, self.bn.beta, dz, st.g(self.bn.gname),
                                st.g(self.bn.bname), B, Ho * Wo, 64)
        dw = torch.empty((192, 64), dtype=torch.float32, device=dp.device)    # rows ky*24 + kx*3 + c
        nn.stem_wgrad(A, dz, dw)
        if self._ones is None or self._ones.shape != A.shape or self._ones.device != A.device:
            self._ones = torch.ones_like(A)
        db = bn_data_beta_grad(self.conv.w, dz, self._ones)          # (flushes the deferred reductions)
        self.conv.dw.view(7, 21, 64).copy_(dw.view(8, 24, 64)[:7, :21])
        st.g(self.bn_data.bname).copy_(db)


class GConvBN(object):
    """Grouped 3x3 (ZeroPadding(1) + valid, stride s, 32 groups, no bias) -> BN -> ReLU."""

    def __init__(self, store, name, bn_name, c, stride):
        self.c, self.cg, self.stride = c, c // GROUPS, stride
        self.wname = store.add(name + "/kernel", (3, 3, self.cg, c), glorot_uniform(9 * self.cg, 9 * self.cg))
        self.bn = BatchNorm(store, bn_name, c, eps=BN_EPS, momentum=BN_MOM)
        self.store = store
        self.wf = self.wd = None

    def pack(self):
        if self.wf is None:
            dev = self.store.flat.device
            self.wf, self.wd = nn.gconv3x3_packed(self.c, dev), nn.gconv3x3_packed(self.c, dev)
        nn.gconv3x3_pack(self.store.p(self.wname), self.wf, self.wd)

    def forward(self, x, B, H, W, train, arena):
        Ho, Wo = (H - 1) // self.stride + 1, (W - 1) // self.stride + 1
        z = torch.empty((B, Ho, Wo, self.c), dtype=BF16, device=x.device)
        stats = arena.take(B, self.c) if train else None
        nn.gconv3x3_fwd(x, self.wf, z, self.cg, self.stride, stats)      # BN statistics in the epilogue
        y, mr = self.bn.normalize(z, stats, B, Ho * Wo, 1, train=train)
        return y, Ho, Wo, (x, z, mr, B, H, W, Ho, Wo)

    def backward(self, dy, saved):
        x, z, mr, B, H, W, Ho, Wo = saved
        st = self.store
        dz = torch.empty_like(z)
        nn.bn_backward_relu(dy, z, mr, self.bn.gamma, self.bn.beta, dz, st.g(self.bn.gname), st.g(self.bn.bname), B,
                            Ho * Wo, self.c)
        nn.gconv3x3_wgrad(x, dz, st.g(self.wname), self.stride)
        dx = torch.empty_like(x)
        nn.gconv3x3_dgrad(dz, self.wd, dx, self.cg, self.stride)
        return dx


def _unit(store, name, bn_name, cin, cout, stride):
    return ConvBN(store, name, 1, cin, cout, stride, bn_name=bn_name, bias=False, eps=BN_EPS, momentum=BN_MOM)


class XBlock(object):
    """[1x1 -> BN -> ReLU] [grouped 3x3 / s -> BN -> ReLU] [1x1 -> BN] + shortcut -> ReLU."""

    def __init__(self, store, name, cin, filters, stride, proj):
        self.sc = _unit(store, name + "_sc", name + "_sc_bn", cin, 2 * filters, stride) if proj else None
        self.c1 = _unit(store, name + "_conv1", name + "_bn1", cin, filters, 1)
        self.g = GConvBN(store, name + "_gconv", name + "_bn2", filters, stride)
        self.c3 = _unit(store, name + "_conv3", name + "_bn3", filters, 2 * filters, 1)
        self.cout = 2 * filters

    def units(self):
        return [u for u in (self.sc, self.c1, self.c3) if u is not None]

    def bns(self):
        return [u.bn for u in self.units()] + [self.g.bn]

    def param_names(self):
        out = [self.g.wname]
        for bn in self.bns():
            out += [bn.gname, bn.bname]
        return out + [u.conv.wname for u in self.units()]

    def forward(self, x, B, H, W, train, arena, tap=False):
        """Returns (block output ReLU(a), the pre-ReLU sum a when tap else None, Ho, Wo, saved)."""
        sv_s, s = None, x
        if self.sc is not None:
            s, sv_s = self.sc.forward(x, B, H, W, relu=False, train=train, arena=arena)
        y1, sv1 = self.c1.forward(x, B, H, W, relu=True, train=train, arena=arena)
        y2, Ho, Wo, sv2 = self.g.forward(y1, B, H, W, train, arena)
        if not tap:
            y3, sv3 = self.c3.forward(y2, B, Ho, Wo, relu=True, residual=s, train=train, arena=arena)
            return y3, None, Ho, Wo, (sv_s, sv1, sv2, sv3)
        # a tapped block forms both a (the feature tap) and ReLU(a): two BN applies of z3
        a, sv3 = self.c3.forward(y2, B, Ho, Wo, relu=False, residual=s, train=train, arena=arena)
        out = torch.empty_like(a)
        bn = self.c3.bn
        nn.bn_apply(sv3[1], sv3[3], bn.gamma, bn.beta, s, out, B, Ho * Wo, self.cout, 1)
        return out, a, Ho, Wo, (sv_s, sv1, sv2, sv3)

    def backward(self, dy, saved, tap=False):
        """dy: gradient of the block output -- of the pre-ReLU sum a for a tapped block (an identity
        block; its buffer becomes dx).  Returns dx."""
        sv_s, sv1, sv2, sv3 = saved
        if tap:
            assert self.sc is None
            dy2 = self.c3.backward(dy, sv3)              # no ReLU: the shortcut's gradient is dy itself
            dy1 = self.g.backward(dy2, sv2)
            self.c1.backward(dy1, sv1, dx_out=dy, dx_beta=1.0)
            return dy
        dx = torch.empty_like(sv1[0])
        g = dx if self.sc is None else torch.empty_like(dy)      # identity: the residual gradient lands in dx
        dy2 = self.c3.backward(dy, sv3, g_out=g)
        dy1 = self.g.backward(dy2, sv2)
        if self.sc is not None:
            self.sc.backward(g, sv_s, dx_out=dx, dx_beta=0.0)
        self.c1.backward(dy1, sv1, dx_out=dx, dx_beta=1.0)
        return dx


class ResNeXt(object):
    """ResNeXt-50 / 101 32x4d up to the three Add taps.  forward(x) -> ([(C3, H3, W3), (C4, ..),
    (C5, ..)], saved), the taps bf16 NHWC pre-ReLU sums."""
    tap_channels = TAP_CHANNELS

    def __init__(self, store, depth="resnext50"):
        self.store = store
        self.stem = XStem(store)
        self.stages = []
        cin = 64
        for si, nb in enumerate(DEPTHS[depth.lower()]):
            f = 128 << si
            stage = []
            for bi in range(nb):
                stage.append(XBlock(store, "stage%d_unit%d" % (si + 1, bi + 1), cin, f,
                                    (1 if si == 0 else 2) if bi == 0 else 1, bi == 0))
                cin = 2 * f
            self.stages.append(stage)

    # ---- parameters -----------------------------------------------------------------------------
    def blocks(self):
        return [b for st in self.stages for b in st]

    def convs(self):
        return [self.stem.conv] + [u.conv for b in self.blocks() for u in b.units()]

    def gconvs(self):
        return [b.g for b in self.blocks()]

    def fold_bn(self):
        """BN folding for inference (ResNet50.fold_bn) is not provided for this network."""
        raise NotImplementedError("fold_bn covers the ResNet v1 bottleneck backbones, not ResNeXt's grouped 3x3 units")

    def bns(self):
        return [self.stem.bn_data, self.stem.bn] + [bn for b in self.blocks() for bn in b.bns()]

    def pack_entries(self):
        """The dense convs' rows of the batched re-pack (ops_nn.PackPlan)."""
        return [self.stem.pack_entry()] + [u.conv.pack_entry() for b in self.blocks() for u in b.units()]

    def pack_grouped(self):
        """The grouped kernels' bf16 slab images (one small launch each, after every update)."""
        for g in self.gconvs():
            g.pack()

    def pack(self):
        self.stem.pack()
        for b in self.blocks():
            for u in b.units():
                u.conv.pack()
        self.pack_grouped()

    def grad_groups(self):
        """[(hook name, parameter names)] in the order backward() finalises them."""
        out = []
        for si in (3, 2, 1):
            out.append(("conv%d" % (si + 2), [n for b in self.stages[si] for n in b.param_names()]))
        stem = [self.stem.bn_data.bname, self.stem.conv.wname, self.stem.bn.gname, self.stem.bn.bname]
        out.append(("conv2_stem", [n for b in self.stages[0] for n in b.param_names()] + stem))
        return out

    # ---- forward / backward -----------------------------------------------------------------------
    def forward(self, x, train=True):
        """x: fp32 NHWC [B,H,W,3].  Returns [C3, C4, C5] (bf16 NHWC, pre-ReLU) and saved state."""
        B = x.shape[0]
        arena = StatsArena(2 * B * sum(bn.c for bn in self.bns()), x.device) if train else None
        h, sv_stem = self.stem.forward(x, train, arena)
        H, W = h.shape[1], h.shape[2]
        saved, taps = [], []
        for si, st in enumerate(self.stages):
            ssv = []
            for bi, b in enumerate(st):
                tap = si >= 1 and bi == len(st) - 1
                h, a, H, W, sv = b.forward(h, B, H, W, train, arena, tap=tap)
                ssv.append(sv)
                if tap:
                    taps.append((a, H, W))
                    ssv[-1] = sv + (a,)
            saved.append(ssv)
        return taps, (sv_stem, saved)

    def backward(self, d_taps, saved, hook=None):
        """d_taps: gradients of [C3, C4, C5] (used in place).  hook(name) fires when a stage's
        parameter gradients are final ("conv5" .. "conv3", then "conv2_stem"), as ResNet50.backward."""
        hook = hook or (lambda name: None)
        sv_stem, ssv = saved
        dh = None
        for si in range(3, -1, -1):
            st = self.stages[si]
            # the stage's 1x1 weight gradients: one batched launch at the stage's end (layers.wgrad_batch)
            with wgrad_batch():
                for bi in range(len(st) - 1, -1, -1):
                    sv = ssv[si][bi]
                    if si >= 1 and bi == len(st) - 1:
                        da = d_taps[si - 1]
                        if dh is not None:               # da = d_tap + d_out * (a > 0)
                            nn.relu_backward(dh, sv[4], da, beta=1.0)
                        dh = st[bi].backward(da, sv[:4], tap=True)
                    else:
                        dh = st[bi].backward(dh, sv)
            if si > 0:
                hook("conv%d" % (si + 2))
        self.stem.backward(dh, sv_stem)
        hook("conv2_stem")
