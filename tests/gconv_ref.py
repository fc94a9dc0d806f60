"""Grouped 3x3 convolution (csrc/conv_group.hip): float64 reference with absolute companions, the two
input sets and the derived error bounds (no GPU needed; imported by test_gconv_ref_host.py,
test_gpu_gconv_plans.py and launch_parity.py).

Semantics (include/cvlite.h "Grouped 3x3 convolution"), NHWC, on the kernels' own operands (bf16 x and
dy, the fp32 master kernel w [3][3][Cg][C] rounded to bf16), pad 1 top / left, stride s in {1, 2},
Ho = (H - 1) // s + 1; output channel o = g * Cg + oo reads input channels g * Cg + i:

    fwd    y [b, oy, ox, g, oo] = sum_{ky, kx, i} x[b, oy s - 1 + ky, ox s - 1 + kx, g, i] w[ky, kx, i, g, oo]
    dgrad  dx[b, iy, ix, g, i]  = sum over the (ky, kx, oo, oy, ox) with oy s - 1 + ky = iy, ox s - 1 + kx = ix
                                  of dy[b, oy, ox, g, oo] w[ky, kx, i, g, oo]            [+ beta * dx_old]
    wgrad  dW[ky, kx, i, g, oo] = sum_{b, oy, ox} x[b, oy s - 1 + ky, ox s - 1 + kx, g, i] dy[b, oy, ox, g, oo]
                                                                                         [+ beta * dW_old]

written as nine shifted einsums over [B, H, W, G, Cg] views (cheap at 64 groups on the device, and fine
on the CPU at test sizes).  Every function returns (t, A): the float64 value and its absolute
companion, the same sum over |x| |w| (|dy| |w|, |x| |dy|) plus |beta * old| -- the scale every
rounding of the accumulation is relative to.

Two input sets from one seeded generator (make_inputs).

EXACT (kind "exact"; "flat" is the same alphabet drawn uniformly).  x and dy are integers in [-2, 2],
master weights are in {-1, -0.5, 0, 0.5, 1} (bf16 numbers, so packing does not round them), `old` is an
integer in [-4, 4].  Every product is a multiple of 0.5 below 2 in magnitude, so in half units a
forward / data-gradient value and each of its partial sums, in any order, is an integer of magnitude at
most 2 * (9 * 32 * 2 * 1 + |beta * old|) <= 2 * (576 + 4) = 1160 < 2^24: each is a float32 number and the
kernel's fp32 accumulator holds t exactly before its one store.  y and dx must therefore equal
t.float().to(bfloat16) bit for bit: one round-to-nearest-even of an exactly known value.  The weight
gradient sums B * Ho * Wo integer products below 4 in magnitude: B * Ho * Wo * 4 <= 2 * 32 * 128 * 4 = 2^15
(the largest map any test uses) < 2^24, so dW and every partial of every chunking is exact, and with
beta = 2 onto 0.25 the result is an integer + 0.5 below 2^15: exact as well.  dW must equal t.float().
    Whether the store rounds at all depends on the size of t: multiples of 0.5 below 128 are bf16
numbers, so at Cg = 4 (|t| <= 72) no store ever rounds, and unbiased draws at Cg = 32 (standard
deviation 17) never reach 128 either.  "exact" therefore draws x, dy and |w| towards the positive end
(P = .03 .05 .07 .25 .60 over the ascending alphabet; the groups' weights alternate in sign): at
Cg = 32 a forward value is 259 +- 18 in magnitude where bf16 spacing is 2, so three values in four are
rounded and one in four (the odd integers) is a tie; a four-tap pixel of the stride-2 data gradient is
115 +- 12 and crosses 128, where half-integers tie.  count_ties() counts them; the host test asserts
the Cg = 32 data has some for both bf16 outputs and both strides.  "flat" keeps |y| small: the fused BN
statistics (sum y, sum y^2 of the stored y) are then exact sums as well (test_gpu_gconv_plans.py checks
the preconditions on the CPU).

RANDOM.  x, dy = randn rounded to bf16; w = 0.3 randn (rounded to bf16 by the pack; the reference
multiplies the rounded values); old = randn (bf16 for dx, fp32 for dW).

Bounds (u = 2^-24, the fp32 unit roundoff).  Nothing here is measured on the code under test.

  bf16 outputs   |got - t| <= 2^-8 (|t| + e) + e,   e = 2^-15 A.
        The fp32 value v the kernel stores is the sum of at most 9 * 32 = 288 exact bf16 x bf16 products
        (zero ones included: the block-diagonal padding), plus beta * old: at most 290 accumulations, each
        rounding by at most u times a partial sum below A, so |v - t| <= 290 u A = 2^-15.8 A for a chain in
        any order; 2^-15 A leaves a factor 1.76 for the MFMA's unspecified internal order (the
        instruction's 32-deep dot product is not a documented chain of fp32 additions).  The store rounds
        v to nearest even: relative error at most 2^-9 < 2^-8 of |v| <= |t| + e.
  dW    |got - t| <= (n + nchunk + 2) u A,   n = B * Ho * Wo.
        n products accumulated in fp32 in some order over the chunk's tiles (n - 1 additions, each within
        u A), nchunk partials added by the reduce kernel, the product beta * old and the final addition.
  BN statistics   (HW + 3) u sum |y| and (HW + 3) u sum y^2 per (image, channel), HW = Ho * Wo, against the
        kernel's own stored y: the form bn_ref.stats_ref derives (fp32 partials of at most HW terms,
        combined in float64 or exact bins).
"""
import torch

U = 2.0 ** -24
BF = torch.bfloat16
F64 = torch.float64

INTS = (-2.0, -1.0, 0.0, 1.0, 2.0)
WVALS = (0.0, 0.5, 1.0)
SKEW = (0.03, 0.05, 0.07, 0.25, 0.60)


def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def _draw(vals, probs, shape, g):
    n = 1
    for d in shape:
        n *= d
    p = torch.tensor(probs if probs is not None else [1.0] * len(vals), dtype=torch.float32)
    idx = torch.multinomial(p, n, replacement=True, generator=g)
    return torch.tensor(vals, dtype=torch.float32)[idx].reshape(shape)


def make_inputs(kind, B, H, W, C, Cg, s, seed=0):
    """CPU tensors of one case: x [B,H,W,C] bf16, w [3,3,Cg,C] fp32 master, dy [B,Ho,Wo,C] bf16, dx_old
    [B,H,W,C] bf16, dw_old [3,3,Cg,C] fp32.  kind: "exact" | "flat" | "random" (module docstring)."""
    Ho, Wo = out_hw(H, W, s)
    salt = {"exact": 0, "flat": 1, "random": 2}[kind]
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 131 * H + 31 * W + C + 17 * Cg + s + (salt << 20))
    if kind == "random":
        x = torch.randn((B, H, W, C), generator=g).to(BF)
        w = torch.randn((3, 3, Cg, C), generator=g) * 0.3
        dy = torch.randn((B, Ho, Wo, C), generator=g).to(BF)
        dx_old = torch.randn((B, H, W, C), generator=g).to(BF)
        dw_old = torch.randn((3, 3, Cg, C), generator=g)
    else:
        skew = SKEW if kind == "exact" else None
        x = _draw(INTS, skew, (B, H, W, C), g).to(BF)
        w = _draw((-1.0, -0.5, 0.0, 0.5, 1.0), skew, (3, 3, Cg, C), g)
        if kind == "exact":        # groups alternate in sign: outputs of both signs, no cancellation inside a sum
            sign = (1.0 - 2.0 * (torch.arange(C // Cg) % 2).float()).repeat_interleave(Cg)
            w = w * sign
        dy = _draw(INTS, skew, (B, Ho, Wo, C), g).to(BF)
        dx_old = torch.randint(-4, 5, (B, H, W, C), generator=g).float().to(BF)
        dw_old = torch.full((3, 3, Cg, C), 0.25)
    return {"kind": kind, "geo": (B, H, W, C, Cg, s), "Ho": Ho, "Wo": Wo, "x": x, "w": w, "dy": dy,
            "dx_old": dx_old, "dw_old": dw_old}


# ---------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------
def _w64(w, Cg):
    """master kernel -> the bf16 values the kernels multiply, float64 [3][3][Cg (in)][G][Cg (out)]"""
    C = w.shape[3]
    return w.to(BF).to(F64).reshape(3, 3, Cg, C // Cg, Cg)


def _padded(x, Cg):
    B, H, W, C = x.shape
    xp = torch.zeros((B, H + 2, W + 2, C // Cg, Cg), dtype=F64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x.to(F64).reshape(B, H, W, C // Cg, Cg)
    return xp


def _tap(xp, ky, kx, s, Ho, Wo):
    return xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]


def fwd_ref(x, w, Cg, s):
    """-> (t, A) float64 [B,Ho,Wo,C]"""
    B, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, s)
    xp, wd = _padded(x, Cg), _w64(w.to(x.device), Cg)
    xa, wa = xp.abs(), wd.abs()
    t = torch.zeros((B, Ho, Wo, C // Cg, Cg), dtype=F64, device=x.device)
    A = torch.zeros_like(t)
    for ky in range(3):
        for kx in range(3):
            t += torch.einsum("bhwgi,igo->bhwgo", _tap(xp, ky, kx, s, Ho, Wo), wd[ky, kx])
            A += torch.einsum("bhwgi,igo->bhwgo", _tap(xa, ky, kx, s, Ho, Wo), wa[ky, kx])
    return t.reshape(B, Ho, Wo, C), A.reshape(B, Ho, Wo, C)


def dgrad_ref(dy, w, Cg, s, H, W, beta=0.0, old=None):
    """-> (t, A) float64 [B,H,W,C]; t = conv^T(dy) + beta * old"""
    B, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == out_hw(H, W, s)
    wd = _w64(w.to(dy.device), Cg)
    wa = wd.abs()
    d = dy.to(F64).reshape(B, Ho, Wo, C // Cg, Cg)
    da = d.abs()
    tp = torch.zeros((B, H + 2, W + 2, C // Cg, Cg), dtype=F64, device=dy.device)
    Ap = torch.zeros_like(tp)
    for ky in range(3):
        for kx in range(3):
            _tap(tp, ky, kx, s, Ho, Wo).add_(torch.einsum("bhwgo,igo->bhwgi", d, wd[ky, kx]))
            _tap(Ap, ky, kx, s, Ho, Wo).add_(torch.einsum("bhwgo,igo->bhwgi", da, wa[ky, kx]))
    t = tp[:, 1:H + 1, 1:W + 1].reshape(B, H, W, C).clone()
    A = Ap[:, 1:H + 1, 1:W + 1].reshape(B, H, W, C).clone()
    if beta != 0.0:
        t += beta * old.to(F64)
        A += (beta * old.to(F64)).abs()
    return t, A


def wgrad_ref(x, dy, Cg, s, beta=0.0, old=None):
    """-> (t, A) float64 [3,3,Cg,C]; t = the weight gradient + beta * old"""
    B, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, s)
    assert tuple(dy.shape) == (B, Ho, Wo, C)
    xp = _padded(x, Cg)
    xa = xp.abs()
    d = dy.to(F64).reshape(B, Ho, Wo, C // Cg, Cg)
    da = d.abs()
    t = torch.zeros((3, 3, Cg, C // Cg, Cg), dtype=F64, device=x.device)
    A = torch.zeros_like(t)
    for ky in range(3):
        for kx in range(3):
            t[ky, kx] = torch.einsum("bhwgi,bhwgo->igo", _tap(xp, ky, kx, s, Ho, Wo), d)
            A[ky, kx] = torch.einsum("bhwgi,bhwgo->igo", _tap(xa, ky, kx, s, Ho, Wo), da)
    t, A = t.reshape(3, 3, Cg, C), A.reshape(3, 3, Cg, C)
    if beta != 0.0:
        t = t + beta * old.to(F64)
        A = A + (beta * old.to(F64)).abs()
    return t, A


def stats_ref(y):
    """(sum y, sum y^2) per (image, channel) of the stored y [B,Ho,Wo,C] in float64 [B,C,2], and the
    (HW + 3) u (sum |y|, sum y^2) bound."""
    yd = y.to(F64)
    S = torch.stack([yd.sum((1, 2)), (yd * yd).sum((1, 2))], -1)
    A = torch.stack([yd.abs().sum((1, 2)), (yd * yd).sum((1, 2))], -1)
    return S, (y.shape[1] * y.shape[2] + 3) * U * A


# ---------------------------------------------------------------------------------------------------
# bounds and checks
# ---------------------------------------------------------------------------------------------------
def out_bound(t, A):
    e = 2.0 ** -15 * A
    return 2.0 ** -8 * (t.abs() + e) + e


def dw_bound(A, n, nchunk):
    return (n + nchunk + 2) * U * A


def expected_bf16(t):
    """The exact set's stored value: one round-to-nearest-even of t (exact in fp32)."""
    assert torch.equal(t.float().to(F64), t), "the exact set's value is not a float32 number"
    return t.float().to(BF)


def count_ties(t):
    """Elements of the exact float64 t that sit exactly half way between two bf16 numbers."""
    lo = t.float().view(torch.int32) & ~0xffff                 # truncation: the bf16 neighbour towards 0
    lo = lo.view(torch.float32).to(F64)
    hi = ((t.float().view(torch.int32) & ~0xffff) + 0x10000).view(torch.float32).to(F64)
    return int(((t != lo) & ((t - lo).abs() == (hi - t).abs())).sum())


def ratio(err, bound):
    """max err / bound over all elements (0/0 = 0, x/0 = inf, NaN stays NaN and fails)."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if not bool(torch.isnan(r).any()) else float("nan")


def check_exact(name, got, want):
    """Bit equality of every element; the message counts and locates the mismatches."""
    if torch.equal(got, want):
        return
    bad = (got.to(F64) != want.to(F64)).nonzero()
    raise AssertionError("%s: %d of %d elements differ from the exact value, first at %s (got %r, want %r)" % (
        name, bad.shape[0], got.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])])))


def check_bound(name, got, t, bound):
    """Every element under its bound; returns the largest err / bound (information)."""
    err = (got.to(F64) - t).abs()
    r = ratio(err, bound)
    if not bool((err <= bound).all()):
        bad = (~(err <= bound)).nonzero()
        raise AssertionError("%s: %d of %d elements over their bound, largest err/bound %.3g, first at %s" % (
            name, bad.shape[0], got.numel(), r, bad[0].tolist()))
    return r
