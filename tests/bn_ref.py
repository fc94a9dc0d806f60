"""BatchNorm backward: float64 reference, the two input sets, derived error bounds, and an fp32
restatement of the kernel arithmetic with mutation switches (no GPU; imported by test_bn_ref_host.py
and test_gpu_bn_backward_forms.py).

Semantics (include/cvlite.h, the comments above BnPG in csrc/nn_ops.hip), on the kernels' own operands
(bf16 dy, z, y, z_sc; fp32 mean_rstd [B][C][2], gamma, beta):

    g      = dy * mask                     mask: y > 0 | bitmap bit | 0 < bn(z) < act_hi | none
    xhat   = (z - mean) * rstd
    S1, S2 = sum_rows g, sum_rows g * xhat          per (image, channel); or the sums handed in
    dz     = gamma * rstd * (g - S1/n - xhat * S2/n) [+ dz_beta * dz_old]      n = HW * (images in the group)
    g_out  = g
    dgamma = sum_b S2 [+ beta_acc * old], dbeta = sum_b S1 [+ beta_acc * old], conv_dbias = 0
    sc_sums = (sum_rows g, sum_rows g * xhat_sc)    per (image, channel)

Two input sets.  EXACT: dy integers in [-4, 4]; z multiples of 0.5 in [-4, 4]; mean multiples of 0.5
in [-1, 1]; rstd in {0.5, 1, 2}; gamma in {0.5, 1, 2, -1}; beta multiples of 0.5 in [-2, 2].  Then
xhat is a multiple of 0.25 with |xhat| <= 10, g * xhat a multiple of 0.25 with |.| <= 40, and every
partial sum over HW <= 1024 rows stays below 40 * 1024 * 4 = 2^17.4 quarter units < 2^24: each
product and each partial sum is a float32 number, so (S1, S2), sc_sums, dgamma and dbeta are the same
bits in ANY summation order and are compared with ==.  bn(z) = gamma * xhat + beta is a multiple of
0.125 below 22 in magnitude (exact in fp32, and many elements sit exactly on 0 and on 6: the strict
inequalities of the mask decide them); y = relu(bn(z) + r), r integers in [-3, 3], is below 32 and so
exact in bf16.  RANDOM: Gaussian bf16 dy and z, mean ~ 0.5 + 0.3 N, rstd in [0.3, 1.3], gamma in
[0.5, 1.5]; z is redrawn until every float64 bn(z) is at least 1e-3 away from 0 and from 6, far more
than the few 2^-24 relative of the kernels' fp32 fma(gamma, (z - mean) * rstd, beta), so reference
and kernel agree on every mask bit and no element is left out of any comparison.

Bounds (u = 2^-24, the fp32 unit roundoff; bf16 stores round to nearest even, relative error at most
2^-9 < ub = 2^-8).  Nothing here is measured on the code under test.

  sums  A sum of HW fp32 terms in any order (one chain is the least favourable: HW - 1 additions, each
        partial below sum |t|) is within (HW - 1) u sum |t| to first order; a term g * xhat carries the
        roundings of z - mean, * rstd and the product (3 u |t|; a fused multiply-add only removes one).
        (HW + 2) u A to first order; the remaining u A covers the second-order part HW^2 u^2 / 2 for
        HW <= 5000.  The partials are combined in float64 (2^-53: nothing).  So per (image, channel)
            |S - ref| <= (HW + 3) u A,    A1 = sum |g|, A2 = sum |g * xhat|.
        bn_stats is the same with terms x and x^2.
  dgamma, dbeta   = float(sum_b S) [+ beta_acc * old]: the per-image bounds add up; the float store
        rounds once, u |ref|; with beta_acc != 0 the product rounds (u |beta_acc * old|), and so does
        float(sum_b S) before the addition, u |sum_b S| -- a term the issue's statement of this bound
        left out; it is added here from the arithmetic (fl(fl(a) + fl(b)) has three roundings), not
        from a kernel result (bn_bwd_f32 below, the correct arithmetic, exceeds the bound without it
        by up to 1.73x when the two addends cancel).  Forms that are handed their sums have no first
        term.
  dz    With k1 = S1/n, k2 = S2/n as the kernel forms them (float(S) * fl(1/n): 3 roundings),
        xh (2), xh * k2 (1), two subtractions, fl(gamma * rstd) and the final product, every one of
        |g|, |k1|, |xh k2| carries at most 10 roundings: 16 u (|g| + |S1/n| + |xhat S2/n|) with room for
        the second order and for the bf16 rounding acting on the error itself.  Where the kernel formed
        the sums, their error (HW + 3) u A / n = (1 + 3/HW) u A / (images in the group) enters through
        k1 and xhat * k2.  All times |gamma * rstd|; plus the bf16 store, ub |ref|; plus
        u |dz_beta * dz_old| for the accumulate's product.
  g_out equals g as a number, always.
"""
import math

import torch

U = 2.0 ** -24
UB = 2.0 ** -8
BF = torch.bfloat16
F64 = torch.float64
INF = float("inf")
MARGIN = 1e-3

# (B, HW, C): the smallest shapes that reach each thread layout and row-chunk case at the default
# chunking (NT = 256 threads, 8 channels per thread, tpr = min(C/8, 256) threads per row, rpp = 256 / tpr
# rows per pass, loads unrolled 4 passes deep and clamped to the chunk).  The tests do not depend on the
# chunking: they stay valid (if less pointed) when it changes.
SHAPES = [
    (2, 1, 64),       # one row, below rpp = 32; pass-1 grid row B + 1
    (1, 4, 2048),     # C/8 = 256: rpp = 1; B = 1
    (2, 9, 2048),     # pass 1: three chunks with a one-row tail; pass 0: nine chunks
    (1, 300, 64),     # pass 1: three chunks, 44-row tail (no multiple of 32 or 128); pass 0: 12-row tail < rpp
    (2, 700, 24),     # tpr = 3, rpp = 85, one idle thread, 20-row tails (MobileNetV2 width)
    (3, 130, 1280),   # tpr = 160, rpp = 1, 96 idle threads, two-row tail (MobileNetV2 width)
    (2, 37, 2056),    # C/8 = 257: a second channel-group iteration with one active thread
]
SMALL = SHAPES[:5]
GROUPED_SHAPE = (5, 37, 96)      # tpr = 12, four idle threads; group 2 leaves a short last group
GROUPS = (1, 2, 5)


def ids(shapes=SHAPES):
    return ["%dx%dx%d" % s for s in shapes]


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def _choice(vals, shape, g):
    t = torch.tensor(vals, dtype=torch.float32)
    return t[torch.randint(0, len(vals), shape, generator=g)]


def _halves(lo, hi, shape, g):
    """multiples of 0.5 in [lo, hi]"""
    return torch.randint(int(2 * lo), int(2 * hi) + 1, shape, generator=g).float() * 0.5


def bn64(z, mr, gamma, beta):
    """float64 gamma * (z - mean) * rstd + beta on the stored operands, [B][HW][C]"""
    xh = (z.to(F64) - mr[:, None, :, 0].to(F64)) * mr[:, None, :, 1].to(F64)
    return gamma.to(F64) * xh + beta.to(F64)


def bn32(z, mr, gamma, beta):
    """The kernels' fp32 bn_affine (bn_acc.h): fma(gamma, (z - mean) * rstd, beta).  The product of two
    fp32 numbers is exact in float64, so one float64 addition and a rounding to fp32 restate the fma."""
    xh = (z.float() - mr[:, None, :, 0]) * mr[:, None, :, 1]
    return (gamma.to(F64) * xh.to(F64) + beta.to(F64)).float()


def make_inputs(kind, B, HW, C, seed=0):
    """CPU tensors of one unit: dy, z, z_sc, y, r (bf16 [B][HW][C]); mr, mr_sc (fp32 [B][C][2]); gamma,
    beta (fp32 [C]).  kind: "exact" | "random" (module docstring)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 31 * HW + C + (0 if kind == "exact" else 1 << 20))
    sh = (B, HW, C)
    if kind == "exact":
        assert HW <= 1024
        dy = torch.randint(-4, 5, sh, generator=g).float()
        z, z_sc = _halves(-4, 4, sh, g), _halves(-4, 4, sh, g)
        mr = torch.stack([_halves(-1, 1, (B, C), g), _choice([0.5, 1.0, 2.0], (B, C), g)], -1)
        mr_sc = torch.stack([_halves(-1, 1, (B, C), g), _choice([0.5, 1.0, 2.0], (B, C), g)], -1)
        gamma, beta = _choice([0.5, 1.0, 2.0, -1.0], (C,), g), _halves(-2, 2, (C,), g)
        r = torch.randint(-3, 4, sh, generator=g).float()
    else:
        assert kind == "random"
        dy = torch.randn(sh, generator=g).to(BF).float()
        z, z_sc = torch.randn(sh, generator=g).to(BF).float(), torch.randn(sh, generator=g).to(BF).float()
        mr = torch.stack([0.5 + 0.3 * torch.randn((B, C), generator=g), 0.3 + torch.rand((B, C), generator=g)], -1)
        mr_sc = torch.stack([0.5 + 0.3 * torch.randn((B, C), generator=g), 0.3 + torch.rand((B, C), generator=g)], -1)
        gamma, beta = 0.5 + torch.rand((C,), generator=g), 0.3 * torch.randn((C,), generator=g)
        r = torch.randn(sh, generator=g).to(BF).float()
        for _ in range(64):                  # redraw until bn(z) keeps MARGIN from both mask thresholds
            a = bn64(z, mr, gamma, beta)
            bad = (a.abs() < MARGIN) | ((a - 6.0).abs() < MARGIN)
            n = int(bad.sum())
            if n == 0:
                break
            z[bad] = torch.randn((n,), generator=g).to(BF).float()
        else:
            raise AssertionError("margin redraw did not converge")
    y = torch.clamp(bn64(z, mr, gamma, beta) + r.to(F64), min=0.0).to(BF)
    if kind == "exact":
        assert torch.equal(y.to(F64), torch.clamp(bn64(z, mr, gamma, beta) + r.to(F64), min=0.0))
    return {"kind": kind, "B": B, "HW": HW, "C": C, "dy": dy.to(BF), "z": z.to(BF), "z_sc": z_sc.to(BF), "y": y,
            "r": r.to(BF), "mr": mr.contiguous(), "mr_sc": mr_sc.contiguous(), "gamma": gamma, "beta": beta}


def mask_disagreements(inp, act_hi):
    """Elements whose mask bit differs between the kernels' fp32 bn_affine and the float64 reference."""
    a64, a32 = bn64(inp["z"], inp["mr"], inp["gamma"], inp["beta"]), bn32(inp["z"], inp["mr"], inp["gamma"], inp["beta"])
    return int((((a64 > 0) & (a64 < act_hi)) != ((a32 > 0) & (a32 < act_hi))).sum())


def handed_sums(inp, flavour, mask, act_hi=INF, seed=0):
    """First-pass sums [B][C][2] float64 as a fused producer hands them over: "own" = the data's float64
    sums under `mask`; "other" = unrelated values (the second pass must use what it is given):
    quarter-unit integers on the exact set (dgamma / dbeta stay exact), Gaussian on the random set."""
    B, HW, C = inp["B"], inp["HW"], inp["C"]
    if flavour == "own":
        return bn_bwd_ref(inp, mask, act_hi=act_hi)["S"].clone()
    g = torch.Generator().manual_seed(77 + seed + B + HW + C)
    if inp["kind"] == "exact":
        return torch.randint(-4 * HW, 4 * HW + 1, (B, C, 2), generator=g).to(F64) * 0.25
    return torch.randn((B, C, 2), generator=g, dtype=F64) * math.sqrt(HW)


def old_params(inp, seed=0):
    """dgamma / dbeta to accumulate onto with beta_acc = 0.5: even integers on the exact set."""
    g = torch.Generator().manual_seed(5 + seed + inp["C"])
    if inp["kind"] == "exact":
        return [torch.randint(-8, 9, (inp["C"],), generator=g).float() * 2.0 for _ in range(2)]
    return [torch.randn((inp["C"],), generator=g) * 3.0 for _ in range(2)]


def old_dz(inp, seed=0):
    g = torch.Generator().manual_seed(9 + seed + inp["HW"])
    sh = (inp["B"], inp["HW"], inp["C"])
    if inp["kind"] == "exact":
        return torch.randint(-4, 5, sh, generator=g).float().to(BF)
    return torch.randn(sh, generator=g).to(BF)


def pack_bits(y):
    """The ReLU sign bitmap of y: uint8 [B*HW][C/8], bit u of a byte = y[8c + u] > 0."""
    on = (y.float() > 0).reshape(-1, y.shape[-1] // 8, 8).to(torch.int32)
    w = (1 << torch.arange(8, dtype=torch.int32, device=y.device))
    return (on * w).sum(-1).to(torch.uint8).reshape(-1)


def unpack_bits(bits, shape):
    sh = torch.arange(8, dtype=torch.int32, device=bits.device)
    return ((bits.reshape(-1, 1).to(torch.int32) >> sh) & 1).bool().reshape(shape)


# ---------------------------------------------------------------------------------------------------
# float64 reference + bounds
# ---------------------------------------------------------------------------------------------------
def _keep64(inp, mask, act_hi, bits=None):
    if mask == "y":
        return inp["y"].to(F64) > 0
    if mask == "bits":
        return unpack_bits(pack_bits(inp["y"]) if bits is None else bits, inp["y"].shape)
    if mask == "z":
        a = bn64(inp["z"], inp["mr"], inp["gamma"], inp["beta"])
        return (a > 0) & (a < act_hi)
    assert mask == "none"
    return torch.ones(inp["dy"].shape, dtype=torch.bool)


def _group_total(t, B, group):
    """[B][...] per-image values -> (per-image copy of its group's total, images in the group [B])"""
    gid = torch.arange(B) // group
    ng = int(gid[-1]) + 1
    tot = torch.zeros((ng,) + tuple(t.shape[1:]), dtype=t.dtype).index_add_(0, gid, t)
    cnt = torch.zeros(ng, dtype=F64).index_add_(0, gid, torch.ones(B, dtype=F64))
    return tot[gid], cnt[gid]


def bn_bwd_ref(inp, mask, act_hi=INF, bits=None, sums=None, group=1, dz_beta=0.0, dz_old=None, beta_acc=0.0,
               dgamma_old=None, dbeta_old=None, sc=False):
    """float64 reference of every BN-backward form and the bound of each output (module docstring).
    mask: "y" | "bits" | "z" | "none"; sums: handed first-pass sums [B][C][2] or None (the form makes
    its own); sc: also the shortcut BN's first pass on g.  Returns a dict: dz, g_out [B][HW][C];
    dgamma, dbeta, conv_dbias [C]; S, A (the data's own sums and absolute sums [B][C][2]); sc_sums,
    A_sc; and b_dz, b_S, b_dgamma, b_dbeta, b_sc, the bounds."""
    B, HW, C = inp["B"], inp["HW"], inp["C"]
    mr, gamma = inp["mr"].to(F64), inp["gamma"].to(F64)
    m, rs = mr[:, None, :, 0], mr[:, None, :, 1]
    xh = (inp["z"].to(F64) - m) * rs
    g = torch.where(_keep64(inp, mask, act_hi, bits), inp["dy"].to(F64), torch.zeros((), dtype=F64))
    S = torch.stack([g.sum(1), (g * xh).sum(1)], -1)
    A = torch.stack([g.abs().sum(1), (g * xh).abs().sum(1)], -1)
    own = sums is None
    T = S if own else sums.to(F64)
    Tg, cnt = _group_total(T, B, group)
    Ag, _ = _group_total(A, B, group)
    n = (HW * cnt)[:, None, None]
    k1, k2 = Tg[:, None, :, 0] / n, Tg[:, None, :, 1] / n
    gr = gamma * rs
    dz = gr * (g - k1 - xh * k2)
    inner = 16 * U * (g.abs() + k1.abs() + (xh * k2).abs())
    if own:
        inner = inner + (1 + 3.0 / HW) * U * (Ag[:, None, :, 0] + xh.abs() * Ag[:, None, :, 1]) / cnt[:, None, None]
    b_dz = gr.abs() * inner
    if dz_beta != 0.0:
        dz = dz + dz_beta * dz_old.to(F64)
        b_dz = b_dz + U * (dz_beta * dz_old.to(F64)).abs()
    b_dz = b_dz + UB * dz.abs()
    out = {"dz": dz, "g_out": g, "S": S, "A": A, "b_dz": b_dz, "b_S": (HW + 3) * U * A,
           "conv_dbias": torch.zeros(C, dtype=F64)}
    for name, col, old in (("dbeta", 0, dbeta_old), ("dgamma", 1, dgamma_old)):
        tot = T[..., col].sum(0)
        ref = tot.clone()
        bound = (HW + 3) * U * A[..., col].sum(0) if own else torch.zeros(C, dtype=F64)
        if beta_acc != 0.0:
            acc = beta_acc * old.to(F64)
            ref = ref + acc
            bound = bound + U * acc.abs() + U * tot.abs()
        out[name] = ref
        out["b_" + name] = bound + U * ref.abs()
    if sc:
        ms, rss = inp["mr_sc"][:, None, :, 0].to(F64), inp["mr_sc"][:, None, :, 1].to(F64)
        xs = (inp["z_sc"].to(F64) - ms) * rss
        out["sc_sums"] = torch.stack([g.sum(1), (g * xs).sum(1)], -1)
        out["A_sc"] = torch.stack([g.abs().sum(1), (g * xs).abs().sum(1)], -1)
        out["b_sc"] = (HW + 3) * U * out["A_sc"]
    return out


def stats_ref(x):
    """bn_stats: (sum x, sum x^2) per (image, channel) in float64 and the (HW + 3) u sum |t| bound."""
    xd = x.to(F64)
    S = torch.stack([xd.sum(1), (xd * xd).sum(1)], -1)
    A = torch.stack([xd.abs().sum(1), (xd * xd).sum(1)], -1)
    return S, (x.shape[1] + 3) * U * A


def bn_apply_ref(inp, residual, relu):
    """float64 y = act(bn(z) [+ r]) rounded to bf16 (relu: 0 none, 1 ReLU, 2 ReLU6); exact on the exact set."""
    o = bn64(inp["z"], inp["mr"], inp["gamma"], inp["beta"])
    if residual:
        o = o + inp["r"].to(F64)
    if relu:
        o = torch.where(o > 0, o, torch.zeros((), dtype=F64))
    if relu == 2:
        o = torch.clamp(o, max=6.0)
    return o.to(BF)


# ---------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    """max err / bound over all elements (0/0 = 0, x/0 = inf, NaN stays NaN and fails)."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if not bool(torch.isnan(r).any()) else float("nan")


def check(out, ref, exact, label=""):
    """Every output present in `out` against `ref` (bn_bwd_ref): each element under its bound, none
    skipped; on the exact set sums and parameter gradients with ==.  Returns {name: largest err/bound}
    (information); raises AssertionError naming every output that failed."""
    ratios, bad = {}, []

    def under(name, got, want, bound, equal):
        got = got.detach().cpu().to(F64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err = (got - want).abs()
        ratios[name] = _ratio(err, bound)
        ok = bool((got == want).all()) if equal else bool((err <= bound).all())
        if not ok:
            bad.append("%s (max err %.3e, err/bound %.3g%s)" % (name, float(torch.nan_to_num(err, nan=INF).max()),
                                                                ratios[name], ", == required" if equal else ""))

    if "dz" in out:
        under("dz", out["dz"], ref["dz"], ref["b_dz"], False)
    if out.get("g_out") is not None:
        under("g_out", out["g_out"], ref["g_out"], torch.zeros_like(ref["g_out"]), True)
    for name in ("dgamma", "dbeta"):
        if name in out:
            under(name, out[name], ref[name], ref["b_" + name], exact)
    if out.get("conv_dbias") is not None:
        under("conv_dbias", out["conv_dbias"], ref["conv_dbias"], torch.zeros_like(ref["conv_dbias"]), True)
    if out.get("sc_sums") is not None:
        under("sc_sums", out["sc_sums"], ref["sc_sums"], ref["b_sc"], exact)
    if out.get("S") is not None:
        under("S", out["S"], ref["S"], ref["b_S"], exact)
    print("%s %s" % (label, " ".join("%s=%.3g" % kv for kv in sorted(ratios.items()))))
    assert not bad, "%s: %s" % (label, "; ".join(bad))
    return ratios


# ---------------------------------------------------------------------------------------------------
# fp32 restatement of the kernel arithmetic (torch, CPU) with mutation switches
# ---------------------------------------------------------------------------------------------------
MUTATIONS = ("drop_last_row", "double_last_row", "hw_minus_1", "mask_ge", "skip_last_group")


def _sum_rows32(t, order, chunk):
    """sum over rows of fp32 t [B][R][C]: fp32 chains (one per (image, channel) for "chain"; one per
    `chunk` rows for "chunked"), the chunk partials combined in float64 -> float64 [B][C]."""
    B, R, C = t.shape
    ch = R if order == "chain" else chunk
    nch = (R + ch - 1) // ch
    pad = torch.zeros((B, nch * ch, C), dtype=torch.float32)
    pad[:, :R] = t
    pad = pad.view(B, nch, ch, C)
    acc = torch.zeros((B, nch, C), dtype=torch.float32)
    for k in range(ch):
        acc = acc + pad[:, :, k]
    return acc.to(F64).sum(1)


def bn_bwd_f32(inp, mask, act_hi=INF, sums=None, group=1, dz_beta=0.0, dz_old=None, beta_acc=0.0, dgamma_old=None,
               dbeta_old=None, sc=False, order="chain", chunk=32, mutate=None, prefill=7.0):
    """bn_bwd_kernel's arithmetic in fp32 torch ops: the outputs as check() takes them (with "S", the
    sums it formed).  order: "chain" | "chunked".  mutate: one of MUTATIONS, a defect a rewrite could
    have; `prefill` is what an unwritten dz element holds."""
    assert mutate is None or mutate in MUTATIONS
    B, HW, C = inp["B"], inp["HW"], inp["C"]
    f = torch.float32
    mr, gamma = inp["mr"], inp["gamma"]
    m, rs = mr[:, None, :, 0], mr[:, None, :, 1]
    z, dy = inp["z"].float(), inp["dy"].float()
    xh = (z - m) * rs
    ge = mutate == "mask_ge"
    if mask in ("y", "bits"):
        yy = inp["y"].float()
        keep = (yy >= 0) if ge else (yy > 0)
    elif mask == "z":
        a = bn32(inp["z"], mr, gamma, inp["beta"])
        keep = ((a >= 0) & (a <= act_hi)) if ge else ((a > 0) & (a < act_hi))
    else:
        keep = torch.ones_like(dy, dtype=torch.bool)
    g = torch.where(keep, dy, torch.zeros((), dtype=f))

    def rows(t):
        if mutate == "drop_last_row":
            return t[:, :-1]
        if mutate == "double_last_row":
            return torch.cat([t, t[:, -1:]], 1)
        return t

    S = torch.stack([_sum_rows32(rows(g), order, chunk), _sum_rows32(rows(g * xh), order, chunk)], -1)
    own = sums is None
    T = S if own else sums.to(F64)
    Tg, cnt = _group_total(T, B, group)
    hw = HW - 1 if mutate == "hw_minus_1" else HW
    inv = (torch.ones((), dtype=f) / (torch.tensor(float(hw), dtype=f) * cnt.float()))[:, None, None]
    k1, k2 = Tg[:, None, :, 0].float() * inv, Tg[:, None, :, 1].float() * inv
    o = (gamma * rs) * (g - k1 - xh * k2)
    if dz_beta != 0.0:
        o = o + torch.tensor(dz_beta, dtype=f) * dz_old.float()
    dz = o.to(BF)
    if mutate == "skip_last_group":
        dz[..., C - 8:] = prefill
    out = {"dz": dz, "g_out": g.to(BF), "conv_dbias": torch.zeros(C, dtype=f)}
    if own:
        out["S"] = S
    for name, col, old in (("dbeta", 0, dbeta_old), ("dgamma", 1, dgamma_old)):
        v = T[..., col].sum(0).float()
        if beta_acc != 0.0:
            v = v + torch.tensor(beta_acc, dtype=f) * old
        out[name] = v
    if sc:
        xs = (inp["z_sc"].float() - inp["mr_sc"][:, None, :, 0]) * inp["mr_sc"][:, None, :, 1]
        out["sc_sums"] = torch.stack([_sum_rows32(rows(g), order, chunk), _sum_rows32(rows(g * xs), order, chunk)], -1)
    return out
