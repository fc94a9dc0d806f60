"""The gate for BatchNorm-backward rewrites: every cvl_bn_backward* entry point (all run
bn_bwd_kernel<PASS, MASK, SC> + bn_colsum_kernel, csrc/nn_ops.hip) against the float64 reference of
tests/bn_ref.py, at every thread layout and row-chunk case, on two input sets.  On the EXACT set every
reduction is exact in fp32, so sums and parameter gradients must be the reference's bits whatever the
summation order; on the RANDOM set each element has a bound derived from the arithmetic (bn_ref.py's
docstring), not tuned.  No element is left out of any comparison.  Also here: bn_stats (PASS 2), writes
that stay inside their buffers (C ABI, guard bytes), and the forward side at the new widths.
profiles/bn_backward_bounds.md records the largest error/bound ratios seen."""
import functools

import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
KINDS = ("exact", "random")
NAN = float("nan")

# form -> (C entry, mask, act_hi, handed sums: None | "acc" (BN accumulator buffer) | "f64", sc, g_out)
FORMS = {
    "backward": ("cvl_bn_backward", "y", R.INF, None, False, True),
    "backward_nomask": ("cvl_bn_backward", "none", R.INF, None, False, True),
    "bits": ("cvl_bn_backward_bits", "bits", R.INF, None, False, True),
    "relu": ("cvl_bn_backward_relu", "z", R.INF, None, False, False),
    "relu6": ("cvl_bn_backward_relu6", "z", 6.0, None, False, False),
    "relu_sums": ("cvl_bn_backward_relu_sums", "z", R.INF, "acc", False, False),
    "relu_sums_6": ("cvl_bn_backward_relu_sums", "z", 6.0, "acc", False, False),
    "res_sums": ("cvl_bn_backward_res_sums", "y", R.INF, "acc", False, True),
    "res_sums_bits": ("cvl_bn_backward_res_sums_bits", "bits", R.INF, "acc", False, True),
    "res_sums_sc": ("cvl_bn_backward_res_sums_sc", "y", R.INF, "acc", True, True),
    "res_sums_sc_bits": ("cvl_bn_backward_res_sums_sc_bits", "bits", R.INF, "acc", True, True),
    "sc": ("cvl_bn_backward_sc", "y", R.INF, None, True, True),
    "sc_bits": ("cvl_bn_backward_sc_bits", "bits", R.INF, None, True, True),
    "sums": ("cvl_bn_backward_sums", "none", R.INF, "f64", False, False),
}


class Calls(object):
    """Records the C entry points ops_nn launches (which mask source a wrapper chose)."""

    def __init__(self, monkeypatch):
        from cvlite import _lib
        self.names = []
        orig = _lib.call

        def call(name, *a):
            self.names.append(name)
            return orig(name, *a)
        monkeypatch.setattr(_lib, "call", call)

    def backward(self):
        return [n for n in self.names if n.startswith("cvl_bn_backward") and "workspace" not in n]


@functools.lru_cache(maxsize=None)
def inputs(kind, shape):
    """(CPU inputs, their device copies) of one (set, shape): shared by the tests, read-only."""
    inp = R.make_inputs(kind, *shape)
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}
    return inp, dev


def _filled(like, value):
    return torch.full_like(like, value)


def _bits_y(d):
    """A y tensor that carries only the bitmap of the real y (its own values are zero): a form that read
    y instead of the bitmap would mask everything."""
    from cvlite import ops_nn as nn
    yb = torch.zeros_like(d["y"])
    bits = nn.attach_relu_bits(yb)
    assert bits is not None
    bits.copy_(R.pack_bits(d["y"]))
    return yb


def run_form(form, inp, d, beta_acc, flavour, with_dbias, fill):
    """One launch of `form` through its cvlite.ops_nn wrapper.  Outputs are pre-filled with `fill`
    (dgamma / dbeta with NaN when beta_acc == 0, else the values to accumulate onto)."""
    from cvlite import ops_nn as nn
    entry, mask, act_hi, handed, sc, has_g = FORMS[form]
    B, HW, C = inp["B"], inp["HW"], inp["C"]
    dev = d["dy"].device
    olds = R.old_params(inp) if beta_acc else (None, None)
    dg = olds[0].to(dev) if beta_acc else torch.full((C,), NAN, device=dev)
    db = olds[1].to(dev) if beta_acc else torch.full((C,), NAN, device=dev)
    cdb = torch.full((C,), 7.0, device=dev) if with_dbias else None
    dz, go = _filled(d["dy"], fill), (_filled(d["dy"], fill) if has_g else None)
    scs = torch.full((B, C, 2), NAN, dtype=F64, device=dev) if sc else None
    sums = R.handed_sums(inp, flavour, "y" if mask == "bits" else mask, act_hi) if handed else None
    y = _bits_y(d) if mask == "bits" else (d["y"].clone() if mask == "y" else None)
    dy, z, mr, ga, be = d["dy"], d["z"], d["mr"], d["gamma"], d["beta"]
    if handed == "acc":
        hs = nn.bn_acc_encode(sums.to(dev))
    elif handed == "f64":
        hs = sums.to(dev)
    if form in ("backward", "backward_nomask", "bits"):
        nn.bn_backward(dy, y, z, mr, ga, dz, go, dg, db, B, HW, C, beta_acc, cdb)
    elif form == "relu":
        nn.bn_backward_relu(dy, z, mr, ga, be, dz, dg, db, B, HW, C, beta_acc, cdb)
    elif form == "relu6":
        nn.bn_backward_relu6(dy, z, mr, ga, be, dz, dg, db, B, HW, C, beta_acc, cdb)
    elif form in ("relu_sums", "relu_sums_6"):
        nn.bn_backward_relu_sums(dy, z, mr, ga, be, hs, dz, dg, db, B, HW, C, beta_acc, cdb, act_hi)
    elif form in ("res_sums", "res_sums_bits"):
        nn.bn_backward_res_sums(dy, y, z, mr, ga, hs, dz, go, dg, db, B, HW, C, beta_acc, cdb)
    elif form in ("res_sums_sc", "res_sums_sc_bits"):
        nn.bn_backward_res_sums_sc(dy, y, z, mr, ga, hs, dz, go, dg, db, d["z_sc"], d["mr_sc"], scs, B, HW, C,
                                   beta_acc, cdb)
    elif form in ("sc", "sc_bits"):
        nn.bn_backward_sc(dy, y, z, mr, ga, dz, go, dg, db, d["z_sc"], d["mr_sc"], scs, B, HW, C, beta_acc, cdb)
    else:
        assert form == "sums"
        nn.bn_backward_sums(dy, z, mr, ga, hs, dz, dg, db, B, HW, C, beta_acc, cdb)
    torch.cuda.synchronize()
    out = {"dz": dz, "g_out": go, "dgamma": dg, "dbeta": db, "conv_dbias": cdb, "sc_sums": scs}
    ref = R.bn_bwd_ref(inp, "y" if mask == "bits" else mask, act_hi=act_hi, sums=sums, beta_acc=beta_acc,
                       dgamma_old=olds[0], dbeta_old=olds[1], sc=sc)
    return out, ref


def _one_mode(form, kind, shape, calls, mode):
    inp, d = inputs(kind, shape)
    exact = kind == "exact"
    n0 = len(calls.backward())
    # beta_acc = 0 onto NaN-filled dgamma / dbeta (and NaN-filled dz, g_out, sc_sums), conv_dbias filled
    # with 7, the data's own sums handed in; then beta_acc = 0.5, no conv_dbias, unrelated sums handed in
    for beta_acc, flavour, with_dbias, fill in ((0.0, "own", True, NAN), (0.5, "other", False, 7.0)):
        out, ref = run_form(form, inp, d, beta_acc, flavour, with_dbias, fill)
        label = "form=%s set=%s shape=%dx%dx%d mode=%s beta_acc=%g" % ((form, kind) + shape + (mode, beta_acc))
        R.check(out, ref, exact, label)
        for k in ("dgamma", "dbeta"):
            assert bool(torch.isfinite(out[k]).all()), k
    assert calls.backward()[n0:] == [FORMS[form][0]] * 2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids())
@pytest.mark.parametrize("form", list(FORMS))
def test_form_against_fp64(form, shape, kind, monkeypatch):
    from cvlite import ops_nn as nn
    calls = Calls(monkeypatch)
    if FORMS[form][3] != "acc":
        _one_mode(form, kind, shape, calls, "-")
        return
    try:                                   # the handed sums travel as a BN accumulator buffer: both modes
        for on in (False, True):
            nn.set_bn_exact(on)
            assert nn.acc_slots() == (nn.ACC_SLOTS if on else 1)
            _one_mode(form, kind, shape, calls, "exact" if on else "f64")
    finally:
        nn.set_bn_exact(False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_y", [True, False], ids=["y", "no_y"])
@pytest.mark.parametrize("group", R.GROUPS)
def test_grouped_against_fp64(group, with_y, kind, monkeypatch):
    """cvl_bn_backward_grouped: a short last group (group 2 of 5 images), dz_beta 0 onto NaN, 0 and 1."""
    from cvlite import ops_nn as nn
    shape = R.GROUPED_SHAPE
    inp, d = inputs(kind, shape)
    B, HW, C = shape
    dev = d["dy"].device
    calls = Calls(monkeypatch)
    mask = "y" if with_y else "none"
    dzo = R.old_dz(inp)
    for dz_beta, prefill in ((0.0, None), (0.0, dzo), (1.0, dzo)):
        dz = torch.full_like(d["dy"], NAN) if prefill is None else prefill.to(dev).clone()
        dg, db = torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
        nn.bn_backward_grouped(d["dy"], d["z"], d["mr"], d["gamma"], dz, dg, db, B, HW, C, group, dz_beta,
                               d["y"] if with_y else None)
        torch.cuda.synchronize()
        ref = R.bn_bwd_ref(inp, mask, group=group, dz_beta=dz_beta, dz_old=dzo)
        label = "form=grouped set=%s shape=%dx%dx%d mode=group%d%s beta_acc=0 dz_beta=%g" % (
            (kind,) + shape + (group, "y" if with_y else "", dz_beta))
        R.check({"dz": dz, "dgamma": dg, "dbeta": db}, ref, kind == "exact", label)
    assert calls.backward() == ["cvl_bn_backward_grouped"] * 3


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids())
def test_grouped_every_geometry(shape, kind):
    """The grouped form (run-time mask selection, pass 1 on pass 0's chunking) at the shapes of the other
    twelve: groups of two images (B = 1: one short group; B = 3: 2 + 1), accumulating onto dz."""
    from cvlite import ops_nn as nn
    inp, d = inputs(kind, shape)
    B, HW, C = shape
    dev = d["dy"].device
    dzo = R.old_dz(inp)
    dz = dzo.to(dev).clone()
    dg, db = torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
    nn.bn_backward_grouped(d["dy"], d["z"], d["mr"], d["gamma"], dz, dg, db, B, HW, C, 2, 1.0, d["y"])
    torch.cuda.synchronize()
    ref = R.bn_bwd_ref(inp, "y", group=2, dz_beta=1.0, dz_old=dzo)
    R.check({"dz": dz, "dgamma": dg, "dbeta": db}, ref, kind == "exact",
            "form=grouped set=%s shape=%dx%dx%d mode=group2y beta_acc=0 dz_beta=1" % ((kind,) + shape))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", R.SHAPES + [R.GROUPED_SHAPE], ids=R.ids(R.SHAPES + [R.GROUPED_SHAPE]))
def test_bn_stats_against_fp64(shape, kind):
    """bn_stats (PASS 2): (sum x, sum x^2) exact on the exact set, within (HW + 3) u sum |t| on the random
    one, under both accumulator modes."""
    from cvlite import ops_nn as nn
    inp, d = inputs(kind, shape)
    B, HW, C = shape
    S, bound = R.stats_ref(inp["dy"])
    try:
        for on in (False, True):
            nn.set_bn_exact(on)
            acc = nn.bn_acc(B, C, d["dy"].device)
            nn.bn_stats(d["dy"], B, HW, C, acc)
            got = nn.bn_acc_value(acc).cpu()
            err = (got - S).abs()
            print("form=bn_stats set=%s shape=%dx%dx%d mode=%s S=%.3g" % ((kind,) + shape + (
                "exact" if on else "f64", R._ratio(err, bound))))
            if kind == "exact":
                assert torch.equal(got, S)
            else:
                assert bool((err <= bound).all())
    finally:
        nn.set_bn_exact(False)


# ---- writes stay inside their buffers (the C ABI, outputs and workspace between guard bytes) ----------
PAD = 208          # 16-byte aligned (the kernels' vector accesses), not a multiple of the allocator's granule


class Guarded(object):
    """`nbytes` usable bytes in the middle of a 0xA5-filled buffer."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.big = torch.full((self.n + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.ptr = self.big.data_ptr() + PAD
        assert self.ptr % 16 == 0

    def view(self, dtype, shape):
        return self.big[PAD:PAD + self.n].view(dtype).view(shape)

    def intact(self):
        return bool((self.big[:PAD] == 0xA5).all()) and bool((self.big[PAD + self.n:] == 0xA5).all())


@pytest.mark.parametrize("shape", [(2, 9, 2048), (2, 700, 24)], ids=["2x9x2048", "2x700x24"])
@pytest.mark.parametrize("entry", ["cvl_bn_backward_sc", "cvl_bn_backward_res_sums_sc", "cvl_bn_backward_grouped"])
def test_c_entry_writes_stay_inside(entry, shape):
    from cvlite import _lib, ops_nn as nn
    inp, d = inputs("random", shape)
    B, HW, C = shape
    dev = d["dy"].device
    p = lambda t: t.data_ptr()
    nws = int(getattr(_lib.load(), entry + "_workspace_size")(B, HW, C))
    assert nws > 0
    ws, dz, go, scs = Guarded(nws), Guarded(B * HW * C * 2), Guarded(B * HW * C * 2), Guarded(B * C * 2 * 8)
    dg, db, cdb = (torch.zeros(C, device=dev) for _ in range(3))
    y = d["y"].clone()
    sums = R.handed_sums(inp, "own", "y")

    def launch(nbytes):
        if entry == "cvl_bn_backward_sc":
            _lib.call(entry, p(d["dy"]), p(y), p(d["z"]), p(d["mr"]), p(d["gamma"]), ws.ptr, nbytes, dz.ptr, go.ptr,
                      p(dg), p(db), 0.0, p(cdb), p(d["z_sc"]), p(d["mr_sc"]), scs.ptr, B, HW, C, _lib.stream())
        elif entry == "cvl_bn_backward_res_sums_sc":
            hs = nn.bn_acc_encode(sums.to(dev))
            _lib.call(entry, p(d["dy"]), p(y), p(d["z"]), p(d["mr"]), p(d["gamma"]), nn.acc_ptr(hs), dz.ptr, go.ptr,
                      p(dg), p(db), 0.0, p(cdb), p(d["z_sc"]), p(d["mr_sc"]), ws.ptr, nbytes, scs.ptr, B, HW, C,
                      _lib.stream())
        else:
            _lib.call(entry, p(d["dy"]), p(y), p(d["z"]), p(d["mr"]), p(d["gamma"]), ws.ptr, nbytes, dz.ptr, 0.0,
                      p(dg), p(db), B, HW, C, 2, _lib.stream())
        torch.cuda.synchronize()

    # a workspace one byte short is refused before anything is enqueued
    with pytest.raises(_lib.CvlError):
        launch(nws - 1)
    for g in (ws, dz, go, scs):
        assert bool((g.big == 0xA5).all())
    launch(nws)
    for name, g in (("workspace", ws), ("dz", dz), ("g_out", go), ("sc_sums", scs)):
        assert g.intact(), name
    grouped = entry == "cvl_bn_backward_grouped"
    ref = R.bn_bwd_ref(inp, "y", sums=sums if "res_sums" in entry else None, group=2 if grouped else 1,
                       sc=not grouped)
    out = {"dz": dz.view(BF, (B, HW, C)), "dgamma": dg, "dbeta": db}
    if grouped:                              # takes neither g_out nor sc_sums: both buffers stay untouched
        assert bool((go.big == 0xA5).all()) and bool((scs.big == 0xA5).all())
    else:
        out.update(g_out=go.view(BF, (B, HW, C)), sc_sums=scs.view(F64, (B, C, 2)), conv_dbias=cdb)
    R.check(out, ref, False, "form=guard:%s set=random shape=%dx%dx%d mode=- beta_acc=0" % ((entry,) + shape))


# ---- the forward side ------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("relu", [0, 1, 2])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids())
def test_bn_apply_exact_set(shape, relu, residual):
    """On the exact set bn(z) [+ r] is exact in fp32 and in bf16: y equals the reference bit for bit."""
    from cvlite import ops_nn as nn
    inp, d = inputs("exact", shape)
    B, HW, C = shape
    y = torch.full_like(d["z"], NAN)
    nn.bn_apply(d["z"], d["mr"], d["gamma"], d["beta"], d["r"] if residual else None, y, B, HW, C, relu)
    torch.cuda.synchronize()
    ref = R.bn_apply_ref(inp, residual, relu)
    assert torch.equal(y.cpu().float(), ref.float())
    assert torch.equal(y.cpu().view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("with_bits", [False, True], ids=["y", "bits"])
@pytest.mark.parametrize("shape", [(2, 700, 24), (3, 130, 1280), (2, 9, 2048)], ids=["2x700x24", "3x130x1280", "2x9x2048"])
def test_finalize_apply_equals_two_launches(shape, with_bits):
    """bn_finalize_apply[_bits] == bn_finalize + bn_apply bit for bit at widths where C/8 does not divide
    the block (3 and 160 threads per row) and at one row per pass; the bitmap equals y > 0."""
    from cvlite import ops_nn as nn
    inp, d = inputs("random", shape)
    B, HW, C = shape
    dev = d["z"].device
    zd = inp["z"].to(F64)
    st = nn.bn_acc_encode(torch.stack([zd.sum(1), (zd * zd).sum(1)], -1)).to(dev)
    eps, mom = 1.001e-5, 0.99
    res = []
    for fused in (True, False):
        y = torch.full_like(d["z"], NAN)
        mr = torch.full((B, C, 2), NAN, device=dev)
        rm, rv = torch.full((C,), 0.25, device=dev), torch.full((C,), 1.5, device=dev)
        if fused:
            if with_bits:
                assert nn.attach_relu_bits(y) is not None
            nn.bn_finalize_apply(st.clone(), mr, rm, rv, d["z"], d["gamma"], d["beta"], d["r"], y, B, HW, C, 1, eps, mom)
        else:
            nn.bn_finalize(st.clone(), mr, rm, rv, B, C, HW, eps, mom)
            nn.bn_apply(d["z"], mr, d["gamma"], d["beta"], d["r"], y, B, HW, C, 1)
        res.append((y, mr, rm, rv))
    torch.cuda.synchronize()
    (y, mr, rm, rv), (y0, mr0, rm0, rv0) = res
    assert bool(torch.isfinite(y0.float()).all()) and float(y0.float().max()) > 0
    assert torch.equal(y.view(torch.int16), y0.view(torch.int16))
    assert torch.equal(mr, mr0) and torch.equal(rm, rm0) and torch.equal(rv, rv0)
    if with_bits:
        assert torch.equal(R.unpack_bits(nn.relu_bits(y), y.shape), y.float() > 0)
