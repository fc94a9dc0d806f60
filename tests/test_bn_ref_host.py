"""The BatchNorm-backward checker of tests/bn_ref.py has teeth (no GPU): an fp32 restatement of the
kernel arithmetic passes every derived bound under the least favourable summation order (one chain per
(image, channel)) and under a chunked one, and is exact on the exact input set; each defect a rewrite
could have -- a dropped or doubled row in the sums, HW - 1 in the divisor, >= in the mask, an unwritten
last channel group -- fails the checker on a small shape; and the margin redraw of the random set leaves
no mask bit on which fp32 and float64 disagree."""
import pytest
import torch

import bn_ref as R

KINDS = ("exact", "random")
# (name, mask, act_hi, handed sums flavour, sc): the arithmetic classes of the thirteen forms
FORMS = [("y", "y", R.INF, None, False), ("relu", "z", R.INF, None, False), ("relu6", "z", 6.0, None, False),
         ("none", "none", R.INF, None, False), ("sc", "y", R.INF, None, True),
         ("res_sums_sc", "y", R.INF, "own", True), ("relu6_sums", "z", 6.0, "other", False),
         ("sums", "none", R.INF, "other", False)]


def _run(inp, form, order, mutate=None, beta_acc=0.0, group=1, dz_beta=0.0):
    name, mask, act_hi, flavour, sc = form
    exact = inp["kind"] == "exact"
    sums = R.handed_sums(inp, flavour, mask, act_hi) if flavour else None
    olds = R.old_params(inp) if beta_acc else (None, None)
    dzo = R.old_dz(inp) if dz_beta else None
    kw = dict(act_hi=act_hi, sums=sums, group=group, dz_beta=dz_beta, dz_old=dzo, beta_acc=beta_acc,
              dgamma_old=olds[0], dbeta_old=olds[1], sc=sc)
    ref = R.bn_bwd_ref(inp, mask, **kw)
    out = R.bn_bwd_f32(inp, mask, order=order, mutate=mutate, **kw)
    return R.check(out, ref, exact, "%s %s %s %s" % (name, inp["kind"], order, mutate or "-"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids())
def test_restatement_passes_every_bound(shape, kind):
    inp = R.make_inputs(kind, *shape)
    for form in FORMS:
        for order in ("chain", "chunked"):
            for beta_acc in (0.0, 0.5):
                ratios = _run(inp, form, order, beta_acc=beta_acc)
                assert all(r <= 1.0 for r in ratios.values())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("group", R.GROUPS)
def test_restatement_grouped(group, kind):
    inp = R.make_inputs(kind, *R.GROUPED_SHAPE)
    for form in (FORMS[0], FORMS[3]):
        for dz_beta in (0.0, 1.0):
            _run(inp, form, "chain", group=group, dz_beta=dz_beta)


def test_exact_set_is_order_independent():
    """The exact set's claim itself: sums formed as one chain and as chunks are the same bits."""
    for shape in R.SHAPES:
        inp = R.make_inputs("exact", *shape)
        a = R.bn_bwd_f32(inp, "z", act_hi=6.0, sc=True, order="chain")
        b = R.bn_bwd_f32(inp, "z", act_hi=6.0, sc=True, order="chunked", chunk=5)
        for k in ("S", "sc_sums", "dgamma", "dbeta"):
            assert torch.equal(a[k], b[k]), (shape, k)
        a6 = R.bn64(inp["z"], inp["mr"], inp["gamma"], inp["beta"])
        assert int((a6 == 0).sum()) > 0 and int((a6 == 6).sum()) > 0, shape     # the thresholds are hit


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_each_mutation_is_caught(mutate):
    caught = []
    for shape in R.SMALL:
        for kind in KINDS:
            inp = R.make_inputs(kind, *shape)
            for form in (FORMS[0], FORMS[2]):
                try:
                    _run(inp, form, "chunked", mutate=mutate)
                except AssertionError as e:
                    caught.append((shape, kind, form[0], str(e)))
    print("%s: caught %d times, e.g. %s" % (mutate, len(caught), caught[:1]))
    assert caught
    # a defect of the sums shows on every small shape with more than one row, on both sets
    if mutate in ("drop_last_row", "double_last_row"):
        hit = {(s, k) for s, k, _, _ in caught}
        assert all((s, k) in hit for s in R.SMALL[1:] for k in KINDS)
    if mutate == "mask_ge":                  # breaks exactness on every exact-set shape
        assert all((s, "exact") in {(s, k) for s, k, _, _ in caught} for s in R.SMALL)


@pytest.mark.parametrize("shape", R.SHAPES + [R.GROUPED_SHAPE], ids=R.ids(R.SHAPES + [R.GROUPED_SHAPE]))
def test_margin_redraw_leaves_no_mask_disagreement(shape):
    inp = R.make_inputs("random", *shape)
    a = R.bn64(inp["z"], inp["mr"], inp["gamma"], inp["beta"])
    assert float(a.abs().min()) >= R.MARGIN and float((a - 6.0).abs().min()) >= R.MARGIN
    for act_hi in (R.INF, 6.0):
        assert R.mask_disagreements(inp, act_hi) == 0


def test_bits_roundtrip_and_stats_ref():
    inp = R.make_inputs("random", 2, 9, 2048)
    bits = R.pack_bits(inp["y"])
    assert bits.dtype == torch.uint8 and bits.numel() == 2 * 9 * 2048 // 8
    assert torch.equal(R.unpack_bits(bits, inp["y"].shape), inp["y"].float() > 0)
    S, b = R.stats_ref(inp["dy"])
    x = inp["dy"].float()
    chain = torch.stack([R._sum_rows32(x, "chain", 0), R._sum_rows32(x * x, "chain", 0)], -1)
    assert bool(((chain - S).abs() <= b).all())
