"""GPU parity of the X-ring weight gradient's read placement (csrc/conv_wgrad_x.hip, template RD):
the loop that issues step t+1's fragment reads one per MFMA gap must write, bit for bit, what the
first placement (CVL_DISPATCH=wgx_reads=0) writes -- every accumulator sees the same steps and 32-row
sub-steps in the same order -- and both must agree with a float64 reference on the same bf16
operands at the bound tests/test_gpu_wgrad_batch.py uses: max |got - ref| <= 2e-5 x max |ref|.

The key is read by the launch planner at every call, so both forms run in one process.

Cases (the smallest at which the loop's bookkeeping can go wrong):
  tower_small  grouped 3x3 256->256, 2 groups, B 2, levels 16 / 8 / 4: padding taps, segment seeks,
               segments shorter than one 128-row chunk; one split per group, so dW is written
               directly (also run with beta = 1).  The planner runs it on the 128-wide tile.
  tower_256    the same with a 64 x 64 level in front and B 4: the fewest rows at which the planner
               picks the 256-wide tile (18 tiles x 14 splits fill the CUs; slabs + reducer), the
               instantiation the FCOS towers run.
  1x1_1024     1x1 1024->256 @ 8 x 8, B 16: 1024 rows, the 128-wide tile with 64-row steps.
  1x1_2688     the same with B 42: five splits of 640 rows, the last one a single 128-row chunk.
  batch        three problems per tile width in one batched call, one stride-2 1x1 on each width.

Step counts: chunks and segments are 128-row aligned (kWgSegM), so a split runs a multiple of four
32-row steps on the 256-wide tile and of two 64-row steps on the 128-wide tile: the pstep(0) /
pstep(1) pair always ends on pstep(1), and 1- or 3-step splits (or an odd step count) do not occur
in the product library.  The shortest split there is, one 128-row chunk (the tail of 1x1_2688), is
two 64-row steps: fewer than the three steps the prologue issues ahead."""
import pytest
import torch

import wgrad_dispatch_cases as wc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
TOL = 2e-5


def _close(got, ref):
    err = float((got.double() - ref).abs().max())
    return err <= TOL * float(ref.abs().max()), err


def _ref_conv(x, dy, k, stride):
    """float64 dW [k][k][cin][cout] of one map: x (B, H, W, cin), dy (B, Ho, Wo, cout), pad k // 2."""
    pad = k // 2
    Ho = dy.shape[1]
    cin, cout = x.shape[-1], dy.shape[-1]
    xp = torch.nn.functional.pad(x.double(), (0, 0, pad, pad, pad, pad))
    ref = torch.zeros((k, k, cin, cout), dtype=F64, device=x.device)
    dyf = dy.double().reshape(-1, cout)
    for r in range(k):
        for s in range(k):
            patch = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Ho - 1) + 1:stride, :]
            ref[r, s] = patch.reshape(-1, cin).t() @ dyf
    return ref.reshape(-1)


def _tower(maps, B=2, cin=256, cout=256, ngroups=2, seed=11):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    d, x, dy = wc._multi(gen, "cuda", B, maps, ngroups, cin, cout, cout, 3)
    refs, row = [], 0
    for g in range(ngroups):
        ref = torch.zeros(9 * cin * cout, dtype=F64, device="cuda")
        for h in maps:
            n = B * h * h
            ref += _ref_conv(x[row:row + n].reshape(B, h, h, cin), dy[row:row + n].reshape(B, h, h, cout), 3, 1)
            row += n
        refs.append(ref)
    return d, x, dy, refs


def _single(B, H, stride, cin, cout, gen):
    from cvlite import ops_nn as nn
    Ho = (H + stride - 1) // stride
    x = (torch.randn((B, H, H, cin), generator=gen, device="cuda") * 0.5).to(BF)
    dy = (torch.randn((B, Ho, Ho, cout), generator=gen, device="cuda") * 0.5).to(BF)
    npad = (cout + 63) // 64 * 64
    w = torch.zeros((npad, cin), dtype=BF, device="cuda")
    d = nn.make_desc(nn.FWD, B, cin, 1, 1, stride, 0, 0, npad, cout, cout, [nn.seg(Ho, Ho, H, H, w, None)])
    return d, x, dy, _ref_conv(x, dy, 1, stride)


@pytest.fixture(scope="module")
def towers():
    return {"tower_small": _tower([16, 8, 4]), "tower_256": _tower([64, 16, 8, 4], B=4)}


@pytest.fixture(scope="module")
def singles():
    gen = torch.Generator(device="cuda").manual_seed(5)
    return {"1x1_1024": _single(16, 8, 1, 1024, 256, gen), "1x1_2688": _single(42, 8, 1, 1024, 256, gen)}


# (B, H, stride, Cin, Cout): 256-wide tiles where Npad % 256 == 0 and Cin >= 256, else 128-wide
BATCH = [(16, 8, 1, 1024, 256), (4, 32, 2, 512, 1024), (5, 16, 1, 256, 512),
         (4, 16, 1, 256, 64), (4, 32, 2, 64, 256), (2, 32, 1, 128, 128)]


@pytest.fixture(scope="module")
def batch():
    gen = torch.Generator(device="cuda").manual_seed(9)
    return [_single(*p, gen) for p in BATCH]


def _both_forms(dispatch, run):
    """run() under the default read placement and under wgx_reads=0"""
    new = run()
    dispatch("wgx_reads=0")
    old = run()
    torch.cuda.synchronize()
    return new, old


def _run_tower(case, beta=0.0, fill=float("nan")):
    from cvlite import ops_nn as nn
    d, x, dy, refs = case
    dws = [torch.full((r.numel(),), fill, dtype=torch.float32, device="cuda") for r in refs]
    nn.conv_wgrad_grouped(d, x, dy, dws, beta)
    return dws


@pytest.mark.parametrize("name,tile,split", [("tower_small", 128, False), ("tower_256", 256, True)])
def test_tower_forms_bit_identical_and_match_float64(name, tile, split, towers, dispatch):
    from cvlite import _lib
    case = towers[name]
    st, kern, t, nsplit, nbytes = wc.plan(_lib.load(), case[0], 2)
    print(name, "plan: kernel", kern, "tile", t, "nsplit", nsplit)
    assert (st, kern, t) == (0, wc.WG_X, tile) and (nsplit > 1) == split
    new, old = _both_forms(dispatch, lambda: _run_tower(case))
    for g, (a, b, ref) in enumerate(zip(new, old, case[3])):
        assert torch.equal(a, b), "group %d: the two read placements differ" % g
        for form, got in (("default", a), ("wgx_reads=0", b)):
            ok, err = _close(got, ref)
            print(name, "group", g, form, "max err %.3g of %.3g" % (err, float(ref.abs().max())))
            assert ok, "%s group %d %s: max err %.3g" % (name, g, form, err)


def test_direct_write_with_beta(towers, dispatch):
    """one split per group: the kernel's epilogue adds beta x dW itself"""
    case = towers["tower_small"]
    new, old = _both_forms(dispatch, lambda: _run_tower(case, beta=1.0, fill=0.5))
    for a, b, ref in zip(new, old, case[3]):
        assert torch.equal(a, b)
        ok, err = _close(a, ref + 0.5)
        assert ok, "max err %.3g" % err


@pytest.mark.parametrize("name,splits", [("1x1_1024", None), ("1x1_2688", 5)])
def test_1x1_forms_bit_identical_and_match_float64(name, splits, singles, dispatch):
    from cvlite import _lib, ops_nn as nn
    d, x, dy, ref = singles[name]
    st, kern, t, nsplit, nbytes = wc.plan(_lib.load(), d, 1)
    print(name, "plan: kernel", kern, "tile", t, "nsplit", nsplit)
    assert (st, kern, t) == (0, wc.WG_X, 128) and splits in (None, nsplit)

    def run():
        dw = torch.full((ref.numel(),), float("nan"), dtype=torch.float32, device="cuda")
        nn.conv_wgrad(d, x, dy, dw)
        return dw

    new, old = _both_forms(dispatch, run)
    assert torch.equal(new, old)
    for form, got in (("default", new), ("wgx_reads=0", old)):
        ok, err = _close(got, ref)
        print(name, form, "max err %.3g of %.3g" % (err, float(ref.abs().max())))
        assert ok, "%s %s: max err %.3g" % (name, form, err)


def test_batch_forms_bit_identical_and_match_float64(batch, dispatch):
    from cvlite import _lib, ops_nn as nn
    descs = [c[0] for c in batch]
    st, kern, launch, nsplit = wc.batch_plan(_lib.load(), descs)
    print("batch plan: kernel", kern, "launch", launch, "nsplit", nsplit)
    assert st == 0 and kern == [wc.WG_X] * len(BATCH)
    assert len(set(launch[:3])) == 1 and len(set(launch[3:])) == 1 and launch[0] != launch[3]   # one launch per width

    def run():
        dws = [torch.full((c[3].numel(),), float("nan"), dtype=torch.float32, device="cuda") for c in batch]
        nn.conv_wgrad_batch(descs, [c[1] for c in batch], [c[2] for c in batch], dws)
        return dws

    new, old = _both_forms(dispatch, run)
    for i, (a, b, c) in enumerate(zip(new, old, batch)):
        assert torch.equal(a, b), "problem %d %s: the two read placements differ" % (i, BATCH[i])
        for form, got in (("default", a), ("wgx_reads=0", b)):
            ok, err = _close(got, c[3])
            assert ok, "problem %d %s %s: max err %.3g" % (i, BATCH[i], form, err)


def test_run_twice_deterministic(towers):
    case = towers["tower_256"]
    first = _run_tower(case)
    second = _run_tower(case)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
