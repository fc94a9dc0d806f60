"""GPU parity of the halo weight gradient's step loop (csrc/conv_wgrad_h.hip, template RD): the
pipelined loop (a sub-step's fragments read under the previous sub-step's MFMAs, one barrier per
step, the DMA a whole step ahead behind an incremental cursor) must write, bit for bit, what the first
form (CVL_DISPATCH=wh_reads=0) writes -- every accumulator sees the same steps and 32-row sub-steps in
the same order -- and both must agree with a float64 reference on the same bf16 operands at the bound
tests/test_gpu_wgrad_batch.py uses: max |got - ref| <= 2e-5 x max |ref|.

The key is read by the launch planner at every call, so both forms run in one process.

Cases, all 3x3 / stride 1 / pad 1 with whole 128-row steps (map = width x height; the kernel is
specialised by width):
  16x8_b1    64 -> 64, B 1: one step in total: prologue and drain only.
  16x8_b3    64 -> 64, B 3: three steps, an odd count, each with its top and bottom image rows in the
             same stage; one chunk, so dW is written directly (also run with beta = 1).
  32x32_b2   64 -> 128, B 2: interior steps with neither border; the image boundary falls between
             two steps.
  128x8_b1   64 -> 64, B 1: one image row per step, the widest halo (pitch 144), top and bottom steps
             distinct.
  64x64_b1   128 -> 128, B 1: four tiles, two rows per step.
  32x12_b6   64 -> 64, B 6: 18 steps in splits of 5 / 5 / 5 / 3 (the last chunk shorter; slabs and
             the reducer); three steps per image, so the cursor wraps to the next image inside a chunk.
  padded     16x8_b3 with dY 64 columns inside rows of 160 at column 32.
  dy_stride  32x12_b6 with each image's dY rows 424 rows apart (dst_img > H x W: 40 unused rows
             behind every image), so the cursor's image wrap adds a non-zero dY step.
  batch      three problems of widths 16 / 32 / 64 and different channel counts in one WH launch.
  exact      32x12_b6 on integer operands in {-2 .. 2}: every sum is exact in fp32, so dW == the
             integer reference."""
import pytest
import torch

import wgrad_dispatch_cases as wc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
TOL = 2e-5

# name -> (B, map width, map height, Cin, Cout)
SHAPES = {"16x8_b1": (1, 16, 8, 64, 64), "16x8_b3": (3, 16, 8, 64, 64), "32x32_b2": (2, 32, 32, 64, 128),
          "128x8_b1": (1, 128, 8, 64, 64), "64x64_b1": (1, 64, 64, 128, 128), "32x12_b6": (6, 32, 12, 64, 64)}
BATCH = [(2, 16, 16, 128, 64), (1, 32, 32, 64, 128), (1, 64, 64, 64, 64)]


def _close(got, ref):
    err = float((got.double() - ref).abs().max())
    return err <= TOL * float(ref.abs().max()), err


def _ref(x, dy):
    """float64 dW [3][3][cin][cout]: x (B, H, W, cin), dy (B, H, W, cout), pad 1"""
    B, H, W, cin = x.shape
    cout = dy.shape[-1]
    xp = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
    dyf = dy.double().reshape(-1, cout)
    ref = torch.zeros((3, 3, cin, cout), dtype=F64, device=x.device)
    for r in range(3):
        for s in range(3):
            ref[r, s] = xp[:, r:r + H, s:s + W, :].reshape(-1, cin).t() @ dyf
    return ref.reshape(-1)


def _case(gen, B, W, H, cin, cout, ld=None, coff=0, ints=False, dimg=None):
    """(desc, x, dy buffer, float64 reference); dY is columns [coff, coff + cout) of rows of ld, an
    image's rows the first H x W of dimg"""
    from cvlite import ops_nn as nn
    ld = cout if ld is None else ld
    dimg = H * W if dimg is None else dimg

    def rnd(shape):
        if ints:
            return torch.randint(-2, 3, shape, generator=gen, device="cuda").to(BF)
        return (torch.randn(shape, generator=gen, device="cuda") * 0.5).to(BF)

    x, dyb = rnd((B, H, W, cin)), rnd((B, dimg, ld))
    w = torch.zeros((cout, 9 * cin), dtype=BF, device="cuda")
    d = nn.make_desc(nn.FWD, B, cin, 3, 3, 1, 1, 1, cout, cout, ld, [nn.seg(H, W, H, W, w, None, dst_img=dimg)],
                     dst_coff=coff)
    return d, x, dyb, _ref(x, dyb[:, :H * W, coff:coff + cout].reshape(B, H, W, cout))


@pytest.fixture(scope="module")
def cases():
    gen = torch.Generator(device="cuda").manual_seed(17)
    out = {k: _case(gen, *v) for k, v in SHAPES.items()}
    out["padded"] = _case(gen, *SHAPES["16x8_b3"], ld=160, coff=32)
    out["dy_stride"] = _case(gen, *SHAPES["32x12_b6"], dimg=32 * 12 + 40)
    out["exact"] = _case(gen, *SHAPES["32x12_b6"], ints=True)
    out["batch"] = [_case(gen, *p) for p in BATCH]
    return out


def _run(case, beta=0.0, fill=float("nan")):
    from cvlite import ops_nn as nn
    d, x, dy, ref = case
    dw = torch.full((ref.numel(),), fill, dtype=torch.float32, device="cuda")
    nn.conv_wgrad(d, x, dy, dw, beta)
    return dw


def _both_forms(dispatch, run):
    """run() under the default loop and under wh_reads=0"""
    new = run()
    dispatch("wh_reads=0")
    old = run()
    torch.cuda.synchronize()
    return new, old


def _plan(d):
    from cvlite import _lib
    st, kern, tile, nsplit, nbytes = wc.plan(_lib.load(), d, 1)
    assert (st, kern) == (0, wc.WG_H)
    return nsplit


# nsplit: what the planner makes of the shape (the chunks are whole steps: 128 rows)
@pytest.mark.parametrize("name,nsplit", [("16x8_b1", 1), ("16x8_b3", 1), ("32x32_b2", 4), ("128x8_b1", 2),
                                         ("64x64_b1", 8), ("32x12_b6", 4), ("padded", 1), ("dy_stride", 4)])
def test_forms_bit_identical_and_match_float64(name, nsplit, cases, dispatch):
    case = cases[name]
    got = _plan(case[0])
    print(name, "plan: nsplit", got)
    assert got == nsplit
    new, old = _both_forms(dispatch, lambda: _run(case))
    assert _plan(case[0]) == nsplit, "wh_reads changed the plan"
    assert torch.equal(new, old), "%s: the two loops differ" % name
    for form, dw in (("default", new), ("wh_reads=0", old)):
        ok, err = _close(dw, case[3])
        print(name, form, "max err %.3g of %.3g" % (err, float(case[3].abs().max())))
        assert ok, "%s %s: max err %.3g" % (name, form, err)


def test_last_chunk_shorter(cases):
    """32x12_b6: 18 steps in four chunks of 5, so the last one has 3.  The plan query reports the split
    count, not the chunk; with equal chunks and no empty split (nsplit = ceil(steps / chunk)), 5 is the
    only chunk that gives 4 splits of 18 steps (4 gives 5 splits, 6 gives 3).  That all 18 steps are
    summed exactly once is what the float64 and exact-integer cases of this shape check."""
    B, W, H = SHAPES["32x12_b6"][:3]
    steps = B * W * H // 128
    nsplit = _plan(cases["32x12_b6"][0])
    chunk = -(-steps // nsplit)
    assert (steps, nsplit, chunk) == (18, 4, 5) and steps - (nsplit - 1) * chunk == 3


@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_direct_write_with_beta(beta, cases, dispatch):
    """one chunk: the kernel's epilogue writes dW itself, adding beta x dW"""
    case = cases["16x8_b3"]
    assert _plan(case[0]) == 1
    new, old = _both_forms(dispatch, lambda: _run(case, beta=beta, fill=0.5))
    assert torch.equal(new, old)
    ok, err = _close(new, case[3] + 0.5 * beta)
    assert ok, "max err %.3g" % err


def test_batch_forms_bit_identical_and_match_float64(cases, dispatch):
    from cvlite import _lib, ops_nn as nn
    batch = cases["batch"]
    descs = [c[0] for c in batch]
    st, kern, launch, nsplit = wc.batch_plan(_lib.load(), descs)
    print("batch plan: kernel", kern, "launch", launch, "nsplit", nsplit)
    assert st == 0 and kern == [wc.WG_H] * len(BATCH) and len(set(launch)) == 1     # one WH launch

    def run():
        dws = [torch.full((c[3].numel(),), float("nan"), dtype=torch.float32, device="cuda") for c in batch]
        nn.conv_wgrad_batch(descs, [c[1] for c in batch], [c[2] for c in batch], dws)
        return dws

    new, old = _both_forms(dispatch, run)
    assert wc.batch_plan(_lib.load(), descs) == (st, kern, launch, nsplit), "wh_reads changed the plan"
    for i, (a, b, c) in enumerate(zip(new, old, batch)):
        assert torch.equal(a, b), "problem %d %s: the two loops differ" % (i, BATCH[i])
        for form, got in (("default", a), ("wh_reads=0", b)):
            ok, err = _close(got, c[3])
            assert ok, "problem %d %s %s: max err %.3g" % (i, BATCH[i], form, err)


def test_exact_on_small_integers(cases, dispatch):
    """operands in {-2 .. 2}: products and sums are integers below 2^24, exact in fp32 in any order"""
    case = cases["exact"]
    assert float(case[3].abs().max()) < 2 ** 24
    new, old = _both_forms(dispatch, lambda: _run(case))
    assert torch.equal(new.double(), case[3]) and torch.equal(old.double(), case[3])


def test_run_twice_deterministic(cases):
    case = cases["32x12_b6"]
    first, second = _run(case), _run(case)
    torch.cuda.synchronize()
    assert torch.equal(first, second)
