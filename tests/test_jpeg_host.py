"""Host half of the JPEG decoder (csrc/jpeg_host.h behind cvl_jpeg_info / cvl_jpeg_entropy_decode):
CPU only.  The entropy decode, followed by the numpy restatement below of the GPU half's integer
arithmetic (include/cvlite.h "JPEG decode"; libjpeg's islow IDCT, fancy upsampling, YCbCr->RGB),
gives exactly the bytes of PIL's Image.open(...).convert("RGB")."""
import ctypes
import io

import numpy as np
import pytest

CVL_OK, CVL_EINVAL, UNSUPPORTED, CORRUPT = 0, 1, 2, 3
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
LUMA = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "grey": (1, 1)}


# ---- test files: seeded smooth gradients plus noise, encoded by Pillow -----------------------------
def make_image(w, h, seed, grey=False):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for c in range(1 if grey else 3):
        g = 128 + 100 * np.sin((xx * (c + 1) + yy * (3 - c)) / (4.0 + w / 7.0) + c) + rng.normal(0, 12, (h, w))
        chans.append(np.clip(g, 0, 255))
    a = np.stack(chans, -1).astype(np.uint8)
    return a[..., 0] if grey else a


def encode(w, h, sampling="420", quality=90, seed=0, **kw):
    from PIL import Image
    grey = sampling == "grey"
    im = Image.fromarray(make_image(w, h, seed, grey))
    buf = io.BytesIO()
    if grey:
        im.save(buf, "JPEG", quality=quality, **kw)
    else:
        im.save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[sampling], **kw)
    return buf.getvalue()


def pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


SIZES = [(8, 8), (9, 7), (17, 23), (33, 50)]
MATRIX = [(w, h, s, q) for (w, h) in SIZES for s in ("444", "422", "420", "grey") for q in (50, 95)]
EXTRAS = [("optimize", 33, 50, "420", dict(optimize=True)),
          ("restart_blocks", 33, 50, "420", dict(restart_marker_blocks=1)),
          ("restart_rows", 33, 50, "422", dict(restart_marker_rows=1))]


def supported_files():
    out = [("%dx%d-%s-q%d" % (w, h, s, q), encode(w, h, s, q, seed=w * 100 + h), (w, h, s, 0))
           for (w, h, s, q) in MATRIX]
    for name, w, h, s, kw in EXTRAS:
        mcux = -(-w // (8 * LUMA[s][0]))
        ri = 1 if "restart_marker_blocks" in kw else (mcux if "restart_marker_rows" in kw else 0)
        out.append((name, encode(w, h, s, 90, seed=7, **kw), (w, h, s, ri)))
    return out


@pytest.fixture(scope="module")
def files():
    return supported_files()


# ---- ctypes access to the two host-only entries ------------------------------------------------------
def jpeg_info(data):
    from cvlite import _lib
    info = (ctypes.c_int32 * 8)()
    st = _lib.load().cvl_jpeg_info(ctypes.c_char_p(data), len(data), info)
    assert st == info[0]
    return list(info)


def entropy_decode(data, cap=None):
    """(status, coef int16 [count], qt uint16 [3][64]); cap overrides the capacity passed."""
    from cvlite import _lib
    info = jpeg_info(data)
    count = info[7] if cap is None else cap
    coef = np.full(max(count, 1), 0x7abc, np.int16)
    guard = np.full(64, 0x7abc, np.int16)                  # the words after the capacity stay untouched
    buf = np.concatenate([coef, guard])
    qt = np.zeros((3, 64), np.uint16)
    st = _lib.load().cvl_jpeg_entropy_decode(ctypes.c_char_p(data), len(data), buf.ctypes.data, count, qt.ctypes.data)
    assert (buf[max(count, 1):] == 0x7abc).all()
    return st, buf[:count], qt


# ---- numpy restatement of the GPU half (int32 arithmetic, arithmetic shifts) -------------------------
def _idct8(x):
    c0_298, c0_390, c0_541, c0_765, c0_899, c1_175 = 2446, 3196, 4433, 6270, 7373, 9633
    c1_501, c1_847, c1_961, c2_053, c2_562, c3_072 = 12299, 15137, 16069, 16819, 20995, 25172
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., i] for i in range(8))
    z1 = (x2 + x6) * c0_541
    t2 = z1 - x6 * c1_847
    t3 = z1 + x2 * c0_765
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * c1_175
    a0, a1, a2, a3 = a0 * c0_298, a1 * c2_053, a2 * c3_072, a3 * c1_501
    z1 = z1 * -c0_899
    z2 = z2 * -c2_562
    z3 = z3 * -c1_961 + z5
    z4 = z4 * -c0_390 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], -1)


def _plane(coef, qt, bh, bw):
    """[bh*bw][64] coefficients -> uint8 plane [bh*8][bw*8]."""
    blk = coef.reshape(bh, bw, 8, 8).astype(np.int32) * qt.reshape(8, 8).astype(np.int32)
    cols = _idct8(np.swapaxes(blk, -1, -2))                # pass 1 over columns: [.., col, out_row]
    ws = np.swapaxes((cols + (1 << 10)) >> 11, -1, -2)
    px = np.clip(((_idct8(ws) + (1 << 17)) >> 18) + 128, 0, 255)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _upsample(p, hs, vs, W, H):
    """Fancy upsampling of the chroma plane p (already cropped to dw x dh) to at least H x W."""
    p = p.astype(np.int32)
    dh, dw = p.shape
    if hs == 1:
        return p
    if dw <= 2:                                            # libjpeg replicates planes this narrow
        return np.repeat(np.repeat(p, vs, 0), 2, 1)
    if vs == 1:
        T = [p]
        lo_round, hi_round, shift = 1, 2, 2
    else:
        up = np.concatenate([p[:1], p[:-1]], 0)
        dn = np.concatenate([p[1:], p[-1:]], 0)
        T = [3 * p + up, 3 * p + dn]                       # output rows 2r, 2r + 1
        lo_round, hi_round, shift = 8, 7, 4
    outs = []
    for t in T:
        left = np.concatenate([t[:, :1], t[:, :-1]], 1)
        right = np.concatenate([t[:, 1:], t[:, -1:]], 1)
        o = np.empty((dh, 2 * dw), np.int32)
        o[:, 0::2] = (3 * t + left + lo_round) >> shift
        o[:, 1::2] = (3 * t + right + hi_round) >> shift
        outs.append(o)
    if vs == 1:
        return outs[0]
    o = np.empty((2 * dh, 2 * dw), np.int32)
    o[0::2], o[1::2] = outs
    return o


def restated_rgb(info, coef, qt):
    _, W, H, nc, hs, vs, _, count = info
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    dims = [(mcuy * vs, mcux * hs)] + [(mcuy, mcux)] * (nc - 1)
    assert sum(a * b for a, b in dims) * 64 == count
    planes, o = [], 0
    for c, (bh, bw) in enumerate(dims):
        planes.append(_plane(coef[o:o + bh * bw * 64], qt[c], bh, bw))
        o += bh * bw * 64
    Y = planes[0][:H, :W].astype(np.int32)
    if nc == 1:
        return np.repeat(Y[..., None], 3, -1).astype(np.uint8)
    dw, dh = -(-W // hs), -(-H // vs)
    cb = _upsample(planes[1][:dh, :dw], hs, vs, W, H)[:H, :W] - 128
    cr = _upsample(planes[2][:dh, :dw], hs, vs, W, H)[:H, :W] - 128
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ---- tests ---------------------------------------------------------------------------------------------
def test_info_reports_size_sampling_restart(files):
    for name, data, (w, h, s, ri) in files:
        info = jpeg_info(data)
        hs, vs = LUMA[s]
        nc = 1 if s == "grey" else 3
        mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
        blocks = mcux * mcuy * (hs * vs + nc - 1)
        assert info == [CVL_OK, w, h, nc, hs, vs, ri, blocks * 64], name


def test_entropy_decode_then_restatement_equals_pillow(files):
    for name, data, _ in files:
        st, coef, qt = entropy_decode(data)
        assert st == CVL_OK, name
        got = restated_rgb(jpeg_info(data), coef, qt)
        ref = pil_rgb(data)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))


def test_narrow_chroma_planes_are_replicated():
    """Chroma planes of at most two columns (width <= 4 at 4:2:x) take libjpeg's plain replication,
    not the triangle filter: the restatement (and the kernel) branch on it."""
    for (w, h, s) in [(3, 5, "420"), (4, 9, "422"), (1, 1, "420"), (2, 17, "420"), (5, 3, "420")]:
        data = encode(w, h, s, 90, seed=w + h)
        st, coef, qt = entropy_decode(data)
        assert st == CVL_OK
        assert np.array_equal(restated_rgb(jpeg_info(data), coef, qt), pil_rgb(data)), (w, h, s)


def _bad_inputs():
    from PIL import Image
    rgb = Image.fromarray(make_image(33, 50, 1))
    out = {}
    b = io.BytesIO(); rgb.save(b, "JPEG", progressive=True); out["progressive"] = (b.getvalue(), UNSUPPORTED)
    b = io.BytesIO(); rgb.convert("CMYK").save(b, "JPEG"); out["cmyk"] = (b.getvalue(), UNSUPPORTED)
    b = io.BytesIO(); rgb.save(b, "PNG"); out["png"] = (b.getvalue(), UNSUPPORTED)
    out["empty"] = (b"", UNSUPPORTED)
    out["random"] = (np.random.default_rng(5).integers(0, 256, 64, dtype=np.uint8).tobytes(), UNSUPPORTED)
    return out


def test_unsupported_inputs_return_their_status():
    for name, (data, want) in _bad_inputs().items():
        info = jpeg_info(data)
        assert info[0] == want and info[1:] == [0] * 7, name
        st, _, _ = entropy_decode(data, cap=64)
        assert st == want, name


def test_truncated_files_are_corrupt_not_crashes(files):
    for name, data, _ in files:
        full = jpeg_info(data)[7]
        for frac in (0.25, 0.5, 0.9):
            cut = data[:int(len(data) * frac)]
            st, _, _ = entropy_decode(cut, cap=full)
            assert st in (UNSUPPORTED, CORRUPT), (name, frac, st)
            if jpeg_info(cut)[0] == CVL_OK:                 # the cut fell inside the scan
                assert st == CORRUPT, (name, frac)


def test_small_coef_cap_is_rejected(files):
    for name, data, _ in files[:4] + files[-3:]:
        full = jpeg_info(data)[7]
        for cap in (0, 64, full - 64, full - 1):
            st, _, _ = entropy_decode(data, cap=cap)
            assert st == CVL_EINVAL, (name, cap)
