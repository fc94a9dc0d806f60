"""GPU half of the JPEG decoder (csrc/jpeg_decode.hip, cvlite/jpeg.py): every pixel equals PIL's
Image.open(...).convert("RGB"), through decode / decode_batch, the C entry, preprocess_data(decode="gpu")
and _raw_batch(jpeg_decode="gpu").  The files are generated with Pillow (tests/test_jpeg_host.py)."""
import ctypes
import io

import numpy as np
import pytest

from test_jpeg_host import encode, make_image, pil_rgb, supported_files

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return torch.from_numpy(a).cuda()


@pytest.fixture(scope="module")
def files():
    """(name, bytes, Pillow's pixels): the host test's matrix, one file of several MCU rows and more
    blocks than one workgroup takes, and one of real size."""
    out = [(name, data, pil_rgb(data)) for name, data, _ in supported_files()]
    for name, data in (("130x70-420", encode(130, 70, "420", 90, seed=3)),
                       ("375x500-420", encode(375, 500, "420", 90, seed=4))):
        out.append((name, data, pil_rgb(data)))
    return out


def _progressive():
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(make_image(40, 24, 9)).save(b, "JPEG", progressive=True)
    return b.getvalue()


def test_decode_equals_pillow(files):
    import torch
    from cvlite import jpeg
    for name, data, ref in files:
        got = jpeg.decode(data, strict=True)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == ref.shape, name
        assert torch.equal(got, _t(ref)), (name, int((got != _t(ref)).sum()))


def test_decode_batch_mixed_with_fallback(files):
    import torch
    from cvlite import _lib, jpeg
    by = {name: (data, ref) for name, data, ref in files}
    names = ["33x50-444-q50", "17x23-422-q95", "9x7-420-q50", "33x50-grey-q95", "130x70-420", "8x8-420-q95",
             "restart_blocks"]
    prog = _progressive()
    srcs = [by[n][0] for n in names[:3]] + [prog] + [by[n][0] for n in names[3:]]
    refs = [by[n][1] for n in names[:3]] + [pil_rgb(prog)] + [by[n][1] for n in names[3:]]
    assert len(srcs) == 8 and jpeg.info(prog).status == jpeg.UNSUPPORTED
    outs = jpeg.decode_batch(srcs)
    for k, (got, ref) in enumerate(zip(outs, refs)):
        assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, _t(ref)), k
    with pytest.raises(_lib.CvlError):
        jpeg.decode_batch(srcs, strict=True)
    with pytest.raises(_lib.CvlError):
        jpeg.decode(prog, strict=True)


def test_c_entry_writes_only_the_images(files):
    """Outputs pointed into a larger buffer pre-filled with a sentinel, at odd offsets: the bytes
    before, between and after the [H][W][3] images stay untouched; a skipped image writes nothing."""
    import torch
    from cvlite import _lib, jpeg
    by = {name: (data, ref) for name, data, ref in files}
    picks = ["17x23-420-q50", "9x7-422-q95", "33x50-444-q95", "8x8-grey-q50", "130x70-420"]
    datas = [by[n][0] for n in picks] + [_progressive()]
    refs = [by[n][1] for n in picks] + [np.zeros((24, 40, 3), np.uint8)]
    n = len(datas)
    gap, offs, o = 37, [], 13
    for r in refs:
        offs.append(o)
        o += r.size + gap
    big = torch.full((o + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    infos = [jpeg.info(d) for d in datas]
    counts = (ctypes.c_int32 * n)(*[i.coef_count for i in infos])
    sb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.call("cvl_jpeg_batch_sizes", counts, n, ctypes.byref(sb), ctypes.byref(wb))
    pinned = torch.empty(sb.value, dtype=torch.uint8).pin_memory()
    work = torch.empty(wb.value, dtype=torch.uint8, device="cuda")
    status = (ctypes.c_int32 * n)()
    _lib.call("cvl_jpeg_decode_batch", (ctypes.c_char_p * n)(*datas), (ctypes.c_size_t * n)(*[len(d) for d in datas]),
              n, (ctypes.c_void_p * n)(*[big.data_ptr() + f for f in offs]), pinned.data_ptr(), pinned.numel(),
              work.data_ptr(), work.numel(), status, _lib.stream())
    torch.cuda.synchronize()
    assert list(status) == [0] * (n - 1) + [jpeg.UNSUPPORTED]
    host = big.cpu().numpy()
    mask = np.ones(host.size, bool)
    for k, (f, r) in enumerate(zip(offs, refs)):
        if status[k] == 0:
            assert np.array_equal(host[f:f + r.size].reshape(r.shape), r), picks[k]
            mask[f:f + r.size] = False
    assert (host[mask] == 0xA5).all()
    # a staging buffer or workspace one byte short is refused before anything is enqueued
    with pytest.raises(_lib.CvlError):
        _lib.call("cvl_jpeg_decode_batch", (ctypes.c_char_p * n)(*datas),
                  (ctypes.c_size_t * n)(*[len(d) for d in datas]), n,
                  (ctypes.c_void_p * n)(*[big.data_ptr() + f for f in offs]), pinned.data_ptr(), sb.value - 1,
                  work.data_ptr(), work.numel(), status, _lib.stream())


def test_back_to_back_batches_reuse_staging(files):
    """Two decode_batch calls on one stream with no synchronisation between them, the second
    different and larger: the first batch's copy must have left the staging buffer before the
    second batch's host threads overwrite it."""
    import torch
    from cvlite import jpeg
    by = {name: (data, ref) for name, data, ref in files}
    first = ["375x500-420", "33x50-420-q95", "17x23-444-q50"]
    second = ["130x70-420", "375x500-420", "33x50-422-q50", "375x500-420", "9x7-grey-q95", "restart_rows"]
    a = jpeg.decode_batch([by[n][0] for n in first])
    b = jpeg.decode_batch([by[n][0] for n in second])
    torch.cuda.synchronize()
    for names, outs in ((first, a), (second, b)):
        for n, got in zip(names, outs):
            assert torch.equal(got, _t(by[n][1])), n


def _sample(path, seed):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0.05, 0.4, (3, 2)).astype(np.float32)
    return dict(image=str(path), objects=dict(bbox=np.concatenate([lo, lo + 0.3], 1), label=np.array([1, 4, 7])),
                l_jitter=96, u_jitter=160, min_side=128.0, max_side=192.0)


@pytest.mark.parametrize("pad_flag", [True, False])
def test_preprocess_data_gpu_decode_matches_host(tmp_path, pad_flag):
    import torch
    from cvlite.data_preprocess import preprocess_data
    path = tmp_path / "img.jpg"
    path.write_bytes(encode(77, 53, "420", 90, seed=11))
    s = _sample(path, 0)
    for seed in (1, 2, 3):                                   # both flip outcomes, several jitter sizes
        h = preprocess_data(s, img_dims=64, pad_flag=pad_flag, rng=np.random.default_rng(seed), decode="host")
        g = preprocess_data(s, img_dims=64, pad_flag=pad_flag, rng=np.random.default_rng(seed), decode="gpu")
        assert torch.equal(h[0], g[0])
        for x, y in zip(h[1:], g[1:]):
            assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        preprocess_data(s, decode="device")


def test_raw_batch_gpu_decode_matches_host(tmp_path):
    import torch
    from PIL import Image
    from cvlite.train_fcos import _raw_batch
    data = []
    for k, (w, h, s) in enumerate([(77, 53, "420"), (64, 48, "444"), (50, 90, "422")]):
        p = tmp_path / ("img%d.jpg" % k)
        p.write_bytes(encode(w, h, s, 85, seed=20 + k))
        data.append(_sample(p, k))
    p = tmp_path / "img3.png"                                # a file the GPU decoder hands to the host
    Image.fromarray(make_image(60, 44, 30)).save(p)
    data.append(_sample(p, 3))
    data.append(dict(_sample(p, 4), image=make_image(40, 56, 31)))     # an already decoded sample
    idx = [3, 0, 2, 1, 4]
    h = _raw_batch(data, idx, np.random.default_rng(5), jpeg_decode="host")
    g = _raw_batch(data, idx, np.random.default_rng(5), jpeg_decode="gpu")
    assert len(h[0]) == len(g[0]) == len(idx)
    for x, y in zip(h[0], g[0]):
        assert torch.equal(x, y)
    for x, y in zip(h[1:], g[1:]):
        assert np.array_equal(x, y)
