"""Batched JPEG decode on MI355X (include/cvlite.h "JPEG decode"): the GPU counterpart of
data_preprocess._parse_image.

  info(data)                        size / sampling / status of a file's bytes (host only)
  decode(src, strict=False)         one file name or bytes object -> uint8 [H,W,3] on the device
  decode_batch(srcs, strict=False)  a list of them, one cvl_jpeg_decode_batch call

The Huffman bit stream is decoded on the host (C++ threads, CVL_JPEG_THREADS of them, default 8),
everything after it in two HIP launches per batch; the pixels are bit-identical to
PIL's Image.open(...).convert("RGB").  A file outside the supported set (PNG, progressive, CMYK,
..., or a damaged stream) is decoded by _parse_image and uploaded, so the caller always gets the
pixels it gets from the host path; strict=True raises CvlError instead.

Staging: one grow-only pinned host buffer and one device workspace per device.  The host threads
write the pinned buffer and the copy out of it is asynchronous, so each batch records an event
behind its work and the next batch waits for that event before it touches either buffer.  The
decode is host work plus a copy: it runs outside a captured step graph, like the preprocessing.
"""
import ctypes
import io
from collections import namedtuple

import torch

from . import _lib

OK, UNSUPPORTED, CORRUPT = 0, 2, 3
STATUS_NAMES = {OK: "ok", 1: "invalid argument", UNSUPPORTED: "unsupported", CORRUPT: "corrupt"}

JpegInfo = namedtuple("JpegInfo", "status width height components hmax vmax restart_interval coef_count")


class _Staging:
    """The pinned staging buffer, the device workspace and the event of the last batch (one per device)."""

    def __init__(self):
        self.pinned = None
        self.work = None
        self.event = None

    def reserve(self, staging_bytes, workspace_bytes, device):
        if self.event is not None:
            self.event.synchronize()             # the previous batch's copy and kernels have run
        if self.pinned is None or self.pinned.numel() < staging_bytes:
            self.pinned = torch.empty(staging_bytes, dtype=torch.uint8).pin_memory()
        if self.work is None or self.work.numel() < workspace_bytes:
            self.work = torch.empty(workspace_bytes, dtype=torch.uint8, device=device)

    def mark(self):
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream())


_staging = {}


def _read(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def info(data):
    """JpegInfo of a file's bytes; status OK (0), UNSUPPORTED (2) or CORRUPT (3), the rest 0 unless OK."""
    data = _read(data)
    out = (ctypes.c_int32 * 8)()
    _lib.load().cvl_jpeg_info(data, len(data), out)
    return JpegInfo(*out)


def _host_decode(src, data, device):
    from .data_preprocess import _parse_image
    img = _parse_image(io.BytesIO(data) if not isinstance(src, str) else src)
    return torch.from_numpy(img.copy()).to(device)      # PIL's array is read-only


def _refused(src, status):
    return _lib.CvlError("jpeg.decode: %s file %s" % (STATUS_NAMES.get(status, status),
                                                      src if isinstance(src, str) else "<bytes>"))


def decode_batch(srcs, strict=False):
    """srcs: file names or bytes objects -> a list of uint8 [H_i, W_i, 3] tensors on the current
    device, the pixels of PIL's convert("RGB").  strict: raise CvlError for a file the GPU decoder
    does not take instead of decoding it on the host."""
    _lib.require_cuda()
    srcs = list(srcs)
    if not srcs:
        return []
    device = torch.device("cuda", torch.cuda.current_device())
    datas = [_read(s) for s in srcs]
    infos = [info(d) for d in datas]
    if strict:
        for s, i in zip(srcs, infos):
            if i.status != OK:
                raise _refused(s, i.status)
    n = len(srcs)
    outs = [torch.empty((i.height, i.width, 3), dtype=torch.uint8, device=device) if i.status == OK else None
            for i in infos]
    status = (ctypes.c_int32 * n)(*[i.status for i in infos])
    if any(o is not None for o in outs):
        counts = (ctypes.c_int32 * n)(*[i.coef_count for i in infos])
        sb, wb = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.call("cvl_jpeg_batch_sizes", counts, n, ctypes.byref(sb), ctypes.byref(wb))
        st = _staging.setdefault(device.index, _Staging())
        st.reserve(sb.value, wb.value, device)
        ptrs = (ctypes.c_char_p * n)(*datas)
        lens = (ctypes.c_size_t * n)(*[len(d) for d in datas])
        optr = (ctypes.c_void_p * n)(*[None if o is None else o.data_ptr() for o in outs])
        try:
            _lib.call("cvl_jpeg_decode_batch", ptrs, lens, n, optr, st.pinned.data_ptr(), st.pinned.numel(),
                      st.work.data_ptr(), st.work.numel(), status, _lib.stream())
        finally:
            st.mark()
    for k in range(n):
        if status[k] != OK:                      # not taken by the header, or damaged inside the scan
            if strict:
                raise _refused(srcs[k], status[k])
            outs[k] = _host_decode(srcs[k], datas[k], device)
    return outs


def decode(src, strict=False):
    """One file name or bytes object -> uint8 [H, W, 3] on the current device."""
    return decode_batch([src], strict=strict)[0]
