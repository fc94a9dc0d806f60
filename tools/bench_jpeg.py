"""A/B of the JPEG decode paths on one MI355X: python tools/bench_jpeg.py [--out DIR] [--rounds R] [--reps K]

16 files of 375 x 500, 4:2:0, quality 90 (seeded images, encoded by Pillow).  Timed per batch of 16,
host clock around work that ends in a device synchronise, the configurations alternating inside
every round:
  (a)  host path: 16 serial data_preprocess._parse_image calls, each followed by its upload
  (b)  cvlite.jpeg.decode_batch at CVL_JPEG_THREADS = 1, 4, 8, 16
plus the parts of (b): the serial host entropy decode alone (cvl_jpeg_entropy_decode, one thread),
an event-timed pinned copy of the batch's staging bytes, and the two kernels' times from a
`rocprofv3 --kernel-trace --stats` run of this script's --child mode (a process of its own, started
before this one touches the GPU).  Prints one JSON line; --out also keeps it as bench_jpeg.json.
"""
import argparse
import csv
import ctypes
import glob
import io
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "cv-lite-object-detection_amd"))

N_FILES, WIDTH, HEIGHT, QUALITY = 16, 375, 500, 90
THREADS = (1, 4, 8, 16)


def make_files():
    import numpy as np
    from PIL import Image
    out = []
    for k in range(N_FILES):
        rng = np.random.default_rng(1000 + k)
        yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH].astype(np.float64)
        chans = [128 + 90 * np.sin((xx * (c + 1) + yy * (3 - c)) / (23.0 + 5 * k) + c) + rng.normal(0, 14, xx.shape)
                 for c in range(3)]
        buf = io.BytesIO()
        Image.fromarray(np.clip(np.stack(chans, -1), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=QUALITY,
                                                                                   subsampling=2)
        out.append(buf.getvalue())
    return out


def child(reps):
    """The profiled run: warm-up + reps batches, nothing else on the GPU."""
    import torch
    from cvlite import jpeg
    files = make_files()
    for _ in range(3 + reps):
        jpeg.decode_batch(files, strict=True)
    torch.cuda.synchronize()


def kernel_times(out_dir, reps):
    """us per batch of the two kernels, from a rocprofv3 run of --child."""
    prof = os.path.join(out_dir, "jpeg_prof")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", prof, "-o", "p", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--reps", str(reps)]
    subprocess.run(cmd, check=True, timeout=280, stdout=subprocess.DEVNULL)
    stats = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under " + prof)
    out = {}
    for r in csv.DictReader(open(stats[0])):
        for key in ("jpeg_idct_kernel", "jpeg_colour_kernel"):
            if key in r["Name"]:
                out[key + "_us"] = round(float(r["TotalDurationNs"]) / float(r["Calls"]) / 1e3, 2)
                out[key + "_calls"] = int(r["Calls"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    os.makedirs(a.out, exist_ok=True)
    res = {"files": N_FILES, "width": WIDTH, "height": HEIGHT, "quality": QUALITY, "sampling": "4:2:0"}
    if not a.no_profile:
        res.update(kernel_times(a.out, a.reps))

    import numpy as np
    import torch
    from cvlite import _lib, jpeg
    from cvlite.data_preprocess import _parse_image
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py measures on the GPU; none found")
    files = make_files()
    res["file_bytes"] = [len(f) for f in files]

    def host_path():
        imgs = [torch.from_numpy(np.array(_parse_image(io.BytesIO(f)))).cuda() for f in files]
        torch.cuda.synchronize()
        return imgs

    def gpu_path():
        imgs = jpeg.decode_batch(files, strict=True)
        torch.cuda.synchronize()
        return imgs

    ref = host_path()
    for t in THREADS:                                     # the results first: faster and different is not faster
        os.environ["CVL_JPEG_THREADS"] = str(t)
        assert all(torch.equal(x, y) for x, y in zip(ref, gpu_path())), "decode_batch differs from the host path"

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        return (time.perf_counter() - t0) / a.reps * 1e3    # ms per batch

    configs = [("host_parse_image", None)] + [("decode_batch_t%d" % t, t) for t in THREADS]
    samples = {name: [] for name, _ in configs}
    for _ in range(a.rounds):
        for name, t in configs:
            if t is not None:
                os.environ["CVL_JPEG_THREADS"] = str(t)
            samples[name].append(timed(host_path if t is None else gpu_path))
    for name, v in samples.items():
        res[name + "_ms"] = round(statistics.median(v), 3)
        res[name + "_ms_range"] = [round(min(v), 3), round(max(v), 3)]

    # the parts of (b): serial entropy decode, and a pinned copy of the same bytes
    infos = [jpeg.info(f) for f in files]
    lib = _lib.load()
    coef = [np.empty(i.coef_count, np.int16) for i in infos]
    qt = np.empty((3, 64), np.uint16)

    def entropy():
        for f, c in zip(files, coef):
            assert lib.cvl_jpeg_entropy_decode(f, len(f), c.ctypes.data, c.size, qt.ctypes.data) == 0
    res["entropy_serial_ms"] = round(statistics.median(timed(entropy) for _ in range(a.rounds)), 3)
    counts = (ctypes.c_int32 * N_FILES)(*[i.coef_count for i in infos])
    sb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.call("cvl_jpeg_batch_sizes", counts, N_FILES, ctypes.byref(sb), ctypes.byref(wb))
    res["staging_bytes"], res["workspace_bytes"] = sb.value, wb.value
    pinned = torch.empty(sb.value, dtype=torch.uint8).pin_memory()
    dev = torch.empty(sb.value, dtype=torch.uint8, device="cuda")
    cp = []
    for _ in range(a.rounds * 3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        dev.copy_(pinned, non_blocking=True)
        e.record()
        torch.cuda.synchronize()
        cp.append(s.elapsed_time(e) * 1e3)
    res["copy_us"] = round(statistics.median(cp), 1)
    res["ratio_host_over_gpu_default"] = round(res["host_parse_image_ms"] / res["decode_batch_t8_ms"], 2)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(a.out, "bench_jpeg.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
