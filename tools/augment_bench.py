"""Times the batched augmentation launch on one MI355X: python tools/augment_bench.py [--out DIR] [--rounds R] [--reps K]

16 uint8 375 x 500 sources (seeded) on the device -> 16 padded 512 x 512 x 3 fp32 images in one batch
tensor (min_side = max_side = 512, stride 128: the bench's fixed input).  Device events around K calls of
each form, after a warm-up of every form, the forms alternating inside every round; the median over
the rounds and the range are reported, per batch of 16:
  per_image       today's path: 16 data_preprocess.preprocess_image launches (flip draws fixed)
  identity        (a) cvlite.augment.augment_batch, AugmentPolicy.identity(): plans + table + copy + launch
  full            (b) the same with the default AugmentPolicy
  identity_launch, full_launch   the cvl_augment_batch launch alone over a prepared device table, back to back
  raw_batch_none / _identity / _full   train_fcos._raw_batch(augment=...) on the same device images: today's
                  per-image preprocess_data (launch + box arithmetic) against the hook with each policy
Before any timing the identity outputs are compared with the per-image outputs (bit for bit).  With
--profile the kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run of --child (a process
of its own, started before this one touches the GPU).  The bytes moved are computed from the shapes
(every source byte read once, every output byte written once) and give the HBM floor at 6.29 TB/s (the
measured streaming rate) that the launch times are compared with.  Prints one JSON line; --out keeps it as
augment_bench.json.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "cv-lite-object-detection_amd"))

B, H, W, SIDE = 16, 375, 500, 512
KW = dict(min_side=512.0, max_side=512.0, stride=128.0)
HBM_BPS = 6.29e12


def make_batch():
    import numpy as np
    import torch
    rng = np.random.default_rng(2024)
    imgs = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(B)]
    boxes, labels = [], []
    for _ in range(B):
        n = int(rng.integers(1, 5))
        c, s = rng.uniform(0.3, 0.7, (n, 2)), rng.uniform(0.1, 0.28, (n, 2))
        boxes.append(np.concatenate([c - s, c + s], 1).astype(np.float32))
        labels.append(rng.integers(0, 20, n))
    return imgs, boxes, labels


def prepared(imgs, plans, batch):
    """A device table of the plans writing into `batch`, and the call that launches over it."""
    from cvlite import _lib
    from cvlite import augment as ag
    host = ag.pinned_table(ag.plan_table(plans), imgs, list(batch.unbind(0)))
    dev = host.to("cuda")
    return host, dev, lambda: _lib.call("cvl_augment_batch", _lib.c_void_p(host.data_ptr()), _lib.ptr(dev), B,
                                        _lib.stream())


def child(reps):
    """The profiled run: warm-up + reps launches of each prepared table, nothing else on the GPU."""
    import numpy as np
    import torch
    from cvlite import augment as ag
    imgs, boxes, labels = make_batch()
    batch = torch.empty((B, SIDE, SIDE, 3), device="cuda")
    for policy in (ag.AugmentPolicy.identity(), ag.AugmentPolicy()):
        rng = np.random.default_rng(7)
        plans = [ag.plan_image((H, W), boxes[k], labels[k], policy, rng, **KW) for k in range(B)]
        keep = prepared(imgs, plans, batch)
        for _ in range(3 + reps):
            keep[2]()
        torch.cuda.synchronize()


def kernel_time(out_dir, reps):
    prof = os.path.join(out_dir, "augment_prof")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", prof, "-o", "p", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--reps", str(reps)]
    subprocess.run(cmd, check=True, timeout=280, stdout=subprocess.DEVNULL)
    stats = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under " + prof)
    for r in csv.DictReader(open(stats[0])):
        if "augment_batch_kernel" in r["Name"]:       # identity and full launches together
            return {"kernel_us_mean_both_policies": round(float(r["TotalDurationNs"]) / float(r["Calls"]) / 1e3, 2),
                    "kernel_calls": int(r["Calls"])}
    raise RuntimeError("augment_batch_kernel is not in " + stats[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    os.makedirs(a.out, exist_ok=True)
    res = {"images": B, "source": [H, W, 3], "padded": [SIDE, SIDE, 3]}
    if a.profile:
        res.update(kernel_time(a.out, a.reps))

    import numpy as np
    import torch
    from cvlite import augment as ag
    from cvlite.data_preprocess import preprocess_image
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench.py measures on the GPU; none found")
    imgs, boxes, labels = make_batch()
    batch = torch.empty((B, SIDE, SIDE, 3), device="cuda")
    other = torch.empty_like(batch)
    ident, full = ag.AugmentPolicy.identity(), ag.AugmentPolicy()
    flips = [bool(k % 2) for k in range(B)]

    def per_image(dst=batch):
        for k in range(B):
            preprocess_image(imgs[k], None, KW["min_side"], KW["max_side"], KW["stride"], True, flip=flips[k], out=dst[k])

    def whole(policy):
        rng = np.random.default_rng(7)
        return lambda: ag.augment_batch(imgs, boxes, labels, policy, rng, out=batch, **KW)

    # the results first: faster and different is not faster
    per_image(other)
    plans = [ag.plan_geometry(H, W, flip=f, **KW) for f in flips]
    ag.run_plans(imgs, plans, out=batch)
    assert torch.equal(batch, other), "the identity launch differs from the per-image launches"
    rng = np.random.default_rng(7)
    plans_i = [ag.plan_image((H, W), boxes[k], labels[k], ident, rng, **KW) for k in range(B)]
    rng = np.random.default_rng(7)
    plans_f = [ag.plan_image((H, W), boxes[k], labels[k], full, rng, **KW) for k in range(B)]
    assert all((p.ph, p.pw) == (SIDE, SIDE) for p in plans_i + plans_f)
    keep_i, keep_f = prepared(imgs, plans_i, batch), prepared(imgs, plans_f, batch)
    # the training hook both ways: here today's path carries its box arithmetic too, as augment_batch does
    from cvlite.train_fcos import _raw_batch
    data = [dict(image=imgs[k], objects=dict(bbox=boxes[k], label=labels[k]), l_jitter=SIDE, u_jitter=SIDE,
                 min_side=KW["min_side"], max_side=KW["max_side"]) for k in range(B)]

    def raw(policy):
        rng = np.random.default_rng(7)
        return lambda: _raw_batch(data, range(B), rng, augment=policy)

    forms = [("per_image", per_image), ("identity", whole(ident)), ("full", whole(full)),
             ("identity_launch", keep_i[2]), ("full_launch", keep_f[2]),
             ("raw_batch_none", raw(None)), ("raw_batch_identity", raw(ident)), ("raw_batch_full", raw(full))]

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps * 1e3             # us per batch

    for _, fn in forms:                                      # warm-up of every form
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _ in forms}
    for _ in range(a.rounds):
        for name, fn in forms:
            samples[name].append(timed(fn))
    for name, v in samples.items():
        res[name + "_us"] = round(statistics.median(v), 1)
        res[name + "_us_range"] = [round(min(v), 1), round(max(v), 1)]
    res["bytes_read"] = B * H * W * 3
    res["bytes_written"] = B * SIDE * SIDE * 3 * 4
    floor_us = (res["bytes_read"] + res["bytes_written"]) / HBM_BPS * 1e6
    res["hbm_floor_us"] = round(floor_us, 2)
    for name in ("identity_launch", "full_launch"):
        res[name + "_share_of_hbm_floor"] = round(floor_us / res[name + "_us"], 3)
    if "kernel_us_mean_both_policies" in res:
        res["kernel_share_of_hbm_floor"] = round(floor_us / res["kernel_us_mean_both_policies"], 3)
    res["ratio_per_image_over_identity"] = round(res["per_image_us"] / res["identity_us"], 2)
    res["ratio_per_image_over_identity_launch"] = round(res["per_image_us"] / res["identity_launch_us"], 2)
    res["ratio_raw_batch_none_over_identity"] = round(res["raw_batch_none_us"] / res["raw_batch_identity_us"], 2)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(a.out, "augment_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
