#!/usr/bin/env python3
"""Headline benchmark: FCOS ResNet-50-FPN training images/sec (whole node), 512x512, bs=16/GPU
(BASELINE.json metric; configs[1] at N=1, configs[2] data-parallel at N>1).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N

A plain run does what the headline figure needs and no more: set-up, W warm-up steps, ONE timed
run of exactly K steps, the result line.  `--full` adds everything else the line can carry: the
median of 3 timed runs (`--runs`), the in-step tower probe and the `roofline` blocks (runs of
their own after the timed steps), the `dist.grad_allreduce` plan / traced step and the
`cpu_baseline` leg.  `--dump-outputs DIR` writes what the last timed step handed its caller
(per-image losses, head outputs, updated parameters) as float32 DIR/<name>.npy; the inputs are
seeded, so two builds run with the same arguments can be compared array by array.

`--gpus N` (N > 1) without a torchrun environment (no WORLD_SIZE) starts the N ranks itself: it
runs `python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1` on this same
command line as a CHILD process (before anything touches the GPU; no exec) and exits with its
status, so `bench.py --gpus 8` measures 8 ranks, one per GPU, over RCCL.  `--dry-run` forms the
process group (RCCL on GPUs, gloo without) and prints the world it saw, without any GPU work.

A step = synthetic batch copy into the static input buffers (device-to-device) + target
assignment + forward + fused loss + backward + (RCCL all-reduce) + clip/SGD + weight re-pack,
i.e. the whole reference train_fcos.py step for 16 images.  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd")]

import torch  # noqa: E402

from cvlite import dist  # noqa: E402
from cvlite import ops_nn as nn  # noqa: E402
from cvlite.fcos_net import FCOSNet  # noqa: E402
from cvlite.layers import WGRAD_BATCH  # noqa: E402
from cvlite.train_fcos import FCOSTrainer, synthetic_batch  # noqa: E402

METRIC = "training images/sec (whole node), FCOS-VOC 512x512 bs=16/GPU"
PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md), no sparsity
NUM_CLASSES = 20               # VOC


def train_flops_per_image(H, W, C=NUM_CLASSES):
    """Algorithmic conv FLOPs of one training image (fwd + dgrad + wgrad; no stem dgrad)."""
    from cvlite.layers import ParamStore
    net = FCOSNet.__new__(FCOSNet)
    net._build_layers(ParamStore(), C)
    fl = 0.0

    def conv(c, h, w, dgrad=True):
        Ho, Wo, _, _ = c.out_hw(h, w)
        f = 2.0 * Ho * Wo * c.cout * c.k * c.k * c.cin
        return f * (3.0 if dgrad else 2.0), Ho, Wo
    h, w = H, W
    f, h, w = conv(net.backbone.stem.conv, h, w, dgrad=False)
    fl += f
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    taps = []
    for st in net.backbone.stages:
        for b in st:
            for u in b.units():
                if u is b.sc:
                    fl += conv(u.conv, h, w)[0]
            f1, h1, w1 = conv(b.c1.conv, h, w)
            f2, _, _ = conv(b.c2.conv, h1, w1)
            f3, _, _ = conv(b.c3.conv, h1, w1)
            fl += f1 + f2 + f3
            h, w = h1, w1
        taps.append((h, w))
    (h3, w3), (h4, w4), (h5, w5) = taps[1:]
    fl += conv(net.c3_1x1, h3, w3)[0] + conv(net.c4_1x1, h4, w4)[0] + conv(net.c5_1x1, h5, w5)[0]
    fl += conv(net.c3_3x3, h3, w3)[0] + conv(net.c4_3x3, h4, w4)[0] + conv(net.c5_3x3, h5, w5)[0]
    f6, h6, w6 = conv(net.c6_3x3, h5, w5)
    fl += f6 + conv(net.c7_3x3, h6, w6)[0]
    for (lh, lw) in FCOSNet.level_shapes(H, W):
        for c in net.cls_tower + net.reg_tower:
            fl += conv(c, lh, lw)[0]
        fl += conv(net.cls_heads[0], lh, lw)[0] + conv(net.reg_heads[0], lh, lw)[0]
    return fl


def measure_tower_conv(net, B, H, W, iters=20):
    """Dominant kernel: one tower layer's 3x3 conv forward, cls + reg towers over all five FPN
    levels in ONE 10-segment launch (FPNDetector._pair_segs), timed with HIP events on the stream
    it is launched on.  Its input is the training step's own layer-1 tower activations (the last
    timed step's buffer), so the launch sees the data the step's tower convs see (synthetic
    N(0, 0.25) only if the step left none)."""
    shapes, off, P = net.layout(B, H, W)
    dev = net.device
    saved = getattr(net, "_saved", None)
    if saved and saved.get("tower_bufs") and tuple(saved["tower_bufs"][0].shape) == (2 * B * P, 256):
        src = saved["tower_bufs"][0]
    else:
        g = torch.Generator(device="cpu").manual_seed(5)
        src = (torch.randn((2 * B * P, 256), generator=g) * 0.5).to(torch.bfloat16).to(dev)
    dst = torch.empty_like(src)
    d = net.cls_tower[1].fwd_desc(B, net._pair_segs(1, B, shapes, off, P, fwd=True), ld_dst=256)
    for _ in range(3):
        nn.conv_igemm(d, src, dst)
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(iters):
        nn.conv_igemm(d, src, dst)
    e1.record(s)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / iters
    M = 2 * B * P
    flops = 2.0 * M * 256 * 9 * 256
    from cvlite import _lib
    L = _lib.load()
    kname = L.cvl_conv_kernel_name(L.cvl_conv_igemm_last_kernel()).decode()
    return ms, flops, kname


def measure_backbone_3x3(net, B, H, W, iters=20, eager=False):
    """roofline.backbone_3x3: the 16 ResNet-50 3x3 convs (conv2_x..conv5_x units' `_2_conv`, the
    shapes north_star names) -- forward (with the BN statistics the step forms), data gradient
    (with the conv1 unit's fused BN-backward first pass, as the step runs it) and weight gradient,
    each distinct launch replayed alone with HIP events on its stream on random N(0, 1) operands
    (the step's own launch descriptors and packed weights); returns the FLOP-weighted fraction
    of the bf16 dense peak over all 48 launches and the per-shape rows."""
    from cvlite import _lib
    L = _lib.load()
    dev = net.device
    bb = net.backbone
    rows, tot_f, tot_t = [], 0.0, 0.0
    h, w = -(-H // 4), -(-W // 4)                 # after the stem's stride 2 and the max-pool
    g = torch.Generator(device="cpu").manual_seed(3)
    s = torch.cuda.current_stream()

    def timed(fn):
        # the launches are captured into a HIP graph and the graph replayed: eager launches of these
        # 10-60 us kernels are host-bound (ctypes + descriptor preparation per call), as the step's
        # own launches are not (the step is graph-replayed too)
        for _ in range(3):
            fn()
        kname = L.cvl_conv_kernel_name(L.cvl_conv_igemm_last_kernel()).decode()
        if eager:                                  # (counter collection: plain launches)
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            return float("nan"), kname
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gs = torch.cuda.current_stream()
        e0.record(gs)
        g.replay()
        e1.record(gs)
        e1.synchronize()
        return e0.elapsed_time(e1) / iters * 1e-3, kname
    for si, stage in enumerate(bb.stages):
        if si > 0:
            h, w = -(-h // 2), -(-w // 2)
        conv = stage[-1].c2.conv                  # every block of a stage has the same 3x3 shape
        bn = stage[-1].c1.bn
        C = conv.cin
        x = torch.randn((B, h, w, C), generator=g).to(torch.bfloat16).to(dev)
        dy = torch.randn((B, h, w, conv.cout_pad), generator=g).to(torch.bfloat16).to(dev)
        dy[..., conv.cout:] = 0
        y = torch.empty((B, h, w, conv.cout), dtype=torch.bfloat16, device=dev)
        st = nn.bn_acc(B, conv.cout, dev)
        dx = torch.empty((B, h, w, C), dtype=torch.bfloat16, device=dev)
        mr = torch.empty((B, C, 2), dtype=torch.float32, device=dev)
        mr[..., 0] = 0.0
        mr[..., 1] = 1.0
        sums = nn.bn_acc(B, C, dev)
        n = len(stage)
        dwb = [torch.zeros_like(conv.dw) for _ in range(n)]
        fd = conv.fwd_desc(B, [nn.seg(h, w, h, w, conv.wf, conv.bias_arg())], ld_dst=conv.cout)
        dd = conv.dgrad_desc(B, [nn.seg(h, w, h, w, conv.wd)], ld_dst=C)
        wd = conv.fwd_desc(B, [nn.seg(h, w, h, w, conv.wf, None)], ld_dst=conv.cout_pad)
        flops = 2.0 * B * h * w * 9 * C * conv.cout
        # the weight gradients as the step runs them (round 6): the stage's n units in one batched call
        # (cvl_conv_wgrad_batch, one launch + the split reductions), timed per unit
        for kind, fn, per in (("fwd", lambda: nn.conv_igemm(fd, x, y, st), 1),
                              ("dgrad", lambda: nn.conv_igemm_dgrad_bnsum(dd, dy, dx, x, mr, bn.gamma, bn.beta, sums), 1),
                              ("wgrad", (lambda: nn.conv_wgrad_batch([wd] * n, [x] * n, [dy] * n, dwb)) if WGRAD_BATCH
                               else (lambda: nn.conv_wgrad(wd, x, dy, dwb[0])), n if WGRAD_BATCH else 1)):
            t, kname = timed(fn)
            t /= per
            rows.append({"shape": "%s 3x3 %d->%d @ %dx%d" % (kind, C, conv.cout, h, w), "count": n,
                         "us": round(t * 1e6, 2), "frac": round(flops / t / 1e12 / PEAK_BF16_TFLOPS, 4),
                         "kernel": kname.split(" (")[0]})
            tot_f += n * flops
            tot_t += n * t
    return {"frac": round(tot_f / tot_t / 1e12 / PEAK_BF16_TFLOPS, 4), "achieved": round(tot_f / tot_t / 1e12, 2),
            "unit": "TFLOP/s", "peak": PEAK_BF16_TFLOPS, "launches": 48, "ms_per_step": round(tot_t * 1e3, 4),
            "gflop_per_step": round(tot_f / 1e9, 2),
            "timing": "each distinct launch captured 20x into a HIP graph and the graph replayed alone (HIP events "
                      "on its stream) after the timed steps; the weight gradients as the step runs them: a stage's "
                      "units in one batched call (cvl_conv_wgrad_batch), time per unit; "
                      "counts from the ResNet-50 stage depths (3/4/6/3)", "per_shape": rows}


PMC_FILE = "profiles/r06z2_pmc_tower_conv.json"


def pmc_traffic(kname):
    """Per-launch HBM bytes of the dominant kernel, measured by tools/pmc3.sh (committed); null
    when the committed measurement is of a different kernel than the one this run launched."""
    p = os.path.join(ROOT, PMC_FILE)
    if not os.path.exists(p):
        return None
    d = json.load(open(p))
    if d["kernel"].split("<")[0] not in kname:
        return None
    return int(d["hbm_bytes"])


def tower_alg_bytes(B, net, H, W):
    P = net.layout(B, H, W)[2]
    return 2 * (2 * (2 * B * P) * 256) + 2 * (2 * 256 * 9 * 256)   # src + dst bf16, 2 towers' weights


def timed_runs(step, load, pool, args, dev):
    """W untimed warm-up steps, then `runs` timed runs of EXACTLY K steps each (one run; three with
    --full), every run bracketed by a barrier + device synchronize on both sides and maxed over
    ranks (100 timed steps, median of 3 runs).  Returns the per-run seconds; the
    reported line uses the median run."""
    for i in range(args.warmup):
        load(pool[i % len(pool)])
        step()
    times = []
    for r in range(args.runs):
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            load(pool[i % len(pool)])
            step()
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        times.append(dist.max_over_ranks(time.perf_counter() - t0, dev))
    return times


def _median_run(times):
    return sorted(times)[len(times) // 2]


DUMP_ELEMS = 4 << 20           # per dumped array: 16 MB of float32, four arrays stay under 64 MB


def dump_outputs(path, tr, net, head_cols=None):
    """--dump-outputs: what the last timed step handed its caller, each as float32 <path>/<name>.npy --
    the per-image losses (`step()`'s return value), the heads' outputs (`tr.outputs`, the columns the
    heads store: head_cols = (reg, cls)) and the updated parameters.  An array of more than DUMP_ELEMS
    elements is written as a fixed sample of its flattened elements (seeded: the same sorted indices
    in every run)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {"losses": tr.losses, "params": net.store.flat}
    if head_cols is not None:
        reg, cls = tr.outputs
        arrays["head_reg"], arrays["head_cls"] = reg[..., :head_cols[0]], cls[..., :head_cols[1]]
    torch.cuda.synchronize()
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > DUMP_ELEMS:
            g = torch.Generator(device="cpu").manual_seed(2024)
            idx = torch.randint(t.numel(), (DUMP_ELEMS,), generator=g).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())


def _cores():
    """Host cores this process may use: the affinity mask capped by OMP_NUM_THREADS (the GPU box
    exports its CPU share there; the affinity mask / nproc show the whole machine)."""
    cores = len(os.sched_getaffinity(0))
    omp = os.environ.get("OMP_NUM_THREADS")
    if omp and omp.isdigit() and int(omp) > 0:
        cores = min(cores, int(omp))
    return cores


def _spread(rates):
    """The spread a CPU baseline carries beside its median: the timed samples' min / max and the
    host it ran on (the GPU boxes differ in CPU model and in co-tenant load, so the same bounded
    sample has measured 2.0-3.0 img/s box to box)."""
    cpu = ""
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), "")
    except OSError:
        pass
    lo, hi = min(rates), max(rates)
    med = sorted(rates)[len(rates) // 2]
    return {"min": round(lo, 4), "max": round(hi, 4), "rel_range": round((hi - lo) / med, 4) if med else None,
            "loadavg_1m": round(os.getloadavg()[0], 2), "host_cpu": cpu}


def cpu_baseline(H, W, cfg1_images=8, bs=16, timed_images=(8, 8, 8)):
    """The torch-CPU restatement of the reference step (oracle/model_ref.py: batch-1 forwards,
    per-image BN, gradient sum, /bs, clip, Keras SGD), SURVEY.md §8d protocol on a bounded sample:
    BASELINE configs[0] (one step on 8 synthetic 512x512 images) as the warm-up, then three timed
    steps (each 8 images of the bs=16 workload: per-image fwd+bwd is the whole cost, so images/s
    does not depend on how a 16-image step is cut), img/s = median over the three.  Threads =
    every core this process may run on (sched_getaffinity)."""
    from oracle import fcos_ref, model_ref
    import numpy as np
    cores = _cores()
    torch.set_num_threads(cores)
    print("[bench] cpu_baseline: %d threads" % cores, file=sys.stderr, flush=True)
    p = FCOSNet.param_dict(NUM_CLASSES, seed=0)
    moms = {k: torch.zeros_like(v) for k, v in p.items()}
    n = cfg1_images + sum(timed_images)
    imgs, boxes, nbox = synthetic_batch(n, H, W, NUM_CLASSES, seed=99, device="cpu")
    tg = []
    for b in range(n):
        outs, _ = fcos_ref.format_data(boxes[b, :int(nbox[b])].numpy(), np.array([H, W], np.float32),
                                       NUM_CLASSES, img_pad=(H, W))
        tg.append(torch.from_numpy(fcos_ref.pack_targets(outs)))
    tg = torch.stack(tg)
    t0 = time.time()
    model_ref.train_step_reference(p, moms, imgs[:cfg1_images], tg[:cfg1_images], NUM_CLASSES, 5e-4)
    cfg1_s = time.time() - t0
    rates, o = [], cfg1_images
    print("[bench] cpu_baseline configs[0] step: %.1f s" % cfg1_s, file=sys.stderr, flush=True)
    for k in timed_images:
        t0 = time.time()
        model_ref.train_step_reference(p, moms, imgs[o:o + k], tg[o:o + k], NUM_CLASSES, 5e-4)
        rates.append(k / (time.time() - t0))
        o += k
        print("[bench] cpu_baseline timed step: %.3f img/s" % rates[-1], file=sys.stderr, flush=True)
    return {"value": round(sorted(rates)[len(rates) // 2], 4), "unit": "images/s", "cores": cores,
            "kind": "port", "configs0_step_s": round(cfg1_s, 3), "timed_img_s": [round(r, 4) for r in rates],
            "spread": _spread(rates),
            "sample": "torch-CPU fp32 restatement of the train_fcos.py step (oracle/model_ref.py): configs[0] "
                      "(one step, %d synthetic %dx%d images, %.1f s) as warm-up, then 3 timed steps of 8 images "
                      "of the bs=%d workload (per-image fwd+bwd, clip, SGD), median img/s, %d threads"
                      % (cfg1_images, H, W, cfg1_s, bs, cores)}


def cpu_baseline_retina(S, C, timed_images=2):
    """configs[4]'s CPU reference: the torch-CPU fp32 restatement of RetinaNet.train_loss + its
    backward + clip / Keras SGD (oracle/model_ref.retina_loss_and_grads, targets from the oracle's
    format_data restatement), one warm-up image then `timed_images` images timed one at a time
    (a batch-1 step each, as train_retinanet_coco.py runs them); img/s = median."""
    import numpy as np
    from oracle import model_ref, retina_ref
    from cvlite.retina_net import RetinaNetNet
    from cvlite.train_retinanet import synthetic_coco_batch
    cores = _cores()
    torch.set_num_threads(cores)
    sizes = [20.0, 40.0, 80.0, 160.0, 320.0]
    p = RetinaNetNet.param_dict(C, seed=0)
    imgs, boxes, nbox = synthetic_coco_batch(1 + timed_images, S, C, n_max=50, seed=4321, device="cpu")
    ad = retina_ref.anchor_dims(sizes)
    cells = [(-(-S // s)) ** 2 for s in (8, 16, 32, 64, 128)]
    rates = []
    for i in range(1 + timed_images):
        outs, _ = retina_ref.format_data(boxes[i, :int(nbox[i])].numpy(), np.array([S, S], np.float32), ad, C,
                                         img_pad=[S, S])
        tg = torch.from_numpy(np.concatenate([np.stack(outs[l]).reshape(-1, 4 + C) for l in range(5)], 0))
        t0 = time.time()
        _, grads, _, _ = model_ref.retina_loss_and_grads(p, imgs[i:i + 1], tg[None].float(), C, cells, 9)
        with torch.no_grad():
            norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
            sc = 1.0 / max(norm, 1.0)
            for k, g in grads.items():
                p[k] -= 0.01 * sc * g
        if i > 0:
            rates.append(1.0 / (time.time() - t0))
        print("[bench] cpu_baseline retinanet image %d: %.1f s" % (i, time.time() - t0), file=sys.stderr, flush=True)
    return {"value": round(sorted(rates)[len(rates) // 2], 4), "unit": "images/s", "cores": cores, "kind": "port",
            "spread": _spread(rates),
            "sample": "torch-CPU fp32 restatement of RetinaNet.train_loss fwd+bwd + clip/SGD (oracle/model_ref.py), "
                      "%dx%d C=%d, 1 warm-up + %d timed single-image steps, median, %d threads" % (S, S, C, timed_images,
                                                                                           cores)}


def cpu_baseline_centernet(S, C, timed_batches=2, sub_batch=2):
    """configs[3]'s CPU reference: tf_centernet_hourglass.train_step restated in torch-CPU fp32
    (oracle/centernet_model_ref.train_step_reference: sub-batch BN, 2.5 cls + 1.0 reg, clip, Keras
    Adam), one warm-up sub-batch step then `timed_batches` timed steps of one sub-batch each; median."""
    import numpy as np
    from oracle import centernet_model_ref as cm, centernet_ref
    from cvlite.hourglass_net import HourglassNet
    from cvlite.train_centernet import synthetic_batch as cn_batch
    cores = _cores()
    torch.set_num_threads(cores)
    p = HourglassNet.param_dict(C, seed=0)
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(t) for k, t in p.items()}
    n = sub_batch * (1 + timed_batches)
    imgs, boxes, nbox = cn_batch(n, S, S, C, n_max=16, seed=77, device="cpu")
    tg = torch.stack([torch.from_numpy(centernet_ref.hourglass_format_data(
        boxes[b, :int(nbox[b])].numpy(), np.array([S, S], np.float32), C, img_pad=[S, S], stride=4)[0]).float()
        for b in range(n)])
    rates = []
    for i in range(1 + timed_batches):
        sl = slice(i * sub_batch, (i + 1) * sub_batch)
        t0 = time.time()
        cm.train_step_reference(p, m, v, i, imgs[sl], tg[sl], C, sub_batch)
        if i > 0:
            rates.append(sub_batch / (time.time() - t0))
        print("[bench] cpu_baseline centernet step %d: %.1f s" % (i, time.time() - t0), file=sys.stderr, flush=True)
    return {"value": round(sorted(rates)[len(rates) // 2], 4), "unit": "images/s", "cores": cores, "kind": "port",
            "spread": _spread(rates),
            "sample": "torch-CPU fp32 restatement of tf_centernet_hourglass.train_step (oracle/centernet_model_ref.py),"
                      " %dx%d C=%d, sub-batch %d: 1 warm-up + %d timed steps of %d images, median, %d threads"
                      % (S, S, C, sub_batch, timed_batches, sub_batch, cores)}


PEAK_HBM_GBS = 8000.0          # MI355X HBM3E (MI355X_MICROARCH.md)


def dominant_conv_roofline(run_step, iters=10):
    """`roofline` of a model's dominant conv launch: every conv launch of one eager forward+backward
    (ops_nn.conv_igemm / conv_wgrad / conv_wgrad_grouped) is recorded, each distinct launch is
    captured `iters`x into a HIP graph and replayed alone (HIP events on its stream), and the launch
    with the most time per step is reported against its bound: MFMA when its algorithmic FLOP/byte
    is above the ridge (2.5 PF / 8 TB/s = 312), else HBM with its algorithmic bytes (operands +
    result once)."""
    from cvlite import _lib
    L = _lib.load()
    calls, counts = {}, {}
    orig = (nn.conv_igemm, nn.conv_wgrad, nn.conv_wgrad_grouped)

    def key(kind, d, extra=()):
        segs = tuple((d.seg[i].Hr, d.seg[i].Wr, d.seg[i].Hs, d.seg[i].Ws) for i in range(d.nseg))
        return (kind, d.mode, d.B, d.Cin, d.KH, d.KW, d.stride, d.Npad, d.n_store, d.dst_f32, segs) + extra

    def work(kind, d, ng=1):
        rows = sum(d.B * d.seg[i].Hr * d.seg[i].Wr for i in range(d.nseg))
        srows = sum(d.B * d.seg[i].Hs * d.seg[i].Ws for i in range(d.nseg))
        K = d.KH * d.KW * d.Cin
        # FLOPs over the forward output pixels: a data gradient's source (Hs, Ws) is dY, its result
        # (Hr, Wr) the forward input -- s^2 times as many pixels for stride s
        fl = 2.0 * (srows if kind == "igemm" and d.mode == 1 else rows) * K * d.n_store
        if kind == "igemm":
            by = srows * d.Cin * 2 + rows * d.n_store * (4 if d.dst_f32 else 2) + d.nseg * d.Npad * K * 2
        else:
            by = srows * d.Cin * 2 + rows * d.n_store * 2 + ng * K * d.n_store * 4
        return fl, by

    def rec(kind, fn, d, args, ng=1):
        k = key(kind, d, (ng,))
        counts[k] = counts.get(k, 0) + 1
        if k not in calls:
            calls[k] = (fn, d, args, work(kind, d, ng), kind)

    def p_igemm(d, src, dst, stats=None):
        orig[0](d, src, dst, stats)
        rec("igemm", orig[0], d, (src, dst, stats))

    def p_wgrad(d, x, dy, dw, beta=0.0):
        orig[1](d, x, dy, dw, beta)
        rec("wgrad", orig[1], d, (x, dy, dw, beta))

    def p_wgrad_g(d, x, dy, dws, beta=0.0):
        orig[2](d, x, dy, dws, beta)
        rec("wgrad", orig[2], d, (x, dy, dws, beta), len(dws))
    nn.conv_igemm, nn.conv_wgrad, nn.conv_wgrad_grouped = p_igemm, p_wgrad, p_wgrad_g
    try:
        run_step()
        torch.cuda.synchronize()
    finally:
        nn.conv_igemm, nn.conv_wgrad, nn.conv_wgrad_grouped = orig
    best = None
    for k, (fn, d, a, (fl, by), kind) in calls.items():
        with nn.deferred_wgrad():                 # split reductions inside the timed launch
            fn(d, *a)
            nn.wgrad_flush()
        kname = L.cvl_conv_kernel_name(L.cvl_conv_igemm_last_kernel()).decode().split(" (")[0]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn(d, *a)
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gs = torch.cuda.current_stream()
        e0.record(gs)
        g.replay()
        e1.record(gs)
        e1.synchronize()
        t = e0.elapsed_time(e1) / iters * 1e-3
        if best is None or t * counts[k] > best[0]:
            best = (t * counts[k], t, k, fl, by, kind, kname, d)
        del g
    tot, t, k, fl, by, kind, kname, d = best
    mfma = fl / by > PEAK_BF16_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)
    s0 = d.seg[0]
    what = "%s %dx%d/%d %d->%d @ %dx%d%s B%d" % ({0: "fwd", 1: "dgrad"}[d.mode] if kind == "igemm" else "wgrad",
                                              d.KH, d.KW, d.stride, d.Cin, d.n_store, s0.Hr, s0.Wr,
                                              " +%d seg" % (d.nseg - 1) if d.nseg > 1 else "", d.B)
    if mfma:
        ach = fl / t / 1e12
        r = {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
             "frac": round(ach / PEAK_BF16_TFLOPS, 4)}
    else:
        ach = by / t / 1e9
        r = {"bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
             "frac": round(ach / PEAK_HBM_GBS, 4)}
    r.update({"traffic": None, "kernel": "%s: %s, x%d per step (%.3f ms/step of %d conv launches)"
              % (kname, what, counts[k], tot * 1e3, sum(counts.values())),
              "ms_per_launch": round(t * 1e3, 4), "algorithmic": {"flop": fl, "bytes": by},
              "timing": "the step's own launch (descriptor, packed weights, activations of one eager step) captured "
                        "%dx into a HIP graph and replayed alone, HIP events on its stream" % iters})
    return r


def centernet_roofline(net, tr, B, S):
    return dominant_conv_roofline(lambda: tr._fwd_bwd(None))


def tower_roofline(net, B, H, W, probe_s=None, probe_n=0, pmc=True):
    """`roofline` of the FPN detectors' dominant launch (one tower layer of both towers over all five
    levels, conv_igemm_x32_kernel): in-step probe timing when given, else the burst timing."""
    k_ms, k_flops, k_name = measure_tower_conv(net, B, H, W)
    in_ms = probe_s * 1e3 if probe_s else k_ms
    achieved = k_flops / (in_ms * 1e-3) / 1e12
    M = 2 * B * net.layout(B, H, W)[2]
    return {"bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": pmc_traffic(k_name) if pmc else None,
            "traffic_note": ("HBM bytes per launch from rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + "
                             "WRITE_SIZE, separate passes (tools/pmc3.sh -> %s; FCOS 512 bs16 geometry)" % PMC_FILE
                             if pmc else "no PMC pass of this geometry") +
                            "; algorithmic bytes per launch %d (src + dst bf16 + weights)" % tower_alg_bytes(B, net, H, W),
            "kernel": "%s, fwd: tower layer 3x3 256->256 of both towers over all 5 levels, one 10-segment launch "
                      "(M=%d, N=256, K=2304)" % (k_name, M),
            "ms_per_launch": round(in_ms, 4),
            "timing": ("mean over the %d tower launches of the timed steps (GPU wall clock from workgroup 0's "
                       "start to the last workgroup's end, stamped inside each launch of the step graph, "
                       "cvl_probe_arm)" % probe_n)
            if probe_s else "the launch repeated back to back on its own (20x, HIP events on its stream)",
            "burst_ms_per_launch": round(k_ms, 4),
            "burst_frac": round(k_flops / (k_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)}


def _line(metric, world, B, args, times, extra):
    el = _median_run(times)
    out = {"metric": metric, "value": round(world * B * args.steps / el, 3), "unit": "images/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1000.0 * el / args.steps, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
           "runs": {"n": len(times), "img_s": [round(world * B * args.steps / t, 3) for t in times],
                    "reported": "median run (SURVEY.md 8d: median of 3 runs of the timed steps)" if len(times) > 1
                                else "the one timed run (--full: median of 3)"}}
    if torch.cuda.is_available():     # peak HBM the step's tensors held (allocator high-water mark)
        out["peak_hbm_gib"] = round(torch.cuda.max_memory_allocated() / 2.0 ** 30, 3)
    out.update(extra)
    return out


def bench_retinanet(args):
    """configs[4]: RetinaNet ResNet-50-FPN 640x640 COCO-80, bs=8/GPU (3*bs candidates per step,
    anchor sizes 20..320 as train_retinanet_coco.py:343)."""
    from cvlite.retinanet import RetinaNet
    from cvlite.train_retinanet import RetinaTrainer, synthetic_coco_batch
    rank, world, local = dist.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    B = args.bs if args.bs != 16 else 8
    S = args.size if args.size != 512 else 640
    rn = RetinaNet(80, {}, anchor_sizes=[20.0, 40.0, 80.0, 160.0, 320.0])
    net = rn.model
    net.tower_probe = torch.zeros(4, dtype=torch.int64, device=dev) if args.full else None
    tr = RetinaTrainer(net, rn, B, S, n_max=50, world=world, use_graph=not args.no_graph)
    pool = [synthetic_coco_batch(3 * B, S, 80, n_max=50, seed=4321 + 97 * rank + i, device=dev) for i in range(2)]
    for i in range(2):                           # capture + one replay before the probe counts
        tr.load_candidates(*pool[i % 2])
        tr.step()
    torch.cuda.synchronize()
    if net.tower_probe is not None:
        net.tower_probe.zero_()
    times = timed_runs(tr.step, lambda b: tr.load_candidates(*b), pool, args, dev)
    if rank != 0:
        dist.barrier()
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, tr, net, head_cols=(36, 9 * 80))
    extra = {
        "data": "synthetic COCO-shaped: 3*bs candidates/step, 1+Poisson(6.3) boxes, C=80; random init",
        "config": {"workload": "RetinaNet R50-FPN train step (assign 3bs candidates + select + fwd + loss + "
                               "bwd + clip/SGD)", "model": "RetinaNet-ResNet50-FPN", "global_batch": B * world,
                   "image_size": S, "parallelism": "dp%d" % world},
        "last_step_losses_cls_reg": [round(x, 3) for x in tr.losses.double().sum(0).cpu().tolist()]}
    if args.full:
        in_s, in_n = nn.probe_seconds(net.tower_probe)
        net.tower_probe = None
        extra["roofline"] = tower_roofline(net, B, S, S, in_s, in_n, pmc=False)
    out = _line("training images/sec (whole node), RetinaNet-R50-FPN COCO 640x640 bs=8/GPU", world, B, args, times,
                extra)
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_retina(S, 80)
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()


def bench_centernet(args):
    """configs[3]: CenterNet hourglass (tf_centernet_hourglass.build_model defaults: separable,
    n_filters 128, 1 stack, 2 repeats) 512x512 VOC-20, bs=8/GPU, BN sub-batches of 2
    (train_hourglass_voc.py:317), Keras Adam."""
    from cvlite.hourglass_net import HourglassNet
    from cvlite.train_centernet import CenterNetTrainer, synthetic_batch as cn_batch
    rank, world, local = dist.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    B = args.bs if args.bs != 16 else 8
    S = args.size
    net = HourglassNet(NUM_CLASSES, device=dev, seed=0)
    tr = CenterNetTrainer(net, B, (S, S), sub_batch_sz=2, n_max=16, world=world, use_graph=not args.no_graph)
    pool = [cn_batch(B, S, S, NUM_CLASSES, n_max=16, seed=777 + 97 * rank + i, device=dev) for i in range(2)]
    times = timed_runs(tr.step, lambda b: tr.load_batch(*b), pool, args, dev)
    if rank != 0:
        dist.barrier()
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, tr, net)
    extra = {
        "data": "synthetic VOC-shaped: U[-1,1) images, 1+Poisson(1.4) boxes, C=20; random init",
        "config": {"workload": "CenterNet hourglass train step (centroid targets + fwd + loss + bwd + clip/Adam), "
                               "BN sub-batch 2", "model": "CenterNet-separable-hourglass-nf128",
                   "global_batch": B * world, "image_size": S, "parallelism": "dp%d" % world},
        "last_step_losses_cls_reg": [round(x, 3) for x in tr.losses.double().sum(0).cpu().tolist()]}
    if args.full:
        extra["roofline"] = centernet_roofline(net, tr, B, S)
    out = _line("training images/sec (whole node), CenterNet-hourglass VOC 512x512 bs=8/GPU", world, B, args, times,
                extra)
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_centernet(S, NUM_CLASSES)
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n, argv):
    """`bench.py --gpus N` outside torchrun: N ranks (one process per GPU) under
    torch.distributed.run, started as a child process; returns its exit status."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC (RCCL peer buffers)
    print("[bench] launching %d ranks: %s" % (n, " ".join(cmd)), file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def dp_timeline(tr, batch):
    """The gradient all-reduce plan of the step (dist.GradSync): per gradient group, in the order
    the backward finalises them, its bucket bytes; when the all-reduce path is live (world > 1, or
    one rank with CVL_DISPATCH=dp_force_sync under a process group) also one traced step's enqueue
    point (device ms from step start at the group's ready point, i.e. after the graph segment that
    finalises it) and the time its all-reduces completed.  Runs on every rank (collectives);
    outside the timed region."""
    sync = tr.sync
    if sync is None or not sync.active:
        plan = dist.GradSync(tr.net.store, tr.net.grad_groups()).plan()
        return {"live": False, "bucket_bytes": dist.BUCKET_BYTES,
                "groups": [{"group": n, "bucket_mb": [round(b / 2 ** 20, 2) for b in bs]} for n, bs in plan]}
    tr.load_batch(*batch)
    torch.cuda.synchronize()
    end = torch.cuda.Event(enable_timing=True)
    sync.begin_trace()
    t0 = sync.trace["t0"]
    tr.step()
    end.record()
    rows = sync.end_trace()
    return {"live": True, "bucket_bytes": dist.BUCKET_BYTES, "traced_step_ms": round(t0.elapsed_time(end), 3),
            "groups": [{"group": n, "bucket_mb": [round(b / 2 ** 20, 2) for b in bs], "ready_ms": round(r, 3),
                        "allreduce_done_ms": None if d is None else round(d, 3)} for n, bs, r, d in rows]}


def dist_info(world):
    import torch.distributed as tdist
    if tdist.is_available() and tdist.is_initialized():
        return {"backend": tdist.get_backend(), "world_size": tdist.get_world_size()}
    return {"backend": None, "world_size": world}


def dry_run(args):
    """Form the process group exactly as a bench run does, report the world, touch no GPU."""
    rank, world, _ = dist.init_from_env()
    info = dist_info(world)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "requested_gpus": args.gpus, "dist": info,
                          "global_batch": args.bs * world}), flush=True)
    dist.barrier()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=None,
                    help="timed runs of --steps steps each; the line reports the median (default 1; 3 with --full)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure: median of 3 timed runs, in-step tower probe, "
                         "roofline blocks, gradient all-reduce plan / trace, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (losses, head outputs, updated parameters) as "
                         "float32 DIR/<name>.npy")
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-probe", action="store_true",
                    help="no in-step tower timing (roofline from the burst timing; measurement-overhead A/B)")
    ap.add_argument("--model", default="fcos", choices=["fcos", "retinanet", "centernet"],
                    help="fcos = the headline metric (configs[1]/[2]); retinanet = configs[4] "
                         "(R50-FPN 640x640 COCO-80 bs=8/GPU), a side line")
    ap.add_argument("--dry-run", action="store_true", help="form the rank group, print the world, no GPU work")
    args = ap.parse_args()
    if args.runs is None:
        args.runs = 3 if args.full else 1
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    if args.dry_run:
        return dry_run(args)
    if args.model == "retinanet":
        return bench_retinanet(args)
    if args.model == "centernet":
        return bench_centernet(args)
    rank, world, local = dist.init_from_env()
    if args.gpus != world:
        print("warning: --gpus %d but WORLD_SIZE %d" % (args.gpus, world), file=sys.stderr)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    B, H, W = args.bs, args.size, args.size
    net = FCOSNet(NUM_CLASSES, device=dev, seed=0)       # identical init on every rank
    # in-step timing of the dominant kernel: each paired tower forward launch times itself from inside
    # (cvl_probe_arm: the slot rides in the launch arguments captured into the step graph); --full only
    net.tower_probe = torch.zeros(4, dtype=torch.int64, device=dev) if args.full and not args.no_probe else None
    tr = FCOSTrainer(net, B, (H, W), world=world, use_graph=not args.no_graph)
    pool = [synthetic_batch(B, H, W, NUM_CLASSES, seed=1234 + 97 * rank + i, device=dev) for i in range(4)]
    for i in range(2):                           # capture + one replay before the probe counts
        tr.load_batch(*pool[i % 4])
        tr.step()
    torch.cuda.synchronize()
    if net.tower_probe is not None:
        net.tower_probe.zero_()                  # count only the timed steps' tower launches
    times = timed_runs(tr.step, lambda b: tr.load_batch(*b), pool, args, dev)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, tr, net, head_cols=(5, NUM_CLASSES))
    losses = tr.losses.detach().double().sum(0).cpu().tolist()
    img_s = world * B * args.steps / _median_run(times)
    fl_img = train_flops_per_image(H, W)
    if args.full:
        in_s, in_n = nn.probe_seconds(net.tower_probe) if net.tower_probe is not None else (None, 0)
        grad_ar = dp_timeline(tr, pool[0])              # (replays the graph: the probe buffer stays live)
    if rank != 0:
        dist.barrier()
        return
    extra = {
        "data": "synthetic VOC-shaped: U[-1,1) 512x512 images, 1+Poisson(1.4) boxes, log-uniform 12-480 px, "
                "C=20; random-init (Keras glorot) weights",
        "config": {"workload": "FCOS ResNet-50-FPN train step (targets + fwd + loss + bwd + clip/SGD), "
                               "512x512, bs=16 per GPU",
                   "model": "FCOS-ResNet50-FPN", "global_batch": B * world, "image_size": H,
                   "parallelism": "dp%d" % world},
        "dist": dist_info(world),
        "model_flops_per_image": fl_img,
        "step_mfma_frac": round(img_s / world * fl_img / 1e12 / PEAK_BF16_TFLOPS, 4),
        "last_step_losses_cls_reg_cen": [round(x, 3) for x in losses]}
    if args.full:
        net.tower_probe = None
        roof = tower_roofline(net, B, H, W, in_s, in_n, pmc=(B, H, W) == (16, 512, 512))
        roof["backbone_3x3"] = measure_backbone_3x3(net, B, H, W)
        extra["roofline"] = roof
        extra["dist"] = dict(dist_info(world), grad_allreduce=grad_ar)
    out = _line(METRIC, world, B, args, times, extra)
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(H, W)
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()


if __name__ == "__main__":
    main()
