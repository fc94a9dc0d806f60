"""One RetinaTrainer step (captured graph) of RetinaNet on a chosen backbone, timed with HIP events:
img/s = batch / median step time.  A single-box figure for DESIGN.md (bench.py is the yardstick of
the flagship workload; this tool is for backbones it does not run).
usage: retina_step.py [--backbone resnext50] [--bs 8] [--size 640] [--classes 80] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cv-lite-object-detection_amd")]
import torch  # noqa: E402

from cvlite.retinanet import RetinaNet  # noqa: E402
from cvlite.train_retinanet import RetinaTrainer, synthetic_coco_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnext50")
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retina_step.py times a training step: it needs the GPU")
    rn = RetinaNet(args.classes, {}, backbone_model=args.backbone)
    tr = RetinaTrainer(rn.model, rn, args.bs, args.size)
    tr.load_candidates(*synthetic_coco_batch(3 * args.bs, args.size, args.classes, seed=1234, device="cuda"))
    for _ in range(args.warmup):
        tr.step()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        losses = tr.step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    med = statistics.median(times)
    print(json.dumps({"backbone": args.backbone, "bs": args.bs, "size": args.size, "classes": args.classes,
                      "step_ms_median": round(med, 3), "step_ms_min": round(min(times), 3),
                      "img_per_s": round(args.bs * 1e3 / med, 1), "loss": float(losses.sum()),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
