"""What batched prediction costs beside the forward: event times of the four launches of computervision.pytorch_amd/render.py
(cvx_letterbox_batch_u8_to_nchw, cvx_det_to_image, cvx_draw_detections, cvx_seg_overlay) and of a whole YOLOv8-n ``predict_batch`` at batch
32, 640 x 640, next to the eval forward of the same process on the same device.

    python tools/predict_cost.py [--batch 32] [--size 640] [--reps 20] [--out profiles/predict_cost.txt]

Each figure is the median over ``--reps`` of a device event pair around the call, after a warm-up; the launches are timed on planted
inputs (300 rows per frame, 64 of them counted).  It sets no bar: the path did not exist before, so there is no earlier figure."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_cost.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("predict_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import render as R
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8

    dev = torch.device("cuda", 0)
    B, S = args.batch, args.size
    cfg = Yolo8DetConfig()
    cfg.arch.input_size = (3, S, S)
    algo = YOLOv8(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    rng = np.random.RandomState(0)
    shapes = [(480, 640), (375, 500), (720, 1280), (S, S)]
    frames = [torch.from_numpy(rng.randint(0, 256, shapes[i % 4] + (3,), dtype=np.uint8)).to(dev) for i in range(B)]
    rows = torch.rand(B, 300, 6, device=dev) * 300
    rows[..., 2:4] += rows[..., 0:2]
    rows[..., 4] = torch.rand(B, 300, device=dev)
    rows[..., 5] = torch.randint(0, 80, (B, 300), device=dev).float()
    counts = torch.full((B,), 64, dtype=torch.int32, device=dev)
    batch = R.FrameBatch(frames, (S, S), True)
    x = batch.network_input()
    logits = torch.randn(B, (S // 4) * (S // 4), 24, device=dev)

    def timed(fn):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    def forward():
        with torch.no_grad():
            model(x)

    arms = [
        ("eval forward", forward),
        ("cvx_letterbox_batch_u8_to_nchw", batch.network_input),
        ("cvx_det_to_image", lambda: R.det_to_image(rows, counts, batch.box_map)),
        ("cvx_draw_detections", lambda: R.draw_detections(frames, rows, counts, batch=batch)),
        ("cvx_seg_overlay (21 classes)", lambda: R.seg_overlay(frames, logits, 21, (S // 4, S // 4), (S, S), batch=batch)),
        ("predict_batch(draw=True, sync=False)", lambda: algo.predict_batch(model, frames, draw=True, sync=False)),
    ]
    lines = [f"batched prediction, YOLOv8-n, batch {B}, {S} x {S}, frames {shapes} in turn, one MI355X; median (min .. max) ms over {args.reps} event pairs"]
    for name, fn in arms:
        med, lo, hi = timed(fn)
        lines.append(f"{name:40s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
