"""What scale and flip test-time augmentation costs a detector beside the plain ``predict_batch``: event times of the two launches of
csrc/det_tta.hip -- ``cvx_det_tta_inputs`` alone, ``cvx_det_fuse_views`` alone in both modes on seeded rows -- and of the whole augmented
``predict_batch(tta=...)`` of YOLOv8-n next to the plain ``predict_batch`` on the same frames in the same process on the same device.

    python tools/det_tta_cost.py [--batch 32] [--size 640] [--reps 20] [--out profiles/det_tta_cost.txt]

Each figure is the median (and the range) over ``--reps`` device event pairs around the call, after a warm-up.  The fusion is timed on
planted rows: 300 per slot, all counted, jittered copies of 40 boxes per frame written in each view's own coordinates.  It sets no bar: the
path did not exist before, so there is no earlier figure; and the weights are random, so there is no accuracy figure either."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_tta_cost.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("det_tta_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import det_tta as T
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
    tta = T.DetTTA()
    V = tta.n_views
    rng = np.random.RandomState(0)
    frames = [torch.from_numpy(rng.randint(0, 256, (480, 640, 3), dtype=np.uint8)).to(dev) for _ in range(B)]
    fb = R.FrameBatch(frames, (S, S), True)
    x = fb.network_input()
    table = T.view_table(tta.views((S, S)), (S, S))
    vmap = tta.view_map(fb.image_hw, (S, S), terms=algo._box_map_terms(fb.image_hw, (S, S)))
    frame_hw = fb.image_hw.to(torch.int32)
    # planted rows: per frame 40 boxes of the picture, every slot holds 300 jittered copies in its view's own coordinates
    m = vmap.cpu().numpy().astype(np.float64)
    base = np.stack([rng.uniform(0, 640 - 120, (B, 40)), rng.uniform(0, 480 - 120, (B, 40))], 2)
    rows = np.zeros((V * B, 300, 6), np.float32)
    for s in range(V * B):
        xy = base[s % B, rng.randint(0, 40, 300)] + rng.uniform(-4, 4, (300, 2))
        xs = np.sort((np.stack([xy[:, 0], xy[:, 0] + 100], 1) - m[s, 1]) / m[s, 0], 1)
        ys = (np.stack([xy[:, 1], xy[:, 1] + 100], 1) - m[s, 3]) / m[s, 2]
        rows[s] = np.concatenate([xs[:, :1], ys[:, :1], xs[:, 1:], ys[:, 1:], rng.uniform(0.1, 1, (300, 1)), rng.randint(0, 80, (300, 1))], 1)
    rows = torch.from_numpy(rows).to(dev)
    counts = torch.full((V * B,), 300, dtype=torch.int32, device=dev)

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

    arms = [
        (f"cvx_det_tta_inputs ({B} -> {V * B} slots)", lambda: T.tta_inputs(x, table)),
        (f"cvx_det_fuse_views, nms ({V * B} x 300 rows)", lambda: T.fuse_views(rows, counts, vmap, frame_hw, algo.iou_threshold, fuse="nms")),
        (f"cvx_det_fuse_views, vote ({V * B} x 300 rows)", lambda: T.fuse_views(rows, counts, vmap, frame_hw, algo.iou_threshold, fuse="vote")),
        ("predict_batch(sync=False)", lambda: algo.predict_batch(model, frames, sync=False)),
        ("predict_batch(sync=False, tta=DetTTA())", lambda: algo.predict_batch(model, frames, sync=False, tta=tta)),
    ]
    lines = [f"detector test-time augmentation, YOLOv8-n (random weights), {B} frames 480 x 640 at {S} x {S}, views "
             f"{list(zip(tta.scales, tta.flips))}, one MI355X; median (min .. max) ms over {args.reps} event pairs"]
    for name, fn in arms:
        med, lo, hi = timed(fn)
        lines.append(f"{name:50s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
