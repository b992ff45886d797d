"""What Weighted Boxes Fusion costs: event times of ``cvx_det_fuse_wbf`` alone beside ``cvx_det_fuse_views`` in ``"vote"`` mode on the same
planted rows (the rows of tools/det_tta_cost.py), of ``predict_batch(tta=DetTTA(fusion=WBF()))`` of YOLOv8-n beside
``predict_batch(tta=DetTTA())`` on the same frames, and of the kernel's worst case: one frame of 8192 candidates, over 20 classes and
class-agnostic.

    python tools/box_fusion_cost.py [--batch 32] [--size 640] [--reps 20] [--out profiles/box_fusion_cost.txt]

Each figure is the median (and the range) over ``--reps`` device event pairs around the call, after a warm-up.  It sets no bar: the path
did not exist before; and the weights are random, so there is no accuracy figure either."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_fusion_cost.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("box_fusion_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import box_fusion as BF
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
    tta, tta_wbf = T.DetTTA(), T.DetTTA(fusion=BF.WBF())
    V = tta.n_views
    rng = np.random.RandomState(0)
    frames = [torch.from_numpy(rng.randint(0, 256, (480, 640, 3), dtype=np.uint8)).to(dev) for _ in range(B)]
    fb = R.FrameBatch(frames, (S, S), True)
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
    # the worst case: one frame of 8192 candidates from 8 sources -- 2048 places of 4 jittered copies each (so about 2048 clusters), and
    # 8192 boxes that overlap nothing (8192 clusters); 20 classes
    place = np.arange(8192) // 4
    corner = np.stack([(place % 64) * 30.0, (place // 64) * 30.0], 1) + rng.uniform(-1, 1, (8192, 2))
    full = np.concatenate([corner, corner + 24.0, rng.uniform(0.1, 1, (8192, 1)), (place % 20)[:, None]], 1).astype(np.float32)
    k = np.arange(8192)
    apart = full.copy()
    apart[:, :4] = np.stack([(k % 128) * 15.0, (k // 128) * 15.0, (k % 128) * 15.0 + 10, (k // 128) * 15.0 + 10], 1)
    order = rng.permutation(8192)
    full_rows, apart_rows = (torch.from_numpy(a[order].reshape(8, 1024, 6)).to(dev) for a in (full, apart))
    full_counts = torch.full((8,), 1024, dtype=torch.int32, device=dev)
    full_map = torch.tensor([[1.0, 0.0, 1.0, 0.0]] * 8, device=dev)
    full_hw = torch.tensor([[2000, 2000]], dtype=torch.int32, device=dev)

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

    def worst(r, agnostic):
        return lambda: BF.fuse_wbf(r, full_counts, full_map, full_hw, class_agnostic=agnostic)

    arms = [
        (f"cvx_det_fuse_views, vote ({V * B} x 300 rows)", lambda: T.fuse_views(rows, counts, vmap, frame_hw, algo.iou_threshold, fuse="vote")),
        (f"cvx_det_fuse_wbf ({V * B} x 300 rows)", lambda: BF.fuse_wbf(rows, counts, vmap, frame_hw)),
        (f"cvx_det_fuse_wbf, class-agnostic ({V * B} x 300 rows)", lambda: BF.fuse_wbf(rows, counts, vmap, frame_hw, class_agnostic=True)),
        ("predict_batch(sync=False, tta=DetTTA())", lambda: algo.predict_batch(model, frames, sync=False, tta=tta)),
        ("predict_batch(sync=False, tta=DetTTA(fusion=WBF()))", lambda: algo.predict_batch(model, frames, sync=False, tta=tta_wbf)),
        ("one frame, 8192 rows in ~2048 clusters, 20 classes", worst(full_rows, False)),
        ("one frame, 8192 rows in ~2048 clusters, agnostic", worst(full_rows, True)),
        ("one frame, 8192 rows in 8192 clusters, 20 classes", worst(apart_rows, False)),
        ("one frame, 8192 rows in 8192 clusters, agnostic", worst(apart_rows, True)),
    ]
    lines = [f"Weighted Boxes Fusion, YOLOv8-n (random weights), {B} frames 480 x 640 at {S} x {S}, views "
             f"{list(zip(tta.scales, tta.flips))}, one MI355X; median (min .. max) ms over {args.reps} event pairs"]
    for name, fn in arms:
        med, lo, hi = timed(fn)
        lines.append(f"{name:56s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
    clusters = [int(BF.fuse_wbf(r, full_counts, full_map, full_hw, class_agnostic=a, max_det=8192)[1][0]) for r in (full_rows, apart_rows) for a in (False, True)]
    lines.append(f"clusters of the four one-frame cases: {clusters}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
