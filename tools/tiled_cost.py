"""What tiled prediction costs beside ``predict_batch``: event times of the two launches of csrc/tiles.hip (cvx_tiles_u8_to_nchw,
cvx_det_merge_tiles) and of a whole YOLOv8-n ``predict_tiled`` on 1080 x 1920 frames at 640 x 640, next to ``predict_batch`` on the same
frames in the same process on the same device.

    python tools/tiled_cost.py [--frames 4] [--size 640] [--reps 20] [--out profiles/tiled_cost.txt]

Each figure is the median over ``--reps`` of a device event pair around the call, after a warm-up; the merge is timed on planted rows (300
per slot, all counted, jittered copies of 40 boxes per frame).  It sets no bar: the path did not exist before, so there is no earlier
figure."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_cost.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tiled_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import render as R
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8

    dev = torch.device("cuda", 0)
    F, S = args.frames, args.size
    cfg = Yolo8DetConfig()
    cfg.arch.input_size = (3, S, S)
    algo = YOLOv8(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    rng = np.random.RandomState(0)
    frames = [torch.from_numpy(rng.randint(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(dev) for _ in range(F)]
    batch = R.TileBatch(frames, (S, S), 0.2, True, True)
    slots = batch.slots
    base = rng.uniform(0, S - 120, (F, 40, 2)).astype(np.float32)
    rows = np.zeros((slots, 300, 6), np.float32)
    for s, f in enumerate(batch.slot_frame):
        xy = base[f, rng.randint(0, 40, 300)] + rng.uniform(-4, 4, (300, 2)).astype(np.float32)
        rows[s] = np.concatenate([xy, xy + 100, rng.uniform(0.1, 1, (300, 1)), rng.randint(0, 80, (300, 1))], 1)
    rows = torch.from_numpy(rows).to(dev)
    counts = torch.full((slots,), 300, dtype=torch.int32, device=dev)

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
        (f"cvx_tiles_u8_to_nchw + letterbox ({slots} slots)", batch.network_input),
        (f"cvx_det_merge_tiles ({slots} x 300 rows)", lambda: R.merge_tiles(rows, counts, batch.slot_map, batch.frame_hw)),
        ("predict_batch(sync=False)", lambda: algo.predict_batch(model, frames, sync=False)),
        ("predict_tiled(sync=False)", lambda: algo.predict_tiled(model, frames, sync=False)),
    ]
    lines = [f"tiled prediction, YOLOv8-n (random weights), {F} frames 1080 x 1920 at {S} x {S}, overlap 0.2, {slots} slots, one MI355X; "
             f"median (min .. max) ms over {args.reps} event pairs"]
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
