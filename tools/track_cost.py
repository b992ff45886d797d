"""What tracking costs beside ``predict_batch``: event times of ``cvx_track_update`` (csrc/track.hip) for a batch of 8 frames at 50, 300 and
1000 detections per frame, next to one YOLOv8-n ``predict_batch`` of 8 frames in the same process on the same device.

    python tools/track_cost.py [--batch 8] [--size 640] [--reps 20] [--out profiles/track_cost.txt]
    python tools/track_cost.py --models [--batch 8] [--reps 20] [--out profiles/track_model_cost.txt]

``--models`` times instead ``cvx_track_update_model`` for the four combinations of ``track.TrackModel`` on the same
three scenes, beside ``cvx_track_update`` in the same process: the calls alternate within every repetition, so all five see the same machine.

The scene is seeded: objects of 3 classes on a canvas that grows with their number (one object per 90 x 90 pixels), integer positions
drifting by up to 4 pixels a frame, 8 % drop-outs, a quarter of the scores from 0.3 .. 0.95.  The tracker first runs 16 frames so that its
tracks are confirmed; the timed call is the next ``--batch`` frames from that state, which is restored (a device copy, outside the event
pair) before every repetition.  Each figure is the median over ``--reps`` of a device event pair around the call.  It sets no bar: the
path did not exist before, so there is no earlier figure."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(np, seed, nobj, frames):
    """(rows (frames, K, 6), counts (frames)) with K = nobj"""
    rng = np.random.RandomState(seed)
    side = 90.0 * nobj ** 0.5
    cx, cy = rng.uniform(0, side, nobj), rng.uniform(0, side, nobj)
    vx, vy = rng.uniform(-4, 4, nobj), rng.uniform(-4, 4, nobj)
    half = rng.randint(12, 36, (nobj, 2))
    cls = rng.randint(0, 3, nobj)
    rows, counts = np.zeros((frames, nobj, 6), np.float32), np.zeros(frames, np.int32)
    for f in range(frames):
        seen = np.flatnonzero(rng.uniform(size=nobj) >= 0.08)
        x, y = np.rint(cx[seen] + vx[seen] * f), np.rint(cy[seen] + vy[seen] * f)
        score = np.where(rng.uniform(size=len(seen)) < 0.25, rng.uniform(0.3, 0.95, len(seen)), rng.uniform(0.6, 0.95, len(seen)))
        found = np.stack([x - half[seen, 0], y - half[seen, 1], x + half[seen, 0], y + half[seen, 1], score, cls[seen]], 1)
        rows[f, :len(seen)], counts[f] = found[rng.permutation(len(seen))], len(seen)
    return rows, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--models", action="store_true", help="time the four (motion, assign) combinations of TrackModel beside cvx_track_update")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "track_model_cost.txt" if args.models else "track_cost.txt")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd.track import ASSIGNS, MOTIONS, Tracker, TrackModel
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8

    dev = torch.device("cuda", 0)
    B, S, WARM = args.batch, args.size, 16

    def timed(fn, before=None):
        ms = []
        for rep in range(3 + args.reps):
            if before is not None:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    def finish(lines):
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(text, end="")

    if args.models:
        lines = [f"tracking with a TrackModel, batch of {B} frames, one stream, default parameters and weights, one MI355X; median (min .. max) ms over",
                 f"{args.reps} event pairs, the five calls alternating within every repetition of one process.  Each tracker first ran {WARM} frames; its",
                 "state and covariances are restored (device copies outside the event pair) before every timed call.  No bar: the paths are new."]
        for nobj in (50, 300, 1000):
            rows, counts = scene(np, nobj, nobj, WARM + B)
            r, c = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev)
            cases = [("cvx_track_update (no model)", Tracker(dev))]
            cases += [(f"{motion} / {assign}", Tracker(dev, model=TrackModel(motion=motion, assign=assign))) for motion in MOTIONS for assign in ASSIGNS]
            saved, ms = [], [[] for _ in cases]
            for _, tracker in cases:
                tracker.update(r[:WARM], c[:WARM])
                saved.append((tracker.state.clone(), None if tracker.ext is None else tracker.ext.clone(), len(tracker.tracks()["id"])))
            for rep in range(3 + args.reps):
                for k, (_, tracker) in enumerate(cases):
                    tracker.state.copy_(saved[k][0])
                    if tracker.ext is not None:
                        tracker.ext.copy_(saved[k][1])
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    tracker.update(r[WARM:], c[WARM:])
                    b.record()
                    b.synchronize()
                    if rep >= 3:
                        ms[k].append(a.elapsed_time(b))
            lines.append(f"{B} x {int(counts[WARM:].mean())} rows per frame")
            for k, (name, tracker) in enumerate(cases):
                after = tracker.tracks()
                label = f"  {name} ({saved[k][2]} tracks -> {len(after['id'])}, ids to {after['next_id']})"
                lines.append(f"{label:78s} {statistics.median(ms[k]):8.3f}  ({min(ms[k]):.3f} .. {max(ms[k]):.3f})")
                assert tracker.overflowed() == 0
        finish(lines)
        return

    lines = [f"tracking, batch of {B} frames, one stream, default parameters, one MI355X; median (min .. max) ms over {args.reps} event pairs"]
    for nobj in (50, 300, 1000):
        rows, counts = scene(np, nobj, nobj, WARM + B)
        r, c = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev)
        tracker = Tracker(dev)
        tracker.update(r[:WARM], c[:WARM])
        start = tracker.state.clone()
        live = len(tracker.tracks()["id"])
        med, lo, hi = timed(lambda: tracker.update(r[WARM:], c[WARM:]), before=lambda: tracker.state.copy_(start))
        after = tracker.tracks()
        name = f"cvx_track_update ({B} x {int(counts[WARM:].mean())} rows, {live} tracks -> {len(after['id'])}, ids to {after['next_id']})"
        lines.append(f"{name:78s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
        assert tracker.overflowed() == 0

    cfg = Yolo8DetConfig()
    cfg.arch.input_size = (3, S, S)
    algo = YOLOv8(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    rng = np.random.RandomState(0)
    frames = [torch.from_numpy(rng.randint(0, 256, (720, 1280, 3), dtype=np.uint8)).to(dev) for _ in range(B)]
    for name, fn in ((f"predict_batch(sync=False), YOLOv8-n (random weights), {B} frames 720 x 1280 at {S} x {S}",
                      lambda: algo.predict_batch(model, frames, sync=False)),
                     ("the same with tracker= (few rows: an untrained network)",
                      lambda t=Tracker(dev): algo.predict_batch(model, frames, sync=False, tracker=t))):
        med, lo, hi = timed(fn)
        lines.append(f"{name:78s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
    finish(lines)


if __name__ == "__main__":
    main()
