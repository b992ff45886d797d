"""What the tracking evaluation costs: event times of ``cvx_mot_frames`` (csrc/track_eval.hip) for a batch of 8 frames at 50, 300 and 1000
objects per frame beside ``cvx_track_update`` on the same frames, and of ``cvx_mot_summary`` at 64 x 200 identities x tracks and at the
capacity, 1024 x 4096.

    python tools/track_eval_cost.py [--batch 8] [--reps 20] [--out profiles/track_eval_cost.txt]

The scenes are those of tools/track_cost.py (seeded; one object per 90 x 90 pixels, integer positions drifting by up to 4 pixels a frame,
8 % drop-outs), with the objects as ground truth and the detections jittered by up to 2 px.  Tracker and evaluator first run 16 frames;
the timed call is the next ``--batch`` frames from that state, which is restored (a device copy, outside the event pair) before every
repetition.  The summary is timed on planted states: every identity overlaps a track of its own for 5 .. 60 frames and two more for
1 .. 5.  Each figure is the median over ``--reps`` of a device event pair around the call.  It sets no bar: the path did not exist
before, so there is no earlier figure."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def planted_c(np, seed, identities, tracks, gi, ti):
    rng = np.random.RandomState(seed)
    c = np.zeros((gi, ti), np.int32)
    own = rng.permutation(tracks)
    for o in range(identities):
        c[o, own[o % tracks]] = rng.randint(5, 61)
        c[o, rng.randint(0, tracks, 2)] += rng.randint(1, 6, 2).astype(np.int32)
    return c


def launch_summary(ev):
    """the launch alone: no host read inside the event pair"""
    from computervision.pytorch_amd import _lib as L
    L.check(L.load().cvx_mot_summary(L.ptr(ev.state), ev.streams, ev.max_gt_ids, ev.max_track_ids, L.ptr(ev.table), L.stream_ptr(ev.device)), "cvx_mot_summary")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_eval_cost.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_eval_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    import track_cost
    from computervision.pytorch_amd.track import Tracker
    from computervision.pytorch_amd.track_eval import HEADER_WORDS, TABLE, TrackingEvaluator

    dev = torch.device("cuda", 0)
    B, WARM = args.batch, 16

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

    def entry(name, times):
        return f"{name:100s} {times[0]:8.3f}  ({times[1]:.3f} .. {times[2]:.3f})"

    lines = [f"tracking evaluation, batch of {B} frames, one stream, default parameters, one MI355X; median (min .. max) ms over {args.reps} event pairs"]
    for nobj in (50, 300, 1000):
        rows, counts = track_cost.scene(np, nobj, nobj, WARM + B)
        # the scene again for its ground truth: the same generator, every object in every frame
        rng = np.random.RandomState(nobj)
        side = 90.0 * nobj ** 0.5
        cx, cy = rng.uniform(0, side, nobj), rng.uniform(0, side, nobj)
        vx, vy = rng.uniform(-4, 4, nobj), rng.uniform(-4, 4, nobj)
        half, cls = rng.randint(12, 36, (nobj, 2)), rng.randint(0, 3, nobj)
        gt = np.zeros((WARM + B, nobj, 6), np.float32)
        for f in range(WARM + B):
            x, y = np.rint(cx + vx * f), np.rint(cy + vy * f)
            gt[f] = np.stack([x - half[:, 0], y - half[:, 1], x + half[:, 0], y + half[:, 1], cls, np.arange(nobj)], 1)
        jit = np.random.RandomState(nobj + 1).randint(-2, 3, rows.shape[:2] + (2,)).astype(np.float32)
        rows[..., 0:2] += jit
        rows[..., 2:4] += jit
        r, c, g = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(gt).to(dev)
        gc = torch.full((WARM + B,), nobj, dtype=torch.int32, device=dev)
        tracker, ev = Tracker(dev), TrackingEvaluator(dev)
        ids = torch.cat([tracker.update(r[:WARM], c[:WARM]), torch.empty(B, nobj, dtype=torch.int32, device=dev)])
        ev.add_frames(r[:WARM], c[:WARM], ids[:WARM], g[:WARM], gc[:WARM])
        t_start, e_start = tracker.state.clone(), ev.state.clone()

        def track():
            ids[WARM:] = tracker.update(r[WARM:], c[WARM:])
        times = timed(track, before=lambda: tracker.state.copy_(t_start))
        lines.append(entry(f"cvx_track_update ({B} x {int(counts[WARM:].mean())} rows)", times))
        times = timed(lambda: ev.add_frames(r[WARM:], c[WARM:], ids[WARM:], g[WARM:], gc[WARM:]), before=lambda: ev.state.copy_(e_start))
        row = dict(zip(TABLE, ev.summary_table()[0].tolist()))
        assert not any(v for k, v in row.items() if k.startswith("flag_")), row
        hyps = int((ids[WARM:] >= 0).sum()) // B
        lines.append(entry(f"cvx_mot_frames   ({B} x {nobj} truths, {hyps} hypotheses; of {row['objects']} objects {row['matches']} matched, "
                           f"{row['switches']} switches)", times))
        tp = row["idtp"]
        lines.append(entry(f"cvx_mot_summary, that state (IDTP {tp})", timed(lambda: launch_summary(ev))))

    for identities, tracks in ((64, 200), (1024, 4096)):
        gi, ti = 1024, 4096
        ev = TrackingEvaluator(dev, max_gt_ids=gi, max_track_ids=ti)
        cmat = planted_c(np, identities, identities, tracks, gi, ti)
        head = np.zeros(8 * HEADER_WORDS + 20 * gi, np.uint8)
        head[8 * HEADER_WORDS + 8 * gi:8 * HEADER_WORDS + 12 * gi].view(np.int32)[:identities] = 100      # present
        ev.state.copy_(torch.from_numpy(np.concatenate([head, cmat.view(np.uint8).ravel()])).to(dev))
        times = timed(lambda: launch_summary(ev))
        tp = int(ev.summary_table()[0, 12])
        lines.append(entry(f"cvx_mot_summary ({identities} identities x {tracks} tracks planted, state {gi} x {ti}; IDTP {tp})", times))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
