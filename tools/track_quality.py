"""The project's first tracking-quality figure: ``track.Tracker`` scored by ``track_eval.TrackingEvaluator`` (CLEAR-MOT and IDF1, DESIGN.md
section 7ac) on seeded SYNTHETIC scenes, at the default parameters and on a small grid of ``alpha``, ``beta`` and ``iou_high``.

    python tools/track_quality.py [--frames 80] [--out profiles/track_quality.txt]
    python tools/track_quality.py --models [--frames 80] [--out profiles/track_model_quality.txt]

``--models`` scores instead the four combinations of ``track.TrackModel`` -- the alpha-beta or the Kalman motion
model, the greedy or the minimum-cost association -- at ``track.DEFAULTS`` and the model's default weights on the same scenes: MOTA,
IDF1, identity switches and fragmentations per scene and over all of them.

The scenes are boxes drawn by a random generator, not footage: constant velocities with a slow sway, detections jittered by up to 2 px,
3 % of them dropped, scores from 0.6 .. 0.95 unless the scene says otherwise, 3 false detections per frame.  They say how the rules
behave where they are expected to differ -- crossings, gaps, low scores, density -- and NOTHING about real footage, whose detector errors
are neither uniform nor independent.  ``track.DEFAULTS`` is not changed by this tool or by its figures.

  lanes     16 objects of one class on 8 lanes, two per lane running against each other: they cross
  gaps      20 objects, each undetected for stretches of 5 .. 20 frames (the ground truth stays)
  lowscore  20 objects, each with stretches of 10 frames at scores 0.2 .. 0.45
  crowd50   50 objects of 3 classes drifting on a canvas of one object per 90 x 90 pixels
  crowd300  300 of them

Every scene is one stream of one tracker and one evaluator: a parameter set is scored in one pass over the five streams, with one host
read (``get_results``) at its end."""
import argparse
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("lanes", "gaps", "lowscore", "crowd50", "crowd300")
GRID = dict(alpha=(0.5, 0.75, 1.0), beta=(0.0, 0.25, 0.5), iou_high=(0.1, 0.2, 0.3))


def scene(np, name, frames, seed):
    """(rows (frames, K, 6), counts, gt (frames, G, 6), gt_counts) of the named scene"""
    rng = np.random.RandomState(seed)
    if name == "lanes":
        n = 16
        lane = np.arange(n) // 2
        cy, cx = 40.0 + 60.0 * lane, np.where(np.arange(n) % 2 == 0, 30.0, 30.0 + 6.0 * frames)
        vx, vy = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * rng.uniform(2.5, 3.5, n), np.zeros(n)
        cls, half = np.zeros(n), np.tile([20, 15], (n, 1))
    else:
        n = {"gaps": 20, "lowscore": 20, "crowd50": 50, "crowd300": 300}[name]
        side = 90.0 * n ** 0.5
        cx, cy = rng.uniform(0, side, n), rng.uniform(0, side, n)
        vx, vy = rng.uniform(-4, 4, n), rng.uniform(-4, 4, n)
        cls, half = rng.randint(0, 3, n), rng.randint(12, 36, (n, 2))
    sway, phase = rng.uniform(0, 6, n), rng.uniform(0, 6.28, n)
    hidden, low = np.zeros((frames, n), bool), np.zeros((frames, n), bool)
    if name in ("gaps", "lowscore"):
        for o in range(n):
            f = rng.randint(8, 20)
            while f < frames:
                length = rng.randint(5, 21) if name == "gaps" else 10
                (hidden if name == "gaps" else low)[f:f + length, o] = True
                f += length + rng.randint(10, 30)
    clutter = 3
    K = n + clutter
    rows, counts = np.zeros((frames, K, 6), np.float32), np.zeros(frames, np.int32)
    gt, gt_counts = np.zeros((frames, n, 6), np.float32), np.full(frames, n, np.int32)
    for f in range(frames):
        x = np.rint(cx + vx * f + sway * np.sin(0.15 * f + phase))
        y = np.rint(cy + vy * f + sway * np.cos(0.15 * f + phase))
        gt[f] = np.stack([x - half[:, 0], y - half[:, 1], x + half[:, 0], y + half[:, 1], cls, np.arange(n)], 1)
        seen = np.flatnonzero((rng.uniform(size=n) >= 0.03) & ~hidden[f])
        jx, jy = rng.randint(-2, 3, len(seen)), rng.randint(-2, 3, len(seen))
        score = np.where(low[f, seen], rng.uniform(0.2, 0.45, len(seen)), rng.uniform(0.6, 0.95, len(seen)))
        found = np.stack([x[seen] - half[seen, 0] + jx, y[seen] - half[seen, 1] + jy, x[seen] + half[seen, 0] + jx, y[seen] + half[seen, 1] + jy,
                          score, cls[seen]], 1)
        fx, fy = rng.uniform(0, max(x.max(), 100.0), clutter), rng.uniform(0, max(y.max(), 100.0), clutter)
        false = np.stack([fx, fy, fx + rng.uniform(20, 60, clutter), fy + rng.uniform(20, 60, clutter), rng.uniform(0.3, 0.7, clutter),
                          rng.randint(0, 3, clutter)], 1)
        both = np.concatenate([found, np.rint(false * [1, 1, 1, 1, 0, 1]) + false * [0, 0, 0, 0, 1, 0]])
        rows[f, :len(both)], counts[f] = both[rng.permutation(len(both))], len(both)
    return rows, counts, gt, gt_counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--models", action="store_true", help="score the four (motion, assign) combinations of TrackModel at the defaults")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "track_model_quality.txt" if args.models else "track_quality.txt")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_quality.py runs the tracker and its evaluation on the MI355X: no device found (there is no CPU path)")
    from computervision.pytorch_amd.track import ASSIGNS, DEFAULTS, MOTIONS, Tracker, TrackModel
    from computervision.pytorch_amd.track_eval import TrackingEvaluator

    dev = torch.device("cuda", 0)
    data = []
    for s, name in enumerate(SCENES):
        arrays = scene(np, name, args.frames, seed=100 + s)
        data.append([torch.from_numpy(a).to(dev) for a in arrays] + [torch.full((args.frames,), s, dtype=torch.int32, device=dev)])

    def score(model=None, **params):
        tracker = Tracker(dev, streams=len(SCENES), model=model, **params)
        evaluator = TrackingEvaluator(dev, streams=len(SCENES), max_gt_ids=512)
        for rows, counts, gt, gt_counts, stream in data:
            for f in range(0, args.frames, 8):                 # batches of 8 frames, as the video path feeds them
                sl = slice(f, f + 8)
                ids = tracker.update(rows[sl], counts[sl], stream[sl])
                evaluator.add_frames(rows[sl], counts[sl], ids, gt[sl], gt_counts[sl], stream[sl])
        assert tracker.overflowed() == 0
        return evaluator.get_results()

    def line(label, res):
        per = "  ".join(f"{r['mota']:6.3f} {r['idf1']:6.3f} {r['num_switches']:4d}" for r in res["streams"] + [res["overall"]])
        return f"{label:34s} {per}"

    def finish(lines):
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(text, end="")

    if args.models:
        names = SCENES + ("overall",)
        lines = [f"tracking quality of the four TrackModel combinations on SYNTHETIC seeded scenes ({args.frames} frames each; tools/track_quality.py says",
                 "what they are): MOTA, IDF1, identity switches and fragmentations per scene and over all of them, the evaluation's gate at IoU 0.5.",
                 "Boxes from a random generator: this says nothing about real footage.  The parameters are track.DEFAULTS and the model's default",
                 "weights; model=None stays the tracker's default, and this table moves nothing.  The first line is the tracker without a model",
                 "(cvx_track_update); the second is the same rules through cvx_track_update_model and must equal it.", "",
                 f"{'motion / assign':26s} " + "  ".join(f"{name:>23s}" for name in names),
                 f"{'':26s} " + "  ".join(f"{'MOTA':>6s} {'IDF1':>6s} {'IDSW':>4s} {'FRAG':>4s}" for _ in names)]

        def model_line(label, res):
            per = "  ".join(f"{r['mota']:6.3f} {r['idf1']:6.3f} {r['num_switches']:4d} {r['num_fragmentations']:4d}" for r in res["streams"] + [res["overall"]])
            return f"{label:26s} {per}"

        plain = score()
        lines.append(model_line("no model", plain))
        for motion in MOTIONS:
            for assign in ASSIGNS:
                res = score(model=TrackModel(motion=motion, assign=assign))
                lines.append(model_line(f"{motion} / {assign}", res))
                if (motion, assign) == ("alpha_beta", "greedy"):
                    counted = ("num_matches", "num_misses", "num_false_positives", "num_switches", "num_fragmentations", "idtp")
                    assert all(res["overall"][k] == plain["overall"][k] for k in counted), "TrackModel() does not score as the tracker without a model"
        finish(lines)
        return

    head = f"{'alpha beta iou_high':34s} " + "  ".join(f"{name:>18s}" for name in SCENES + ("overall",))
    sub = f"{'':34s} " + "  ".join(f"{'MOTA':>6s} {'IDF1':>6s} {'IDSW':>4s}" for _ in range(len(SCENES) + 1))
    lines = [f"tracking quality on SYNTHETIC seeded scenes ({args.frames} frames each; tools/track_quality.py says what they are): MOTA, IDF1 and identity",
             "switches of track.Tracker per scene and over all of them, the evaluation's gate at IoU 0.5.  Boxes from a random generator: this says",
             "nothing about real footage.  The other parameters are track.DEFAULTS, which this table does not change.", "", head, sub]
    default = score()
    lines.append(line(f"{DEFAULTS['alpha']:.2f} {DEFAULTS['beta']:.2f} {DEFAULTS['iou_high']:.2f}  (the defaults)", default))
    grid = []
    for alpha, beta, iou_high in itertools.product(GRID["alpha"], GRID["beta"], GRID["iou_high"]):
        res = score(alpha=alpha, beta=beta, iou_high=iou_high)
        grid.append(((alpha, beta, iou_high), res))
        lines.append(line(f"{alpha:.2f} {beta:.2f} {iou_high:.2f}", res))
    by_idf1 = max(grid, key=lambda g: g[1]["overall"]["idf1"])
    by_mota = max(grid, key=lambda g: g[1]["overall"]["mota"])
    lines += ["", f"the defaults:              overall MOTA {default['overall']['mota']:.4f}, IDF1 {default['overall']['idf1']:.4f}, "
                  f"{default['overall']['num_switches']} switches",
              f"best overall IDF1 of the grid: alpha {by_idf1[0][0]}, beta {by_idf1[0][1]}, iou_high {by_idf1[0][2]}: MOTA "
              f"{by_idf1[1]['overall']['mota']:.4f}, IDF1 {by_idf1[1]['overall']['idf1']:.4f}, {by_idf1[1]['overall']['num_switches']} switches",
              f"best overall MOTA of the grid: alpha {by_mota[0][0]}, beta {by_mota[0][1]}, iou_high {by_mota[0][2]}: MOTA "
              f"{by_mota[1]['overall']['mota']:.4f}, IDF1 {by_mota[1]['overall']['idf1']:.4f}, {by_mota[1]['overall']['num_switches']} switches",
              "Whether to move a default on the strength of generated boxes is left to a later change."]
    finish(lines)


if __name__ == "__main__":
    main()
