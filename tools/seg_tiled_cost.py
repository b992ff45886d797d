"""What sliding-window segmentation costs beside ``predict_batch``: event times of the ``cvx_seg_stitch`` launch alone (csrc/seg_tiles.hip)
and of a whole DeepLabv3+ ``segment_tiled(sync=False)`` on 1024 x 2048 frames at 513 x 513 -- at the default batch size (equal chunks) and at one that
leaves unequal chunks, beside the forwards alone --, next to ``predict_batch`` on the same frames in the same process on the same device.

    python tools/seg_tiled_cost.py [--frames 2] [--height 1024] [--width 2048] [--size 513] [--reps 20] [--out profiles/seg_tiled_cost.txt]

Each figure is the median (and the range) over ``--reps`` of a device event pair around the call, after a warm-up; the stitch is timed on
seeded normal logits, with and without the overlay and the confusion counts.  It sets no bar: the path did not exist before, so there is
no earlier figure."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_tiled_cost.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("seg_tiled_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import render as R
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA

    dev = torch.device("cuda", 0)
    F, S, H, W = args.frames, args.size, args.height, args.width
    cfg = DeeplabV3PlusConfig()
    cfg.arch.input_size, cfg.arch.backbone_pretrained = (3, S, S), False
    algo = DeeplabV3PlusA(cfg, dev)
    nc = algo.num_classes
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    rng = np.random.RandomState(0)
    frames = [torch.from_numpy(rng.randint(0, 256, (H, W, 3), dtype=np.uint8)).to(dev) for _ in range(F)]
    targets = [torch.from_numpy(rng.randint(0, nc, (H, W)).astype(np.uint8)).to(dev) for _ in range(F)]
    batch = R.TileBatch(frames, (S, S), args.overlap, full_frame=False)
    slots = batch.slots
    with torch.no_grad():
        one = model.forward_rows(batch.network_input()[:1])
    lh, lw = model._last_engine.graph.level_hw[0]
    ld = int(one.shape[2])
    logits = torch.randn(slots, lh * lw, ld, device=dev)
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)

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

    # the engine re-plans its per-batch buffers (and waits for its streams) whenever a forward's batch size differs from the previous
    # one, which is why segment_tiled cuts the slots into equal chunks (render.slot_chunks); the last arm shows unequal ones
    chunks = R.slot_chunks(slots, 16)
    uneven = next((b for b in range(16, 0, -1) if len({c1 - c0 for c0, c1 in R.slot_chunks(slots, b)}) > 1), 16)
    x_all = batch.network_input()

    def forward_only():
        with torch.no_grad():
            for c0, c1 in chunks:
                chunk = x_all[c0:c1]
                model.forward_rows(chunk if chunk.data_ptr() % 8 == 0 else chunk.clone())      # as segment_tiled does

    def stitch(**kw):
        return lambda: R.stitch_segmentation(frames, logits, nc, (lh, lw), (S, S), batch, **kw)

    arms = [
        (f"cvx_tiles_u8_to_nchw ({slots} slots)", batch.network_input),
        ("cvx_seg_stitch, labels, linear", stitch()),
        ("cvx_seg_stitch, labels, mean", stitch(weight="mean")),
        ("cvx_seg_stitch, labels + overlay", stitch(draw=True)),
        ("cvx_seg_stitch, labels + overlay + counts", stitch(draw=True, targets=targets, counts=counts)),
        ("predict_batch(sync=False)", lambda: algo.predict_batch(model, frames, sync=False)),
        (f"forward_rows alone, chunks {[c1 - c0 for c0, c1 in chunks]}", forward_only),
        ("segment_tiled(sync=False), batch_size 16", lambda: algo.segment_tiled(model, frames, overlap=args.overlap, sync=False)),
        (f"segment_tiled(sync=False), batch_size {uneven}: {[c1 - c0 for c0, c1 in R.slot_chunks(slots, uneven)]}",
         lambda: algo.segment_tiled(model, frames, overlap=args.overlap, batch_size=uneven, sync=False)),
    ]
    lines = [f"sliding-window segmentation, DeepLabv3+ R101 (random weights, {nc} classes, ld {ld}), {F} frames {H} x {W} at {S} x {S}, "
             f"overlap {args.overlap}, {slots} slots, logits level {lh} x {lw}, one MI355X; median (min .. max) ms over {args.reps} event pairs"]
    for name, fn in arms:
        med, lo, hi = timed(fn)
        lines.append(f"{name:58s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
