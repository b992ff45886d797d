"""What multi-scale / flip test-time augmentation costs beside the plain evaluation: event times of the ``cvx_seg_tta_inputs`` launches and of
the ``cvx_seg_fuse`` launch alone (csrc/seg_tta.hip) -- both modes, with and without the confusion counts and the probabilities --, and of
the whole augmented evaluation of one batch (``SegTTA.run`` + ``cvx_seg_fuse``) next to the plain ``forward_rows`` + ``cvx_seg_criterion_eval`` of the
same batch, in the same process on the same device.

    python tools/seg_tta_cost.py [--batch 8] [--size 513] [--scales 0.5 0.75 1.0 1.25 1.5 1.75] [--no-flip] [--reps 20] [--out profiles/seg_tta_cost.txt]

Each figure is the median (and the range) over ``--reps`` of a device event pair around the call, after a warm-up; the fusion is timed on
seeded normal logits at the level sizes the views really have.  It sets no bar: the path did not exist before, so there is no earlier
figure."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--scales", type=float, nargs="+", default=[0.5, 0.75, 1.0, 1.25, 1.5, 1.75])
    ap.add_argument("--no-flip", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_tta_cost.txt"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("seg_tta_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import seg_tta as T
    from computervision.pytorch_amd.deeplab import SegLoss
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from core.trainer.segmentation_trainer import SegmentationMetrics

    dev = torch.device("cuda", 0)
    B, S, flip = args.batch, args.size, not args.no_flip
    cfg = DeeplabV3PlusConfig()
    cfg.arch.input_size, cfg.arch.backbone_pretrained = (3, S, S), False
    algo = DeeplabV3PlusA(cfg, dev)
    nc = algo.num_classes
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    ld = model.layout.nc_pad
    g = torch.Generator().manual_seed(1)
    images = torch.rand(B, 3, S, S, generator=g).to(dev)
    targets = torch.randint(0, nc, (B, S, S), generator=g).to(dev)
    tta = {m: T.SegTTA(args.scales, flip, m) for m in ("logits", "prob")}
    sizes = tta["prob"].view_sizes(S, S)
    real = tta["prob"].run(model, images)                  # the first use of every engine; the level size of every view
    drawn = [T.SegView(3.0 * torch.randn(v.rows.shape, device=dev, generator=torch.Generator(dev).manual_seed(2 + k)), v.level_hw, v.flip)
             for k, v in enumerate(real)]
    del real
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    metrics, criterion, loss = SegmentationMetrics(nc, device=dev), SegLoss("ce"), torch.zeros(1, device=dev)

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

    def fuse(mode, **kw):
        return lambda: T.fuse(drawn, nc, ld, (S, S), mode=mode, **kw)

    def plain():
        with torch.no_grad():
            rows = model.forward_rows(images)
        metrics.add_rows(rows, targets, model._last_engine.graph.level_hw[0], criterion, loss)

    def forwards_only():
        tta["prob"].run(model, images)

    def augmented(mode):
        def fn():
            views = tta[mode].run(model, images)
            tta[mode].fuse(views, nc, ld, (S, S), targets=targets, counts=counts, labels=False)
        return fn

    with_counts = dict(targets=targets, counts=counts)
    arms = [(f"cvx_seg_tta_inputs, {S} -> {hw[0]} x {hw[1]}", (lambda hw=hw: T.tta_inputs(images, hw, flip))) for hw in sizes]
    arms += [
        ("cvx_seg_fuse, logits, labels", fuse("logits")),
        ("cvx_seg_fuse, logits, labels + counts", fuse("logits", **with_counts)),
        ("cvx_seg_fuse, logits, counts alone", fuse("logits", labels=False, **with_counts)),
        ("cvx_seg_fuse, prob, labels", fuse("prob")),
        ("cvx_seg_fuse, prob, labels + counts", fuse("prob", **with_counts)),
        ("cvx_seg_fuse, prob, labels + counts + probabilities", fuse("prob", probs=True, **with_counts)),
        ("plain: forward_rows + cvx_seg_criterion_eval", plain),
        ("SegTTA.run alone (inputs + forwards)", forwards_only),
        ("augmented evaluation of the batch, logits", augmented("logits")),
        ("augmented evaluation of the batch, prob", augmented("prob")),
    ]
    lines = [f"test-time augmentation, DeepLabv3+ R101 (random weights, {nc} classes, ld {ld}), batch {B} at {S} x {S}, scales {args.scales}, "
             f"flip {flip}: {len(drawn)} views, inputs {sizes}, levels {[v.level_hw for v in drawn][::2 if flip else 1]}, one MI355X; "
             f"median (min .. max) ms over {args.reps} event pairs"]
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
