"""What the boundary metrics cost: event times of ``cvx_seg_boundary`` (csrc/seg_boundary.hip) -- the entry alone on prepared tables, and
the whole ``seg_boundary.boundary_counts`` call -- on 16 maps of 513 x 513 with widths (1, 2, 4, 8, 15) and on two maps of 1024 x 2048 with
``ratio=(0.02,)`` (d = 46), beside ``cvx_seg_fuse`` with one view and ``cvx_seg_stitch`` on the same frames; then one ``evaluate_on_voc``
batch of DeepLabv3+ with and without ``boundary=``.

    python tools/seg_boundary_cost.py [--reps 20] [--out profiles/seg_boundary_cost.txt]

Each figure is the median (and the range) over ``--reps`` of a device event pair around the call, after a warm-up.  It sets no bar: the path
did not exist before, so there is no earlier figure.  The maps are blobs about 48 pixels across (the arg max of interpolated coarse noise planes); the prediction is
the target moved by two pixels with 2 % of the pixels redrawn ("near"), or an unrelated map of such blobs ("unrelated": many contour pixels
find no pixel of their class nearby, the longest search).  "Fine texture" is the dear input, a map in which most pixels lie on a contour."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_boundary_cost.txt"))
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("seg_boundary_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import render as R
    from computervision.pytorch_amd import seg_boundary as SB
    from computervision.pytorch_amd import seg_tta as T
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from core.trainer.segmentation_trainer import SegmentationMetrics

    dev = torch.device("cuda", 0)
    S = args.size
    cfg = DeeplabV3PlusConfig()
    cfg.arch.input_size, cfg.arch.backbone_pretrained = (3, S, S), False
    algo = DeeplabV3PlusA(cfg, dev)
    nc = algo.num_classes
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()

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

    gen = torch.Generator(device=dev).manual_seed(1)

    def blobby(n, h, w, cell=48):
        """labels 0 .. nc - 1 in blobs about ``cell`` pixels across: the arg max of noise planes drawn on a coarse grid and interpolated"""
        z = torch.rand(n, nc, h // cell + 2, w // cell + 2, device=dev, generator=gen)
        return F.interpolate(z, size=(h, w), mode="bilinear", align_corners=False).argmax(1).to(torch.uint8)

    def texture(n, h, w, blur=31):
        """the dear input: the arg max of box-blurred per-pixel noise, a fine texture in which most pixels lie on a contour"""
        out = []
        for _ in range(n):
            z = torch.rand(1, nc, h, w, device=dev, generator=gen)
            out.append(F.avg_pool2d(z, blur, 1, blur // 2).argmax(1)[0].to(torch.uint8))
        return torch.stack(out)

    def near(target):
        p = torch.roll(target, (2, -2), (1, 2)).clone()
        redraw = torch.rand(target.shape, device=dev, generator=gen) < 0.02
        p[redraw] = torch.randint(0, nc, (int(redraw.sum()),), device=dev, generator=gen, dtype=torch.uint8)
        return p

    lines = []
    with torch.no_grad():
        one = model.forward_rows(torch.rand(1, 3, S, S, device=dev, generator=gen))
    lh, lw = model._last_engine.graph.level_hw[0]
    ld = int(one.shape[2])
    for n, h, w, spec in ((args.batch, S, S, SB.SegBoundary((1, 2, 4, 8, 15))), (2, 1024, 2048, SB.SegBoundary(ratio=(0.02,)))):
        target, fine = blobby(n, h, w), texture(n, h, w)
        target[:, : h // 8, : w // 8] = 255                                   # a void corner
        frames = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
        batch = R.TileBatch(frames, (S, S), args.overlap, full_frame=False)
        lines.append(f"{n} maps {h} x {w}, {nc} classes, widths {spec.frame_widths(h, w)}  ({batch.slots} slots at {S} x {S})")
        logits = torch.randn(batch.slots, lh * lw, ld, device=dev, generator=gen)
        med, lo, hi = timed(lambda: R.stitch_segmentation(frames, logits, nc, (lh, lw), (S, S), batch))
        lines.append(f"  {'cvx_seg_stitch, labels (for scale)':66s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
        view = [T.SegView(torch.randn(n, lh * lw, ld, device=dev, generator=gen), (lh, lw), False)]
        med, lo, hi = timed(lambda: T.fuse(view, nc, ld, (h, w), mode="prob"))
        lines.append(f"  {'cvx_seg_fuse, one view, labels (for scale)':66s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
        for name, pred, target in (("blobs, near prediction", near(target), target), ("blobs, unrelated prediction", blobby(n, h, w), target),
                                   ("fine texture, near prediction", near(fine), fine)):
            found = SB.boundary_counts(pred, target, nc, spec)
            contour = tuple(round(100.0 * int(found.bf[0, :, j].sum()) / (n * h * w), 1) for j in (1, 3))
            for what, fn in (("cvx_seg_boundary alone", found._launch),
                             ("boundary_counts", lambda: SB.boundary_counts(pred, target, nc, spec)),
                             ("boundary_counts, planes", lambda: SB.boundary_counts(pred, target, nc, spec, planes=True))):
                med, lo, hi = timed(fn)
                lines.append(f"  {name + ': ' + what:66s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})   contour pixels (pred, target) {contour} %")
    # one evaluate_on_voc batch: the plain pass, the one-view label-writing pass, and that pass with the boundary call
    n = args.batch
    images = torch.rand(n, 3, S, S, device=dev, generator=gen)
    targets = blobby(n, S, S).long()
    targets[:, : S // 8, : S // 8] = -100
    criterion = algo.build_loss()
    metrics = SegmentationMetrics(nc, dev)
    slot = torch.zeros(1, dtype=torch.float32, device=dev)
    tta = T.SegTTA((1.0,), False, "prob")
    bm = SB.BoundaryMetrics(nc, SB.SegBoundary((1, 2, 4, 8, 15)), dev)
    counts = metrics.add_labels_counts(dev)

    def plain():
        with torch.no_grad():
            rows = model.forward_rows(images)
            metrics.add_rows(rows, targets, model._last_engine.graph.level_hw[0], criterion, slot)

    def one_view(boundary):
        with torch.no_grad():
            views = tta.run(model, images)
            labels = tta.fuse(views, nc, model.layout.nc_pad, (S, S), targets=targets, counts=counts, labels=boundary)
            if boundary:
                bm.add_labels(labels, targets)

    lines.append(f"one evaluate_on_voc batch, {n} x {S} x {S}")
    for what, fn in (("plain pass: forward_rows + cvx_seg_criterion_eval", plain),
                     ("one-view pass: SegTTA((1.0,)) + cvx_seg_fuse, no labels", lambda: one_view(False)),
                     ("boundary=: one-view pass with labels + cvx_seg_boundary", lambda: one_view(True))):
        med, lo, hi = timed(fn)
        lines.append(f"  {what:66s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
    need = int(SB.L.load().cvx_seg_boundary_workspace_bytes(2, 1024, 2048))
    head = (f"boundary metrics, 64 x 32 tiles, workspace 6 bytes per pixel ({need / 2 ** 20:.1f} MiB for two 1024 x 2048 frames); DeepLabv3+ "
            f"R101 (random weights, {nc} classes), one MI355X; median (min .. max) ms over {args.reps} event pairs; no bar: the path is new")
    text = "\n".join([head] + lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
