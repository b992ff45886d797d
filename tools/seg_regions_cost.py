"""What connected-component regions cost: event times of ``cvx_seg_regions`` (csrc/seg_regions.hip) -- the entry alone on prepared tables,
and the whole ``seg_regions.label_regions`` call -- on a blobby seeded map, on one full-frame region and on salt-and-pepper noise, beside
``cvx_seg_stitch`` on the same frames; then DeepLabv3+ ``segment_tiled`` without and ``predict_regions`` with the regions on 1024 x 2048
frames at 513 x 513.

    python tools/seg_regions_cost.py [--reps 20] [--out profiles/seg_regions_cost.txt]

Each figure is the median (and the range) over ``--reps`` of a device event pair around the call, after a warm-up.  It sets no bar: the path
did not exist before, so there is no earlier figure.  ``segment_tiled`` without regions is untouched code; its line stands next to the
10.8 ms of DESIGN.md section 7l as a sanity check, not as a gate."""
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
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_regions_cost.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("seg_regions_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import render as R
    from computervision.pytorch_amd import seg_regions as G
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA

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

    def blobby(n, h, w, blur=31):
        """labels 0 .. nc - 1 in blobs: the arg max of box-blurred noise planes"""
        z = torch.rand(n, nc, h, w, device=dev, generator=gen)
        return F.avg_pool2d(z, blur, 1, blur // 2).argmax(1).to(torch.uint8)

    def noise(n, h, w):
        return (torch.rand(n, h, w, device=dev, generator=gen) < 0.5).to(torch.uint8)

    lines = []
    for n, h, w in ((2, 1024, 2048), (8, 513, 513)):
        frames = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
        batch = R.TileBatch(frames, (S, S), args.overlap, full_frame=False)
        with torch.no_grad():
            one = model.forward_rows(batch.network_input()[:1])
        lh, lw = model._last_engine.graph.level_hw[0]
        logits = torch.randn(batch.slots, lh * lw, int(one.shape[2]), device=dev)
        lines.append(f"{n} frames {h} x {w}  ({batch.slots} slots at {S} x {S})")
        med, lo, hi = timed(lambda: R.stitch_segmentation(frames, logits, nc, (lh, lw), (S, S), batch))
        lines.append(f"  {'cvx_seg_stitch, labels (for scale)':66s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
        inputs = (("blobby map", blobby(n, h, w), G.SegRegions()),
                  ("one full-frame region", torch.ones(n, h, w, dtype=torch.uint8, device=dev), G.SegRegions()),
                  ("salt-and-pepper noise, min_area 64", noise(n, h, w), G.SegRegions(min_area=64)))
        for name, labels, regions in inputs:
            conf = torch.rand(n, h, w, device=dev, generator=gen)
            found = G.label_regions(labels, regions)
            totals = found.total.tolist()
            for what, fn in (("cvx_seg_regions alone", found._launch),
                             ("label_regions", lambda: G.label_regions(labels, regions)),
                             ("label_regions, conf + region maps", lambda: G.label_regions(labels, regions, conf=conf, region_maps=True))):
                med, lo, hi = timed(fn)
                lines.append(f"  {name + ': ' + what:66s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})   regions per frame {totals}")
        if (h, w) == (1024, 2048):
            for what, fn in (("segment_tiled(sync=False), no regions (section 7l: 10.8 ms)", lambda: algo.segment_tiled(model, frames, overlap=args.overlap, sync=False)),
                             ("predict_regions(draw=True)", lambda: algo.predict_regions(model, frames, draw=True, overlap=args.overlap))):
                med, lo, hi = timed(fn)
                lines.append(f"  {what:66s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
    need = int(G.L.load().cvx_seg_regions_workspace_bytes(2, 1024, 2048))
    head = (f"connected-component regions, 64 x 32 tiles, workspace 28 bytes per pixel ({need / 2 ** 20:.1f} MiB for two 1024 x 2048 frames); DeepLabv3+ "
            f"R101 (random weights, {nc} classes), one MI355X; median (min .. max) ms over {args.reps} event pairs; no bar: the path is new")
    text = "\n".join([head] + lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
