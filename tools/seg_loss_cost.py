"""What the segmentation criterion costs on the device: the criterion's launches ALONE (``SegLoss.op``: pixel kernel, selection,
reduction, adjoint gather), timed with device events at the benchmark's DeepLab shape -- batch 16, 513 x 513 labels, 21 classes, logits
rows 129 x 129 with 24 columns.

    arms     plain      cross-entropy without options, the Ce<false> kernels (3 launches)
             weights    class weights + label smoothing 0.1, the Ce<true> kernels (3 launches)
             ohem       OHEM thresh 0.7, min_kept 100000 per image (13 launches)
             all        weights + smoothing + OHEM
             ohem_few   OHEM thresh 1e-4: the rank decides, 100000 pixels per image are kept and the gradients of the rest are zeroed
             dice       the Dice region loss alone, base 0 (5 launches)
             ce_dice    cross-entropy + Dice (7 launches: the plain chain's two, the region's four, the adjoint)
             all_tversky   weights + smoothing + OHEM + focal Tversky (0.3 / 0.7, gamma 0.75) per image
             lovasz     the Lovasz-Softmax loss alone, base 0 (23 launches and a memset: keys, four sort passes, scan, value, gradient, adjoint)
             ce_lovasz  cross-entropy + Lovasz-Softmax (the plain chain's two launches in front)

Every arm has its own criterion (workspace) and gradient buffer and the same rows and targets.  The arms are interleaved in blocks; each
block times `--reps` back-to-back calls of every arm between two device events after a warm-up of every arm, and an arm's figure is the
median over the blocks of the time per call, with the smallest and the largest block next to it.  Bytes per call are what the chain must
move: the fp32 rows and int64 targets read once, the (B, nc, H, W) fp32 per-pixel gradients written once and read once by the adjoint,
the fp16 row gradients written once; under OHEM a 4-byte key plane and a 4-byte loss plane written once, the keys read by the four
histogram passes and the masked sum (with the loss plane and the targets), which also writes nc zeros for every valid pixel that is not
kept (counted from the arm's own kept / valid figures).  A region term reads the rows and the targets once more for its sums and, in
its gradient pass, a third time; with a base that pass reads and rewrites the gradient plane, without one it writes the plane (then
the rows and targets are read twice in all, by the two region passes).  The partial sums (3 nc doubles per 2048 pixels) are not counted.
The Lovasz term moves, per pixel and class: key + payload written once (8 bytes), read by each of the four histogram passes (4) and
scatter passes (8) and written by each scatter (8), the payload read by the flag count (4), both read by the value pass (8), which
writes the coefficient plane (4) that the gradient pass reads (4); it reads the rows and the targets three times (count and keys, then
the gradient pass; the count reads the targets alone).  The sort's per-tile histograms (1 KB per 1024 keys and pass, written, scanned
in place and read) are not counted.

    python tools/seg_loss_cost.py --blocks 9 --reps 20 --out profiles/seg_loss_cost.json
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_loss_cost.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("seg_loss_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd.deeplab import SegLoss

    dev = torch.device("cuda", 0)
    B, H, W, nc, lh, lw, ld = args.batch, 513, 513, 21, 129, 129, 24
    g = torch.Generator().manual_seed(0)
    rows = torch.zeros(B, lh * lw, ld)
    rows[..., :nc] = torch.randn(B, lh * lw, nc, generator=g) * 2
    target = torch.randint(0, nc, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.02] = -100
    weights = torch.rand(nc, generator=g) + 0.1
    rows, target = rows.to(dev), target.to(dev)
    ohem = dict(thresh=0.7, min_kept=100000)
    npix, nlow = B * H * W, B * lh * lw
    base = nlow * ld * 4 + npix * 8 + 2 * npix * nc * 4 + nlow * ld * 2
    mined = base + 2 * npix * 4 + 4 * npix * 4 + npix * (4 + 4 + 8)
    arms = {"plain": (SegLoss("ce"), base), "weights": (SegLoss("ce", class_weights=weights, label_smoothing=0.1), base),
            "ohem": (SegLoss("ce", ohem=ohem), mined), "all": (SegLoss("ce", class_weights=weights, label_smoothing=0.1, ohem=ohem), mined),
            "ohem_few": (SegLoss("ce", ohem=dict(thresh=1e-4, min_kept=ohem["min_kept"])), mined)}
    again = nlow * ld * 4 + npix * 8                       # one more read of the rows and the targets
    arms.update({"dice": (SegLoss("ce", region=dict(kind="dice", base_weight=0.0)), base + again),
                 "ce_dice": (SegLoss("ce", region=dict(kind="dice")), base + 2 * again + 2 * npix * nc * 4),
                 "all_tversky": (SegLoss("ce", class_weights=weights, label_smoothing=0.1, ohem=ohem,
                                         region=dict(kind="tversky", gamma=0.75, per_image=True)), mined + 2 * again + 2 * npix * nc * 4)})
    lov = npix * nc * (8 + 4 * (4 + 8 + 8) + 4 + 8 + 4 + 4)
    arms.update({"lovasz": (SegLoss("ce", lovasz=dict(base_weight=0.0)), base + again + npix * 8 + lov),
                 "ce_lovasz": (SegLoss("ce", lovasz={}), base + 2 * again + npix * 8 + 2 * npix * nc * 4 + lov)})
    runs, values = {}, {}
    for name, (crit, _) in arms.items():
        crit.nc = nc
        dpred = torch.empty(B, lh * lw, ld, dtype=torch.float16, device=dev)
        runs[name] = lambda crit=crit, dpred=dpred: crit.op(rows, target, (lh, lw), 65536.0, dpred, check=False)
        for _ in range(args.warmup):
            loss, _ = runs[name]()
        values[name] = {"loss": float(loss), "stats": [v if math.isfinite(v) else None for v in crit.last_stats.tolist()] if crit.last_stats is not None else None}
    torch.cuda.synchronize(dev)
    names, us = list(arms), {name: [] for name in arms}
    for blk in range(args.blocks):
        for name in names[blk % len(names):] + names[:blk % len(names)]:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.reps):
                runs[name]()
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / args.reps)
    out = {"method": f"{args.blocks} blocks, every arm in every block ({args.reps} back-to-back criterion calls between two device events after "
                     f"{args.warmup} warm-up calls per arm), median over blocks of the time per call; one MI355X",
           "shape": {"batch": B, "labels": [H, W], "classes": nc, "rows": [lh, lw], "ld": ld}, "ohem": ohem, "arms": {}}
    for name in names:
        med = statistics.median(us[name])
        st = values[name]["stats"]
        needed = arms[name][1] + (int(st[1] - st[0]) * nc * 4 if st else 0)
        out["arms"][name] = {"median_us": round(med, 1), "min_us": round(min(us[name]), 1), "max_us": round(max(us[name]), 1),
                             "needed_bytes": needed, "needed_TB_per_s": round(needed / med * 1e-6, 3), **values[name]}
    print(json.dumps({k: (v["median_us"], v["min_us"], v["max_us"]) for k, v in out["arms"].items()}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
