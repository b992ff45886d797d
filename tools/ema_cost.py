"""What the weight average costs per train step: three arms of the YOLOv8-n 640 x 640, batch-32 fused step in ONE process on one device,

    none     FlatAdam.step as bench.py runs it (no average attached)
    fused    ModelEMA attached: parameters averaged inside the Adam kernel (cvx_adam_ema_step_dev) + one cvx_ema_update for the statistics
    unfused  ModelEMA attached, FlatAdam.ema_fused = False: the Adam kernel, then cvx_ema_update on both arenas

interleaved in blocks (none, fused, unfused, none, ...) and timed as bench.py times its steps: a host clock around `--steps` steps that end
in a device synchronise, after a warm-up of every arm.  All arms run on the same model and optimiser state (the average only reads them), so
they execute the same kernels on the same data apart from the average itself.

    python tools/ema_cost.py --blocks 8 --steps 30 --out profiles/ema_step_cost.json [--bench-parent MS --bench-this MS]

Writes per-arm medians, the spread of the blocks (min, max, interquartile range) and the median of the per-block differences.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("none", "fused", "unfused")


def summary(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "iqr_ms": q[2] - q[0], "blocks_ms": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_step_cost.json"))
    ap.add_argument("--bench-parent", type=float, nargs="*", default=None, help="bench.py step_ms figures of the parent commit, same device, alternated")
    ap.add_argument("--bench-this", type=float, nargs="*", default=None, help="bench.py step_ms figures of this tree")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ema_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import synth
    from computervision.pytorch_amd.ema import ModelEMA
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.train import FlatAdam, FusedTrainStep, V8DetectionLoss
    from configs import Yolo8DetConfig

    dev = torch.device("cuda", 0)
    cfg = Yolo8DetConfig()
    torch.manual_seed(0)
    model = Yolo8("n", 80, loss_scale=cfg.engine.loss_scale).to(dev).train()
    opt = FlatAdam(model, lr=cfg.train.initial_lr)
    step = FusedTrainStep(model, V8DetectionLoss(cfg, model), opt, n_buckets=cfg.engine.allreduce_buckets)
    ema = ModelEMA(model)
    x = synth.images(args.batch, args.size, args.size, seed=1).to(dev)
    batch = {k: v.to(dev) for k, v in synth.targets(args.batch, seed=2).items()}

    def arm(name):
        opt.attach_ema(None if name == "none" else ema)
        opt.ema_fused = name != "unfused"

    def timed(n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            step(x, batch)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n * 1e3

    for name in ARMS:
        arm(name)
        timed(args.warmup)
    ms = {name: [] for name in ARMS}
    for b in range(args.blocks):
        order = ARMS[b % 3:] + ARMS[:b % 3]                  # every arm takes every position in the block
        for name in order:
            arm(name)
            ms[name].append(timed(args.steps))
    n_params, n_stats = model.flat_params.numel(), model.flat_stats.numel()
    diff = lambda a, b: statistics.median([p - q for p, q in zip(ms[a], ms[b])])
    out = {
        "workload": f"yolov8n train step, batch {args.batch}, {args.size}x{args.size}, one MI355X, eager launches",
        "method": f"{args.blocks} blocks x 3 arms interleaved in one process, {args.steps} steps per block, host clock around steps ending in a device synchronise",
        "arms": {name: summary(ms[name]) for name in ARMS},
        "median_of_block_differences_ms": {"fused_minus_none": diff("fused", "none"), "unfused_minus_none": diff("unfused", "none"),
                                           "fused_minus_unfused": diff("fused", "unfused")},
        "extra_bytes_per_step": {"fused": 8 * n_params + 12 * n_stats, "unfused": 12 * (n_params + n_stats)},
        "n_params": n_params, "n_stats": n_stats,
    }
    if args.bench_parent or args.bench_this:
        out["bench_py_default_path_step_ms"] = {"parent_commit": args.bench_parent, "this_change": args.bench_this,
                                               "note": "python bench.py --gpus 1 --steps 30 --warmup 5 --no-cpu-baseline, parent and this tree alternated on the same device; bench.py attaches no average"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("median_of_block_differences_ms",)} | {"medians_ms": {n: out["arms"][n]["median_ms"] for n in ARMS}}))


if __name__ == "__main__":
    main()
