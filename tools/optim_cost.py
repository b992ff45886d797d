"""What an optimiser step costs on the device: the step launch(es) ALONE, timed with device events on arenas of the real sizes.

    arenas   YOLOv8-n (3.16 M values) and YOLOv7-l (37.6 M values), with the group maps FlatSGD / FlatAdamW build for them
    arms     adam            cvx_adam_step_dev, what FlatAdam runs (with --parent-lib also the same entry of another build: adam_parent)
             adam+ema        cvx_adam_ema_step_dev
             sgd, adamw      cvx_optim_step, each with one group or three (g3), with clipping (clip: cvx_grad_norm first) and with the fused
                             average (ema)

Every arm works on its own arenas of the same seeded values.  The arms are interleaved in blocks, each block times `--reps` back-to-back
steps of every arm between two device events after a warm-up of every arm, and the figure of an arm is the median over the blocks of the
time per step.  Bytes per step are what the algorithm must move (4 bytes per value and read or write, a quarter byte of map), so the rate
is a share of what the kernel needs, not of what it happens to fetch.

    python tools/optim_cost.py --blocks 9 --reps 50 --out profiles/optim_step_cost.json [--parent-lib path/to/parent/libcvx_engine.so]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_cost.json"))
    ap.add_argument("--parent-lib", default=None, help="libcvx_engine.so of the parent commit: its cvx_adam_step_dev is timed as the arm adam_parent")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import _lib as L
    from computervision.pytorch_amd import engine as E
    from computervision.pytorch_amd import optim as O
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.yolov7 import Yolo7L

    dev = torch.device("cuda", 0)
    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.cvx_adam_step_dev.restype, parent.cvx_adam_step_dev.argtypes = L.PROTOTYPES["cvx_adam_step_dev"]

    def arena_arms(model):
        n = model.flat_params.numel()
        maps = {1: O.GroupPlan(model, None).gmap, 3: O.GroupPlan(model, O.NO_DECAY_NORM_BIAS).gmap}
        gen = torch.Generator().manual_seed(0)
        p0, g0 = (torch.randn(n, generator=gen) * 0.1).to(dev), (torch.randn(n, generator=gen) * 0.01).to(dev)
        arms = {}

        def tensors(k):
            return [p0.clone(), g0.clone()] + [torch.zeros(n, device=dev) for _ in range(k)]

        def adam(lib_fn=None, ema=False):
            p, g, m, v = tensors(2)
            e = p.clone() if ema else None
            state = torch.tensor([1e-4, 0.0, 0.0, 0.0], device=dev)
            if lib_fn is not None:
                st = L.stream_ptr(dev)
                return lambda: lib_fn(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, 0.9, 0.999, 1e-8, L.ptr(state), None, 0, 1.0, st), 28 * n
            if ema:
                return lambda: E.adam_ema_step_dev(p, g, m, v, (0.9, 0.999), 1e-8, state, e, 0.999, 0.001, None, False, 1.0), 36 * n
            return lambda: E.adam_step_dev(p, g, m, v, (0.9, 0.999), 1e-8, state, None, False, 1.0), 28 * n

        def grouped(kind, groups, clip, ema):
            adamw = kind == E.OPTIM_ADAM
            p, g, a, b = tensors(2)
            b = b if adamw else None
            e = p.clone() if ema else None
            gmap = torch.from_numpy(maps[groups]).to(dev)
            G = int(maps[groups][maps[groups] != E.OPTIM_UNMAPPED].max()) + 1
            rows = [[1e-4, 0.0 if adamw else 5e-4, O.decay_factor(1e-4, 0.05) if adamw else 1.0, 0.0, 0.0 if adamw else 0.937, 0.0 if adamw else 1.0, 0.0, 0.0]
                    for _ in range(G)]
            gs =torch.tensor(rows, dtype=torch.float32, device=dev)
            state, clip_state, ws = torch.zeros(4, device=dev), torch.zeros(4, device=dev), torch.zeros(E.grad_norm_workspace(n), device=dev)

            def run():
                if clip:
                    E.grad_norm(g, gmap, gs, 10.0, clip_state, ws)
                E.optim_step(kind, p, g, a, b, gmap, gs, state, (0.9, 0.999), 1e-8, None, False, 1.0, clip_state if clip else None, e, 0.999, 0.001)

            words = (7 if adamw else 5) + (1 if clip else 0) + (2 if ema else 0)         # reads + writes per value; the gradients are not zeroed here
            return run, 4 * words * n + (n // 4) * (2 if clip else 1)

        arms["adam"] = adam()
        if parent is not None:
            arms["adam_parent"] = adam(parent.cvx_adam_step_dev)
        arms["adam+ema"] = adam(ema=True)
        for name, kind in (("sgd", E.OPTIM_SGD), ("adamw", E.OPTIM_ADAM)):
            for groups in (1, 3):
                for clip in (False, True):
                    for ema in (False, True):
                        arms[name + ("_g3" if groups == 3 else "") + ("_clip" if clip else "") + ("_ema" if ema else "")] = grouped(kind, groups, clip, ema)
        return n, arms

    out ={"method": f"{args.blocks} blocks, every arm in every block ({args.reps} back-to-back steps between two device events after {args.warmup} warm-up "
                     "steps per arm), median over blocks of the time per step; one MI355X; the steps do not zero the gradients",
           "arenas": {}}
    for label, make in (("yolov8n", lambda: Yolo8("n", 80)), ("yolov7l", lambda: Yolo7L(80))):
        torch.manual_seed(0)
        model = make()
        n, arms = arena_arms(model)
        for run, _ in arms.values():
            for _ in range(args.warmup):
                run()
        torch.cuda.synchronize(dev)
        us = {name: [] for name in arms}
        names = list(arms)
        for blk in range(args.blocks):
            for name in names[blk % len(names):] + names[:blk % len(names)]:
                run = arms[name][0]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.reps):
                    run()
                t1.record()
                t1.synchronize()
                us[name].append(t0.elapsed_time(t1) * 1e3 / args.reps)
        res = {}
        for name in names:
            med = statistics.median(us[name])
            res[name] = {"median_us": round(med, 2), "min_us": round(min(us[name]), 2), "max_us": round(max(us[name]), 2),
                         "needed_bytes": arms[name][1], "needed_TB_per_s": round(arms[name][1] / med * 1e-6, 3)}
        out["arenas"][label] = {"n_values": n, "arms": res}
        print(label, n, json.dumps({k: v["median_us"] for k, v in res.items()}))
        del arms, model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
