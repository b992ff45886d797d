"""What Soft-NMS costs: ``cvx_soft_nms`` beside ``cvx_nms_variant`` on the same planted candidates (B = 32, A = 8400, nc = 80, 300 and 1024
candidates per image), one block at the capacity of 16384 candidates over 20 classes and class-agnostic, and ``predict_batch`` of YOLOv8-n
on 32 frames with and without ``cfg.decode.soft_nms``.

    python tools/soft_nms_cost.py [--batch 32] [--size 640] [--reps 20] [--alt-lib PATH] [--out profiles/soft_nms_cost.txt]

The kernel figures are the median (and the range) over ``--reps`` device event pairs around the call, after a warm-up; the
``predict_batch`` figures are a host clock around ``--reps`` calls that end in a synchronise, the settings alternating, three rounds.
``--alt-lib``: a second build of the library (say with ``-DSNMS_FLY=1``, the sweep without loads in flight) whose ``cvx_soft_nms`` is timed
beside the first and must give the same bits.  It sets no bar: the path did not exist before; the weights are random, so there is no
accuracy figure either."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_nms_cost.txt"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("soft_nms_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    import eval_tail_cases as T
    import soft_nms_restatement as S
    from computervision.pytorch_amd import _lib as L
    from computervision.pytorch_amd import engine as E
    from computervision.pytorch_amd import soft_nms as SN
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8

    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def say(*a):
        line = " ".join(str(x) for x in a)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def timed(fn, warm=3, iters=args.reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) for a, b in ev)
        return "median %.3f ms (%.3f .. %.3f)" % (t[len(t) // 2], t[0], t[-1])

    def wall(fn, warm=3, iters=args.reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    alt = None
    if args.alt_lib:
        lib = ctypes.CDLL(args.alt_lib)
        for name in ("cvx_soft_nms", "cvx_soft_nms_workspace_bytes"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = L.PROTOTYPES[name]

        def alt(y, conf, soft, iou, max_det):
            B, ch, A = y.shape
            ws = torch.empty(int(lib.cvx_soft_nms_workspace_bytes(B, A)), dtype=torch.uint8, device=y.device)
            rows = torch.empty(B, max_det, 6, device=y.device)
            index = torch.empty(B, max_det, dtype=torch.int32, device=y.device)
            counts = torch.empty(B, dtype=torch.int32, device=y.device)

            def call():
                rc = lib.cvx_soft_nms(L.ptr(y), B, A, ch - 4, conf, iou, max_det, SN.METHODS[soft.method], soft.sigma, soft.min_score,
                                      SN.FLAG_CLASS_AGNOSTIC if soft.class_agnostic else 0, L.ptr(rows), L.ptr(index), L.ptr(counts), L.ptr(ws),
                                      ws.numel(), L.stream_ptr(y.device))
                assert rc == 0
                return rows, index, counts
            return call

    say(f"device {torch.cuda.get_device_name(0)}, {args.reps} repetitions")
    # ---- 1. the launch beside cvx_nms_variant ----
    for planted in (300, 1024):
        y = torch.from_numpy(T.clustered(900 + planted, 8400, 80, (planted,) * args.batch)).to(dev)
        say(f"B={args.batch} A=8400 nc=80, {planted} planted candidates per image (six classes, 40 clusters), conf 0.25, max_det 300")
        say("  cvx_nms_variant tv0141_cuda iou 0.7:", timed(lambda: E.nms(y, 0.25, 0.7, 300)))
        say("  cvx_nms_variant vanilla     iou 0.7:", timed(lambda: E.nms(y, 0.25, 0.7, 300, variant="vanilla")))
        for method, iou in (("hard", 0.7), ("linear", 0.7), ("linear", 0.3), ("gaussian", 0.7)):
            for agnostic in (False, True):
                soft = SN.SoftNMS(method, class_agnostic=agnostic)
                t = timed(lambda: SN.soft_nms(y, 0.25, soft, iou, 300))
                rows = float(SN.soft_nms(y, 0.25, soft, iou, 300)[2].float().mean())
                say(f"  cvx_soft_nms {method:8s} iou {iou} class_agnostic={agnostic!s:5s}: {t}, rows/image {rows:.1f}")
                if alt is not None and method != "hard":
                    call = alt(y, 0.25, soft, iou, 300)
                    say("      the other build:", timed(call))
                    assert all(torch.equal(p, q) for p, q in zip(call(), SN.soft_nms(y, 0.25, soft, iou, 300)))
    # ---- 2. one block at capacity ----
    y = torch.from_numpy(S.spread_classes(T.clustered(950, 16384, 20, 16384), 951, tuple(range(20)))).to(dev)
    say("one block at capacity: 16384 candidates of 16384 anchors, 20 classes, conf 0.25, max_det 16384")
    say("  cvx_nms_variant vanilla iou 0.7:", timed(lambda: E.nms(y, 0.25, 0.7, 16384, variant="vanilla"), 1, 3))
    for method, iou in (("hard", 0.7), ("linear", 0.3), ("gaussian", 0.7)):
        for agnostic in (False, True):
            soft = SN.SoftNMS(method, class_agnostic=agnostic)
            rows = int(SN.soft_nms(y, 0.25, soft, iou, 16384)[2][0])
            say(f"  cvx_soft_nms {method:8s} iou {iou} class_agnostic={agnostic!s:5s}:", timed(lambda: SN.soft_nms(y, 0.25, soft, iou, 16384), 0, 3),
                f"rows {rows}")
            if alt is not None and method == "gaussian":
                say("      the other build:", timed(alt(y, 0.25, soft, iou, 16384), 0, 3))
    # ---- 3. predict_batch ----
    g = torch.Generator().manual_seed(5)
    frames = [torch.randint(0, 256, (args.size, args.size, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(args.batch)]
    built = []
    for soft in (None, dict(method="linear"), dict(method="gaussian"), dict(method="gaussian", class_agnostic=True)):
        cfg = Yolo8DetConfig()
        cfg.arch.input_size, cfg.decode.soft_nms = (3, args.size, args.size), soft
        algo = YOLOv8(cfg, dev)
        torch.manual_seed(0)
        model = algo.build_model()[0].to(dev).eval()
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        for k in [k for k in sd if ".cv3." in k and k.endswith(".2.bias")]:
            sd[k] += 3.0                                       # random-init class biases leave no score above 0.001
        model.load_state_dict(sd)
        built.append((soft, algo, model))
    for conf in (0.25, 0.001, 0.0005):
        for round_ in range(3):
            for soft, algo, model in built:
                rows = float(algo.predict_batch(model, frames, conf_threshold=conf, sync=False)[1].float().mean())
                t = wall(lambda: algo.predict_batch(model, frames, conf_threshold=conf, sync=False))
                say(f"predict_batch YOLOv8-n {args.batch} x {args.size}^2, round {round_}, conf {conf}, soft_nms={soft}: {t:.3f} ms, rows/frame {rows:.1f}")
    out.close()


if __name__ == "__main__":
    main()
