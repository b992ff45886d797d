"""What the detector diagnostics cost: event times of ``cvx_det_confusion`` beside ``cvx_det_match`` on the same planted rows (the rows of
tools/det_tta_cost.py: per frame 40 boxes of the picture, 300 jittered copies, here with the 40 boxes as ground truth), of the kernel's
largest block (one frame of 16384 rows against 1024 ground truths) and of both kernels at 8192 x 1024, which ``cvx_det_match`` still
holds; of ``cvx_coco_match`` on the same planted rows and on one frame of 4096 x 1024; of ``cvx_det_conf_curves``, ``cvx_det_ap`` and
``cvx_coco_accumulate`` at 80 classes over 10^5 records (``--kernels-only`` stops here: the arms an A/B run of two builds needs); and of one ``evaluate_on_voc`` batch of YOLOv8-n -- the rows of the
model's tail and ``cvx_det_match`` -- with and without the ``cvx_det_confusion`` launch that ``diagnostics=`` adds, alternating.

    python tools/det_diag_cost.py [--batch 32] [--size 640] [--reps 20] [--kernels-only] [--out profiles/det_diag_cost.txt]

Each figure is the median (and the range) over ``--reps`` device event pairs around the call, after a warm-up; the end of an evaluation
(``results`` and ``write_report``) is a host clock around work that ends in the host read.  It sets no bar: the path did not exist
before; and the weights are random, so the recommended threshold means nothing about a trained model."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_diag_cost.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="the kernel arms alone: no model, no evaluate_on_voc batch (A/B runs of two builds)")
    args = ap.parse_args()

    def finish(lines):
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(text, end="")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("det_diag_cost.py measures on the MI355X: no device found (there is nothing to time on a CPU)")
    from computervision.pytorch_amd import coco_eval, det_diag, det_eval
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8

    dev = torch.device("cuda", 0)
    B, S, reps = args.batch, args.size, args.reps
    rng = np.random.RandomState(0)
    nc, calls = 80, reps + 4

    def planted(frames, K, G, extent):
        """per frame G boxes of 100 x 100 (the ground truth, one in eight difficult) and K rows: jittered copies of them, nine in ten with
        the box's class"""
        corner = rng.uniform(0, extent - 120, (frames, G, 2))
        gcls = rng.randint(0, nc, (frames, G))
        gt = np.concatenate([gcls[..., None], corner, corner + 100, (rng.rand(frames, G, 1) < 0.125)], 2).astype(np.int32)
        pick = rng.randint(0, G, (frames, K))
        xy = np.take_along_axis(corner, pick[..., None], 1) + rng.uniform(-4, 4, (frames, K, 2))
        cls = np.where(rng.rand(frames, K) < 0.9, np.take_along_axis(gcls, pick, 1), rng.randint(0, nc, (frames, K)))
        rows = np.concatenate([xy, xy + 100, rng.uniform(0.1, 1, (frames, K, 1)), cls[..., None]], 2).astype(np.float32)
        t = [torch.from_numpy(a).to(dev) for a in (rows, np.full(frames, K, np.int32), gt, np.full(frames, G, np.int32))]
        return t

    def timed(fn):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    def matcher(t, K):
        ev = det_eval.DetectionEvaluator(nc, K, int(t[0].shape[0]) * K * calls, dev)
        return ev, lambda: ev.add_batch(*t)

    def counter(t, K):
        diag = det_diag.DetectionDiagnostics(nc, K, dev)
        return diag, lambda: diag.add_batch(*t)

    def coco_matcher(t, K):
        ev = coco_eval.CocoEvaluator(nc, K, int(t[0].shape[0]) * K * calls, dev, truncate_boxes=True, quantize_scores=True)
        gt = coco_eval.voc_gt_to_coco(t[2])
        return ev, lambda: ev.add_batch(t[0], t[1], gt, t[3])

    small, half, full = planted(B, 300, 40, 640), planted(1, 8192, 1024, 4000), planted(1, 16384, 1024, 4000)
    quarter = [half[0][:, :4096].contiguous(), torch.full_like(half[1], 4096), half[2], half[3]]
    arms = [(f"cvx_det_match ({B} x 300 rows, 40 ground truths)", matcher(small, 300)[1]),
            (f"cvx_det_confusion ({B} x 300 rows, 40 ground truths)", counter(small, 300)[1]),
            (f"cvx_coco_match ({B} x 300 rows, 40 ground truths)", coco_matcher(small, 300)[1]),
            ("cvx_coco_match, one frame 4096 x 1024 (its LDS holds no 8192)", coco_matcher(quarter, 4096)[1]),
            ("cvx_det_match, one frame 8192 x 1024", matcher(half, 8192)[1]),
            ("cvx_det_confusion, one frame 8192 x 1024", counter(half, 8192)[1]),
            ("cvx_det_confusion, one frame 16384 x 1024", counter(full, 16384)[1])]

    # 10^5 records over 80 classes of unequal size, as cvx_det_ap leaves them
    n = 100000
    cls = np.sort(rng.choice(nc, n, p=np.arange(1, nc + 1) / (nc * (nc + 1) / 2)))
    seg_off = np.searchsorted(cls, np.arange(nc + 1)).astype(np.int64)
    score, flag = np.zeros(n, np.float32), np.zeros(n, np.int32)
    prec, rec = np.zeros(n), np.zeros(n)
    gt_per_class = np.zeros(nc, np.int64)
    for c in range(nc):
        lo, hi = seg_off[c], seg_off[c + 1]
        s = np.sort(rng.uniform(0.001, 1, hi - lo).astype(np.float32))[::-1]
        f = np.where(rng.rand(hi - lo) < s.astype(np.float64) ** 2, 1, 0)
        tp, fp = np.cumsum(f == 1), np.cumsum(f == 0)
        gt_per_class[c] = tp[-1] + 10 if hi > lo else 10
        score[lo:hi], flag[lo:hi] = s, f
        rec[lo:hi], prec[lo:hi] = tp / float(gt_per_class[c]), tp / np.maximum(tp + fp, 1)
    rt = [torch.from_numpy(a).to(dev) for a in (score, prec, rec, flag, seg_off, gt_per_class, np.full(nc, 500, np.int64))]
    records = dict(score=rt[0], prec=rt[1], rec=rt[2], flag=rt[3], seg_off=rt[4])
    arms.append((f"cvx_det_conf_curves ({nc} classes, {n} records, 1001 points, window 101)",
                 lambda: det_diag.conf_curves(records, rt[5], rt[6], nc, True, 1001, 101)))

    # the two per-class reductions over the same 10^5 records: cvx_det_ap rewrites prec / rec with what it computes from the flags (the
    # curves arm above has run by then), cvx_coco_accumulate reads seeded ranks and 40-bit masks
    from computervision.pytorch_amd import _lib as L
    lib, st = L.load(), L.stream_ptr(dev)
    stats = torch.zeros(nc * 8 + 8, dtype=torch.float64, device=dev)
    arms.append((f"cvx_det_ap ({nc} classes, {n} records)",
                 lambda: L.check(lib.cvx_det_ap(L.ptr(rt[0]), L.ptr(rt[3]), L.ptr(rt[4]), L.ptr(rt[5]), nc, 0.5, 1, L.ptr(rt[1]), L.ptr(rt[2]),
                                                L.ptr(stats), st), "cvx_det_ap")))
    ct = [torch.from_numpy(a).to(dev) for a in (rng.randint(0, 100, n).astype(np.int32), rng.randint(0, 1 << 40, n).astype(np.int64),
                                                (rng.randint(0, 1 << 40, n) & rng.randint(0, 1 << 40, n)).astype(np.int64),
                                                np.full((nc, 4), 500, np.int64), coco_eval.REC_THRS)]
    precision = torch.empty(10, 101, nc, 4, 3, dtype=torch.float64, device=dev)
    recall = torch.empty(10, nc, 4, 3, dtype=torch.float64, device=dev)
    arms.append((f"cvx_coco_accumulate ({nc} classes, {n} records)",
                 lambda: L.check(lib.cvx_coco_accumulate(L.ptr(ct[0]), L.ptr(ct[1]), L.ptr(ct[2]), L.ptr(rt[4]), L.ptr(ct[3]), nc, L.ptr(ct[4]),
                                                         L.ptr(precision), L.ptr(recall), st), "cvx_coco_accumulate")))

    lines = [f"Detector diagnostics, one MI355X; median (min .. max) ms over {reps} event pairs; {nc} classes unless stated"]
    for name, fn in arms:
        med, lo, hi = timed(fn)
        lines.append(f"{name:74s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})")
    if args.kernels_only:
        finish(lines)
        return

    # one evaluate_on_voc batch of YOLOv8-n: class biases raised by 3 so that rows pass conf_threshold = 0.001
    cfg = Yolo8DetConfig()
    cfg.arch.input_size = (3, S, S)
    algo = YOLOv8(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for k in [k for k in sd if ".cv3." in k and k.endswith(".2.bias")]:
        sd[k] += 3.0
    model.load_state_dict(sd)
    mnc = algo.num_classes
    images = torch.rand(B, 3, S, S, device=dev)
    corner = rng.uniform(0, 400, (B, 8, 2))
    gt = torch.from_numpy(np.concatenate([rng.randint(0, mnc, (B, 8, 1)), corner, corner + 80, np.zeros((B, 8, 1))], 2).astype(np.int32)).to(dev)
    meta = dict(image_hw=torch.tensor([[480, 640]] * B, device=dev), gt=gt, gt_counts=torch.full((B,), 8, dtype=torch.int32, device=dev))
    tail = algo._evaluation_rows(model)
    max_det = algo.eval_max_det
    with torch.no_grad():
        rows, counts, box_map = tail(images, meta)
    K = int(rows.shape[1])
    ev = det_eval.DetectionEvaluator(mnc, max_det, B * K * calls * 2, dev)
    diag = det_diag.DetectionDiagnostics(mnc, max_det, dev, det_diag.DetDiagnostics(conf=0.001))

    def batch(with_diag):
        def run():
            with torch.no_grad():
                r, c, m = tail(images, meta)
            ev.add_batch(r, c, meta["gt"], meta["gt_counts"], m)
            if with_diag:
                diag.add_batch(r, c, meta["gt"], meta["gt_counts"], m)
        return run

    # alternating, so that a drift of the box touches both arms alike
    plain, with_diag = [], []
    for fn in (batch(False), batch(True)):
        for _ in range(3):
            fn()
    for _ in range(reps):
        for fn, ms in ((batch(False), plain), (batch(True), with_diag)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
    lines.append(f"YOLOv8-n (random weights, {mnc} classes) evaluate_on_voc batch, {B} x {S} x {S}, {K} row slots, rows kept per image "
                 f"{int(counts.min())} .. {int(counts.max())}")
    for name, ms in (("rows + cvx_det_match (the batch as it was)", plain), ("rows + cvx_det_match + cvx_det_confusion (diagnostics=)", with_diag)):
        lines.append(f"{name:74s} {statistics.median(ms):8.3f}  ({min(ms):.3f} .. {max(ms):.3f})")
    ev.reset()
    diag.reset()
    batch(True)()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.results()
    t1 = time.perf_counter()
    diag.results(ev)
    t2 = time.perf_counter()
    with tempfile.TemporaryDirectory() as tmp:
        diag.write_report(tmp, [str(c) for c in range(mnc)])
    t3 = time.perf_counter()
    lines.append(f"end of that evaluation, host clock: DetectionEvaluator.results {1e3 * (t1 - t0):.3f} ms, DetectionDiagnostics.results "
                 f"{1e3 * (t2 - t1):.3f} ms, write_report (three files, host text) {1e3 * (t3 - t2):.3f} ms")
    finish(lines)


if __name__ == "__main__":
    main()
