"""Write tests/golden/det_map_ref.npz: seeded synthetic detections and ground truths, and what the REFERENCE's ``get_map`` makes of them.

    python tools/make_map_fixture.py          # CPU only; needs the reference tree (CVX_REFERENCE), never runs on the GPU box

The detection and ground-truth text files are written to a temporary directory in the reference's format, ``get_map(0.5, draw_plot=False,
score_threshold=0.5, path=...)`` of the reference is called on it, and a wrapper around its ``voc_ap`` records every class's ``rec``,
``prec`` and ``ap`` at full precision.  Stored: the inputs, those captures, the returned mAP and the text of ``results/results.txt``.
Scores are k / 10000 as float32, so the writers' ``str(score)[:6]`` is the identity.  The tool asserts that the data holds every case the
matching rules distinguish (see ``check_cases``).  Data only: no reference program text goes into the fixture.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import det_eval_restatement as R  # noqa: E402
from oracle import make_golden  # noqa: E402  (its stubs and its way of importing the reference)

SEED = 7
N_IMG, MAX_DET, MAX_GT, SIZE = 40, 16, 6, 64
NAMES = ["dog", "aeroplane", "car", "bird", "person", "boat"]      # name order differs from index order; "person": GT only, "boat": detections only
NC = len(NAMES)


def make_data():
    rs = np.random.RandomState(SEED)
    dets, gts = [], []
    for img in range(N_IMG):
        gt = []
        for _ in range(0 if img in (3, 17) else rs.randint(1, MAX_GT + 1)):
            l, t = rs.randint(0, SIZE - 8, 2)
            w, h = rs.randint(2, 24, 2)
            gt.append([int(rs.randint(0, 5)), int(l), int(t), int(min(l + w, SIZE)), int(min(t + h, SIZE)), int(rs.rand() < 0.25)])
        det = []
        for _ in range(0 if img in (5, 17, 22) else rs.randint(1, MAX_DET + 1)):
            if gt and rs.rand() < 0.6:
                g = gt[rs.randint(0, len(gt))]
                box = [int(v) for v in np.asarray(g[1:5]) + rs.randint(-2, 3, 4)]
                cls = g[0] if rs.rand() < 0.9 else int(rs.randint(0, NC))
            else:
                l, t = rs.randint(0, SIZE - 8, 2)
                box = [int(l), int(t), int(l + rs.randint(1, 24)), int(t + rs.randint(1, 24))]
                cls = int(rs.randint(0, NC))
            if cls == 4:
                cls = 5                                            # "person" is never detected
            k = int(rs.randint(1, 21)) * 500 - 1 if rs.rand() < 0.4 else int(rs.randint(10, 10000))   # a coarse grid: equal scores
            det.append([cls, k] + box)
        dets.append(det)
        gts.append(gt)
    # planted: a detection between two ground truths of equal IoU (the first in file order wins), one touching a ground truth by one
    # pixel, and one of the ground truth's class that overlaps nothing
    gts[0] = [[0, 10, 10, 19, 19, 0], [0, 14, 10, 23, 19, 0], [2, 40, 40, 50, 50, 0]] + gts[0][:3]
    dets[0] = [[0, 6000, 12, 10, 21, 19], [2, 3000, 50, 50, 60, 60], [2, 2500, 0, 0, 5, 5]] + dets[0][:13]
    return dets, gts


def check_cases(dets, gts):
    """every case the rules distinguish is in the data"""
    dl = [[(d[0], float(R.score_text(np.float32(d[1] / 10000))), *d[2:]) for d in per] for per in dets]
    out = R.get_map(dl, [[tuple(g) for g in per] for per in gts], NC)
    seen = dict.fromkeys(("two_on_one", "difficult_best", "tie_in_image", "tie_across", "equal_iou", "no_overlap", "touching"), False)
    by_score = {}
    for img in range(N_IMG):
        chosen = {}
        for row, d in enumerate(dets[img]):
            g, ov, reach = out["detail"][img][row]
            if g >= 0 and ov >= 0.5:
                chosen.setdefault(g, []).append(row)
                seen["difficult_best"] |= bool(gts[img][g][5])
                seen["equal_iou"] |= reach > 1
            seen["no_overlap"] |= g < 0 and any(gt[0] == d[0] for gt in gts[img])
            for gt in gts[img]:
                if gt[0] == d[0] and (d[4] == gt[1] or d[2] == gt[3] or d[5] == gt[2] or d[3] == gt[4]) and \
                        min(d[4], gt[3]) - max(d[2], gt[1]) + 1 > 0 and min(d[5], gt[4]) - max(d[3], gt[2]) + 1 > 0:
                    seen["touching"] = True
            key = (d[0], d[1])
            seen["tie_in_image"] |= any(i == img for i in by_score.get(key, []))
            seen["tie_across"] |= any(i != img for i in by_score.get(key, []))
            by_score.setdefault(key, []).append(img)
        seen["two_on_one"] |= any(len(v) > 1 and not gts[img][g][5] for g, v in chosen.items())
    res = out["res"]
    assert all(seen.values()), seen
    assert any(res["n_det"][c] > 0 and res["n_gt"][c] == 0 and not any(g[0] == c for per in gts for g in per) for c in range(NC)), "detections, no GT"
    assert any(res["n_det"][c] == 0 and res["n_gt"][c] > 0 for c in range(NC)), "GT, no detection"
    assert any(len(d) == 0 and len(g) > 0 for d, g in zip(dets, gts)) and any(len(g) == 0 and len(d) > 0 for d, g in zip(dets, gts))
    assert any(f == R.FLAG_TP for f in out["flags"]) and any(f == R.FLAG_NEITHER for f in out["flags"])
    return out


def main():
    dets, gts = make_data()
    assert len(dets) == N_IMG and max(len(d) for d in dets) <= MAX_DET and max(len(g) for g in gts) <= MAX_GT
    ours = check_cases(dets, gts)
    tmp = tempfile.mkdtemp(prefix="det_map_")
    os.makedirs(os.path.join(tmp, "ground-truth"))
    os.makedirs(os.path.join(tmp, "detection-results"))
    for img in range(N_IMG):
        with open(os.path.join(tmp, "detection-results", f"img_{img:03d}.txt"), "w") as f:
            for cls, k, l, t, r, b in dets[img]:
                score = str(np.float32(k / 10000))
                assert score[:6] == score, score
                f.write(f"{NAMES[cls]} {score[:6]} {int(l)} {int(t)} {int(r)} {int(b)}\n")
        with open(os.path.join(tmp, "ground-truth", f"img_{img:03d}.txt"), "w") as f:
            for cls, l, t, r, b, difficult in gts[img]:
                f.write(f"{NAMES[cls]} {l} {t} {r} {b}" + (" difficult\n" if difficult else "\n"))

    make_golden._import_reference()
    from core.metrics import mAP as ref            # the reference's
    assert os.path.abspath(ref.__file__).startswith(make_golden.REF), ref.__file__
    captured = []
    inner = ref.voc_ap

    def recording_voc_ap(rec, prec):
        rec_in, prec_in = list(rec), list(prec)
        got = inner(rec, prec)
        captured.append((rec_in, prec_in, got[0]))
        return got

    ref.voc_ap = recording_voc_ap
    m = ref.get_map(0.5, draw_plot=False, score_threshold=0.5, path=tmp)
    ref.voc_ap = inner
    text = open(os.path.join(tmp, "results", "results.txt")).read()

    gt_classes = sorted(c for c in range(NC) if any(g[0] == c and not g[5] for per in gts for g in per))
    by_name = sorted(gt_classes, key=lambda c: NAMES[c])
    assert len(captured) == len(by_name)
    rec = [np.zeros(0)] * NC
    prec = [np.zeros(0)] * NC
    ap = np.zeros(NC)
    for c, (r, p, a) in zip(by_name, captured):
        rec[c], prec[c], ap[c] = np.asarray(r, np.float64), np.asarray(p, np.float64), a
    off = np.concatenate(([0], np.cumsum([len(r) for r in rec]))).astype(np.int64)
    det_arr = np.array([[img] + d for img in range(N_IMG) for d in dets[img]], np.int32)
    gt_arr = np.array([[img] + g for img in range(N_IMG) for g in gts[img]], np.int32)
    # the restatement agrees before anything is stored (tests/test_det_eval_cpu.py checks it again from the file)
    assert abs(ours["res"]["mAP"] - m) < 1e-9 and all(abs(ours["res"]["ap"][c] - ap[c]) < 1e-9 for c in gt_classes)
    path = os.path.join(ROOT, "tests", "golden", "det_map_ref.npz")
    np.savez_compressed(path, dets=det_arr, gts=gt_arr, n_images=np.int64(N_IMG), names=np.array(NAMES), curve_off=off,
                        rec=np.concatenate(rec), prec=np.concatenate(prec), ap=ap, gt_classes=np.array(gt_classes, np.int64), mAP=np.float64(m),
                        results_txt=np.array(text))
    print(f"wrote {path}: {len(det_arr)} detections, {len(gt_arr)} ground truths, mAP {m:.6f}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
