"""Write tests/golden/coco_inputs_ref.npz: what the REFERENCE's ``preprocess_gt`` / ``preprocess_dr`` (core/metrics/mAP.py:837-927) make of
the 40-image case of tools/make_map_fixture.py, and that case extended with what COCO data has and VOC data lacks.

    python tools/make_coco_fixture.py          # CPU only; needs the reference tree (CVX_REFERENCE), never runs on the GPU box

The detection and ground-truth text files are written to a temporary directory in the reference's format and the reference's two
converters are called on them.  Stored: their annotation and result lists as arrays (``ref_gt``: image, category id, x, y, w, h, area,
iscrowd, id; ``ref_dt``: image, category id, x, y, w, h, score), ordered by image -- ``os.listdir`` order is not kept -- and the extended
case (``coco_gt``: image, class, x, y, w, h, area, iscrowd; ``coco_dt``: image, class, x, y, w, h, score).  pycocotools is not installed,
so no COCOeval output is stored: tests/coco_eval_restatement.py is the reference for that part.  The tool asserts that the extended
case holds every situation the matching rules distinguish (``check_cases``).  Data only: no reference program text goes into the fixture.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import coco_eval_restatement as C  # noqa: E402
import make_map_fixture as M  # noqa: E402
from oracle import make_golden  # noqa: E402  (its stubs and its way of importing the reference)

NC = M.NC


def planted():
    """(ground truths, detections) added to the converted VOC case: (image, class, x, y, w, h, area, iscrowd) and (image, class, x, y, w,
    h, score); corners and sizes are multiples of 1/8 and the scores float32 values, so a float32 row holds them exactly"""
    s = lambda v: float(np.float32(v))  # noqa: E731
    gts = [
        (1, 0, 70.125, 70.5, 20.25, 10.375, 20.25 * 10.375, 0), (1, 0, 100.5, 100.25, 8.75, 30.5, 200.0, 0),              # float boxes
        (2, 1, 80.0, 80.0, 40.0, 40.0, 1600.0, 1),                                                                         # a crowd box
        (3, 2, 100.0, 100.0, 32.0, 32.0, 1024.0, 0), (3, 2, 200.0, 100.0, 96.0, 96.0, 9216.0, 0),                         # the bin edges
        (3, 2, 300.0, 300.0, 20.0, 20.0, 1024.0 + 0.5, 0),
        (4, 0, 200.0, 200.0, 16.0, 16.0, 256.0, 0), (4, 0, 230.0, 200.0, 16.0, 16.0, 256.0, 0),                           # under the >100 rows
        (6, 3, 110.0, 110.0, 10.0, 10.0, 100.0, 0), (6, 3, 114.0, 110.0, 10.0, 10.0, 100.0, 0),                           # equal IoUs
        (7, 5, 90.0, 90.0, 30.0, 30.0, 900.0, 1),                                                                          # class 5: crowd only
        (8, 1, 100.0, 100.0, 10.0, 20.0, 200.0, 0), (8, 1, 150.0, 100.0, 40.0, 10.0, 400.0, 0),                           # IoU == threshold
        (8, 2, 100.0, 150.0, 10.0, 10.0, 100.0, 0), (8, 2, 100.0, 150.0, 10.0, 10.0, 100.0, 1),                           # crowd twin
    ]
    dts = [
        (1, 0, 70.25, 70.5, 20.125, 10.375, s(0.9)), (1, 0, 100.625, 101.0, 8.5, 29.75, s(0.85)), (1, 0, 71.0, 71.125, 30.5, 9.0, s(0.2)),
        (2, 1, 82.0, 82.0, 10.0, 10.0, s(0.95)), (2, 1, 100.0, 100.0, 12.0, 12.0, s(0.9)), (2, 1, 118.0, 118.0, 10.0, 10.0, s(0.7)),
        (3, 2, 100.0, 100.0, 32.0, 32.0, s(0.8)), (3, 2, 200.0, 100.0, 96.0, 96.0, s(0.75)), (3, 2, 300.0, 300.0, 20.0, 21.0, s(0.6)),
        (3, 2, 400.0, 400.0, 32.0, 32.0, s(0.5)),                                                                          # unmatched, area 1024
        (6, 3, 112.0, 110.0, 10.0, 10.0, s(0.9)), (6, 3, 112.0, 110.0, 10.0, 10.0, s(0.8)), (6, 3, 112.0, 110.0, 10.0, 10.0, s(0.7)),
        (7, 5, 95.0, 95.0, 10.0, 10.0, s(0.9)), (7, 5, 300.0, 300.0, 10.0, 10.0, s(0.8)),
        (8, 1, 100.0, 100.0, 10.0, 10.0, s(0.9)), (8, 1, 150.0, 100.0, 30.0, 10.0, s(0.8)),
        (8, 2, 100.0, 150.0, 10.0, 10.0, s(0.9)), (8, 2, 100.0, 150.0, 10.0, 10.0, s(0.8)), (8, 2, 101.0, 150.0, 10.0, 10.0, s(0.7)),
        (9, 0, 300.0, 300.0, 5.0, 5.0, s(0.9)), (10, 0, 300.0, 300.0, 5.0, 5.0, s(0.9)),                                  # equal scores across images
    ]
    rs = np.random.RandomState(11)
    for j in range(110):                                                   # more than 100 rows of one class in one image
        near = j % 3 == 0
        x, y = (200.0 + 30.0 * (j % 2) + rs.randint(-3, 4), 200.0 + rs.randint(-3, 4)) if near else (rs.randint(250, 400), rs.randint(250, 400))
        dts.append((4, 0, float(x), float(y), 16.0, 16.0, s((rs.randint(100, 9000) if j else 9500) / 10000)))
    return gts, dts


def extended_case(ref_gt, ref_dt):
    gts = [dict(image=int(r[0]), category=int(r[1]) - 1, bbox=[float(v) for v in r[2:6]], area=float(r[6]), iscrowd=int(r[7])) for r in ref_gt]
    dts = [dict(image=int(r[0]), category=int(r[1]) - 1, bbox=[float(v) for v in r[2:6]], score=float(np.float32(r[6]))) for r in ref_dt]
    pg, pd = planted()
    gts += [dict(image=g[0], category=g[1], bbox=list(g[2:6]), area=g[6], iscrowd=g[7]) for g in pg]
    dts += [dict(image=d[0], category=d[1], bbox=list(d[2:6]), score=d[6]) for d in pd]
    gts.sort(key=lambda g: g["image"])                                   # stable: (image, row) order
    dts.sort(key=lambda d: d["image"])
    return gts, dts


def check_cases(gts, dts):
    """every case the rules distinguish is in the data"""
    n = M.N_IMG
    out = C.coco_eval(gts, dts, range(n), NC)
    rank, matched, ignored = C.detection_masks(out["eval_imgs"], dts, NC)
    seen = dict.fromkeys(("float_boxes", "crowd_twice", "area_1024", "area_9216", "over_100", "equal_iou", "tie_across", "crowd_only_class",
                          "iou_is_threshold", "det_area_edge", "gt_only_class"), False)
    seen["float_boxes"] = any(v != int(v) for d in dts for v in d["bbox"]) and any(v != int(v) for g in gts for v in g["bbox"])
    seen["area_1024"] = any(g["area"] == 1024 and not g["iscrowd"] for g in gts)
    seen["area_9216"] = any(g["area"] == 9216 and not g["iscrowd"] for g in gts)
    seen["det_area_edge"] = any(d["bbox"][2] * d["bbox"][3] == 1024 and not (matched[i] & 1) for i, d in enumerate(dts))
    seen["over_100"] = bool((rank >= 100).any())
    per = {}
    for i, d in enumerate(dts):
        per.setdefault((d["image"], d["category"]), []).append(i)
    for (img, cat), idx in per.items():
        g_here = [g for g in gts if g["image"] == img and g["category"] == cat]
        for g in g_here:
            if g["iscrowd"]:
                hit = [i for i in idx if C.bbox_iou(dts[i]["bbox"], g["bbox"], 1) >= 0.5 and (matched[i] & 1) and (ignored[i] & 1)]
                lone = not any(not h["iscrowd"] and C.bbox_iou(dts[i]["bbox"], h["bbox"], 0) > 0 for h in g_here for i in hit)
                seen["crowd_twice"] |= len(hit) >= 2 and lone
        for i in idx:
            v = [C.bbox_iou(dts[i]["bbox"], g["bbox"], g["iscrowd"]) for g in g_here]
            seen["equal_iou"] |= any(v.count(x) >= 2 and x >= 0.5 for x in v)
            seen["iou_is_threshold"] |= any(x == t for x in v for t in C.IOU_THRS[[0, 5]])
    by_score = {}
    for d in dts:
        by_score.setdefault((d["category"], d["score"]), set()).add(d["image"])
    seen["tie_across"] = any(len(v) > 1 for v in by_score.values())
    for k in range(NC):
        g_k = [g for g in gts if g["category"] == k]
        d_k = [d for d in dts if d["category"] == k]
        seen["crowd_only_class"] |= len(g_k) > 0 and all(g["iscrowd"] for g in g_k) and len(d_k) > 0
        seen["gt_only_class"] |= len(g_k) > 0 and not d_k
    assert all(seen.values()), seen
    assert (out["npig"].sum(0) > 0).all(), "every area range has a counted ground truth"
    assert (out["stats"] > 0.01).all() and 0.05 < out["stats"][0] < 0.95, out["stats"]
    return out


def main():
    dets, gts = M.make_data()
    tmp = tempfile.mkdtemp(prefix="coco_inputs_")
    os.makedirs(os.path.join(tmp, "ground-truth"))
    os.makedirs(os.path.join(tmp, "detection-results"))
    for img in range(M.N_IMG):
        with open(os.path.join(tmp, "detection-results", f"img_{img:03d}.txt"), "w") as f:
            for cls, k, l, t, r, b in dets[img]:
                f.write(f"{M.NAMES[cls]} {str(np.float32(k / 10000))[:6]} {int(l)} {int(t)} {int(r)} {int(b)}\n")
        with open(os.path.join(tmp, "ground-truth", f"img_{img:03d}.txt"), "w") as f:
            for cls, l, t, r, b, difficult in gts[img]:
                f.write(f"{M.NAMES[cls]} {l} {t} {r} {b}" + (" difficult\n" if difficult else "\n"))

    make_golden._import_reference()
    from core.metrics import mAP as ref            # the reference's
    assert os.path.abspath(ref.__file__).startswith(make_golden.REF), ref.__file__
    got_gt = ref.preprocess_gt(os.path.join(tmp, "ground-truth"), M.NAMES)
    got_dt = ref.preprocess_dr(os.path.join(tmp, "detection-results"), M.NAMES)
    image_of = lambda s: int(str(s).split("_")[1])  # noqa: E731
    assert [c["id"] for c in got_gt["categories"]] == list(range(1, NC + 1))
    assert sorted(image_of(i["id"]) for i in got_gt["images"]) == list(range(M.N_IMG))
    ref_gt = np.array(sorted(([image_of(a["image_id"]), a["category_id"]] + list(a["bbox"]) + [a["area"], a["iscrowd"], a["id"]]
                              for a in got_gt["annotations"]), key=lambda r: r[0]), np.float64)
    ref_dt = np.array(sorted(([image_of(d["image_id"]), d["category_id"]] + list(d["bbox"]) + [d["score"]] for d in got_dt),
                             key=lambda r: r[0]), np.float64)
    assert len(ref_gt) == sum(len(g) for g in gts) and len(ref_dt) == sum(len(d) for d in dets)

    cg, cd = extended_case(ref_gt, ref_dt)
    out = check_cases(cg, cd)
    rows, counts, gt, gt_counts = C.arrays_from_lists(cg, cd, M.N_IMG)
    assert rows.shape[1] <= 128 and gt.shape[1] <= 16, (rows.shape, gt.shape)
    coco_gt = np.array([[g["image"], g["category"]] + g["bbox"] + [g["area"], g["iscrowd"]] for g in cg], np.float64)
    coco_dt = np.array([[d["image"], d["category"]] + d["bbox"] + [d["score"]] for d in cd], np.float64)
    path = os.path.join(ROOT, "tests", "golden", "coco_inputs_ref.npz")
    np.savez_compressed(path, ref_gt=ref_gt, ref_dt=ref_dt, coco_gt=coco_gt, coco_dt=coco_dt, coco_n_images=np.int64(M.N_IMG),
                        num_classes=np.int64(NC), names=np.array(M.NAMES))
    print(f"wrote {path}: {len(ref_gt)} + {len(coco_gt) - len(ref_gt)} ground truths, {len(ref_dt)} + {len(coco_dt) - len(ref_dt)} detections, "
          f"stats {np.round(out['stats'], 4).tolist()}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
