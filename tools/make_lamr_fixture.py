"""Write tests/golden/det_lamr_ref.npz: what the REFERENCE's ``log_average_miss_rate`` (core/metrics/mAP.py:34-70) makes of the data of
tests/golden/det_map_ref.npz and of a few synthetic edge arrays.

    python tools/make_lamr_fixture.py          # CPU only; needs the reference tree (CVX_REFERENCE), never runs on the GPU box

Per ground-truth class of the mAP fixture the function is called as ``get_map`` calls it (:634-636): with the class's recall array (the
reference's own capture, stored in det_map_ref.npz), its cumulative FP counts (from the sequential restatement's flags, which
tests/test_det_eval_cpu.py holds to the reference) and ``counter_images_per_class``.  The edge cases: an empty class; one image with a
false positive first; 100 images with cumulative FP counts that hit 1 / 100 and 100 / 100, the first and the last reference point, so
that the ``<=`` is exercised at both ends.  Stored: the inputs of every call and the returned LAMR.  Data only: no reference program
text goes into the fixture.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import det_diag_restatement as D  # noqa: E402
import det_eval_restatement as R  # noqa: E402
from oracle import make_golden  # noqa: E402  (its stubs and its way of importing the reference)


def edge_cases():
    """(name, rec, fp_cum, n_images)"""
    hundred_fp = np.array([0, 1, 1, 2, 50, 99, 100, 101], np.int64)
    return [("empty", np.zeros(0), np.zeros(0, np.int64), 3),
            ("one_image_fp_first", np.array([0.0, 0.5, 0.5, 1.0]), np.array([1, 1, 2, 2], np.int64), 1),
            ("hundred_images", np.array([0.125, 0.125, 0.25, 0.25, 0.375, 0.5, 0.5, 0.625]), hundred_fp, 100)]


def main():
    z = np.load(os.path.join(ROOT, "tests", "golden", "det_map_ref.npz"), allow_pickle=False)
    nc = len(z["names"])
    dets, gts, _ = R.fixture_inputs(z)
    ours = R.get_map(dets, gts, nc)
    flags = D.flags_per_class(dets, ours["flags"], nc)
    images = D.confusion(dets, gts, nc)["images_per_class"]
    off = z["curve_off"]

    make_golden._import_reference()
    from core.metrics import mAP as ref            # the reference's
    assert os.path.abspath(ref.__file__).startswith(make_golden.REF), ref.__file__

    lamr = np.full(nc, np.nan)
    fp_cum, fp_off = [], [0]
    for c in range(nc):
        fp = D.fp_cumsum(flags[c])
        if c in z["gt_classes"].tolist():
            rec = z["rec"][off[c]:off[c + 1]]
            assert len(rec) == len(fp) and images[c] > 0
            lamr[c] = ref.log_average_miss_rate(np.array(rec), np.array(fp), int(images[c]))[0]
            fp_cum.append(fp)
        else:
            fp_cum.append(np.zeros(0, np.int64))
        fp_off.append(fp_off[-1] + len(fp_cum[-1]))
    edges = edge_cases()
    edge_lamr = np.array([ref.log_average_miss_rate(np.array(rec), np.array(fp), n)[0] for _, rec, fp, n in edges], np.float64)
    # the restatement agrees before anything is stored (tests/test_det_diag_cpu.py checks it again from the file)
    for (_, rec, fp, n), want in zip(edges, edge_lamr):
        assert D.lamr(D.miss_rates(rec, fp, n), len(rec), n) == want, want
    for c in z["gt_classes"].tolist():
        rec = z["rec"][off[c]:off[c + 1]]
        assert D.lamr(D.miss_rates(rec, fp_cum[c], images[c]), len(rec), images[c]) == lamr[c], (c, lamr[c])
    path = os.path.join(ROOT, "tests", "golden", "det_lamr_ref.npz")
    np.savez_compressed(path, lamr=lamr, images_per_class=images, fp_cum=np.concatenate(fp_cum), fp_off=np.array(fp_off, np.int64),
                        edge_names=np.array([e[0] for e in edges]), edge_rec=np.concatenate([e[1] for e in edges]),
                        edge_fp_cum=np.concatenate([e[2] for e in edges]), edge_off=np.cumsum([0] + [len(e[1]) for e in edges]).astype(np.int64),
                        edge_n_images=np.array([e[3] for e in edges], np.int64), edge_lamr=edge_lamr)
    print(f"wrote {path}: LAMR {lamr.tolist()}, edges {edge_lamr.tolist()}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
