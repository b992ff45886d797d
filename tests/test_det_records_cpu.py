"""What the detection metrics share on the host (computervision/pytorch_amd/det_records.py) and the LDS layouts of csrc/det_common.h:
``check_batch`` for both ground-truth formats, the record order on a hand-built input, and the two layout functions against the closed
forms of their sizes (tests/det_lds_check.cpp, a host program).  No GPU is needed."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from computervision.pytorch_amd import coco_eval, det_diag, det_eval, det_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "computervision.pytorch_amd", "csrc")
CPU = torch.device("cpu")
FORMATS = [(torch.int32, 6), (torch.float64, 7)]


def batch(dtype, width, B=3, K=5, G=2):
    return dict(rows=torch.zeros(B, K, 6), counts=torch.zeros(B, dtype=torch.int32), gt=torch.zeros(B, G, width, dtype=dtype),
                gt_counts=torch.zeros(B, dtype=torch.int32), box_map=torch.zeros(B, 4))


def check(args, dtype, width, max_det=8, device=CPU):
    return det_records.check_batch(args["rows"], args["counts"], args["gt"], args["gt_counts"], args["box_map"], max_det, device, dtype, width)


def test_old_import_paths_are_the_shared_objects():
    for module in (det_eval, coco_eval):
        assert module.check_batch is det_records.check_batch and module.default_capacity is det_records.default_capacity
        assert (module.MAX_ROWS, module.MAX_GT) == (det_records.MAX_ROWS, det_records.MAX_GT) == (16384, 1024)
    assert det_diag.check_batch is det_records.check_batch and det_diag.MAX_ROWS == 16384
    assert issubclass(det_eval.DetectionEvaluator, det_records.RecordEvaluator) and issubclass(coco_eval.CocoEvaluator, det_records.RecordEvaluator)
    assert not issubclass(det_diag.DetectionDiagnostics, det_records.RecordEvaluator)


@pytest.mark.parametrize("dtype,width", FORMATS)
def test_check_batch_accepts(dtype, width):
    args = batch(dtype, width)
    args["rows"] = torch.zeros(3, 6, 5).transpose(1, 2)                        # not contiguous: returned contiguous
    out = check(args, dtype, width)
    assert len(out) == 5 and all(t.is_contiguous() for t in out) and out[0].shape == (3, 5, 6)
    args["box_map"] = None
    assert check(args, dtype, width)[4] is None
    args["gt"] = torch.zeros(3, 0, 1, dtype=dtype)                             # no ground-truth slot: the width is not looked at
    assert check(args, dtype, width)[2].shape[1] == 0
    args["rows"], args["gt"] = torch.zeros(3, 8, 6), torch.zeros(3, det_records.MAX_GT, width, dtype=dtype)
    check(args, dtype, width)                                                   # K == max_det and G == MAX_GT are inside


def test_check_batch_is_int32_by_6_by_default():
    args = batch(torch.int32, 6)
    assert det_records.check_batch(args["rows"], args["counts"], args["gt"], args["gt_counts"], None, 8, CPU)[2].dtype == torch.int32


REJECTED = [
    ("rows", lambda d, w: torch.zeros(3, 30), "rows: \\(B, K <= 8, 6\\) float32"),                                # rank
    ("rows", lambda d, w: torch.zeros(3, 5, 7), "rows: "),                                                        # last dimension
    ("rows", lambda d, w: torch.zeros(3, 5, 6, dtype=torch.float64), "rows: "),                                   # dtype
    ("rows", lambda d, w: torch.zeros(3, 9, 6), "rows: "),                                                        # K past max_det
    ("rows", lambda d, w: torch.zeros(3, 0, 6), "rows: "),                                                        # no row slot
    ("gt", lambda d, w: torch.zeros(3, 2 * w, dtype=d), "gt: \\(B, G <= 1024, [67]\\) (int32|float64), got"),      # rank
    ("gt", lambda d, w: torch.zeros(3, 2, w + 1, dtype=d), "gt: "),                                               # last dimension
    ("gt", lambda d, w: torch.zeros(3, 2, w, dtype=torch.float32), "gt: "),                                       # dtype
    ("gt", lambda d, w: torch.zeros(3, 2, w, dtype=torch.float64 if d == torch.int32 else torch.int32), "gt: "),  # the other format's
    ("gt", lambda d, w: torch.zeros(3, 1025, w, dtype=d), "gt: "),                                                # G past MAX_GT
    ("gt", lambda d, w: torch.zeros(2, 2, w, dtype=d), "gt: "),                                                   # another batch size
    ("counts", lambda d, w: torch.zeros(3, dtype=torch.int64), "counts and gt_counts"),
    ("counts", lambda d, w: torch.zeros(4, dtype=torch.int32), "counts and gt_counts"),
    ("gt_counts", lambda d, w: torch.zeros(3, dtype=torch.int64), "counts and gt_counts"),
    ("gt_counts", lambda d, w: torch.zeros(2, dtype=torch.int32), "counts and gt_counts"),
    ("box_map", lambda d, w: torch.zeros(3, 3), "box_map: \\(B, 4\\) float32"),
    ("box_map", lambda d, w: torch.zeros(4, 4), "box_map: "),
    ("box_map", lambda d, w: torch.zeros(3, 4, dtype=torch.float64), "box_map: "),
]


@pytest.mark.parametrize("dtype,width", FORMATS)
@pytest.mark.parametrize("name,make,message", REJECTED)
def test_check_batch_rejects(dtype, width, name, make, message):
    args = batch(dtype, width)
    args[name] = make(dtype, width)
    with pytest.raises(ValueError, match=message):
        check(args, dtype, width)


@pytest.mark.parametrize("dtype,width", FORMATS)
def test_check_batch_rejects_another_device(dtype, width):
    with pytest.raises(ValueError, match="every tensor lives on the evaluator's device"):
        check(batch(dtype, width), dtype, width, device=torch.device("meta"))
    args = batch(dtype, width)
    args["box_map"] = torch.zeros(3, 4, device="meta")
    with pytest.raises(ValueError, match="every tensor lives on the evaluator's device"):
        check(args, dtype, width)


def test_record_order_on_a_hand_built_input():
    nc = 3
    #                 slot:   0    1    2    3    4    5    6    7    8    9
    cls = torch.tensor([2,   0,   3,   2,   0,   2,   3,   0,   2,   0], dtype=torch.int32)          # 3 == nc: unwritten
    score = torch.tensor([.5, .25, 0., .75, .25, .5,  0., .9,  .5,  1e-4], dtype=torch.float32)
    order, sorted_cls, seg_off = det_records.record_order(cls, score, nc)
    # class ascending; inside a class the score descends; equal scores (slots 1, 4 and 0, 5, 8) keep their append order; class 1 is empty
    assert order.tolist() == [7, 1, 4, 9, 3, 0, 5, 8, 2, 6]
    assert sorted_cls.tolist() == [0, 0, 0, 0, 2, 2, 2, 2, 3, 3] and sorted_cls.dtype == torch.int64
    assert seg_off.tolist() == [0, 4, 4, 8] and seg_off.numel() == nc + 1 and seg_off.dtype == torch.int64
    assert sorted_cls.is_contiguous() and seg_off.is_contiguous()
    s = score[order]
    for c in range(nc):
        seg = s[seg_off[c]:seg_off[c + 1]]
        assert bool((seg[:-1] >= seg[1:]).all())
    # nothing written at all: every slot behind every class
    order, sorted_cls, seg_off = det_records.record_order(torch.full((4,), nc, dtype=torch.int32), torch.zeros(4), nc)
    assert order.tolist() == [0, 1, 2, 3] and seg_off.tolist() == [0, 0, 0, 0]


def test_record_order_against_a_python_sort():
    rs = np.random.RandomState(0)
    nc, n = 5, 400
    cls = rs.randint(0, nc + 1, n).astype(np.int32)
    score = rs.choice(np.linspace(0.001, 1, 12).astype(np.float32), n)
    order, _, seg_off = det_records.record_order(torch.from_numpy(cls), torch.from_numpy(score), nc)
    assert order.tolist() == sorted(range(n), key=lambda i: (cls[i], -float(score[i]), i))
    assert seg_off.tolist() == [int((cls < c).sum()) for c in range(nc + 1)]


def test_default_capacity_and_the_base_class_checks():
    assert det_records.default_capacity([0] * 7, 8, 300, "x") == 7 * 8 * 300 and det_records.default_capacity([0] * 7, 8, 16384, "x") == 7 * 8 * 1024
    with pytest.raises(Exception, match="evaluate_on_voc: a dataloader without len\\(\\) needs capacity="):
        det_records.default_capacity(iter(()), 8, 300, "evaluate_on_voc")
    for make, entry, entries in ((det_eval.DetectionEvaluator, "cvx_det_match", "cvx_det_match / cvx_det_ap"),
                                 (coco_eval.CocoEvaluator, "cvx_coco_match", "cvx_coco_match / cvx_coco_accumulate")):
        with pytest.raises(ValueError, match=f"max_det 16385: {entry} holds 1 .. 16384 rows per image"):
            make(4, 16385, 10, CPU)
        with pytest.raises(ValueError, match="num_classes and capacity are positive"):
            make(4, 16, 0, CPU)
        ev = make(4, 16, 10, CPU)
        ev.reset()                                                                   # nothing allocated yet: nothing to clear
        with pytest.raises(Exception, match=re.escape(f"{make.__name__} runs on an MI355X only ({entries}): there is no CPU path")):
            ev.add_batch(*[None] * 4)


def _build(out):
    src = os.path.join(ROOT, "tests", "det_lds_check.cpp")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-I", CSRC, src, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout
    return cmd


def test_lds_layouts_return_the_closed_forms(tmp_path):
    """the grid max_det in {1, 255, 256, 257, 16384} x G in {0, 1, 2, 1023, 1024}: 32 + 32 * slots(G) + 8 * ((max_det + 3) & ~3) for
    det_match_kernel and 36 * slots(G) + 4 * max_det for det_confusion_kernel, slots(G) = (G + 1) & ~1"""
    exe = str(tmp_path / "det_lds_check")
    print(" ".join(_build(exe)))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert re.search(r"det_lds_check: 25 cases ok", r.stdout), r.stdout
    lines = dict(((int(m.group(1)), int(m.group(2))), (int(m.group(3)), int(m.group(4))))
                 for m in re.finditer(r"max_det\s+(\d+) G\s+(\d+): det_match (\d+) .*? det_confusion (\d+) ", r.stdout))
    assert len(lines) == 25
    for (max_det, G), (match, confusion) in lines.items():                     # the closed forms once more, on this side
        slots = (G + 1) & ~1
        assert match == 32 + 32 * slots + 8 * ((max_det + 3) & ~3) and confusion == 36 * slots + 4 * max_det, (max_det, G)
