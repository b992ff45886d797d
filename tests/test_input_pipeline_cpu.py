"""CPU: the host side of the input pipeline -- validation ``draw_params``, the restated validation boxes and images against
tests/golden/aug_val_ref.npz (the REAL reference ``DetectionDataset(train=False)`` run over seeded pictures, tools/make_aug_val_golden.py), the
restated per-image regrouping against tests/golden/aug_ref.npz, and the exported symbols.  Like aug_ref.npz, the fixture does not pin the
bicubic resize against OpenCV's bytes (its ``note``)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import aug_restatement as R
import input_pipeline_restatement as P
from computervision.pytorch_amd import LIB_PATH, CvxError, augment
from computervision.pytorch_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def val(gold):
    g = gold("aug_val_ref.npz")
    assert "NOT checked against OpenCV" in str(g["note"])
    return P.load_val_cases(g)


def test_validation_draw_params_leaves_the_random_state_untouched():
    rng = np.random.RandomState(5)
    before = rng.get_state()
    p = augment.draw_params(rng, [(375, 500)], (300, 300), False, train=False)
    aug = augment.DeviceAugmenter((300, 300), mosaic=True, mosaic_prob=1.0, seed=5, train=False)
    assert not aug.want_mosaic() and not aug.mosaic
    for r in (rng, aug.rng):
        after = r.get_state()
        assert after[0] == before[0] and np.array_equal(after[1], before[1]) and after[2:] == before[2:]
    assert p["r"] is None and p["cut"] is None and np.array_equal(p["lut"], R.identity_lut())
    assert p["jobs"] == [dict(ih=375, iw=500, nh=225, nw=300, dx=0, dy=37, flip=0, quad=-1, rect=(0, 0, 300, 300))]
    with pytest.raises(ValueError):
        augment.draw_params(rng, [(8, 8)] * 4, (64, 96), True, train=False)


def test_validation_geometry_equals_the_fixture(val):
    H, W, cases = val
    kinds = set()
    for c in cases:
        ih, iw = (int(v) for v in c["sizes"][0])
        p = augment.draw_params(np.random.RandomState(0), [(ih, iw)], (H, W), False, train=False)
        assert p["jobs"] == [c["job"]] == [P.val_job(ih, iw, H, W)]
        jb = c["job"]
        kinds.add("bars left and right" if jb["dx"] > 0 else "bars top and bottom" if jb["dy"] > 0 else "fills the canvas")
        kinds.add("upscaled" if jb["nh"] > ih else "downscaled" if jb["nh"] < ih else "same size")
    assert kinds == {"bars left and right", "bars top and bottom", "fills the canvas", "upscaled", "downscaled", "same size"}


def test_restated_validation_boxes_equal_the_fixture_bit_for_bit(val):
    H, W, cases = val
    clamped = discarded = empty = False
    for c in cases:
        got = R.targets([[(c["job"], c["boxes"])]], H, W)
        assert got.dtype == np.float32 and got.shape == c["labels"].shape and np.array_equal(got, c["labels"])
        empty |= len(c["boxes"]) == 0
        discarded |= 0 < len(c["labels"]) < len(c["boxes"])
        if len(got):
            x1, x2 = got[:, 2] - got[:, 4] / 2, got[:, 2] + got[:, 4] / 2
            clamped |= bool((np.abs(x1) < 1e-6).any() and (np.abs(x2 - 1) < 1e-6).any())
    assert clamped and discarded and empty


def test_restated_validation_images_equal_the_fixture(val):
    """no colour transform: the fixture picture is the pasted resize itself"""
    H, W, cases = val
    n = 0
    for c in cases:
        if c["image"] is None:
            continue
        plain = P.render_plain([c["job"]], [c["picture"]], H, W)
        assert np.array_equal(plain, c["image"])
        assert not np.array_equal(R.render([c["job"]], [c["picture"]], R.identity_lut(), H, W), plain)   # HSV round trip is lossy in 8 bits
        n += 1
    assert n == 3


def test_restated_regrouping_equals_the_per_image_rows_of_the_training_fixture(gold):
    H, W, cases = R.load_cases(gold("aug_ref.npz"))
    rows = R.targets([list(zip(c["jobs"], c["job_boxes"])) for c in cases], H, W)
    most = max(len(c["labels"]) for c in cases)
    assert most > 4 and any(len(c["labels"]) == 0 for c in cases)
    labels, counts, overflow = P.regroup(rows, len(cases), most)
    assert overflow == 0 and labels.dtype == np.float32 and counts.dtype == np.int32
    for b, c in enumerate(cases):
        n = len(c["labels"])
        assert counts[b] == n and np.array_equal(labels[b, :n], c["labels"][:, 1:]) and not labels[b, n:].any()
        assert np.array_equal(P.per_image_rows(rows, len(cases))[b][:, 1:], c["labels"][:, 1:])
    cut, counts4, overflow4 = P.regroup(rows, len(cases), 4)
    assert overflow4 == 1
    for b, c in enumerate(cases):
        n = min(len(c["labels"]), 4)
        assert counts4[b] == n and np.array_equal(cut[b, :n], c["labels"][:n, 1:]) and not cut[b, n:].any()


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("cvx_aug_images_plain", "cvx_aug_boxes_padded"):
        assert name in declared and name in L.PROTOTYPES and hasattr(lib, name)
    assert len(L.PROTOTYPES["cvx_aug_images_plain"][1]) == 7 and len(L.PROTOTYPES["cvx_aug_boxes_padded"][1]) == 13
    assert len(L.PROTOTYPES["cvx_aug_images"][1]) == 8 and len(L.PROTOTYPES["cvx_aug_boxes"][1]) == 10       # unchanged
    assert augment.JOB_DTYPE.itemsize == 64


def test_formats_targets_and_loader_arguments():
    aug = augment.DeviceAugmenter((64, 96), seed=0)
    with pytest.raises(ValueError):
        aug.apply([], [], [], fmt="voc")
    for fmt in ("ssd", "centernet"):
        with pytest.raises(ValueError, match="target"):                       # no algorithm object / spec given
            aug.apply([], [], [], fmt=fmt)
    with pytest.raises(CvxError):                                             # still no CPU path
        augment.DeviceAugmenter((64, 96), train=False)([torch.zeros(8, 8, 3, dtype=torch.uint8)], [np.zeros((0, 5), np.float32)])
    source = [(torch.zeros(8, 8, 3, dtype=torch.uint8), np.zeros((0, 5), np.float32))] * 5
    val_aug = augment.DeviceAugmenter((64, 96), train=False)
    assert len(augment.DeviceAugLoader(source, 2, val_aug, device="cpu")) == 2                      # the reference's drop_last=True
    assert len(augment.DeviceAugLoader(source, 2, val_aug, device="cpu", drop_last=False)) == 3
    assert len(augment.DeviceAugLoader(source, 2, aug, length=7, device="cpu")) == 7
    with pytest.raises(ValueError):
        augment.DeviceAugLoader(source, 2, aug, device="cpu")                 # a training loader needs its length

    class Alg:                                                                # what target_spec reads of Ssd / CenterNetA
        anchors, num_classes, overlap_threshold, variance = np.zeros((8, 4), np.float32), 20, 0.5, np.array([0.1, 0.1, 0.2, 0.2], np.float32)

    spec = augment.target_spec("ssd", Alg())
    assert spec.num_classes == 20 and spec.variances == pytest.approx((0.1, 0.2)) and spec.overlap_threshold == 0.5
