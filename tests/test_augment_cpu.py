"""CPU: the host side of the device augmentation (``computervision.pytorch_amd.augment.draw_params``) and the host restatement of its
kernels (tests/aug_restatement.py) against tests/golden/aug_ref.npz -- the REAL reference ``DetectionDataset`` code run over seeded pictures
(tools/make_aug_golden.py).  The fixture pins geometry, draw order, LUTs, box arithmetic and box merging; it does not pin the pixel
primitives against OpenCV's bytes (its ``note``)."""
import ctypes
import os
import re

import numpy as np
import pytest

import aug_restatement as R
from computervision.pytorch_amd import LIB_PATH, CvxError, augment
from computervision.pytorch_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture(gold):
    g = gold("aug_ref.npz")
    assert "NOT checked against OpenCV" in str(g["note"])
    return R.load_cases(g)


def test_draw_params_reproduces_every_recorded_parameter_and_lut(fixture):
    H, W, cases = fixture
    assert sum(int(c["mosaic"]) for c in cases) >= 3 and sum(1 - int(c["mosaic"]) for c in cases) >= 8
    for c in cases:
        rng = np.random.RandomState(int(c["seed"]))
        if c["mosaic"]:
            rng.rand()                                   # DetectionDataset.__getitem__'s mosaic_prob draw (DeviceAugmenter.want_mosaic)
        p = augment.draw_params(rng, [tuple(s) for s in c["sizes"]], (H, W), bool(c["mosaic"]), nboxes=[len(b) for b in c["job_boxes"]])
        assert p["jobs"] == c["jobs"], (int(c["seed"]), p["jobs"], c["jobs"])
        assert p["lut"].dtype == np.uint8 and np.array_equal(p["lut"], c["lut"])
        if c["mosaic"]:
            assert p["cut"] == tuple(int(v) for v in c["cut"])


def test_restatement_boxes_equal_the_reference_bit_for_bit(fixture):
    H, W, cases = fixture
    kinds = set()
    for c in cases:
        got = R.targets([list(zip(c["jobs"], c["job_boxes"]))], H, W)
        assert got.dtype == np.float32 and got.shape == c["labels"].shape and np.array_equal(got, c["labels"]), int(c["seed"])
        jb = c["jobs"][0]
        if c["mosaic"]:
            cx, cy = c["cut"]
            for j, b in zip(c["jobs"], c["job_boxes"]):
                pre = R.boxes_of_job(j, b, H, W, merge=False)
                if len(pre) and ((pre[:, 0] <= cx) & (pre[:, 2] >= cx) & (pre[:, 1] <= cy) & (pre[:, 3] >= cy)).any():
                    kinds.add("straddles both cuts")
        else:
            kinds.add("flipped" if jb["flip"] else "plain")
            if jb["dy"] < 0 or jb["dx"] < 0:
                kinds.add("overhanging")
            if len(c["labels"]) < len(c["boxes"]):
                kinds.add("filtered")
    assert kinds == {"plain", "flipped", "overhanging", "filtered", "straddles both cuts"}, kinds


def test_restatement_merge_equals_reference_merge_bboxes(gold):
    g = gold("aug_ref.npz")
    cutx, cuty = (int(v) for v in g["merge_cut"])
    got = np.concatenate([R.merge_boxes(g["merge_in"][q], q, cutx, cuty) for q in range(4)], 0)
    assert 0 < len(g["merge_out"]) < 40                               # some dropped, some kept
    assert np.array_equal(got, g["merge_out"])
    clipped = sum(int((R.merge_boxes(g["merge_in"][q], q, cutx, cuty)[:, :4] == v).any()) for q in range(4) for v in (cutx, cuty))
    assert clipped > 0                                                 # a coordinate was moved to a cut


def test_restatement_composition_equals_the_reference_images(fixture):
    """paste position, canvas / source flip and the quadrant order, through the same pixel primitives the fixture's stand-in cv2 used"""
    H, W, cases = fixture
    seen = set()
    for c in cases:
        if c["image"] is None:
            continue
        srcs = [R.synth_picture(int(s[0]), int(s[1]), int(k)) for s, k in zip(c["sizes"], c["src_seeds"])]
        assert np.array_equal(R.render(c["jobs"], srcs, c["lut"], H, W), c["image"])
        seen.add(int(c["mosaic"]))
    assert seen == {0, 1}


def test_pixel_primitives_basic_properties():
    pic = R.synth_picture(37, 53, 1)
    assert np.array_equal(R.resize_cubic(pic, (53, 37)), pic)                     # same size: weights (0, 2048, 0, 0)
    s, w = R.cubic_taps(61, 53)
    assert (abs(w.sum(1) - 2048) <= 1).all() and s.min() == -2 and s.max() == 51     # fx(0) = -0.07: taps -2 .. 1, clamped to the picture
    grey = np.full((2, 2, 3), 128, np.uint8)
    assert np.array_equal(R.colour(grey, R.identity_lut()), grey)
    assert R.SDIV[255] == 4096 and R.HDIV[1] == 122880 and R.SDIV[0] == 0 and R.HDIV[0] == 0


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("cvx_aug_images", "cvx_aug_boxes"):
        assert name in declared and name in L.PROTOTYPES and hasattr(lib, name)
    assert len(L.PROTOTYPES["cvx_aug_images"][1]) == 8 and len(L.PROTOTYPES["cvx_aug_boxes"][1]) == 10
    assert "cvx_aug_job" in header and augment.JOB_DTYPE.itemsize == 64


def test_no_cpu_path():
    import torch
    aug = augment.DeviceAugmenter((64, 96), seed=0)
    with pytest.raises(CvxError):
        aug([torch.zeros(8, 8, 3, dtype=torch.uint8)], [np.zeros((0, 5), np.float32)])
