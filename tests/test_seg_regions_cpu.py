"""No GPU: the numpy restatement of connected-component regions (tests/seg_regions_restatement.py) against hand-derived answers and against
``scipy.ndimage.label``, and the surface of ``seg_regions`` -- parameter validation, the refusal of host tensors, the table layouts, the
symbols in header, library and binding."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd._lib import LIB_PATH
import seg_regions_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- 1. the restatement against answers worked out by hand -----------------------------------------------------------------------------------
DIAGONAL = np.array([[0, 0, 0, 0, 0, 0, 0],
                     [0, 1, 1, 0, 0, 0, 0],
                     [0, 1, 1, 0, 0, 0, 0],
                     [0, 0, 0, 1, 1, 1, 0],
                     [0, 0, 0, 0, 0, 0, 0]], np.uint8)


def test_two_blobs_that_touch_diagonally():
    r8 = SR.regions(DIAGONAL, connectivity=8, min_area=1, max_det=4)
    assert r8["total"] == 1 and r8["count"] == 1
    assert r8["rows"][0].tolist() == [1.0, 1.0, 6.0, 4.0, 1.0, 1.0] and r8["areas"].tolist() == [7, -1, -1, -1] and r8["seeds"].tolist() == [8, -1, -1, -1]
    assert not r8["rows"][1:].any()
    assert np.array_equal(r8["region_map"], np.where(DIAGONAL == 1, 0, -1))
    r4 = SR.regions(DIAGONAL, connectivity=4, min_area=1, max_det=4)
    assert r4["total"] == 2 and r4["count"] == 2
    assert r4["rows"][:2].tolist() == [[1.0, 1.0, 3.0, 3.0, 1.0, 1.0], [3.0, 3.0, 6.0, 4.0, 1.0, 1.0]]      # area 4 before area 3
    assert r4["areas"].tolist() == [4, 3, -1, -1] and r4["seeds"].tolist() == [8, 24, -1, -1]
    want = np.full((5, 7), -1, np.int32)
    want[1:3, 1:3], want[3, 3:6] = 0, 1
    assert np.array_equal(r4["region_map"], want)


def test_equal_areas_are_ordered_by_seed_and_classes_do_not_connect():
    m = np.array([[2, 2, 0, 1, 1],
                  [0, 0, 0, 0, 0],
                  [1, 1, 2, 2, 3]], np.uint8)
    r = SR.regions(m, connectivity=8, min_area=1, max_det=8)
    assert r["total"] == 5
    assert r["seeds"][:5].tolist() == [0, 3, 10, 12, 14] and r["areas"][:5].tolist() == [2, 2, 2, 2, 1]
    assert r["rows"][:5, 5].tolist() == [2.0, 1.0, 1.0, 2.0, 3.0]
    assert r["rows"][3].tolist() == [2.0, 2.0, 4.0, 3.0, 1.0, 2.0]
    # the 2 at (2, 2) touches the 1 at (2, 1) and the 3 at (2, 4) touches the 2 at (2, 3): different labels never join
    assert r["region_map"].tolist() == [[0, 0, -1, 1, 1], [-1, -1, -1, -1, -1], [2, 2, 3, 3, 4]]


def test_foreground_leaves_out_labels_0_and_255():
    m = np.array([[0, 0, 255, 255],
                  [7, 7, 255, 0]], np.uint8)
    r = SR.regions(m, "foreground", 4, 1, 4)
    assert r["total"] == 1 and r["rows"][0].tolist() == [0.0, 1.0, 2.0, 2.0, 1.0, 7.0]
    r = SR.regions(m, "all", 4, 1, 4)
    assert r["total"] == 4 and r["areas"].tolist() == [3, 2, 2, 1] and r["seeds"].tolist() == [2, 0, 4, 7]
    assert r["rows"][:, 5].tolist() == [255.0, 0.0, 7.0, 0.0]
    r = SR.regions(m, [255], 4, 1, 4)
    assert r["total"] == 1 and r["rows"][0].tolist() == [2.0, 0.0, 4.0, 2.0, 1.0, 255.0]
    assert SR.class_mask("foreground").sum() == 254 and SR.class_mask("all").all() and SR.class_mask([3, 9]).nonzero()[0].tolist() == [3, 9]


def test_min_area_keeps_the_boundary_and_fill_paints_the_rest():
    m = np.array([[1, 1, 1, 0, 2, 2],
                  [0, 0, 0, 0, 0, 0],
                  [3, 0, 1, 1, 0, 255]], np.uint8)
    r = SR.regions(m, "foreground", 4, min_area=2, max_det=4, fill=9)
    assert r["total"] == 3 and r["areas"].tolist() == [3, 2, 2, -1] and r["seeds"].tolist() == [0, 4, 14, -1]     # area == min_area stays
    assert r["region_map"].tolist() == [[0, 0, 0, -1, 1, 1], [-1] * 6, [-1, -1, 2, 2, -1, -1]]
    assert r["clean_map"].tolist() == [[1, 1, 1, 0, 2, 2], [0] * 6, [9, 0, 1, 1, 0, 255]]       # the 255 is not selected: not painted
    r = SR.regions(m, "foreground", 4, min_area=3, max_det=4, fill=0)
    assert r["total"] == 1 and r["clean_map"].tolist() == [[1, 1, 1, 0, 0, 0], [0] * 6, [0, 0, 0, 0, 0, 255]]
    assert SR.regions(m, "foreground", 4, min_area=4, max_det=4)["total"] == 0 and SR.regions(m, min_area=4)["clean_map"] is None


def test_max_det_cuts_but_total_counts():
    m = np.array([[1, 0, 1, 1, 0, 1, 1, 1],
                  [0, 0, 0, 0, 0, 0, 0, 0],
                  [2, 2, 0, 2, 0, 0, 0, 0]], np.uint8)
    r = SR.regions(m, "foreground", 4, 1, max_det=2)
    assert r["total"] == 5 and r["count"] == 2
    assert r["areas"].tolist() == [3, 2] and r["seeds"].tolist() == [5, 2]
    assert r["rows"].shape == (2, 6) and r["rows"][1].tolist() == [2.0, 0.0, 4.0, 1.0, 1.0, 1.0]
    # the regions past the cut are not in the region map
    assert r["region_map"].tolist() == [[-1, -1, 1, 1, -1, 0, 0, 0], [-1] * 8, [-1] * 8]


def test_scores_from_a_confidence_plane_with_nan_and_values_outside_0_1():
    m = np.array([[1, 1, 1, 1, 0, 2, 2]], np.uint8)
    conf = np.array([[0.5, np.nan, -1.0, 2.0, 0.9, 1.0, 0.25]], np.float32)
    q = SR.quantise(conf)
    # 0.5 * 65535 = 32767.5 rounds to even; NaN -> 0; -1 -> 0; 2 -> 65535; 0.25 * 65535 = 16383.75 -> 16384
    assert q.tolist() == [[32768, 0, 0, 65535, 58982, 65535, 16384]]
    r = SR.regions(m, "foreground", 4, 1, 2, conf=conf)
    assert r["areas"].tolist() == [4, 2]
    want = np.array([np.float32((32768 + 65535) / (4 * 65535.0)), np.float32((65535 + 16384) / (2 * 65535.0))], np.float32)
    assert np.array_equal(bits(r["rows"][:2, 4]), bits(want))
    assert abs(float(want[0]) - 98303 / 262140) <= 2.0 ** -26 and abs(float(want[1]) - 81919 / 131070) <= 2.0 ** -25      # half an ulp
    ones = SR.regions(m, "foreground", 4, 1, 2, conf=np.ones((1, 7), np.float32))
    assert np.array_equal(bits(ones["rows"][:2, 4]), bits([1.0, 1.0]))


def test_capacity_flags_the_frame():
    full = SR.regions(SR.checkerboard(128, 128), "foreground", 4, 1, 8192)
    assert full["total"] == 8192 and full["count"] == 8192 and full["areas"].tolist() == [1] * 8192
    assert np.array_equal(full["seeds"], np.flatnonzero(SR.checkerboard(128, 128)))
    over = SR.regions(SR.checkerboard(128, 130), "foreground", 4, 1, 8192, fill=0)
    assert over["total"] == 8320 and over["count"] == -1 and not over["rows"].any() and (over["region_map"] == -1).all() and (over["seeds"] == -1).all()
    assert np.array_equal(over["clean_map"], SR.checkerboard(128, 130)) and SR.regions(SR.checkerboard(128, 130), "foreground", 8, 1, 8)["total"] == 1


def test_the_shapes_the_gpu_tests_use_are_what_they_say():
    for make in (SR.serpentine, SR.spiral):
        m = make(97, 131)
        r4, r8 = SR.regions(m, min_area=1, connectivity=4), SR.regions(m, min_area=1, connectivity=8)
        assert r4["total"] == r8["total"] == 1 and r4["seeds"][0] == 0 and r4["areas"][0] == int(m.sum()) and 6000 < int(m.sum()) < 97 * 131 * 0.55
        near = sum(np.pad(m, 1)[1 + dy:98 + dy, 1 + dx:132 + dx] for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)))
        assert int((near[m == 1] == 1).sum()) == 2 and int((near[m == 1] > 2).sum()) == 0          # a path: two ends, no branch
    assert SR.spiral(97, 131)[48, 40:90].any()                                                    # it ends in the middle rows
    comb = SR.comb(70, 133)
    r = SR.regions(comb, min_area=1, connectivity=4)
    assert r["total"] == 1 and r["rows"][0].tolist() == [0.0, 0.0, 133.0, 70.0, 1.0, 1.0]
    assert SR.regions(comb[:-1], min_area=1, connectivity=4, max_det=100)["total"] == 67          # without the last row: the teeth alone
    two = SR.regions(SR.two_combs(70, 133), min_area=1, connectivity=8)
    assert two["total"] == 2 and sorted(two["rows"][:2, 5].tolist()) == [1.0, 2.0] and two["seeds"][:2].tolist() in ([133, 0], [0, 133])


# ---- 2. the restatement against scipy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("hw,seed", [((37, 53), 1), ((64, 64), 2), ((65, 129), 3)])
def test_restatement_equals_scipy_label(hw, seed, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    m = SR.blobby(*hw, seed)
    assert sorted(np.unique(m).tolist()) == [0, 1, 2]
    r = SR.regions(m, "all", connectivity, 1, 8192)
    assert 5 <= r["total"] <= 500, r["total"]                                  # a degenerate map cannot pass silently
    structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    seeds, areas, found = [], [], 0
    for c in range(3):
        lab, n = ndimage.label(m == c, structure)
        found += n
        mine = np.where(m == c, r["roots"], -1)
        for k in range(1, n + 1):                                              # scipy numbers a class's regions in raster order of their seeds
            member = lab == k
            seed_k = int(np.flatnonzero(member)[0])
            assert np.array_equal(mine == seed_k, member), (c, k)              # the same set of pixels, keyed by the same seed
            seeds.append(seed_k)
            areas.append(int(member.sum()))
        per_class = np.unique(mine[mine >= 0])
        assert np.array_equal(per_class, np.sort(np.array(seeds[len(seeds) - n:])))
    assert found == r["total"] == r["count"]
    order = np.lexsort((np.array(seeds), -np.array(areas)))
    assert np.array_equal(r["seeds"][:found], np.array(seeds)[order]) and np.array_equal(r["areas"][:found], np.array(areas)[order])


# ---- 3. surface -----------------------------------------------------------------------------------------------------------------------------
def test_seg_regions_parameters_are_validated():
    from computervision.pytorch_amd.seg_regions import REGION_CAP, SegRegions
    d = SegRegions()
    assert (d.connectivity, d.min_area, d.classes, d.max_det, d.fill) == (8, 64, "foreground", 300, None) and REGION_CAP == 8192
    assert list(inspect.signature(SegRegions.__init__).parameters)[1:] == ["connectivity", "min_area", "classes", "max_det", "fill"]
    assert np.array_equal(d.mask, SR.class_mask("foreground")) and np.array_equal(SegRegions(classes="all").mask, SR.class_mask("all"))
    some = SegRegions(4, 1, [15, 3, 255, 32], 8192, 0)
    assert some.classes == (3, 15, 32, 255) and np.array_equal(some.mask, SR.class_mask([3, 15, 32, 255])) and some.fill == 0
    assert some.mask_words.dtype == np.dtype("<u4") and some.mask_words.tolist() == [(1 << 3) | (1 << 15), 1, 0, 0, 0, 0, 0, 1 << 31]
    assert d.mask_words.tolist() == [0xFFFFFFFE] + [0xFFFFFFFF] * 6 + [0x7FFFFFFF]
    for bad in (dict(connectivity=6), dict(connectivity=True), dict(min_area=0), dict(min_area=1.5), dict(max_det=0), dict(max_det=8193),
                dict(fill=-1), dict(fill=256), dict(fill=1.5), dict(classes="background"), dict(classes=[256]), dict(classes=[-1]), dict(classes=[]),
                dict(classes=[1.0]), dict(classes=7)):
        with pytest.raises(ValueError):
            SegRegions(**bad)


def test_label_regions_refuses_host_tensors_and_bad_arguments():
    from computervision.pytorch_amd import seg_regions
    params = inspect.signature(seg_regions.label_regions).parameters
    assert list(params)[:4] == ["labels", "regions", "conf", "region_maps"] and params["conf"].default is None and params["region_maps"].default is False
    with pytest.raises(CvxError, match="MI355X only"):
        seg_regions.label_regions([torch.zeros(4, 5, dtype=torch.uint8)])
    with pytest.raises(CvxError, match="MI355X only"):
        seg_regions.label_regions(torch.zeros(2, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        seg_regions.label_regions([torch.zeros(4, 5, dtype=torch.uint8)], regions="foreground")
    with pytest.raises(ValueError):
        seg_regions.label_regions(torch.zeros(4, 5, dtype=torch.uint8))                     # one 2-d tensor is neither a list nor a batch
    with pytest.raises(ValueError):
        seg_regions.label_regions([])
    assert {"rows", "counts", "total", "areas", "seeds", "region_maps", "clean_maps", "overflow"} <= \
        set(inspect.signature(seg_regions.RegionBatch.__init__).parameters) and callable(seg_regions.RegionBatch.read)


def test_table_layouts_match_the_header_structs():
    from computervision.pytorch_amd import seg_regions
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    for name, dtype in (("cvx_seg_plane", L.SEG_PLANE_DTYPE), ("cvx_seg_imap", L.SEG_IMAP_DTYPE), ("cvx_seg_map", seg_regions.SEG_MAP_DTYPE)):
        assert re.search(r"typedef struct %s \{[^}]*\bdata;\s*int32_t pitch, reserved;\s*\} %s;" % (name, name), header), name
        assert dtype.itemsize == 16 and dtype.names == ("data", "pitch", "reserved") and dtype.fields["pitch"][1] == 8, name

    class Plane(ctypes.Structure):                                                         # the C layout of a pointer and two int32
        _fields_ = [("data", ctypes.c_void_p), ("pitch", ctypes.c_int32), ("reserved", ctypes.c_int32)]
    assert ctypes.sizeof(Plane) == 16 and Plane.pitch.offset == 8 and Plane.reserved.offset == 12


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    assert os.path.exists(LIB_PATH), "build() leaves the cross-compiled library in the tree"
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("cvx_seg_regions", "cvx_seg_regions_workspace_bytes"):
        assert name in declared and name in L.PROTOTYPES and hasattr(lib, name), name
    assert len(L.PROTOTYPES["cvx_seg_regions"][1]) == 22 and L.PROTOTYPES["cvx_seg_regions_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int32] * 3)
    assert "\"seg_regions.hip\"" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "((0xFFFFFFFF - area) << 32) | seed" in header and "tests/seg_regions_restatement.py" in header
    lib.cvx_abi_version.restype = ctypes.c_int32
    assert lib.cvx_abi_version() == 6 and L.ABI_VERSION == 6
    # the workspace query is host arithmetic: 28 bytes per pixel and the candidates, 0 for what the entry refuses
    fn = lib.cvx_seg_regions_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int32] * 3
    px = 2 * 1024 * 2048
    assert 28 * px <= fn(2, 1024, 2048) <= 28 * px + 2 * 33 * 1024 + 8 * 256
    assert fn(0, 4, 4) == 0 and fn(1, 0, 4) == 0 and fn(1, 65536, 32768) == 0 and fn(1, 1, 1) > 0


def test_deeplab_surface():
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from scripts import detect
    p = inspect.signature(DeeplabV3PlusA.predict_regions).parameters
    assert list(p)[:3] == ["self", "model", "frames"]
    assert [p[k].default for k in ("regions", "conf", "draw", "tracker", "sync")] == [None, False, False, None, False]
    for fn in (DeeplabV3PlusA.segment_frames, detect.segment_frames, detect.segment_video):
        q = inspect.signature(fn).parameters
        assert q["regions"].default is None and q["track"].default is None
    frame = torch.zeros(20, 30, 3, dtype=torch.uint8)
    host = DeeplabV3PlusA(DeeplabV3PlusConfig(), "cpu")
    with pytest.raises(CvxError, match="MI355X only"):
        host.predict_regions(None, [frame])
    with pytest.raises(CvxError, match="MI355X only"):
        host.segment_frames(None, [frame], 2, regions=None, track={})
    algo = DeeplabV3PlusA(DeeplabV3PlusConfig(), "cuda:0")                                  # a device name alone touches no GPU
    with pytest.raises(CvxError, match="probabilities"):
        algo.predict_regions(None, [frame], conf=True)
    for bad in ({"draw": False}, {"sync": True}):                                           # segment_frames still rejects draw / sync
        with pytest.raises(ValueError, match="neither draw nor sync"):
            algo.segment_frames(None, [frame], 2, **bad)
        with pytest.raises(ValueError, match="neither draw nor sync"):
            algo.segment_frames(None, [frame], 2, regions=None, track=None, **bad)
    with pytest.raises(ValueError):
        algo.segment_frames(None, [frame], 0)
