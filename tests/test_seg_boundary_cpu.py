"""No GPU: the numpy restatement of the boundary metrics (tests/seg_boundary_restatement.py) against hand-derived answers and against scipy
(``binary_erosion`` for the Boundary IoU bands, the chessboard distance transform for the nearest-contour planes), the mutants that show
each rule matters, and the surface of ``seg_boundary`` -- the ratio rule, parameter validation, the refusal of host tensors, the table
layouts, the symbols in header, library and binding."""
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
import seg_boundary_restatement as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rules(**flipped):
    return dict(BR.RULES, **flipped)


# ---- 1. the restatement against answers worked out by hand -----------------------------------------------------------------------------------
SQUARE = np.zeros((5, 5), np.uint8)
SQUARE[1:4, 1:4] = 1


def test_a_square_in_a_five_by_five_map():
    """every pixel of the ring touches the square and every pixel of the square but its centre touches the ring"""
    c = BR.counts(SQUARE, SQUARE, 2, [1, 2])
    d = np.ones((5, 5), np.uint8)
    d[2, 2] = 2
    n = np.ones((5, 5), np.uint8)                                   # the contour is everything but the centre, and it meets itself at 0
    n[2, 2] = 0
    for i in range(4):
        assert np.array_equal(c["planes"][i], d), i
    assert np.array_equal(c["planes"][4], n) and np.array_equal(c["planes"][5], n)
    assert c["trimap"].tolist() == [[[16, 0], [0, 8]], [[16, 0], [0, 9]]]
    assert c["biou"].tolist() == [[[16, 16, 16], [8, 8, 8]], [[16, 16, 16], [9, 9, 9]]]
    assert c["bf"].tolist() == [[[16, 16, 16, 16], [8, 8, 8, 8]]] * 2
    assert BR.fold(c["trimap"][0], c["biou"][0], c["bf"][0])[0] == (1.0, 1.0, 1.0)


def test_two_classes_side_by_side():
    g = np.repeat(np.array([[0, 0, 0, 1, 1, 1]], np.uint8), 4, 0)
    c = BR.counts(g, g, 2, [1, 3])
    assert c["planes"][1].tolist() == [[3, 2, 1, 1, 2, 3]] * 4                               # noedge: the distance to the other class alone
    assert c["planes"][0].tolist() == [[1] * 6, [1, 2, 1, 1, 2, 1], [1, 2, 1, 1, 2, 1], [1] * 6]     # edge: the picture border as well
    assert c["trimap"].tolist() == [[[4, 0], [0, 4]], [[12, 0], [0, 12]]]
    assert c["biou"].tolist() == [[[10, 10, 10], [10, 10, 10]], [[12, 12, 12], [12, 12, 12]]]
    assert c["bf"].tolist() == [[[4, 4, 4, 4], [4, 4, 4, 4]]] * 2
    assert c["planes"][4].tolist() == [[0, 0, 1, 1, 0, 0]] * 4


VOID_G = np.repeat(np.array([[0, 0, 255, 1, 1]], np.uint8), 3, 0)
VOID_P = np.repeat(np.array([[0, 0, 0, 1, 1]], np.uint8), 3, 0)


def test_a_void_outline_between_two_classes():
    """the void column is no class, voids the prediction under it, and still ends both classes' runs: the trimap band lies along it"""
    c = BR.counts(VOID_P, VOID_G, 2, [1])
    assert c["planes"][1].tolist() == [[2, 1, 0, 1, 2]] * 3 and c["planes"][3].tolist() == [[2, 1, 0, 1, 2]] * 3
    assert c["trimap"].tolist() == [[[3, 0], [0, 3]]]
    assert c["biou"].tolist() == [[[6, 6, 6], [6, 6, 6]]]                                      # three rows: every pixel is at the border or the void
    assert c["bf"].tolist() == [[[3, 3, 3, 3], [3, 3, 3, 3]]]


def test_one_class_only():
    """no label change: trimap and contours are empty, Boundary IoU comes from the picture border alone"""
    g = np.zeros((4, 4), np.uint8)
    c = BR.counts(g, g, 2, [1, 2])
    assert not c["trimap"].any() and not c["bf"].any() and not c["planes"][4:].any()
    assert c["biou"].tolist() == [[[12, 12, 12], [0, 0, 0]], [[16, 16, 16], [0, 0, 0]]]
    assert c["planes"][1].tolist() == [[3] * 4] * 4 and c["planes"][0].tolist() == [[1] * 4, [1, 2, 2, 1], [1, 2, 2, 1], [1] * 4]
    (tri, biou, bf), _ = BR.fold(c["trimap"][0], c["biou"][0], c["bf"][0])
    assert np.isnan(tri) and biou == 1.0 and np.isnan(bf)


SHIFT_G = np.repeat(np.array([[0, 0, 0, 0, 1, 1, 1, 1]], np.uint8), 6, 0)
SHIFT_P = np.repeat(np.array([[0, 0, 0, 0, 0, 1, 1, 1]], np.uint8), 6, 0)


def test_a_prediction_shifted_by_one_pixel():
    """every contour pixel finds its class's contour one pixel away, so BF at d = 1 is 1; the bands overlap in part only"""
    c = BR.counts(SHIFT_P, SHIFT_G, 2, [1])
    assert c["bf"].tolist() == [[[6, 6, 6, 6], [6, 6, 6, 6]]]
    assert c["planes"][4].tolist() == [[0, 0, 0, 0, 2, 2, 0, 0]] * 6 and c["planes"][5].tolist() == [[0, 0, 0, 2, 2, 0, 0, 0]] * 6
    assert c["biou"].tolist() == [[[12, 16, 18], [10, 16, 14]]]                                # worked out in DESIGN.md section 7z
    assert c["trimap"].tolist() == [[[6, 0], [6, 0]]]                                          # columns 3 and 4 of the target, both predicted 0
    (tri, biou, bf), _ = BR.fold(c["trimap"][0], c["biou"][0], c["bf"][0])
    assert bf == 1.0 and biou == (12 / 22 + 10 / 20) / 2 < 1 and tri == (6 / 12 + 0 / 6) / 2


# ---- 2. mutants: each rule flipped changes a named output ------------------------------------------------------------------------------------
def test_mutants_change_the_expected_outputs():
    one = np.zeros((4, 4), np.uint8)
    base = BR.counts(one, one, 2, [1, 2])
    assert BR.counts(one, one, 2, [1, 2], rules(trimap_edge=True))["trimap"][:, 0, 0].tolist() == [12, 16] and not base["trimap"].any()
    assert not BR.counts(one, one, 2, [1, 2], rules(biou_edge=False))["biou"].any() and base["biou"][0, 0].tolist() == [12, 12, 12]
    strict = BR.counts(SHIFT_P, SHIFT_G, 2, [1], rules(strict=True))                            # < for <=: nothing lies below distance 1
    assert strict["bf"].tolist() == [[[0, 6, 0, 6], [0, 6, 0, 6]]] and not strict["trimap"].any()
    assert BR.fold(strict["trimap"][0], strict["biou"][0], strict["bf"][0])[0][2] == 0.0
    as0 = BR.counts(VOID_P, VOID_G, 2, [1], rules(void_is_class0=True))                        # the void column counts as class 0
    assert as0["trimap"].tolist() == [[[3, 0], [0, 3]]] and as0["biou"][0, 0].tolist() == [8, 8, 8] and as0["bf"][0, 0].tolist() == [3, 3, 3, 3]
    assert as0["planes"][1].tolist() == [[2, 2, 1, 1, 2]] * 3
    four = BR.counts(SQUARE, SQUARE, 2, [1], rules(contour4=True))                             # the ring's corners touch the square diagonally
    assert four["bf"].tolist() == [[[12, 12, 12, 12], [8, 8, 8, 8]]]
    kept = BR.counts(VOID_P, VOID_G, 2, [1], rules(void_pred=False))                           # the prediction under the void column stays
    assert kept["biou"].tolist() == [[[5, 6, 8], [6, 6, 6]]] and kept["planes"][3].tolist() == [[2, 2, 1, 1, 2]] * 3
    city = BR.counts(SQUARE, SQUARE, 2, [1], rules(cityblock=True))                            # a corner is two steps from the square
    assert city["trimap"].tolist() == [[[12, 0], [0, 8]]] and city["planes"][1][0].tolist() == [2, 1, 1, 1, 2]


# ---- 3. against scipy --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 3, 21])
def test_restatement_equals_scipy_erosion_and_distance_transform(nc):
    from scipy import ndimage
    widths = [1, 3, 7]
    dmax = max(widths)
    classes = max(nc, 2)                                                                       # nc = 1: class 1 of the map is void
    for seed, (h, w) in enumerate([(37, 53), (24, 70)]):
        g = BR.blobby(h, w, 300 + seed + nc, classes=classes, cell=7)
        p = BR.jitter(g, 400 + seed + nc, classes, wild=True)
        c = BR.counts(p, g, nc, widths)
        gv, pv = BR.voided(p, g, nc)
        assert (gv == BR.VOID).any() and (pv[gv != BR.VOID] == BR.VOID).any()
        for k, d in enumerate(widths):
            for cls in range(nc):
                bands = []
                for m in (gv == cls, pv == cls):
                    inner = ndimage.binary_erosion(m, structure=np.ones((3, 3)), iterations=d, border_value=0) if m.any() else m
                    bands.append(m & ~inner)
                assert c["biou"][k, cls].tolist() == [int((bands[0] & bands[1]).sum()), int(bands[0].sum()), int(bands[1].sum())], (k, cls)
        kg, kp = BR.contour(gv), BR.contour(pv)
        for plane, (ka, kb) in ((4, (kp, kg)), (5, (kg, kp))):
            want = np.zeros((h, w), np.int64)
            for cls in range(nc):
                on = ka == cls
                if not on.any():
                    continue
                far = ndimage.distance_transform_cdt(kb != cls, metric="chessboard") if (kb == cls).any() else np.full((h, w), dmax + 1)
                want[on] = np.minimum(far[on], dmax + 1) + 1
            assert np.array_equal(c["planes"][plane], want), plane
        # the trimap band of width d is the dilation of the label changes: every pixel within d of a pixel of another (or void) label
        for k, d in enumerate(widths):
            change = np.zeros((h, w), bool)
            for cls in list(range(nc)) + [BR.VOID]:
                m = gv == cls
                change |= ndimage.binary_dilation(m, structure=np.ones((3, 3)), iterations=d) & ~m & (gv != BR.VOID)
            band = change & (pv != BR.VOID)
            want = np.zeros((nc, nc), np.int64)
            np.add.at(want, (gv[band], pv[band]), 1)
            assert np.array_equal(c["trimap"][k], want), k


def test_a_prediction_equal_to_the_target_folds_to_one():
    g = BR.blobby(40, 60, 9, classes=4)
    c = BR.counts(g, g, 4, [1, 5])
    for k in range(2):
        (tri, biou, bf), _ = BR.fold(c["trimap"][k], c["biou"][k], c["bf"][k])
        assert (tri, biou, bf) == (1.0, 1.0, 1.0)


# ---- 4. the surface ------------------------------------------------------------------------------------------------------------------------------
def test_ratio_rule_and_clamps():
    from computervision.pytorch_amd import seg_boundary as SB
    spec = SB.SegBoundary(ratio=(0.02, 0.005))
    assert spec.frame_widths(513, 513) == [15, 4] and spec.frame_widths(1024, 2048) == [46, 11] and spec.frame_widths(375, 500) == [13, 3]
    assert spec.frame_widths(8, 8) == [1, 1]                                                   # 0.23 rounds to 0: clamped up
    assert SB.SegBoundary(ratio=(0.5,)).frame_widths(1024, 2048) == [64]                       # 1145: clamped down
    assert SB.SegBoundary(ratio=(0.1,)).frame_widths(3, 4) == [1] and SB.SegBoundary(ratio=(0.3,)).frame_widths(3, 4) == [2]   # 0.5 -> 1, 1.5 -> 2
    for hw in ((513, 513), (97, 129), (3, 4)):
        assert spec.frame_widths(*hw) == [BR.ratio_width(r, *hw) for r in (0.02, 0.005)]
    assert spec.keys == (0.02, 0.005) and spec.K == 2 and spec.widths is None
    plain = SB.SegBoundary()
    assert plain.widths == plain.keys == (1, 2, 4, 8) and plain.ratio is None and plain.frame_widths(10, 2000) == [1, 2, 4, 8]
    assert SB.SegBoundary(widths=None, ratio=(0.01,)).K == 1


def test_parameters_are_validated_and_host_tensors_refused():
    from computervision.pytorch_amd import seg_boundary as SB
    for bad in (dict(widths=()), dict(widths=(0,)), dict(widths=(65,)), dict(widths=(1.5,)), dict(widths=(True,)), dict(widths=(1, 1)),
                dict(widths=tuple(range(1, 10))), dict(widths=3), dict(widths=None), dict(widths=(1, 2), ratio=(0.02,)), dict(ratio=()),
                dict(ratio=(0.0,)), dict(ratio=(1.5,)), dict(ratio=(float("nan"),)), dict(ratio=(-0.1,)), dict(ratio=0.02),
                dict(ratio=("0.02",)), dict(ratio=(0.02, 0.02))):
        with pytest.raises(ValueError):
            SB.SegBoundary(**bad)
    host = torch.zeros(4, 5, dtype=torch.uint8)
    with pytest.raises(CvxError, match="MI355X only"):
        SB.boundary_counts([host], [host], 3)
    with pytest.raises(CvxError, match="MI355X only"):
        SB.boundary_counts(torch.zeros(2, 4, 5, dtype=torch.uint8), torch.zeros(2, 4, 5, dtype=torch.uint8), 3, SB.SegBoundary((2,)))
    with pytest.raises(CvxError, match="MI355X only"):
        SB.BoundaryMetrics(3, SB.SegBoundary(), "cpu")
    with pytest.raises(CvxError, match="MI355X only"):
        SB.BoundaryMetrics(3, SB.SegBoundary(), "cuda:0").add_labels([host], [host.long()])    # a device name alone touches no GPU
    for nc in (0, 256, 2.5, True):
        with pytest.raises(ValueError):
            SB.boundary_counts([host], [host], nc)
        with pytest.raises(ValueError):
            SB.BoundaryMetrics(nc, None, "cuda:0")
    with pytest.raises(ValueError):
        SB.boundary_counts([host], [host], 3, spec=(1, 2))
    with pytest.raises(ValueError):
        SB.boundary_counts(host, host, 3)                                                      # one 2-d tensor is neither a list nor a batch
    with pytest.raises(ValueError):
        SB.boundary_counts([], [], 3)
    with pytest.raises(ValueError):
        SB.BoundaryMetrics(3, (1, 2), "cuda:0")
    assert list(inspect.signature(SB.boundary_counts).parameters) == ["pred", "target", "num_classes", "spec", "out", "planes"]
    assert list(inspect.signature(SB.SegBoundary.__init__).parameters) == ["self", "widths", "ratio"]
    assert inspect.signature(SB.SegBoundary.__init__).parameters["widths"].default == (1, 2, 4, 8)
    assert all(callable(getattr(SB.BoundaryMetrics, n)) for n in ("add_labels", "reset", "get_results"))


def test_fold_counts_equals_the_restatements_fold():
    from computervision.pytorch_amd import seg_boundary as SB
    g = BR.blobby(40, 60, 5, classes=4)
    p = BR.jitter(g, 6, 4, wild=True)
    c = BR.counts(p, g, 5, [1, 3])                                                             # class 4 never occurs: NaN, left out of the means
    r = SB.fold_counts(c["trimap"], c["biou"], c["bf"], (1, 3))
    assert set(r) == {"Trimap mIoU", "Boundary IoU", "BF", "Class Trimap IoU", "Class Boundary IoU", "Class BF"}
    for k, key in enumerate((1, 3)):
        (tri, biou, bf), per_class = BR.fold(c["trimap"][k], c["biou"][k], c["bf"][k])
        assert 0 < biou < 1 and 0 < bf < 1 and 0 < tri < 1
        for name, want in (("Trimap mIoU", tri), ("Boundary IoU", biou), ("BF", bf)):
            assert abs(r[name][key] - want) <= 1e-15, (name, key)                              # two summation orders of at most five doubles
        for name, want in zip(("Class Trimap IoU", "Class Boundary IoU", "Class BF"), per_class):
            assert np.array_equal(np.array(r[name][key]), want, equal_nan=True) and np.isnan(r[name][key][4]), (name, key)
    hist = torch.from_numpy(c["trimap"][0]).double()                                           # the trimap folds as SegmentationMetrics folds its own
    from core.trainer.segmentation_trainer import SegmentationMetrics
    m = SegmentationMetrics(5)
    m.confusion_matrix += hist
    assert m.get_results()["Mean IoU"] == r["Trimap mIoU"][1]
    empty = SB.BoundaryMetrics(3, SB.SegBoundary((2,)), "cuda:0").get_results()                # nothing added: no class anywhere
    assert all(np.isnan(empty[name][2]) for name in ("Trimap mIoU", "Boundary IoU", "BF"))
    lines = SB.report_lines(r, (1, 3))
    assert [l.split(":")[0] for l in lines] == ["Trimap mIoU@1", "Boundary IoU@1", "BF@1", "Trimap mIoU@3", "Boundary IoU@3", "BF@3"]
    assert lines[1] == f"Boundary IoU@1: {r['Boundary IoU'][1]}"


def test_table_layout_matches_the_header():
    from computervision.pytorch_amd import seg_boundary as SB
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    assert "#define CVX_SEG_BOUNDARY_MAX_WIDTH 64" in header and SB.MAX_WIDTH == BR.MAX_WIDTH == 64
    assert "#define CVX_SEG_BOUNDARY_MAX_WIDTHS 8" in header and SB.MAX_WIDTHS == BR.MAX_WIDTHS == 8
    for text in ("(K, nc, nc) int64: trimap[k][G'[p]][P'[p]] += 1", "(K, nc, 3) int64 (I, Gb, Pb)", "(K, nc, 4) int64 (mp, cp, mg, cg)",
                 "(frames, 6, max_h, max_w) uint8", "widths (frames, K) int32 on the device", "tests/seg_boundary_restatement.py"):
        assert text in header, text
    flat, trimap, biou, bf = SB.new_tables(3, 2, "cpu")
    assert flat.dtype == torch.int64 and flat.numel() == 2 * 3 * (3 + 3 + 4) and not flat.any()
    assert (tuple(trimap.shape), tuple(biou.shape), tuple(bf.shape)) == ((2, 3, 3), (2, 3, 3), (2, 3, 4))
    assert trimap.data_ptr() == flat.data_ptr() and biou.data_ptr() == flat.data_ptr() + 8 * 18 and bf.data_ptr() == flat.data_ptr() + 8 * 36
    c = BR.counts(SQUARE, SQUARE, 3, [1, 2])                                                   # the restatement's tables have the same shapes
    assert (c["trimap"].shape, c["biou"].shape, c["bf"].shape, c["planes"].shape) == ((2, 3, 3), (2, 3, 3), (2, 3, 4), (6, 5, 5))
    assert SB.SEG_MAP_DTYPE.itemsize == 16 and SB.VOID == BR.VOID == 255


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    assert os.path.exists(LIB_PATH), "build() leaves the cross-compiled library in the tree"
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("cvx_seg_boundary", "cvx_seg_boundary_workspace_bytes"):
        assert name in declared and name in L.PROTOTYPES and hasattr(lib, name), name
    assert len(L.PROTOTYPES["cvx_seg_boundary"][1]) == 16 and L.PROTOTYPES["cvx_seg_boundary_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int32] * 3)
    assert "\"seg_boundary.hip\"" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    # the workspace query is host arithmetic: 6 bytes per pixel, 0 for what the entry refuses
    fn = lib.cvx_seg_boundary_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int32] * 3
    px = 2 * 1024 * 2048
    assert 6 * px <= fn(2, 1024, 2048) <= 6 * px + 8 * 256
    assert fn(0, 4, 4) == 0 and fn(1, 0, 4) == 0 and fn(1, 65536, 32768) == 0 and fn(1, 1, 1) > 0


def test_the_entry_refuses_bad_arguments_without_a_launch():
    """every refusal comes before the first HIP call, so it can be shown without a GPU; the pointers are never dereferenced"""
    lib = L.load()
    one = ctypes.c_void_p(256)
    need = lib.cvx_seg_boundary_workspace_bytes(1, 8, 8)

    def call(frames=1, max_h=8, max_w=8, nc=3, K=2, ws_bytes=need, widths=one):
        return lib.cvx_seg_boundary(one, one, one, frames, max_h, max_w, nc, widths, K, one, one, one, None, one, ws_bytes, None)

    for bad, text in ((dict(nc=256), "nc lies in"), (dict(nc=0), "nc lies in"), (dict(K=9), "K lies in"), (dict(K=0), "K lies in"),
                      (dict(max_h=65536, max_w=32768, ws_bytes=2 ** 40), "2^31"), (dict(ws_bytes=need - 1), "workspace too small"),
                      (dict(frames=0), "bad sizes"), (dict(widths=None), "null arguments")):
        assert call(**bad) != 0, bad
        assert text in lib.cvx_last_error().decode(), (bad, lib.cvx_last_error())


def test_deeplab_surface():
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from core.trainer import segmentation_trainer as ST
    from computervision.pytorch_amd import seg_boundary as SB
    assert inspect.signature(DeeplabV3PlusA.segment_tiled).parameters["boundary"].default is None
    assert inspect.signature(DeeplabV3PlusA.evaluate_on_voc).parameters["boundary"].default is None
    assert list(inspect.signature(ST.fused_evaluation_boundary).parameters) == ["model", "metrics", "dataloader", "device", "tta", "boundary"]
    frame = torch.zeros(20, 30, 3, dtype=torch.uint8)
    host = DeeplabV3PlusA(DeeplabV3PlusConfig(), "cpu")
    with pytest.raises(CvxError, match="MI355X only"):
        host.evaluate_on_voc(None, "unused", dataloader=[], boundary=SB.SegBoundary((1, 4)))
    algo = DeeplabV3PlusA(DeeplabV3PlusConfig(), "cuda:0")                                  # a device name alone touches no GPU
    with pytest.raises(ValueError, match="SegBoundary"):
        algo.evaluate_on_voc(None, "unused", dataloader=[], boundary=(1, 4))
    bm = SB.BoundaryMetrics(21, SB.SegBoundary((1, 4)), "cuda:0")
    with pytest.raises(ValueError, match="needs targets"):
        algo.segment_tiled(None, [frame], boundary=bm)
    with pytest.raises(ValueError, match="BoundaryMetrics"):
        algo.segment_tiled(None, [frame], targets=[frame[..., 0]], boundary=SB.SegBoundary())
    with pytest.raises(ValueError, match="come together"):                                  # without the keyword the old rule stands
        algo.segment_tiled(None, [frame], targets=[frame[..., 0]])
