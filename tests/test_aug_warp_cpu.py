"""CPU: the host restatement of stage 2 of the device augmentation (tests/aug_warp_restatement.py: warp, MixUp, box rule) against answers
derived by hand, and the host side in ``computervision.pytorch_amd.augment`` -- ``warp_matrix``, ``draw_warp``'s draws, ``view_table``, the
refusals and ``DeviceAugLoader(close_after=...)``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import aug_warp_restatement as WR
from computervision.pytorch_amd import LIB_PATH, augment
from computervision.pytorch_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
H, W = 12, 20


def canvas(h=H, w=W, seed=0):
    return (np.random.RandomState(seed).randint(0, 256, (3, h, w)).astype(F) / F(255)).astype(F)


# ---- the pixel rule ---------------------------------------------------------------------------------------------
def test_identity_returns_the_canvas_bit_for_bit():
    c = canvas()
    out = WR.warp_image(c, np.eye(3))
    assert out.dtype == F and np.array_equal(out, c)
    assert np.array_equal(WR.warp_mix(c[None], np.eye(3)[None])[0], c)


def test_integer_translation_is_an_exact_shift_with_grey_fill():
    c = canvas()
    tx, ty = 3, -2                                                     # M moves the canvas right by 3 and up by 2
    minv = np.array([[1, 0, -tx], [0, 1, -ty], [0, 0, 1]], np.float64)
    out = WR.warp_image(c, minv)
    ref = np.full_like(c, WR.GREY)
    ref[:, :H + ty, tx:] = c[:, -ty:, :W - tx]
    assert np.array_equal(out, ref) and WR.GREY == F(128) / F(255) and (out[:, :, :tx] == WR.GREY).all() and (out[:, H + ty:] == WR.GREY).all()


def test_quarter_turn_permutes_the_pixels_of_a_square_canvas():
    n = 9
    c = canvas(n, n, 1)
    minv = np.array([[0, 1, 0], [-1, 0, n - 1], [0, 0, 1]], np.float64)   # output (x, y) reads canvas (u, v) = (y, n - 1 - x)
    out = WR.warp_image(c, minv)
    yy, xx = np.mgrid[0:n, 0:n]
    assert np.array_equal(out, c[:, n - 1 - xx, yy])
    assert np.array_equal(np.sort(out.reshape(3, -1), 1), np.sort(c.reshape(3, -1), 1))


def test_half_pixel_shift_and_the_border_taps():
    c = np.zeros((3, 2, 4), F)
    c[:, :, 1] = 1.0
    out = WR.warp_image(c, np.array([[1, 0, -0.5], [0, 1, 0], [0, 0, 1]]))    # u = x - 0.5: the mean of two neighbours, exactly
    g = WR.GREY
    assert np.array_equal(out[0, 0], np.array([g * F(0.5) + F(0) * F(0.5), 0.5, 0.5, 0], F))
    far = WR.warp_image(c, np.array([[1, 0, 100], [0, 1, 0], [0, 0, 1]]))      # no tap on the canvas: the grey itself
    assert (far == g).all()


def test_mixup_of_two_constant_canvases():
    a, b = np.full((3, 4, 6), 0.25, F), np.full((3, 4, 6), 0.75, F)
    eye = np.tile(np.eye(3), (2, 1, 1))
    out = WR.warp_mix(np.stack([a, b]), eye, partner=[1, -1], r=np.array([0.5, 1], F), r1=np.array([0.5, 0], F))
    assert (out[0] == F(0.5)).all() and np.array_equal(out[1], b)             # 0.25 * 0.5 + 0.75 * 0.5, exact in binary
    both = WR.warp_mix(np.stack([a, b]), eye, partner=[1, 0], r=np.array([0.75, 0.25], F), r1=np.array([0.25, 0.75], F))
    assert (both[0] == F(0.375)).all() and (both[1] == F(0.375)).all()        # the mutual pair reads canvases, not each other's output
    shifted = np.stack([np.eye(3), np.array([[1, 0, -2], [0, 1, 0], [0, 0, 1]], np.float64)])
    out = WR.warp_mix(np.stack([a, b]), shifted, partner=[1, -1], r=np.array([0.5, 1], F), r1=np.array([0.5, 0], F))
    assert (out[0, :, :, 2:] == F(0.5)).all() and (out[0, :, :, :2] == F(0.25) * F(0.5) + WR.GREY * F(0.5)).all()   # the partner's own matrix


# ---- the box rule -----------------------------------------------------------------------------------------------
BH, BW = 128, 256          # powers of two: the normalised labels and their way back to pixels are exact


def label(x1, y1, x2, y2, cls=3):
    return np.array([[cls, (x1 + x2) / 2 / BW, (y1 + y2) / 2 / BH, (x2 - x1) / BW, (y2 - y1) / BH]], F)


def test_box_corners_min_max_and_clip():
    lab = label(40, 20, 80, 60)
    assert [float(v[0]) for v in WR.box_corners(lab, BH, BW)] == [40, 20, 80, 60]
    assert [float(v[0]) for v in WR.warp_corners(lab, np.eye(3), BH, BW)] == [40, 20, 80, 60]
    turn = np.array([[0, -1, 100], [1, 0, 0], [0, 0, 1]], np.float64)            # (x, y) -> (100 - y, x): corners change roles
    assert [float(v[0]) for v in WR.warp_corners(lab, turn, BH, BW)] == [40, 40, 80, 80]
    shear = np.array([[1, 0.5, 0], [0, 1, 0], [0, 0, 1]], np.float64)            # x + y / 2: min from (x1, y1), max from (x2, y2)
    assert [float(v[0]) for v in WR.warp_corners(lab, shear, BH, BW)] == [50, 20, 110, 60]
    move = np.array([[1, 0, 200], [0, 1, -30], [0, 0, 1]], np.float64)
    assert [float(v[0]) for v in WR.warp_corners(lab, move, BH, BW)] == [240, 0, 256, 30]    # clipped to [0, W] x [0, H]
    halve = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 2]], np.float64)              # w = 2: the divide is taken
    assert [float(v[0]) for v in WR.warp_corners(lab, halve, BH, BW)] == [20, 10, 40, 30]
    out = WR.warp_boxes(lab, move, 1.0, BH, BW)
    assert out.shape == (1, 5) and np.array_equal(out[0], np.array([3, 248 / 256, 15 / 128, 16 / 256, 30 / 128], F))


def test_each_candidate_test_just_inside_and_just_outside():
    up, down = np.nextafter(F(2), F(3)), np.nextafter(F(2), F(1))
    size, area, aspect = WR.candidates(w1=[10, 10, 10], h1=[10, 10, 10], w2=[up, F(2), 10], h2=[10, 10, down], s=1.0)
    assert size.tolist() == [True, False, False] and area.tolist() == [True, True, True] and aspect.tolist() == [True, True, True]
    # area: w2 h2 / (w1 s h1 s) against 0.1, with s = 2: 40 / 400 rounds to fp32(0.1) itself, which is not above it; 41 / 400 is
    size, area, aspect = WR.candidates(w1=[10, 10, 10], h1=[10, 10, 10], w2=[4, 4.1, 40], h2=[10, 10, 10], s=2.0)
    assert F(40) / F(400) == F(0.1) and area.tolist() == [False, True, True] and size.all()
    assert WR.candidates(10, 10, 4, 10, 1.0)[1]                                   # the same box without the zoom passes: s counts
    # aspect: max(w2 / h2, h2 / w2) against 100, both ways round
    size, area, aspect = WR.candidates(w1=[300] * 4, h1=[300] * 4, w2=[300, 299, 3, 3], h2=[3, 3, 300, 299], s=1.0)
    assert aspect.tolist() == [False, True, False, True] and size.all()
    assert WR.candidates(10, 10, 0, 0, 1.0) == (False, False, False)             # 0 / 0: every comparison is false
    kept = WR.warp_boxes(np.concatenate([label(10, 10, 12, 40), label(10, 10, 13, 40)]), np.eye(3), 1.0, BH, BW)
    assert len(kept) == 1 and kept[0, 3] == F(3) / F(BW)                         # through warp_boxes: w2 = 2 is dropped, 3 stays
    assert len(WR.warp_boxes(label(10, 10, 12, 40), np.eye(3), 1.0, BH, BW, min_wh=1.5)) == 1


def test_outputs_carry_their_own_boxes_then_their_partners():
    labs = [label(10, 10, 50, 50, 0), np.zeros((0, 5), F), np.concatenate([label(20, 20, 90, 90, 2), label(0, 0, 1, 1, 9)])]
    eye, s = np.tile(np.eye(3), (3, 1, 1)), np.ones(3)
    per = WR.boxes_per_output(labs, eye, s, [2, 0, -1], BH, BW)
    assert [k[:, 0].tolist() for k in per] == [[0, 2], [0], [2]]
    rows = WR.compact(per)
    assert rows[:, 0].tolist() == [0, 0, 1, 2] and rows[:, 1].tolist() == [0, 2, 0, 2]
    labels, counts, over = WR.padded(per, 1)
    assert counts.tolist() == [1, 1, 1] and over == 1 and labels[0, 0, 0] == 0
    labels, counts, over = WR.padded(per, 3)
    assert counts.tolist() == [2, 1, 1] and over == 0 and not labels[0, 2:].any()


# ---- the host side ------------------------------------------------------------------------------------------------
def test_warp_matrix_is_yolov5s_composition():
    eight = (0.0003, -0.0002, 12.0, 0.8, 4.0, -3.0, 0.45, 0.57)
    M = augment.warp_matrix(eight, (64, 96))
    assert M.dtype == np.float64 and np.array_equal(M, WR.matrix(eight, 64, 96))
    assert np.allclose(augment.warp_matrix((0, 0, 0, 1, 0, 0, 0.5, 0.5), (64, 96)), np.eye(3), atol=0, rtol=0)      # centred, nothing drawn
    M = augment.warp_matrix((0, 0, 90, 1, 0, 0, 0.5, 0.5), (64, 64))             # cv2.getRotationMatrix2D: positive angles turn anti-clockwise
    assert np.allclose(M @ [32 + 10, 32, 1], [32, 32 - 10, 1], atol=1e-12)
    M = augment.warp_matrix((0, 0, 0, 2, 0, 0, 0.5, 0.5), (64, 96))
    assert np.allclose(M @ [0, 0, 1], [-48, -32, 1]) and np.allclose(M @ [48, 32, 1], [48, 32, 1])


class Spy(np.random.RandomState):
    """records the draws made through it"""

    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def uniform(self, lo=0.0, hi=1.0, size=None):
        self.calls.append(("uniform", lo, hi))
        return super().uniform(lo, hi, size)

    def rand(self, *a):
        self.calls.append(("rand",))
        return super().rand(*a)

    def randint(self, *a, **k):
        self.calls.append(("randint",) + a)
        return super().randint(*a, **k)

    def beta(self, a, b, size=None):
        self.calls.append(("beta", a, b))
        return super().beta(a, b, size)


AFF = dict(degrees=10, translate=0.2, scale=0.4, shear=5, perspective=0.0005)


def test_draw_warp_count_and_order():
    rng = Spy(7)
    w = augment.draw_warp(rng, 3, (64, 96), AFF, 0.6)
    eight = [("uniform", -0.0005, 0.0005)] * 2 + [("uniform", -10.0, 10.0), ("uniform", 1 - 0.4, 1 + 0.4)] + [("uniform", -5.0, 5.0)] * 2 + \
        [("uniform", 0.5 - 0.2, 0.5 + 0.2)] * 2
    assert rng.calls == eight * 3 + [("rand",), ("randint", 2), ("beta", 32.0, 32.0)] * 3
    # the same numbers, drawn by hand
    ref = np.random.RandomState(7)
    for i in range(3):
        e = [ref.uniform(lo, hi) for _, lo, hi in eight]
        assert np.array_equal(w["M"][i], WR.matrix(e, 64, 96)) and w["s"][i] == e[3]
    assert np.allclose(w["Minv"] @ w["M"], np.eye(3), atol=1e-9)
    for i in range(3):
        take, j, ratio = ref.rand() < 0.6, ref.randint(2), F(ref.beta(32, 32))
        assert w["partner"][i] == ((j + (j >= i)) if take else -1) and w["r"][i] == (ratio if take else F(1))
    assert w["r"].dtype == F and w["r1"].dtype == F and np.array_equal(w["r1"], F(1) - w["r"])
    assert set(w["partner"].tolist()) != {-1} and all(p != i for i, p in enumerate(w["partner"]))
    assert ref.rand() == rng.rand()                                              # and nothing further was drawn
    # one option at a time; B = 1 has no MixUp
    rng = Spy(1)
    w = augment.draw_warp(rng, 2, (64, 96), None, 1.0)
    assert rng.calls == [("rand",), ("randint", 1), ("beta", 32.0, 32.0)] * 2 and w["partner"].tolist() == [1, 0] and np.array_equal(w["M"][0], np.eye(3))
    rng = Spy(1)
    w = augment.draw_warp(rng, 1, (64, 96), {}, 1.0)                             # {}: the default affine
    assert len(rng.calls) == 8 and w["partner"].tolist() == [-1] and rng.calls[3] == ("uniform", 0.5, 1.5) and rng.calls[6] == ("uniform", 0.4, 0.6)


def test_options_off_draw_nothing():
    for B, affine, mixup in ((4, None, 0.0), (1, None, 1.0)):
        rng = np.random.RandomState(5)
        before = rng.get_state()
        assert augment.draw_warp(rng, B, (64, 96), affine, mixup) is None
        after = rng.get_state()
        assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    aug = augment.DeviceAugmenter((64, 96), seed=0)
    assert aug.affine is None and aug.mixup == 0.0 and aug.last_warp is None


def test_view_table_rounds_once_and_refuses_bad_partners():
    w = augment.draw_warp(np.random.RandomState(3), 4, (64, 96), AFF, 1.0)
    v = augment.view_table(w, 4)
    assert v.dtype.itemsize == 96 and v.shape == (4,)
    assert np.array_equal(v["m"], w["M"].reshape(4, 9).astype(F)) and np.array_equal(v["inv"], np.linalg.inv(w["M"]).reshape(4, 9).astype(F))
    assert np.array_equal(v["s"], w["s"].astype(F)) and np.array_equal(v["partner"], w["partner"]) and np.array_equal(v["r1"], F(1) - v["r"])
    v = augment.view_table({"M": np.tile(np.eye(3), (2, 1, 1))}, 2)
    assert v["partner"].tolist() == [-1, -1] and v["s"].tolist() == [1, 1] and v["r"].tolist() == [1, 1] and v["r1"].tolist() == [0, 0]
    eye = np.tile(np.eye(3), (2, 1, 1))
    for bad in ({"M": eye, "partner": [0, -1]}, {"M": eye, "partner": [2, -1]}, {"M": eye, "partner": [-2, -1]}, {"M": eye[:1]},
                {"M": eye * np.nan}, {"M": eye, "s": [1, 0]}):
        with pytest.raises(ValueError):
            augment.view_table(bad, 2)


def test_refusals():
    with pytest.raises(ValueError, match="perspective"):
        augment.DeviceAugmenter((640, 640), affine=dict(perspective=0.001))      # 0.001 * 640 = 0.64
    augment.DeviceAugmenter((640, 640), affine=dict(perspective=0.0007))         # 0.448
    with pytest.raises(ValueError, match="perspective"):
        augment.DeviceAugmenter((64, 96), affine=dict(perspective=0.5 / 96))     # the longer side counts, and 0.5 itself is refused
    with pytest.raises(ValueError, match="perspective"):
        augment.draw_warp(np.random.RandomState(0), 2, (64, 96), dict(perspective=0.01), 0.0)
    for bad in (dict(rotate=3), dict(scale=1.0), dict(degrees=-1), dict(shear=90), dict(max_aspect=1), dict(translate=float("nan"))):
        with pytest.raises(ValueError):
            augment.DeviceAugmenter((64, 96), affine=bad)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            augment.DeviceAugmenter((64, 96), mixup=bad)
    with pytest.raises(ValueError, match="training"):
        augment.DeviceAugmenter((64, 96), train=False, affine={})
    with pytest.raises(ValueError, match="training"):
        augment.DeviceAugmenter((64, 96), train=False, mixup=0.5)
    with pytest.raises(ValueError):
        augment.DeviceAugLoader([], 2, augment.DeviceAugmenter((64, 96), train=False), close_after=1)
    with pytest.raises(ValueError):
        augment.DeviceAugLoader([1], 2, augment.DeviceAugmenter((64, 96)), length=1, close_after=-1)


# ---- close mosaic ------------------------------------------------------------------------------------------------
class Recorder(augment.DeviceAugmenter):
    """the real draws, no launches: ``apply`` notes what it was handed"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.batches, self.mosaic_draws = [], 0

    def want_mosaic(self):
        self.mosaic_draws += 1
        return super().want_mosaic()

    def apply(self, params, sources, boxes, fmt="yolo8", exact=True, max_boxes=None, warp=None):
        self.batches.append((len(params), [len(g) for g in sources], warp))
        return None, None


def test_close_after_switches_mosaic_and_mixup_off_at_the_right_epoch():
    source = [(torch.zeros(20 + i, 30, 3, dtype=torch.uint8), np.zeros((0, 5), F)) for i in range(5)]
    aug = Recorder((64, 96), mosaic=True, mosaic_prob=1.0, seed=2, affine={}, mixup=1.0)
    loader = augment.DeviceAugLoader(source, 2, aug, length=3, fmt="yolo7", device="cpu", close_after=2)
    assert loader.epoch == 0 and loader.close_after == 2
    for epoch in range(4):
        aug.batches, aug.mosaic_draws = [], 0
        assert len(list(loader)) == 3 and loader.epoch == epoch + 1
        open_ = epoch < 2
        assert aug.mosaic_draws == (6 if open_ else 0)                           # closed: the draw is not made at all
        for n, group_sizes, warp in aug.batches:
            assert n == 2 and group_sizes == ([4, 4] if open_ else [1, 1])
            assert warp is not None and warp["M"].shape == (2, 3, 3)             # affine stays on
            assert (sorted(warp["partner"].tolist()) == [0, 1]) if open_ else (warp["partner"].tolist() == [-1, -1])
    loader.epoch = 1                                                             # a resumed run
    aug.batches = []
    list(loader)
    assert loader.epoch == 2 and aug.batches[0][1] == [4, 4]
    # without close_after the loader never closes, and a closed epoch's draws are those of an augmenter without mosaic and MixUp
    free = augment.DeviceAugLoader(source, 2, Recorder((64, 96), mosaic=True, mosaic_prob=1.0, seed=2, mixup=1.0), length=1, fmt="yolo7", device="cpu")
    for _ in range(3):
        list(free)
    assert free.epoch == 3 and free.augmenter.batches[-1][1] == [4, 4]
    a = Recorder((64, 96), mosaic=True, mosaic_prob=1.0, seed=9, affine={}, mixup=1.0)
    b = Recorder((64, 96), seed=9, affine={})
    list(augment.DeviceAugLoader(source, 2, a, length=2, fmt="yolo7", device="cpu", close_after=0))
    list(augment.DeviceAugLoader(source, 2, b, length=2, fmt="yolo7", device="cpu"))
    assert all(np.array_equal(x[2]["M"], y[2]["M"]) for x, y in zip(a.batches, b.batches)) and a.rng.rand() == b.rng.rand()


# ---- the library ---------------------------------------------------------------------------------------------------
def test_stage_2_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("cvx_aug_warp_mix", "cvx_aug_boxes_warp"):
        assert name in declared and name in L.PROTOTYPES and hasattr(lib, name), name
    assert len(L.PROTOTYPES["cvx_aug_warp_mix"][1]) == 7 and len(L.PROTOTYPES["cvx_aug_boxes_warp"][1]) == 16
    assert "cvx_aug_view" in header and augment.VIEW_DTYPE.itemsize == 96
