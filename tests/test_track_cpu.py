"""CPU: the tracking rules as tests/track_restatement.py states them, against hand-derived answers and a seeded
property test; the new symbols; the surface that needs no GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import track_restatement as TS
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import render as R
from computervision.pytorch_amd import track as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = [10, 10, 50, 50]


def frame(*dets, K=4):
    """rows (K, 6) and the count from (box, score, cls) triples"""
    rows = np.zeros((K, 6), np.float32)
    for i, (box, score, cls) in enumerate(dets):
        rows[i] = list(box) + [score, cls]
    return rows, len(dets)


def feed(state, frames, **kw):
    prm = TS.params(**kw)
    return [TS.step(state, rows, n, prm)[0][:max(n, 0)].tolist() for rows, n in frames]


def test_two_frames_one_object_by_hand():
    st = TS.new_state()
    # frame 2: the prediction is the old box (v = 0); inter 36 * 40 = 1440, union 1600 + 1600 - 1440: IoU 0.818 > 0.2
    assert feed(st, [frame((A, 0.9, 1)), frame(([14, 10, 54, 50], 0.9, 1))]) == [[0], [0]]
    (k,) = st["tracks"]
    # r = [4, 0, 4, 0]: p = p + 0.75 r, v = 0 + 0.25 r
    assert k["p"].tolist() == [13, 10, 53, 50] and k["v"].tolist() == [1, 0, 1, 0] and k["p"].dtype == k["v"].dtype == np.float32
    assert (k["id"], k["hits"], k["miss"], k["cls"]) == (0, 2, 0, 1) and st["next_id"] == 1 and st["frame"] == 2
    # frame 3: predicted [14, 10, 54, 50], seen at [18, 10, 58, 50]: r = 4 -> p = 17, v = 2
    assert feed(st, [frame(([18, 10, 58, 50], 0.9, 1))]) == [[0]]
    assert st["tracks"][0]["p"].tolist() == [17, 10, 57, 50] and st["tracks"][0]["v"].tolist() == [2, 0, 2, 0]


def test_iou_value_by_hand():
    assert TS.iou_value(A, [14, 10, 54, 50]) == np.float32(1440) / np.float32(1760)
    assert TS.iou_value(A, [50, 10, 90, 50]) == 0 and TS.iou_value(A, A) == 1
    assert np.isnan(TS.iou_value([10, 10, 10, 20], [10, 10, 10, 20]))         # 0 / 0: passes no threshold
    assert TS.iou_matrix([A, A], [A, [14, 10, 54, 50], [0, 0, 1, 1]]).shape == (2, 3)


def test_start_up_rule_a_late_track_is_unlabelled_until_its_third_hit():
    st = TS.new_state()
    empty = frame()
    assert feed(st, [empty] * 4 + [frame((A, 0.9, 0))] * 3) == [[], [], [], [], [-1], [-1], [0]]
    assert st["tracks"][0]["hits"] == 3
    early = TS.new_state()                                   # born in frame 2 <= min_hits: labelled from birth, and in frame 3 by hits or frame
    assert feed(early, [empty] + [frame((A, 0.9, 0))] * 3) == [[], [0], [0], [0]]
    late = TS.new_state()                                    # born in frame 3, second hit in frame 4 > min_hits: unlabelled once
    assert feed(late, [empty] * 2 + [frame((A, 0.9, 0))] * 3) == [[], [], [0], [-1], [0]]


def test_a_tentative_track_that_misses_once_is_gone_and_its_id_is_not_reused():
    st = TS.new_state()
    empty = frame()
    assert feed(st, [empty] * 4 + [frame((A, 0.9, 0)), empty]) == [[]] * 4 + [[-1], []]
    assert st["tracks"] == [] and st["next_id"] == 1
    assert feed(st, [frame((A, 0.9, 0))] * 3) == [[-1], [-1], [1]]
    assert st["next_id"] == 2


@pytest.mark.parametrize("gap,back", [(30, True), (31, False)])
def test_a_confirmed_track_survives_max_age_misses(gap, back):
    st = TS.new_state()
    ids = feed(st, [frame((A, 0.9, 0))] * 3 + [frame()] * gap + [frame((A, 0.9, 0))])
    assert ids[:3] == [[0]] * 3
    if back:
        assert ids[-1] == [0] and st["next_id"] == 1 and st["tracks"][0]["miss"] == 0 and st["tracks"][0]["hits"] == 4
    else:
        assert ids[-1] == [-1] and st["next_id"] == 2 and [k["id"] for k in st["tracks"]] == [1]      # a new track, past the start-up frames


def test_score_stages():
    seen, low, empty = frame((A, 0.9, 0)), frame((A, 0.35, 0)), frame()
    st = TS.new_state()                                      # a low detection keeps a track that was seen in the previous frame
    assert feed(st, [seen] * 3 + [low, low]) == [[0]] * 5 and st["tracks"][0]["hits"] == 5
    st = TS.new_state()                                      # ... does not rescue one that was already missing, and gives no birth
    assert feed(st, [seen] * 3 + [empty, low]) == [[0]] * 3 + [[], [-1]]
    assert st["next_id"] == 1 and st["tracks"][0]["miss"] == 2
    assert feed(st, [seen]) == [[0]]                         # the high detection finds it again
    st = TS.new_state()                                      # ... and not a tentative one
    assert feed(st, [empty] * 3 + [seen, low]) == [[], [], [], [-1], [-1]] and st["tracks"] == []
    st = TS.new_state()                                      # alone it never gives birth, nor does a high one below new_score
    assert feed(st, [low, frame((A, 0.55, 0))]) == [[-1], [-1]] and st["next_id"] == 0
    # a low detection needs IoU > 0.5: [10, 10, 50, 50] against [24, 10, 64, 50] is 26 * 40 / (3200 - 1040) = 0.481
    st = TS.new_state()
    assert feed(st, [seen] * 3 + [frame(([24, 10, 64, 50], 0.35, 0))]) == [[0]] * 3 + [[-1]]
    st = TS.new_state()                                      # ... where a high one needs 0.2
    assert feed(st, [seen] * 3 + [frame(([24, 10, 64, 50], 0.9, 0))]) == [[0]] * 4


def test_exact_tie_the_lower_id_wins():
    for reverse in (False, True):
        st = TS.new_state()
        assert feed(st, [frame((A, 0.9, 0), (A, 0.8, 0))]) == [[0, 1]]
        if reverse:
            st["tracks"].reverse()                           # the order inside the table is not part of the contract
        assert feed(st, [frame((A, 0.9, 0))]) == [[0]]
        assert [k["id"] for k in st["tracks"]] == [0]        # track 1 was tentative and unmatched
    # one track, two identical detections: the lower row index wins, the other gives birth
    st = TS.new_state()
    assert feed(st, [frame((A, 0.9, 0)), frame((A, 0.9, 0), (A, 0.9, 0))]) == [[0], [0, 1]]
    # IoU decides before the id: track 1 fits better
    st = TS.new_state()
    assert feed(st, [frame((A, 0.9, 0), ([20, 10, 60, 50], 0.9, 0)), frame(([19, 10, 59, 50], 0.9, 0))]) == [[0, 1], [1]]


def test_class_gating_and_class_agnostic():
    st = TS.new_state()
    assert feed(st, [frame((A, 0.9, 1)), frame((A, 0.9, 2))]) == [[0], [1]]
    assert [(k["id"], k["cls"]) for k in st["tracks"]] == [(1, 2)]
    st = TS.new_state()
    assert feed(st, [frame((A, 0.9, 1)), frame((A, 0.9, 2))], class_agnostic=True) == [[0], [0]]
    assert [(k["id"], k["cls"], k["hits"]) for k in st["tracks"]] == [(0, 2, 2)]


def test_a_nan_coordinate_row_is_ignored():
    st = TS.new_state()
    nan = float("nan")
    assert feed(st, [frame(([nan, 10, 50, 50], 0.9, 1), (A, 0.9, 1), ([10, 10, 50, nan], 0.9, 1))]) == [[-1, 0, -1]]
    assert st["next_id"] == 1
    assert feed(st, [frame(([10, nan, 50, 50], 0.9, 1))]) == [[-1]] and st["tracks"] == []            # no match either: the track goes
    # a NaN score is low: it can keep a confirmed track and cannot give birth
    st = TS.new_state()
    assert feed(st, [frame((A, 0.9, 0))] * 3 + [frame((A, nan, 0))]) == [[0]] * 4
    assert feed(TS.new_state(), [frame((A, nan, 0))]) == [[-1]]


def test_bad_counts_and_streams_are_flagged_and_the_tracks_age():
    prm = TS.params()
    states = [TS.new_state(), TS.new_state()]
    rows = np.stack([frame((A, 0.9, 0))[0]] * 6)
    ids, ov = TS.run(states, rows, [1, 1, 1, -1, 5, 1], prm, frame_stream=[0, 0, 0, 0, 0, 2])
    assert ov == 3 and ids[:, 0].tolist() == [0, 0, 0, -1, -1, -1]
    assert states[0]["frame"] == 5 and states[0]["tracks"][0]["miss"] == 2 and states[1] == TS.new_state()


def test_capacity_is_flagged_never_evicted():
    n = TS.TRACK_CAP + 3
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0], rows[:, 2], rows[:, 3], rows[:, 4] = np.arange(n) * 20, np.arange(n) * 20 + 10, 10, 0.9
    st = TS.new_state()
    ids, ov = TS.step(st, rows, n, TS.params())
    assert ov == 3 and ids.tolist() == list(range(TS.TRACK_CAP)) + [-1] * 3 and st["next_id"] == TS.TRACK_CAP


# ---- the lane scene -------------------------------------------------------------------------------------------------------------------------
def lanes(seed, nobj=8, frames=30, K=32):
    rng = np.random.RandomState(seed); out = []
    x0 = rng.uniform(20, 200, nobj); vx = rng.uniform(2, 9, nobj) * rng.choice([-1, 1], nobj); x0 = np.where(vx < 0, x0 + 400, x0)
    for f in range(frames):
        rows = np.zeros((K, 6), np.float32); owner = []
        for o in rng.permutation(nobj):
            if f > 3 and (f + o) % 7 < 2: continue
            cx = x0[o] + vx[o] * f + rng.uniform(-1, 1); cy = 30 + 50 * o + rng.uniform(-1, 1)
            sc = 0.35 if (f + 2 * o) % 5 == 0 and f > 3 else rng.uniform(0.65, 0.95)
            rows[len(owner)] = [cx - 20, cy - 15, cx + 20, cy + 15, sc, o % 2]; owner.append(o)
        out.append((rows, len(owner), owner))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_lane_scene_keeps_every_identity(seed):
    st, prm = TS.new_state(), TS.params()
    of_object, total, unlabelled = {}, 0, 0
    for rows, n, owner in lanes(seed):
        ids, ov = TS.step(st, rows, n, prm)
        assert ov == 0 and (ids[n:] == -1).all()
        for d, o in enumerate(owner):
            total += 1
            if ids[d] < 0:
                unlabelled += 1
            else:
                of_object.setdefault(o, set()).add(int(ids[d]))
    print(f"seed {seed}: {total} object detections, {unlabelled} unlabelled, ids {sorted(map(sorted, of_object.values()))}, next_id {st['next_id']}")
    assert all(len(s) == 1 for s in of_object.values()) and len(set.union(*of_object.values())) == len(of_object) == 8      # no switches
    assert st["next_id"] == 8
    assert total == 180 and unlabelled <= 5


# ---- ABI and surface ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name in ("cvx_track_state_bytes", "cvx_track_update", "cvx_draw_tracks"):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
    assert len(L.PROTOTYPES["cvx_track_state_bytes"][1]) == 1 and len(L.PROTOTYPES["cvx_track_update"][1]) == 11
    assert len(L.PROTOTYPES["cvx_draw_tracks"][1]) == len(L.PROTOTYPES["cvx_draw_detections"][1]) + 1 == 13
    assert "cvx_track_stream" in header and "cvx_track_params" in header and "#define CVX_TRACK_CAP 1024" in header
    assert T.STREAM_DTYPE.itemsize == 16 + 48 * T.TRACK_CAP and ctypes.sizeof(T.TrackParams) == 40 and T.TRACK_CAP == TS.TRACK_CAP == 1024
    assert [f[0] for f in T.TrackParams._fields_[:9]] == list(T.DEFAULTS) == list(TS.DEFAULTS) and T.DEFAULTS == TS.DEFAULTS
    assert "track.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "iou_value" in open(os.path.join(ROOT, "computervision.pytorch_amd", "csrc", "box_overlap.h")).read()


def test_tracker_refuses_bad_parameters_and_the_cpu():
    for bad in (dict(high=1.5), dict(new_score=-0.1), dict(iou_high=2), dict(iou_low=float("nan")), dict(min_hits=0), dict(max_age=-1),
                dict(alpha=float("inf")), dict(speed=1), dict(min_hits=2.5)):
        with pytest.raises(ValueError):
            T.Tracker("cpu", **bad)
    with pytest.raises(ValueError):
        T.Tracker("cpu", streams=0)
    with pytest.raises(CvxError):
        T.Tracker("cpu")
    assert T.check_params(max_age=0)["max_age"] == 0 and T.check_params() == T.DEFAULTS


def test_track_keywords_on_the_four_detectors_and_not_on_deeplab():
    from configs import CenternetConfig, DeeplabV3PlusConfig, SsdConfig, Yolo7Config, Yolo8DetConfig
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from core.algorithms.ssd import Ssd
    from core.algorithms.yolo_v7 import YOLOv7
    from core.algorithms.yolo_v8 import YOLOv8
    from scripts import detect
    frame_ = torch.zeros(200, 300, 3, dtype=torch.uint8)
    for cls, cfg in ((YOLOv8, Yolo8DetConfig), (YOLOv7, Yolo7Config), (Ssd, SsdConfig), (CenterNetA, CenternetConfig)):
        algo = cls(cfg(), "cpu")
        for name in ("predict_batch", "predict_tiled"):
            assert inspect.signature(getattr(algo, name)).parameters["tracker"].default is None
        with pytest.raises(CvxError):                                       # no CPU path
            algo.detect_frames(None, [frame_], 2, track={"min_hits": 1})
    for fn in (YOLOv8.detect_frames, detect.detect_frames, detect.detect_video):
        assert inspect.signature(fn).parameters["track"].default is None
    cfg = DeeplabV3PlusConfig()
    cfg.arch.backbone_pretrained = False
    with pytest.raises(CvxError, match="no detections to track"):
        DeeplabV3PlusA(cfg, "cpu").detect_frames(None, [frame_], 2, track={})
    assert "tracker" not in inspect.signature(DeeplabV3PlusA.predict_batch).parameters
    assert "ids" in inspect.signature(R.draw_tracks).parameters and "ids" in inspect.signature(R.read_detections).parameters


def test_draw_tracks_restatement_by_hand():
    white = np.full((40, 60, 3), 255, np.uint8)
    rows = np.array([[5, 20, 30, 35, 0.9, 7], [40, 20, 55, 35, 0.9, 7]], np.float32)
    out, painted = TS.draw_tracks(white, rows, [-1, 1234567], 2)
    assert not painted[:, :38].any() and painted[20, 40]                                   # the row with id -1 paints nothing
    lut = R.palette(256)
    assert out[20, 40].tolist() == lut[(1234567 + 1) % 256].tolist()                       # the colour follows the id
    assert TS.track_label(1234567, 7) == "234567:7" and TS.track_label(5, 19) == "5:19"
    tag_w = (6 * len("234567:7") + 1) * 2
    assert painted[2:20, 40:60].all() and tag_w > 20                                       # the tag above the box, cut at the right edge
    one, _ = TS.draw_tracks(white, rows, [-1, 7], 2)
    same, _ = TS.draw_tracks(white, rows, [-1, 7 + 256], 2)                                # one LUT period on: the same colour, another label
    assert same[20, 40].tolist() == one[20, 40].tolist() == lut[8].tolist() and (same != one).any()
