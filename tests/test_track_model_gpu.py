"""MI355X: the tracker's optional Kalman motion model and minimum-cost association.  ``cvx_track_update_model``
against the numpy restatement (tests/track_model_restatement.py) -- ids as integers, the final tracks' boxes, velocities and covariances as
bit patterns --, ``TrackModel()`` against ``cvx_track_update`` byte for byte, and ``predict_batch`` / ``detect_frames`` with a model end to
end.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import track_model_restatement as TM
import track_restatement as TS
from computervision.pytorch_amd.track import EXT_BYTES, TRACK_CAP, Tracker, TrackModel
from test_track_gpu import PRM, on, scene, video
from test_track_gpu import yolov8  # noqa: F401  (the module's fixture: YOLOv8-n with random weights)

pytestmark = pytest.mark.gpu
OTHERS = [c for c in TM.COMBINATIONS if c != ("alpha_beta", "greedy")]
MOTIONS = ("alpha_beta", "kalman")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def crossing_scene(seed, nobj, frames, K, pairs=10):
    """``test_track_gpu.scene`` plus planted pairs of objects of one class and one size (48 x 40) on one line.  ``pairs`` crossings: 36 px
    apart, each moving 3 px a frame towards the other, so they overlap from the start and pass each other in frame 6.  ``pairs`` jumps: at
    rest 10 px apart, until in one frame the left one is seen 8 px to the left and the right one 6 px to the left, where they stay: the
    greedy walk takes the best pair (IoU 44/52) and leaves the worst (30/66), the least sum takes the two in between (40/56, 42/54)"""
    rows, counts = scene(seed, nobj, frames, K - 4 * pairs)
    rng = np.random.RandomState(seed + 1000)
    out = np.zeros((frames, K, 6), np.float32)
    y0, x0 = rng.randint(40, 680, 2 * pairs), rng.randint(60, 860, 2 * pairs)
    for f in range(frames):
        planted = []
        for q in range(pairs):
            for x in (x0[q] + 3 * f, x0[q] + 36 - 3 * f):
                planted.append([x, y0[q], x + 48, y0[q] + 40, rng.uniform(0.6, 0.95), q % 3])
        for q in range(pairs, 2 * pairs):
            moved = f >= 3 + (q - pairs) % 8
            for x in ((x0[q] - 8, x0[q] + 4) if moved else (x0[q], x0[q] + 10)):
                planted.append([x, y0[q], x + 48, y0[q] + 40, rng.uniform(0.6, 0.95), q % 3])
        both = np.concatenate([rows[f, :counts[f]], np.array(planted, np.float32)])
        out[f, :len(both)] = both[rng.permutation(len(both))]
        counts[f] = len(both)
    return out, counts


def restate(rows, counts, mdl, frame_stream=None, streams=1, **kw):
    states, prm = [TM.new_state() for _ in range(streams)], TM.params(**kw)
    ids, ov = TM.run(states, rows, counts, prm, mdl, frame_stream)
    return ids, ov, states


@functools.lru_cache(maxsize=None)
def restated_crowd(motion, assign):
    """the crossing crowd with the restatement's ids and final state -- worked out once, shared, never changed"""
    rows, counts = crossing_scene(0, 150, 12, 232)
    mdl = TM.model(motion=motion, assign=assign)
    ids, ov, (state,) = restate(rows, counts, mdl)
    assert ov == 0
    for a in (rows, counts, ids):
        a.setflags(write=False)
    return rows, counts, ids, state, mdl


def assert_tracks(got, state, mdl):
    want = TM.tracks_by_id(state, mdl)
    assert got["frame"] == state["frame"] and got["next_id"] == state["next_id"]
    for key in ("id", "hits", "miss"):
        assert np.array_equal(got[key], want[key]), key
    floats = ("box", "velocity", "cls") + (("cov",) if mdl["motion"] == "kalman" else ())
    assert ("cov" in got) == (mdl["motion"] == "kalman")
    for key in floats:
        assert got[key].dtype == np.float32 and got[key].shape == want[key].shape, key
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key


def tracker_of(dev, mdl, streams=1, **kw):
    return Tracker(dev, streams=streams, model=TrackModel(**mdl), **kw)


def run_and_compare(dev, rows, counts, mdl, split=None, frame_stream=None, **kw):
    want, ov, (state,) = restate(rows, counts, mdl, frame_stream, **kw)
    tracker = tracker_of(dev, mdl, **kw)
    arrays = on(dev, [rows, counts] + ([] if frame_stream is None else [frame_stream]))
    got, f = [], 0
    for k in split or (len(rows),):
        got.append(tracker.update(*[a[f:f + k] for a in arrays]))
        f += k
    got = torch.cat(got).cpu().numpy()
    for f in range(len(rows)):
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:8], got[f][got[f] != want[f]][:8], want[f][got[f] != want[f]][:8])
    assert tracker.overflowed() == ov
    assert_tracks(tracker.tracks(), state, mdl)
    return want, state


# ---- 1. the default model is the old entry, byte for byte -----------------------------------------------------------------------------------
def test_default_model_equals_cvx_track_update_byte_for_byte(dev):
    rows, counts = scene(1, 40, 12, 64, (320, 240))
    r, c = on(dev, [rows, counts])
    old, new = Tracker(dev), Tracker(dev, model=TrackModel())
    assert old.ext is None and new.ext.numel() == EXT_BYTES
    ids_old = torch.cat([old.update(r[:5], c[:5]), old.update(r[5:], c[5:])])
    ids_new = torch.cat([new.update(r[:5], c[:5]), new.update(r[5:], c[5:])])
    assert (ids_old >= 0).sum() > 200 and torch.equal(ids_old, ids_new)
    assert len(old.tracks()["id"]) > 20 and torch.equal(old.state, new.state)                      # the state starts zeroed: also the bytes past the live tracks
    assert not new.ext.any() and "cov" not in new.tracks()                     # the extension is not touched without the Kalman model
    assert old.overflowed() == new.overflowed() == 0


# ---- 2. the crossing crowd, in one call, frame by frame and in two parts --------------------------------------------------------------------
def test_the_models_differ_on_the_crossing_crowd():
    base = restated_crowd("alpha_beta", "greedy")
    print(f"crossing crowd: up to {base[1].max()} detections per frame, {base[3]['next_id']} ids issued")
    for motion, assign in OTHERS:
        rows, counts, ids, state, _ = restated_crowd(motion, assign)
        boxes, base_boxes = TS.tracks_by_id(state)["box"], TS.tracks_by_id(base[3])["box"]
        print(f"  {motion} / {assign}: {int((ids != base[2]).sum())} labels differ from alpha-beta / greedy, {state['next_id']} ids issued")
        if assign == "optimal":
            assert not np.array_equal(ids, base[2])                            # the association matters on this scene
        assert boxes.shape != base_boxes.shape or not np.array_equal(boxes, base_boxes)      # ... and so does the motion model
    assert base[1].max() > 128 and len(base[3]["tracks"]) > 128


@pytest.mark.parametrize("split", [(12,), (1,) * 12, (5, 7)], ids=["one_call", "frame_by_frame", "5_7"])
@pytest.mark.parametrize("motion,assign", OTHERS)
def test_crossing_crowd_equals_the_restatement(dev, motion, assign, split):
    rows, counts, want, state, mdl = restated_crowd(motion, assign)
    r, c = on(dev, [rows, counts])
    tracker = tracker_of(dev, mdl)
    got, f = [], 0
    for k in split:
        got.append(tracker.update(r[f:f + k], c[f:f + k]))
        f += k
    got = torch.cat(got).cpu().numpy()
    for f in range(len(rows)):
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:8])
    assert_tracks(tracker.tracks(), state, mdl)
    assert tracker.overflowed() == 0


# ---- 3. the solver's edges ------------------------------------------------------------------------------------------------------------------
def cluster(rng, n, score, base=(100, 100, 300, 300), jitter=3):
    """n rows around one box, integer coordinates: every pair of them overlaps by far more than any threshold"""
    out = np.zeros((n, 6), np.float32)
    out[:, :4] = np.array(base) + rng.randint(-jitter, jitter + 1, (n, 4))
    out[:, 4] = score
    return out


def frames_of(*per_frame):
    K = max(len(r) for r in per_frame)
    rows, counts = np.zeros((len(per_frame), K, 6), np.float32), np.array([len(r) for r in per_frame], np.int32)
    for f, r in enumerate(per_frame):
        rows[f, :len(r)] = r
    return rows, counts


@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("tracks,dets", [(1, 1), (1, 2), (3, 70), (70, 3), (64, 64)])
def test_solver_edges_small(dev, motion, tracks, dets):
    """``tracks`` tracks born around one box, then ``dets`` rows around it twice: every pair is allowed, so nothing is taken before the solver
    (but 1 x 1, which step (a) takes); 64 x 64 with identical boxes: every cost is 0, pure ties"""
    rng = np.random.RandomState(tracks * 100 + dets)
    jitter = 0 if (tracks, dets) == (64, 64) else 3
    per_frame = [cluster(rng, tracks, 0.9, jitter=jitter), cluster(rng, dets, 0.55, jitter=jitter), cluster(rng, dets, 0.55, jitter=jitter),
                 cluster(rng, dets, 0.3, jitter=jitter)]                       # below new_score: no births; the last frame: stage 2
    mdl = TM.model(motion=motion, assign="optimal")
    want, state = run_and_compare(dev, *frames_of(*per_frame), mdl)
    assert (want[1] >= 0).sum() == min(tracks, dets)
    if (tracks, dets) == (64, 64):
        assert want[1, :64].tolist() == list(range(64))                        # ascending id, then row


@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("n", [1024, 1025, 4096])
def test_solver_edges_many_rows(dev, motion, n):
    """two tracks and n rows that all overlap both: n columns go to the solver -- 1024: one per lane, the frame staged in LDS; 1025: the
    frame read from global memory, four columns per lane; 4096: the most the optimal association takes.  Scores below new_score: no births"""
    rng = np.random.RandomState(n)
    per_frame = [cluster(rng, 2, 0.9), cluster(rng, n, 0.55), cluster(rng, n, 0.55), cluster(rng, n, 0.3)]
    mdl = TM.model(motion=motion, assign="optimal")
    want, state = run_and_compare(dev, *frames_of(*per_frame), mdl)
    assert [(w >= 0).sum() for w in want] == [2, 2, 2, 2] and state["next_id"] == 2


# ---- 4. capacity, and more rows than the kernel stages --------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion,assign", OTHERS)
def test_capacity_and_1100_rows(dev, motion, assign):
    K, n = 1152, 1100
    rng = np.random.RandomState(3)
    rows = np.zeros((3, K, 6), np.float32)
    k = np.arange(n)                                                           # 16 x 16 boxes 10 apart along x: neighbours overlap by 6 / 26 > 0.2
    rows[0, :n] = np.stack([(k % 40) * 10, (k // 40) * 24, (k % 40) * 10 + 16, (k // 40) * 24 + 16, rng.uniform(0.6, 0.95, n), np.zeros(n)], 1)
    pick = np.concatenate([rng.choice(TRACK_CAP, 7, replace=False), TRACK_CAP + rng.choice(n - TRACK_CAP, 3, replace=False)])
    pick = pick[rng.permutation(10)]
    rows[1, :10] = rows[0, pick]
    rows[1, :10, :4] += rng.randint(-3, 4, (10, 1))
    rows[2, :n] = rows[0, rng.permutation(n)]
    rows[2, :n, :4] += 1
    counts = np.array([n, 10, n], np.int32)
    mdl = TM.model(motion=motion, assign=assign)
    want, ov, (state,) = restate(rows, counts, mdl, min_hits=1, max_age=5)
    assert ov >= n - TRACK_CAP and len(state["tracks"]) == TRACK_CAP
    tracker = tracker_of(dev, mdl, min_hits=1, max_age=5)
    r, c = on(dev, [rows, counts])
    got = torch.cat([tracker.update(r[:1], c[:1]), tracker.update(r[1:], c[1:])]).cpu().numpy()
    for f in range(3):
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:8])
    assert tracker.overflowed() == ov
    assert_tracks(tracker.tracks(), state, mdl)


# ---- 5. streams, reset, NaN rows, bad counts and a bad stream -------------------------------------------------------------------------------
def test_two_interleaved_streams_and_reset(dev):
    mdl = TM.model(motion="kalman", assign="optimal")
    a, b = scene(1, 40, 8, 64, (320, 240)), scene(2, 40, 8, 64, (320, 240))
    rows, counts = np.zeros((16, 64, 6), np.float32), np.zeros(16, np.int32)
    rows[0::2], rows[1::2], counts[0::2], counts[1::2] = a[0], b[0], a[1], b[1]
    stream = np.tile(np.array([0, 1], np.int32), 8)
    want, ov, states = restate(rows, counts, mdl, stream, streams=2)
    alone_b, _, (state_b,) = restate(*b, mdl)
    assert ov == 0 and np.array_equal(want[1::2], alone_b)
    r, c, s = on(dev, [rows, counts, stream])
    tracker = tracker_of(dev, mdl, streams=2)
    ids = torch.cat([tracker.update(r[:6], c[:6], s[:6]), tracker.update(r[6:], c[6:], s[6:])]).cpu().numpy()
    assert np.array_equal(ids, want)
    assert_tracks(tracker.tracks(0), states[0], mdl)
    assert_tracks(tracker.tracks(1), states[1], mdl)
    tracker.reset(stream=1)
    empty = tracker.tracks(1)
    assert len(empty["id"]) == 0 and empty["frame"] == 0 and empty["next_id"] == 0 and empty["cov"].shape == (0, 3)
    assert not tracker.ext[EXT_BYTES:].any() and tracker.ext[:EXT_BYTES].any()
    assert_tracks(tracker.tracks(0), states[0], mdl)
    again = tracker.update(*on(dev, [b[0], b[1], np.ones(8, np.int32)])).cpu().numpy()       # a reset stream starts over
    assert np.array_equal(again, alone_b) and tracker.overflowed() == 0
    assert_tracks(tracker.tracks(1), state_b, mdl)
    tracker.reset()
    assert len(tracker.tracks(0)["id"]) == 0 and tracker.tracks(0)["frame"] == 0 and not tracker.ext.any() and not tracker.state.any()


@pytest.mark.parametrize("motion,assign", OTHERS)
def test_nan_rows_bad_counts_and_a_bad_stream(dev, motion, assign):
    box, nan, K = [10, 10, 50, 50], float("nan"), 3
    frames = [([(box, 0.9, 0), ([100, 10, 140, 50], 0.9, 1)], 2)] * 3
    frames += [([], 0), ([(box, 0.9, 0)], -1), ([(box, 0.9, 0)], K + 1)]
    frames += [([([nan, 10, 50, 50], 0.9, 0), (box, 0.9, 0), ([100, 10, nan, 50], 0.9, 1)], 3)]
    frames += [([(box, 0.9, 0)], 1), ([(box, 0.9, 0)], 1)]
    stream = np.array([0] * 7 + [5, 0], np.int32)
    rows = np.zeros((len(frames), K, 6), np.float32)
    for f, (dets, _) in enumerate(frames):
        for d, (b, score, cls) in enumerate(dets):
            rows[f, d] = b + [score, cls]
    counts = np.array([n for _, n in frames], np.int32)
    mdl = TM.model(motion=motion, assign=assign)
    want, ov, (state,) = restate(rows, counts, mdl, stream)
    assert ov == 3 and want[6].tolist() == [-1, 0, -1] and want[7].tolist() == [-1, -1, -1] and want[8, 0] == 0
    r, c, s = on(dev, [rows, counts, stream])
    for split in ((9,), (4, 5)):
        tracker, got, f = tracker_of(dev, mdl), [], 0
        for k in split:
            got.append(tracker.update(r[f:f + k], c[f:f + k], s[f:f + k]))
            f += k
        assert np.array_equal(torch.cat(got).cpu().numpy(), want)
        assert tracker.overflowed() == 3
        assert_tracks(tracker.tracks(), state, mdl)


def test_optimal_refuses_more_than_4096_rows(dev):
    rows, counts = torch.zeros(1, 4097, 6, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="4096"):
        Tracker(dev, model=TrackModel(assign="optimal")).update(rows, counts)
    assert Tracker(dev, model=TrackModel(motion="kalman")).update(rows, counts).shape == (1, 4097)      # the greedy association takes them


# ---- 6. no host read ------------------------------------------------------------------------------------------------------------------------
def test_update_does_not_wait_on_the_host(dev):
    rows, counts, want, _, mdl = restated_crowd("kalman", "optimal")
    r, c = on(dev, [rows, counts])
    tracker_of(dev, mdl).update(r[:1], c[:1])                                  # first use
    tracker = tracker_of(dev, mdl)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ids = tracker.update(r, c)
        tracker.reset(0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(ids.cpu().numpy(), want) and tracker.tracks()["frame"] == 0


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion,assign", [("kalman", "optimal")])
def test_yolov8_predict_batch_and_detect_frames_with_a_model(dev, yolov8, motion, assign):  # noqa: F811
    from scripts import detect
    algo, model = yolov8
    mdl = TM.model(motion=motion, assign=assign)
    host = video(21, 6)
    rows0, counts0 = algo.predict_batch(model, on(dev, host), conf_threshold=0.001, sync=False)
    tracker = Tracker(dev, model=TrackModel(**mdl), **PRM)
    rows, counts, ids = algo.predict_batch(model, on(dev, host), conf_threshold=0.001, sync=False, tracker=tracker)
    assert torch.equal(rows.view(torch.int32), rows0.view(torch.int32)) and torch.equal(counts, counts0)
    assert ids.shape == rows.shape[:2] and ids.dtype == torch.int32
    rows, counts, ids = rows.cpu().numpy(), counts.cpu().numpy(), ids.cpu().numpy()
    want, _, (state,) = restate(rows, counts, mdl, **PRM)
    print("YOLOv8-n detections per frame:", counts.tolist(), "labelled:", (want >= 0).sum(1).tolist(), "ids issued:", state["next_id"])
    assert counts.min() > 0 and (want >= 0).sum() > 0 and np.array_equal(ids, want)
    assert_tracks(tracker.tracks(), state, mdl)
    # detect_frames takes the model inside the dict of the tracker's keywords: it paints what draw_tracks paints for the restated ids
    shown = on(dev, host)
    algo.conf_threshold, saved = 0.001, algo.conf_threshold
    try:
        batches = list(detect.detect_frames(algo, model, iter(shown), 3, track=dict(model=dict(motion=motion, assign=assign), **PRM)))
    finally:
        algo.conf_threshold = saved
    torch.cuda.synchronize()
    assert [len(b) for b in batches] == [3, 3]
    for b in range(6):
        painted, mask = TS.draw_tracks(host[b], rows[b], want[b], counts[b])
        assert np.array_equal(shown[b].cpu().numpy(), painted), b
    assert mask.any()
