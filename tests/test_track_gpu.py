"""MI355X: multi-object tracking on the device.  ``cvx_track_update`` against the numpy restatement
(tests/track_restatement.py) -- ids as integers, the final tracks' boxes and velocities as bit patterns --, ``cvx_draw_tracks`` byte for
byte, and ``predict_batch`` / ``predict_tiled`` / ``detect_frames`` with a tracker end to end.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import render_restatement as RS
import track_restatement as TS
from computervision.pytorch_amd import render as R
from computervision.pytorch_amd.track import TRACK_CAP, Tracker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def scene(seed, nobj, frames, K, size=(960, 720), clutter=5):
    """(rows (frames, K, 6), counts (frames)): objects of 3 classes drifting over a canvas of ``size`` (w, h) at up to 4 px per frame, INTEGER
    coordinates (so exact IoU ties occur), 8 % drop-outs, a quarter of the scores from 0.3 .. 0.95 and the rest from 0.6 .. 0.95, ``clutter``
    low-score boxes per frame, the rows of each frame shuffled"""
    rng = np.random.RandomState(seed)
    cx, cy = rng.uniform(0, size[0], nobj), rng.uniform(0, size[1], nobj)
    vx, vy = rng.uniform(-4, 4, nobj), rng.uniform(-4, 4, nobj)
    bw, bh = rng.randint(24, 72, nobj), rng.randint(24, 72, nobj)
    cls = rng.randint(0, 3, nobj)
    rows, counts = np.zeros((frames, K, 6), np.float32), np.zeros(frames, np.int32)
    for f in range(frames):
        found = []
        for o in range(nobj):
            if rng.uniform() < 0.08:
                continue
            x, y = np.rint(cx[o] + vx[o] * f + rng.uniform(-1, 1)), np.rint(cy[o] + vy[o] * f + rng.uniform(-1, 1))
            score = rng.uniform(0.3, 0.95) if rng.uniform() < 0.25 else rng.uniform(0.6, 0.95)
            found.append([x - bw[o] // 2, y - bh[o] // 2, x + bw[o] // 2, y + bh[o] // 2, score, cls[o]])
        for _ in range(clutter):
            x, y = rng.randint(0, size[0] - 60), rng.randint(0, size[1] - 60)
            found.append([x, y, x + rng.randint(20, 60), y + rng.randint(20, 60), rng.uniform(0.1, 0.45), rng.randint(0, 3)])
        found = np.array(found, np.float32)[rng.permutation(len(found))]
        assert len(found) <= K
        rows[f, :len(found)], counts[f] = found, len(found)
    return rows, counts


@functools.lru_cache(maxsize=None)
def restated(seed, nobj, frames, K, size=(960, 720), **kw):
    """the scene with the restatement's ids per frame, its final state and statistics -- worked out once, shared, never changed"""
    rows, counts = scene(seed, nobj, frames, K, size)
    state, prm = TS.new_state(), TS.params(**kw)
    ids, live = np.zeros((frames, K), np.int32), []
    for f in range(frames):
        ids[f], ov = TS.step(state, rows[f], counts[f], prm)
        assert ov == 0
        live.append(len(state["tracks"]))
    for a in (rows, counts, ids):
        a.setflags(write=False)
    return rows, counts, ids, state, max(live)


def assert_tracks(got, state):
    want = TS.tracks_by_id(state)
    assert got["frame"] == state["frame"] and got["next_id"] == state["next_id"]
    for key in ("id", "hits", "miss"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("box", "velocity", "cls"):
        assert got[key].dtype == np.float32 and got[key].shape == want[key].shape
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key


# ---- 1. a crowded scene, in one call, frame by frame and in two parts -----------------------------------------------------------------------
CROWD = (0, 150, 12, 192)
SMALL = (1, 40, 8, 64, (320, 240))                                             # 40 objects close enough for their classes to matter


def test_the_crowded_scene_is_crowded():
    rows, counts, ids, state, live = restated(*CROWD)
    print(f"crowded scene: up to {counts.max()} detections and {live} live tracks per frame, {state['next_id']} ids issued, "
          f"{int((ids >= 0).sum())} labels")
    assert counts.max() > 128 and live > 128 and state["next_id"] > live      # past two waves of rows and of tracks; deletions and re-births
    low = rows[..., 4] < 0.5
    assert int(((ids >= 0) & low).sum()) > 20                                  # labels handed out in stage 2


@pytest.mark.parametrize("split", [(12,), (1,) * 12, (5, 7)])
def test_crowded_scene_equals_the_restatement(dev, split):
    rows, counts, want, state, _ = restated(*CROWD)
    r, c = on(dev, [rows, counts])
    tracker = Tracker(dev)
    got, f = [], 0
    for k in split:
        got.append(tracker.update(r[f:f + k], c[f:f + k]))
        f += k
    got = torch.cat(got).cpu().numpy()
    for f in range(len(rows)):
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:8])
    assert_tracks(tracker.tracks(), state)
    assert tracker.overflowed() == 0


# ---- 2. two streams in one batch ------------------------------------------------------------------------------------------------------------
def test_two_interleaved_streams_equal_the_streams_alone(dev):
    a, b = restated(*SMALL), restated(2, *SMALL[1:])
    rows, counts = np.zeros((16, 64, 6), np.float32), np.zeros(16, np.int32)
    rows[0::2], rows[1::2], counts[0::2], counts[1::2] = a[0], b[0], a[1], b[1]
    stream = np.tile(np.array([0, 1], np.int32), 8)
    r, c, s = on(dev, [rows, counts, stream])
    tracker = Tracker(dev, streams=2)
    ids = torch.cat([tracker.update(r[:6], c[:6], s[:6]), tracker.update(r[6:], c[6:], s[6:])]).cpu().numpy()
    assert np.array_equal(ids[0::2], a[2]) and np.array_equal(ids[1::2], b[2])
    assert_tracks(tracker.tracks(0), a[3])
    assert_tracks(tracker.tracks(1), b[3])
    alone = Tracker(dev)                                                       # stream 1's frames through a tracker of its own
    assert np.array_equal(alone.update(*on(dev, [b[0], b[1]])).cpu().numpy(), b[2])
    tracker.reset(stream=1)
    empty = tracker.tracks(1)
    assert len(empty["id"]) == 0 and empty["frame"] == 0 and empty["next_id"] == 0
    assert_tracks(tracker.tracks(0), a[3])
    again = tracker.update(*on(dev, [b[0], b[1], np.ones(8, np.int32)])).cpu().numpy()      # a reset stream starts over
    assert np.array_equal(again, b[2]) and tracker.overflowed() == 0
    tracker.reset()
    assert len(tracker.tracks(0)["id"]) == 0 and tracker.tracks(0)["frame"] == 0


# ---- 3. capacity ----------------------------------------------------------------------------------------------------------------------------
def test_capacity_is_flagged_never_evicted(dev):
    K, n = 1152, 1100                                                          # more rows than the kernel stages, more than one pass of births
    rng = np.random.RandomState(3)
    rows = np.zeros((3, K, 6), np.float32)
    k = np.arange(n)
    rows[0, :n] = np.stack([(k % 40) * 24, (k // 40) * 24, (k % 40) * 24 + 16, (k // 40) * 24 + 16, rng.uniform(0.6, 0.95, n), k % 3], 1)
    pick = np.concatenate([rng.choice(TRACK_CAP, 7, replace=False), TRACK_CAP + rng.choice(n - TRACK_CAP, 3, replace=False)])
    pick = pick[rng.permutation(10)]                                           # frame 2: ten of them, moved a little; three had no track
    rows[1, :10] = rows[0, pick]
    rows[1, :10, :4] += rng.randint(-3, 4, (10, 1))
    rows[2, :n] = rows[0, rng.permutation(n)]                                  # frame 3: all again, against the ten tracks frame 2 left
    rows[2, :n, :4] += 1
    counts = np.array([n, 10, n], np.int32)
    state, prm = TS.new_state(), TS.params()
    want0, ov0 = TS.step(state, rows[0], n, prm)
    assert ov0 == n - TRACK_CAP == 76 and want0[:n].tolist() == list(range(TRACK_CAP)) + [-1] * 76
    want1, ov1 = TS.step(state, rows[1], 10, prm)
    assert ov1 == 0 and len(state["tracks"]) == 10 and (want1[:10] >= 0).sum() == 10
    want2, ov2 = TS.step(state, rows[2], n, prm)
    assert ov2 == n - TRACK_CAP and len(state["tracks"]) == TRACK_CAP and len(set(want2[:n].tolist()) & set(want1[:10].tolist())) == 10
    r, c = on(dev, [rows, counts])
    tracker = Tracker(dev)
    got = tracker.update(r, c).cpu().numpy()
    for f, want in enumerate((want0, want1, want2)):
        assert np.array_equal(got[f], want), (f, np.flatnonzero(got[f] != want)[:8])
    assert tracker.overflowed() == 2 * 76
    assert_tracks(tracker.tracks(), state)


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------------
def test_edges(dev):
    box = [10, 10, 50, 50]
    nan = float("nan")
    K = 3
    frames = [([(box, 0.9, 0), ([100, 10, 140, 50], 0.9, 1)], 2)] * 3                      # two confirmed tracks
    frames += [([], 0), ([(box, 0.9, 0)], -1), ([(box, 0.9, 0)], K + 1)]                    # an empty frame; two bad counts: the tracks age
    frames += [([([nan, 10, 50, 50], 0.9, 0), (box, 0.9, 0), ([100, 10, nan, 50], 0.9, 1)], 3)]      # NaN rows beside a good one
    frames += [([(box, 0.9, 0)], 1), ([(box, 0.9, 0)], 1)]                                  # the first of them goes to a stream that does not exist
    stream = np.array([0] * 7 + [5, 0], np.int32)
    rows = np.zeros((len(frames), K, 6), np.float32)
    for f, (dets, _) in enumerate(frames):
        for d, (b, score, cls) in enumerate(dets):
            rows[f, d] = b + [score, cls]
    counts = np.array([n for _, n in frames], np.int32)
    states, prm = [TS.new_state()], TS.params()
    want, ov = TS.run(states, rows, counts, prm, stream)
    assert ov == 3 and want[6].tolist() == [-1, 0, -1] and want[7].tolist() == [-1, -1, -1] and want[8, 0] == 0
    assert states[0]["frame"] == 8 and [k["miss"] for k in states[0]["tracks"]] == [0, 5]
    r, c, s = on(dev, [rows, counts, stream])
    for split in ((9,), (4, 5)):
        tracker, got, f = Tracker(dev), [], 0
        for k in split:
            got.append(tracker.update(r[f:f + k], c[f:f + k], s[f:f + k]))
            f += k
        assert np.array_equal(torch.cat(got).cpu().numpy(), want)
        assert tracker.overflowed() == 3
        assert_tracks(tracker.tracks(), states[0])
    # max_det = 1
    one = np.array([[box + [0.9, 0]]] * 4, np.float32)
    tracker = Tracker(dev)
    assert tracker.update(*on(dev, [one, np.array([1, 1, 0, 1], np.int32)])).cpu().numpy().tolist() == [[0], [0], [-1], [-1]]
    assert tracker.tracks()["next_id"] == 2                                                 # the tentative track went with its miss


# ---- 5. other parameters --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(class_agnostic=True), dict(min_hits=1, max_age=0), dict(high=0.6, new_score=0.7, iou_high=0.3, iou_low=0.4,
                                                                                              alpha=0.5, beta=0.125, min_hits=2, max_age=2)],
                         ids=["class_agnostic", "min_hits_1_max_age_0", "all_changed"])
def test_other_parameters(dev, kw):
    rows, counts, want, state, _ = restated(*SMALL, **kw)
    assert not np.array_equal(want, restated(*SMALL)[2])                 # the parameters matter on this scene
    tracker = Tracker(dev, **kw)
    got = tracker.update(*on(dev, [rows, counts])).cpu().numpy()
    assert np.array_equal(got, want)
    assert_tracks(tracker.tracks(), state)


# ---- 6. drawing -----------------------------------------------------------------------------------------------------------------------------
def pictures(shapes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def draw_case(h, w, many, seed):
    """the rows tests/test_predict_batch_gpu.py draws: outside the frame, across its edges, degenerate, inverted, NaN, overlapping, random"""
    rng = np.random.RandomState(seed)
    rows = [[w + 50, h + 50, w + 90, h + 80, 0.5, 3], [-300, -300, -200, -250, 0.7, 4], [-7.6, -3.2, 12.9, 9.4, 0.99949997, 0],
            [w - 9.5, h - 6.5, w + 30.2, h + 11.9, 0.0625, 19], [w // 2, 4, w // 2, h - 3, 1.0, 79], [20, h - 4, 10, h - 9, 0.9, 5],
            [float("nan"), 2, 9, 9, 0.9, 5]]
    for k in range(5):
        rows.append([6 + 3 * k, 8 + 2 * k, w - 12 + 2 * k, h - 14 + 3 * k, 0.25 + 0.1 * k, [0, 19, 79, 7, 250][k]])
    for _ in range(many):
        x, y = rng.uniform(-10, w), rng.uniform(-10, h)
        rows.append([x, y, x + rng.uniform(-2, 40), y + rng.uniform(-2, 40), rng.uniform(0, 1), rng.randint(0, 80)])
    return np.array(rows, np.float32)


def test_draw_tracks_equals_the_restatement(dev):
    shapes = [(37, 53), (64, 64), (10, 14)]                                    # contiguous; a padded pitch (below); smaller than a tag
    per_frame = [draw_case(37, 53, 0, 1), draw_case(64, 64, 40, 2), draw_case(10, 14, 0, 3)]
    K = max(len(r) for r in per_frame)
    rows, ids = np.zeros((3, K, 6), np.float32), np.full((3, K), -1, np.int32)
    rng = np.random.RandomState(4)
    for b, r in enumerate(per_frame):
        rows[b, :len(r)] = r
        ids[b, :len(r)] = rng.randint(0, 3000, len(r))
        ids[b, 7] = 987654 + b                                                 # a 6-digit id, and beyond
        ids[b, 8] = 1234567
        ids[b, [2, 9]] = [-1, -7]                                              # negative: not painted
    ids[0, 3] = 2 ** 31 - 1
    counts = np.array([len(r) for r in per_frame], np.int32)
    host = pictures(shapes, 5)
    padded = torch.zeros(64, 64 * 3 + 16, dtype=torch.uint8, device=dev)
    frames = on(dev, host)
    frames[1] = padded[:, :64 * 3].view(64, 64, 3)
    frames[1].copy_(torch.from_numpy(host[1]))
    r, i, c = on(dev, [rows, ids, counts])
    R.draw_tracks(frames, r, i, c)
    plain = on(dev, host)
    R.draw_detections(plain, r, c)                                             # the other instance of the shared body, on the same rows
    torch.cuda.synchronize()
    for b in range(3):
        want, painted = TS.draw_tracks(host[b], rows[b], ids[b], counts[b])
        got = frames[b].cpu().numpy()
        assert painted.any() and np.array_equal(got, want), (b, np.argwhere((got != want).any(2))[:5])
        assert np.array_equal(plain[b].cpu().numpy(), RS.draw(host[b], rows[b], counts[b])[0]), b
    assert not padded[:, 64 * 3:].any()                                        # the bytes between the rows
    thin = on(dev, host[:1])
    R.draw_tracks(thin, r[:1], i[:1], c[:1], thickness=1, font_scale=1)
    assert np.array_equal(thin[0].cpu().numpy(), TS.draw_tracks(host[0], rows[0], ids[0], counts[0], thickness=1, font_scale=1)[0])


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def yolov8(dev):
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8
    cfg = Yolo8DetConfig()
    cfg.dataset.num_classes, cfg.arch.input_size = 20, (3, 128, 128)
    algo = YOLOv8(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for k in [k for k in sd if ".cv3." in k and k.endswith(".2.bias")]:
        sd[k] += 3.0                                           # random-init class biases leave no score above 0.001 (tests/test_det_eval_gpu.py)
    model.load_state_dict(sd)
    return algo, model


def video(seed, n, shape=(97, 200)):
    """n frames of one picture drifting two pixels a frame: consecutive frames give similar detections"""
    rng = np.random.RandomState(seed)
    h, w = shape
    big = rng.randint(0, 256, (h, w + 2 * n, 3), dtype=np.uint8)
    return [np.ascontiguousarray(big[:, 2 * k:2 * k + w]) for k in range(n)]


PRM = dict(high=0.0015, new_score=0.002, min_hits=2)                           # an untrained network's scores lie just above the 0.001 it is asked for


def restate(rows, counts, **kw):
    state, prm = TS.new_state(), TS.params(**kw)
    return TS.run([state], rows, counts, prm)[0], state


def test_yolov8_predict_batch_with_a_tracker(dev, yolov8):
    from scripts import detect
    algo, model = yolov8
    host = video(21, 6)
    rows0, counts0 = algo.predict_batch(model, on(dev, host), conf_threshold=0.001, sync=False)
    tracker = Tracker(dev, **PRM)
    rows, counts, ids = algo.predict_batch(model, on(dev, host), conf_threshold=0.001, sync=False, tracker=tracker)
    assert torch.equal(rows.view(torch.int32), rows0.view(torch.int32)) and torch.equal(counts, counts0)
    rows, counts, ids = rows.cpu().numpy(), counts.cpu().numpy(), ids.cpu().numpy()
    want, state = restate(rows, counts, **PRM)
    print("YOLOv8-n detections per frame:", counts.tolist(), "labelled:", (want >= 0).sum(1).tolist(), "ids issued:", state["next_id"])
    assert counts.min() > 0 and (want >= 0).sum() > 0 and len(np.unique(want[want >= 0])) > 1
    assert ids.dtype == np.int32 and np.array_equal(ids, want)
    assert_tracks(tracker.tracks(), state)
    # sync=True: one host read, a fourth element
    found = algo.predict_batch(model, on(dev, host), conf_threshold=0.001, sync=True, tracker=Tracker(dev, **PRM))
    plain = algo.predict_batch(model, on(dev, host), conf_threshold=0.001, sync=True)
    assert len(found) == len(plain) == 6
    for b, (four, three) in enumerate(zip(found, plain)):
        assert len(four) == 4 and len(three) == 3 and all(np.array_equal(x, y) for x, y in zip(four[:3], three))
        assert four[3].dtype == np.int32 and np.array_equal(four[3], want[b, :counts[b]])
    # detect_frames in two batches of three paints what draw_tracks paints for the restated ids
    shown = on(dev, host)
    algo.conf_threshold, saved = 0.001, algo.conf_threshold
    try:
        batches = list(detect.detect_frames(algo, model, iter(shown), 3, track=PRM))
    finally:
        algo.conf_threshold = saved
    torch.cuda.synchronize()
    assert [len(b) for b in batches] == [3, 3]
    for b in range(6):
        painted, mask = TS.draw_tracks(host[b], rows[b], want[b], counts[b])
        assert np.array_equal(shown[b].cpu().numpy(), painted), b
    assert mask.any()


def test_yolov8_predict_tiled_with_a_tracker(dev, yolov8):
    algo, model = yolov8
    host = video(22, 2, (150, 260))
    kw = dict(conf_threshold=0.001, max_det=100)
    rows0, counts0 = algo.predict_tiled(model, on(dev, host), sync=False, **kw)
    tracker = Tracker(dev, **PRM)
    shown = on(dev, host)
    rows, counts, ids = algo.predict_tiled(model, shown, sync=False, draw=True, tracker=tracker, **kw)
    assert torch.equal(rows.view(torch.int32), rows0.view(torch.int32)) and torch.equal(counts, counts0)
    rows, counts, ids = rows.cpu().numpy(), counts.cpu().numpy(), ids.cpu().numpy()
    want, state = restate(rows, counts, **PRM)
    print("tiled detections per frame:", counts.tolist(), "labelled:", (want >= 0).sum(1).tolist())
    assert counts.min() > 0 and (want[1] >= 0).sum() > 0
    assert np.array_equal(ids, want)
    assert_tracks(tracker.tracks(), state)
    for b in range(2):
        assert np.array_equal(shown[b].cpu().numpy(), TS.draw_tracks(host[b], rows[b], want[b], counts[b])[0]), b


def test_tracking_does_not_wait_on_the_host(dev, yolov8):
    algo, model = yolov8
    host = video(23, 5)
    algo.predict_batch(model, on(dev, host[:2]), conf_threshold=0.001, draw=True, sync=False, tracker=Tracker(dev, **PRM))      # first use
    algo.predict_batch(model, on(dev, host[:3]), conf_threshold=0.001, draw=True, sync=False, tracker=Tracker(dev, **PRM))
    frames, tracker = on(dev, host), Tracker(dev, **PRM)
    algo.conf_threshold, saved = 0.001, algo.conf_threshold
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            caught = False
        except RuntimeError:
            caught = True
        if not caught:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a read-back on this build")
        rows, counts, ids = algo.predict_batch(model, frames[:2], draw=True, sync=False, tracker=tracker)
        batches = list(algo.detect_frames(model, iter(frames[2:]), 3, track=tracker))
        tracker.reset(0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        algo.conf_threshold = saved
    torch.cuda.synchronize()
    assert [len(b) for b in batches] == [3] and ids.shape == rows.shape[:2] and (ids >= 0).any()
    assert tracker.tracks()["frame"] == 0
