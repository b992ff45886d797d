"""MI355X: tracking evaluation on the device.  ``cvx_mot_frames`` and ``cvx_mot_summary`` against the numpy
restatement (tests/track_eval_restatement.py): the state blocks byte for byte, the table integer for integer; ``evaluate_tracking`` end
to end.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest
import torch

import track_eval_restatement as TE
from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd.track import Tracker
from computervision.pytorch_amd.track_eval import TrackingEvaluator, flags_of, results_of

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def assert_equal(ev, states):
    """the evaluator's state blocks and its table against the restatement's"""
    gi, ti = ev.max_gt_ids, ev.max_track_ids
    for s, st in enumerate(states):
        got, want = ev.state_block(s), TE.pack(st)
        if not np.array_equal(got, want):
            g = TE.unpack(got, gi, ti)
            diff = {k: (g[k].ravel()[np.flatnonzero(g[k].ravel() != st[k].ravel())[:6]].tolist(),
                        st[k].ravel()[np.flatnonzero(g[k].ravel() != st[k].ravel())[:6]].tolist()) for k in st if not np.array_equal(g[k], st[k])}
            raise AssertionError(f"stream {s}: (got, want) {diff}; head {dict(zip(TE.HEAD, g['head'].tolist()))}")
    table, want = ev.summary_table(), TE.summary(states)
    assert table.dtype == np.int64 and np.array_equal(table, want), (table.tolist(), want.tolist())
    return table


# ---- 1. a crowded scene with planted id swaps ---------------------------------------------------------------------------------------------
def crowd(seed, nobj, frames, K, G, size=(960, 720), swap=0.03, drop=0.08, clutter=6):
    """(rows, counts, ids, gt, gt_counts) of ``frames`` frames: objects of 3 classes drifting over the canvas, INTEGER coordinates (exact
    ties occur), every object's hypothesis jittered by up to 3 px, dropped with probability ``drop``, its track id replaced by a fresh one
    or exchanged with a neighbour's with probability ``swap``; ``clutter`` unmatched hypotheses with fresh ids per frame; 5 % of the
    identities absent per frame; rows and ground truths of each frame shuffled"""
    rng = np.random.RandomState(seed)
    cx, cy = rng.uniform(0, size[0], nobj), rng.uniform(0, size[1], nobj)
    vx, vy = rng.uniform(-4, 4, nobj), rng.uniform(-4, 4, nobj)
    bw, bh = rng.randint(24, 72, nobj), rng.randint(24, 72, nobj)
    cls = rng.randint(0, 3, nobj)
    track, nxt = list(range(nobj)), nobj
    rows, counts, ids = np.zeros((frames, K, 6), np.float32), np.zeros(frames, np.int32), np.full((frames, K), -1, np.int32)
    gt, gt_counts = np.zeros((frames, G, 6), np.float32), np.zeros(frames, np.int32)
    for f in range(frames):
        truths, hyps = [], []
        for o in range(nobj):
            if rng.uniform() < swap:
                if rng.uniform() < 0.5:
                    track[o], nxt = nxt, nxt + 1
                else:
                    other = (o + 1) % nobj
                    track[o], track[other] = track[other], track[o]
        for o in range(nobj):
            if rng.uniform() < 0.05:
                continue
            x, y = np.rint(cx[o] + vx[o] * f), np.rint(cy[o] + vy[o] * f)
            truths.append([x - bw[o] // 2, y - bh[o] // 2, x + bw[o] // 2, y + bh[o] // 2, cls[o], o])
            if rng.uniform() >= drop:
                dx, dy = rng.randint(-3, 4), rng.randint(-3, 4)
                hyps.append([x - bw[o] // 2 + dx, y - bh[o] // 2 + dy, x + bw[o] // 2 + dx, y + bh[o] // 2 + dy, rng.uniform(0.3, 0.95), cls[o], track[o]])
        for _ in range(clutter):
            x, y = rng.randint(0, size[0] - 60), rng.randint(0, size[1] - 60)
            hyps.append([x, y, x + rng.randint(20, 60), y + rng.randint(20, 60), rng.uniform(0.1, 0.45), rng.randint(0, 3), -1 if rng.uniform() < 0.3 else nxt])
            nxt += 1
        truths = np.array(truths, np.float32)[rng.permutation(len(truths))]
        hyps = np.array(hyps, np.float64)[rng.permutation(len(hyps))]
        assert len(hyps) <= K and len(truths) <= G
        rows[f, :len(hyps)], ids[f, :len(hyps)], counts[f] = hyps[:, :6], hyps[:, 6], len(hyps)
        gt[f, :len(truths)], gt_counts[f] = truths, len(truths)
    return rows, counts, ids, gt, gt_counts


CROWD = dict(seed=0, nobj=150, frames=12, K=192, G=160)
SIZES = dict(max_gt_ids=256, max_track_ids=1024)


@functools.lru_cache(maxsize=None)
def crowd_restated():
    """the crowded scene and the restatement's final state -- worked out once, shared, never changed"""
    data = crowd(**CROWD)
    st = TE.new_state(**SIZES)
    TE.run([st], *data, TE.params())
    for a in data + tuple(st.values()):
        a.setflags(write=False)
    return data, st


def test_the_crowded_scene_is_crowded():
    data, st = crowd_restated()
    r = TE.results(TE.summary_row(st))
    print("crowded scene:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    assert data[1].max() > 128 and data[4].max() > 128 and not any(TE.flags(TE.summary_row(st)).values())
    assert r["num_switches"] > 20 and r["num_fragmentations"] > 5 and r["num_misses"] > 50 and r["num_false_positives"] > 50
    assert 0 < r["idtp"] < r["num_matches"] and r["mostly_tracked"] > 0 and r["partially_tracked"] > 0


@pytest.mark.parametrize("split", [(12,), (1,) * 12, (5, 7)])
def test_crowded_scene_equals_the_restatement(dev, split):
    data, st = crowd_restated()
    t = on(dev, data)
    ev = TrackingEvaluator(dev, **SIZES)
    f = 0
    for k in split:
        ev.add_frames(*[a[f:f + k] for a in t])
        f += k
    table = assert_equal(ev, [st])
    res = ev.get_results()
    assert res["overall"] == res["streams"][0] == results_of(table[0]) == TE.results(table[0])


def test_add_frames_and_reset_do_not_wait_on_the_host(dev):
    data, st = crowd_restated()
    t = on(dev, data)
    ev = TrackingEvaluator(dev, **SIZES)
    ev.add_frames(*[a[:2] for a in t])                        # first use
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
        ev.add_frames(*[a[2:] for a in t])
        ev.reset(0)
        ev.add_frames(*t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_equal(ev, [st])


# ---- 2. two streams in one batch, and reset -----------------------------------------------------------------------------------------------
def test_two_interleaved_streams_and_reset(dev):
    a, b = crowd(1, 40, 8, 64, 48, (320, 240)), crowd(2, 40, 8, 64, 48, (320, 240))
    mixed = [np.zeros((16,) + x.shape[1:], x.dtype) for x in a]
    for m, x, y in zip(mixed, a, b):
        m[0::2], m[1::2] = x, y
    stream = np.tile(np.array([0, 1], np.int32), 8)
    states = [TE.new_state(), TE.new_state()]                 # the default sizes
    TE.run(states, *mixed, TE.params(), frame_stream=stream)
    alone = TE.new_state()
    TE.run([alone], *b, TE.params())
    assert np.array_equal(TE.pack(alone), TE.pack(states[1]))
    t, s = on(dev, mixed), on(dev, [stream])[0]
    ev = TrackingEvaluator(dev, streams=2)
    ev.add_frames(*[x[:6] for x in t], frame_stream=s[:6])
    ev.add_frames(*[x[6:] for x in t], frame_stream=s[6:])
    table = assert_equal(ev, states)
    assert np.array_equal(table[2], table[0] + table[1]) and table[0, 3] > 0 and table[1, 3] > 0
    res = ev.get_results()
    assert len(res["streams"]) == 2 and res["overall"]["num_objects"] == res["streams"][0]["num_objects"] + res["streams"][1]["num_objects"]
    ev.reset(0)
    assert_equal(ev, [TE.new_state(), states[1]])
    ev.add_frames(*on(dev, a))                                # stream 0 again, from nothing
    fresh = TE.new_state()
    TE.run([fresh], *a, TE.params())
    assert_equal(ev, [fresh, states[1]])
    ev.reset()
    assert_equal(ev, [TE.new_state(), TE.new_state()])


# ---- 3. single frames: rectangular both ways, ties, the matrix in LDS and in the workspace ------------------------------------------------
def random_frame(seed, ng, nh, distinct, canvas=400, jitter=3):
    """one frame of ``ng`` truths and ``nh`` hypotheses drawn from ``distinct`` base boxes (integer, jittered by up to ``jitter`` px): with
    few base boxes and no jitter, exact ties"""
    rng = np.random.RandomState(seed)
    x, y = rng.randint(0, canvas, distinct), rng.randint(0, canvas, distinct)
    w, h = rng.randint(30, 60, distinct), rng.randint(30, 60, distinct)
    base = np.stack([x, y, x + w, y + h], 1).astype(np.float32)
    cls = rng.randint(0, 2, distinct).astype(np.float32)

    def draw(n):
        pick = rng.randint(0, distinct, n)
        d = rng.randint(-jitter, jitter + 1, (n, 2)) if jitter else np.zeros((n, 2), np.int64)
        return base[pick] + np.concatenate([d, d], 1).astype(np.float32), cls[pick]
    gbox, gcls = draw(ng)
    hbox, hcls = draw(nh)
    rows, gt = np.zeros((1, max(nh, 1), 6), np.float32), np.zeros((1, max(ng, 1), 6), np.float32)
    rows[0, :nh, :4], rows[0, :nh, 4], rows[0, :nh, 5] = hbox, 0.9, hcls
    gt[0, :ng, :4], gt[0, :ng, 4], gt[0, :ng, 5] = gbox, gcls, rng.permutation(ng)
    ids = np.full((1, max(nh, 1)), -1, np.int32)
    ids[0, :nh] = rng.permutation(nh) + 5
    return rows, np.array([nh], np.int32), ids, gt, np.array([ng], np.int32)


@pytest.mark.parametrize("ng,nh,distinct,jitter", [(1, 1, 1, 0), (3, 70, 6, 2), (70, 3, 6, 2), (70, 70, 200, 3), (300, 300, 40, 0), (128, 128, 60, 2),
                                                   (129, 128, 60, 2), (128, 129, 60, 2), (200, 520, 150, 3)])
def test_single_frames_equal_the_restatement(dev, ng, nh, distinct, jitter):
    sizes = dict(max_gt_ids=512, max_track_ids=1024)
    prm = dict(iou=0.3, class_agnostic=(ng + nh) % 2 == 1)
    states, ev = [TE.new_state(**sizes)], TrackingEvaluator(dev, **sizes, **prm)
    for seed in (0, 1):                                       # the second frame of other boxes: memories without continuity's help
        data = random_frame(seed * 1000 + ng * 7 + nh, ng, nh, distinct, jitter=jitter)
        TE.run(states, *data, TE.params(**prm))
        ev.add_frames(*on(dev, data))
    table = assert_equal(ev, states)
    r = TE.results(table[0])
    print(f"{ng} x {nh}: {r['num_matches']} matches, {r['num_switches']} switches, cost {table[0, 8]}, IDTP {r['idtp']}")
    assert r["num_matches"] > 0 and (ng * nh <= TE.MAT_LDS) == ((ng, nh) in ((1, 1), (3, 70), (70, 3), (70, 70), (128, 128)))


# ---- 4. the empty frames and every flag ---------------------------------------------------------------------------------------------------
def test_empty_frames_and_every_flag(dev):
    A, FAR = [0, 0, 100, 100], [500, 500, 600, 600]
    B, K, G = 12, 8, 6
    rows, ids, gt = np.zeros((B, K, 6), np.float32), np.full((B, K), -1, np.int32), np.zeros((B, G, 6), np.float32)
    counts, gt_counts, stream = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)

    def put(b, truths, hyps, s=0):
        for i, (box, cls, tid) in enumerate(hyps):
            rows[b, i], ids[b, i] = list(box) + [0.9, cls], tid
        for i, (box, cls, ident) in enumerate(truths):
            gt[b, i] = list(box) + [cls, ident]
        counts[b], gt_counts[b], stream[b] = len(hyps), len(truths), s
    put(0, [(A, 0, 0)], [(A, 0, 1)])
    put(1, [], [(A, 0, 1), (FAR, 0, 2)])                                                       # no ground truth
    put(2, [(A, 0, 0), (FAR, 0, 1)], [])                                                       # no rows
    put(3, [], [])
    put(4, [(A, 0, 0), ([NAN, 0, 1, 1], 0, 1)], [([0, NAN, 100, 100], 0, 1), (A, 0, 2)])        # two NaN boxes
    put(5, [(A, 0, 0), (FAR, 0, 1)], [(A, 0, 4), (FAR, 0, 4), (FAR, 0, 4)])                     # the id twice more
    put(6, [(A, 0, 2), (FAR, 0, 2)], [(A, 0, 4), (FAR, 0, 5)])                                  # the identity again
    put(7, [(A, 0, 16), (A, 0, -1), (A, 0, 1.5), (A, 0, NAN), (A, 0, 15)], [(FAR, 0, 32), (A, 0, 31)])
    put(8, [(A, 0, 0)], [(A, 0, 1)], s=2)                                                       # nobody's frame
    put(9, [(A, 0, 0)], [(A, 0, 1)], s=1)
    put(10, [(A, 0, 0)], [(A, 0, 1)], s=1)
    put(11, [(A, 0, 0)], [(A, 0, 1)])
    counts[10], gt_counts[11] = K + 1, -1                                                       # bad counts
    sizes = dict(max_gt_ids=16, max_track_ids=32)
    states = [TE.new_state(**sizes), TE.new_state(**sizes)]
    TE.run(states, rows, counts, ids, gt, gt_counts, TE.params(), frame_stream=stream)
    ev = TrackingEvaluator(dev, streams=2, **sizes)
    ev.add_frames(*on(dev, [rows, counts, ids, gt, gt_counts]), frame_stream=on(dev, [stream])[0])
    table = assert_equal(ev, states)
    assert flags_of(table[0]) == dict(nan=2, dup_row=2, dup_gt=1, identity=4, track=1, frame=2, excess=0) and flags_of(table[1])["frame"] == 1
    assert table[0, 0] == 8 and table[1, 0] == 1
    with pytest.raises(CvxError, match="skipped"):
        ev.get_results()
    # more than 1024 hypotheses in a frame, in rows beyond one pass of the workgroup
    K = 1100
    rows, ids = np.zeros((1, K, 6), np.float32), np.full((1, K), -1, np.int32)
    rows[0, :, 0], rows[0, :, 2], rows[0, :, 3] = np.arange(K) * 20, np.arange(K) * 20 + 10, 10
    ids[0, 40:1070] = np.arange(1030)
    gt = np.zeros((1, 2, 6), np.float32)
    gt[0, 0], gt[0, 1] = [400 * 20, 0, 400 * 20 + 10, 10, 0, 3], [1069 * 20, 0, 1069 * 20 + 10, 10, 0, 2]
    data = (rows, np.array([K], np.int32), ids, gt, np.array([2], np.int32))
    st = TE.new_state(8, 4096)
    TE.run([st], *data, TE.params())
    ev = TrackingEvaluator(dev, max_gt_ids=8)
    ev.add_frames(*on(dev, data))
    table = assert_equal(ev, [st])
    assert flags_of(table[0])["excess"] == 6 and table[0, 2] == 1024 and table[0, 3] == 1 and table[0, 4] == 1


# ---- 5. the summary on planted states -----------------------------------------------------------------------------------------------------
def planted(seed, gi, ti, rows, cols, density, values):
    """a state whose c has ``rows`` x ``cols`` non-empty entries region (scattered over the identities and tracks) drawn from ``values``"""
    rng = np.random.RandomState(seed)
    st = TE.new_state(gi, ti)
    r, k = np.sort(rng.permutation(gi)[:rows]), np.sort(rng.permutation(ti)[:cols])
    sub = rng.choice(values, (rows, cols)) * (rng.uniform(size=(rows, cols)) < density)
    st["c"][np.ix_(r, k)] = sub
    st["present"][:] = rng.randint(0, 3, gi)
    st["present"][r] = np.maximum(sub.max(1, initial=0), 1) + rng.randint(0, 4, rows)
    st["matched"][:] = (st["present"] * rng.uniform(0, 1, gi)).astype(np.int32)
    st["matched"][::7] = (st["present"][::7] * 4 + 4) // 5    # some identities exactly on the 0.8 boundary
    st["matched"][1::7] = st["present"][1::7] // 5
    st["head"][:9] = rng.randint(0, 1 << 40, 9, dtype=np.int64)
    return st


@pytest.mark.parametrize("rows,cols,density,values", [(1, 1, 1.0, [5]), (64, 200, 0.2, list(range(1, 40))), (200, 64, 0.2, list(range(1, 40))),
                                                      (0, 0, 1.0, [1]), (90, 120, 0.5, [3]), (120, 90, 1.0, [2, 3]), (256, 256, 0.05, list(range(1, 9)))])
def test_summary_equals_the_restatement(dev, rows, cols, density, values):
    gi, ti = 256, 256
    states = [planted(10 * rows + cols, gi, ti, rows, cols, density, values), planted(7, gi, ti, 5, 9, 0.6, [1, 2])]
    ev = TrackingEvaluator(dev, streams=2, max_gt_ids=gi, max_track_ids=ti)
    ev.state.copy_(torch.from_numpy(np.concatenate([TE.pack(s) for s in states])).to(dev))
    table = assert_equal(ev, states)
    brute = table[0, 12]
    print(f"{rows} x {cols}: IDTP {brute}, MT/PT/ML {table[0, 9:12].tolist()}, {table[0, 20]} identities, {table[0, 21]} tracks")
    assert (brute > 0) == (rows > 0) and table[0, 21] <= cols
    again = ev.summary_table()                                # the summary changes no state
    assert np.array_equal(again, table)


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
PRM = dict(high=0.0015, new_score=0.002, min_hits=2)          # an untrained network's scores lie just above the 0.001 it is asked for


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


def video(seed, n, shape):
    """n frames of one picture drifting two pixels a frame: consecutive frames give similar detections"""
    h, w = shape
    big = np.random.RandomState(seed).randint(0, 256, (h, w + 2 * n, 3), dtype=np.uint8)
    return [np.ascontiguousarray(big[:, 2 * k:2 * k + w]) for k in range(n)]


def truths_from(rows, counts, ids):
    """a ground truth made of the tracker's own output: the labelled rows of every other frame, a pixel off, under identities of their
    own, and one box nobody finds"""
    truths = []
    for b in range(len(rows)):
        lab = np.flatnonzero(ids[b, :counts[b]] >= 0)[:8] if b % 2 == 0 else np.zeros(0, np.int64)
        g = np.zeros((len(lab) + 1, 6), np.float32)
        g[:len(lab), :4], g[:len(lab), 4], g[:len(lab), 5] = rows[b, lab, :4] + 1, rows[b, lab, 5], ids[b, lab] % 64
        g[len(lab)] = [150, 5, 190, 45, 0, 100 + b % 2]
        _, first = np.unique(g[:, 5], return_index=True)       # an identity once per frame
        truths.append(np.ascontiguousarray(g[np.sort(first)]))
    return truths


def restated_results(rows, counts, ids, truths):
    st = TE.new_state()
    for b in range(len(rows)):
        TE.step(st, rows[b], int(counts[b]), ids[b], truths[b], len(truths[b]), TE.params())
    return TE.results(TE.summary_row(st))


def test_yolov8_evaluate_tracking(dev, yolov8, tmp_path):
    algo, model = yolov8
    host = video(21, 6, (97, 200))
    algo.conf_threshold, saved = 0.001, algo.conf_threshold
    try:
        rows, counts, ids = algo.predict_batch(model, on(dev, host), sync=False, tracker=Tracker(dev, **PRM))
        rows, counts, ids = rows.cpu().numpy(), counts.cpu().numpy(), ids.cpu().numpy()
        assert counts.min() > 0 and (ids >= 0).sum() > 6
        truths = truths_from(rows, counts, ids)
        sequence = list(zip(on(dev, host), on(dev, truths)))
        res = algo.evaluate_tracking(model, sequence, str(tmp_path), tracker=PRM, batch_size=3)
    finally:
        algo.conf_threshold = saved
    want = restated_results(rows, counts, ids, truths)
    print("YOLOv8-n tracking scores:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in want.items()})
    assert res["overall"] == res["streams"][0] == want and want["num_matches"] > 0 and want["num_misses"] >= 6
    text = open(os.path.join(str(tmp_path), "results", "tracking.txt")).read()
    assert text.splitlines()[-1].split()[0] == "overall" and f"{want['mota']:.6f}" in text


def test_yolov8_evaluate_tracking_tiled(dev, yolov8, tmp_path):
    algo, model = yolov8
    host = video(22, 4, (150, 260))
    kw = dict(conf_threshold=0.001, max_det=100)
    tracker = Tracker(dev, **PRM)
    rows, counts, ids = algo.predict_tiled(model, on(dev, host), sync=False, tracker=tracker, **kw)
    rows, counts, ids = rows.cpu().numpy(), counts.cpu().numpy(), ids.cpu().numpy()
    # what the rest needs of the scene: a labelled row in the frames that give the truths (the untrained network finds one box per
    # frame here; the kernels meet crowds in the tests above, this one is about the tiled path)
    assert counts.min() > 0 and (ids[0] >= 0).any() and (ids[2] >= 0).any()
    truths = truths_from(rows, counts, ids)
    tracker.reset()                                           # a Tracker of the caller's is used as it is
    res = algo.evaluate_tracking(model, list(zip(on(dev, host), on(dev, truths))), str(tmp_path), tracker=tracker, batch_size=4, tiled=kw)
    want = restated_results(rows, counts, ids, truths)
    print("tiled tracking scores:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in want.items()})
    assert res["overall"] == want and want["num_matches"] > 0 and os.path.exists(os.path.join(str(tmp_path), "results", "tracking.txt"))
    with pytest.raises(ValueError):
        algo.evaluate_tracking(model, [], str(tmp_path), tiled=dict(draw=True))
