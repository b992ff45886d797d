"""CPU: the tracking-evaluation rules as tests/track_eval_restatement.py states them, against hand-derived answers;
its solver against scipy's; IDTP against Ristani's dummy-node formulation; the new symbols; the surface that needs no GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import track_eval_restatement as TE
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import track as T
from computervision.pytorch_amd import track_eval as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, FAR = [0, 0, 100, 100], [500, 500, 600, 600]
NAN = float("nan")


def arrays(truths, hyps, K=8, G=8):
    """rows (K, 6), count, ids (K), gt (G, 6), gt_count from truths [(box, cls, identity)] and hypotheses [(box, cls, track id)]"""
    rows, ids, gt = np.zeros((K, 6), np.float32), np.full(K, -1, np.int32), np.zeros((G, 6), np.float32)
    for i, (box, cls, tid) in enumerate(hyps):
        rows[i], ids[i] = list(box) + [0.9, cls], tid
    for i, (box, cls, ident) in enumerate(truths):
        gt[i] = list(box) + [cls, ident]
    return rows, len(hyps), ids, gt, len(truths)


def play(frames, state=None, small=True, **kw):
    """runs [(truths, hypotheses)] through the restatement; returns (state, the matches of every frame)"""
    state = state if state is not None else (TE.new_state(16, 32) if small else TE.new_state())
    prm = TE.params(**kw)
    return state, [TE.step(state, *arrays(t, h), prm) for t, h in frames]


def scores(state):
    row = TE.summary_row(state)
    return TE.results(row), TE.flags(row)


# ---- hand-derived answers -----------------------------------------------------------------------------------------------------------------
def test_one_object_whose_track_changes_after_four_of_ten_frames():
    st, m = play([([(A, 0, 0)], [(A, 0, 1)])] * 4 + [([(A, 0, 0)], [(A, 0, 2)])] * 6)
    r, f = scores(st)
    assert m == [[(0, 1, 0)]] * 4 + [[(0, 2, 0)]] * 6 and not any(f.values())
    assert (r["num_switches"], r["num_matches"], r["num_misses"], r["num_false_positives"], r["num_objects"]) == (1, 10, 0, 0, 10)
    assert r["mota"] == 0.9 and r["motp"] == 1.0
    assert (r["idtp"], r["idfp"], r["idfn"]) == (6, 4, 4) and r["idf1"] == 0.6 and r["idp"] == 0.6 and r["idr"] == 0.6
    assert (r["mostly_tracked"], r["partially_tracked"], r["mostly_lost"], r["num_fragmentations"]) == (1, 0, 0, 0)
    assert st["c"][0, 1] == 4 and st["c"][0, 2] == 6 and st["c"].sum() == 10 and st["mem"][0] == 3 and st["last"][0] == 10


def test_continuity_keeps_a_worse_pair_than_the_assignment_would_choose():
    # frame 2: A-1 IoU 6000 / 10000, A-2 IoU 1, B-1 IoU 6000 / 7000, B-2 IoU 7000 / 10000.  The assignment alone takes A-2 and B-1
    # (cost 0 + 9362); continuity keeps A-1 (26214) and leaves B-2 (19661).
    B, one, two = [0, 0, 100, 70], [0, 0, 100, 60], [0, 0, 100, 100]
    first = ([(A, 0, 0)], [(A, 0, 1)])
    second = ([(A, 0, 0), (B, 0, 1)], [(one, 0, 1), (two, 0, 2)])
    st, m = play([first, second])
    assert m[1] == [(0, 1, 26214), (1, 2, 19661)]
    assert st["head"][TE.H["switches"]] == 0 and st["head"][TE.H["cost"]] == 26214 + 19661
    st, m = play([second])                                                   # without the memory: the optimum
    assert m[0] == [(0, 2, 0), (1, 1, 9362)]
    cost = TE.pair_costs(np.array([A, B]), [0, 0], np.array([one, two]), [0, 0], TE.params())
    assert cost.tolist() == [[26214, 0], [9362, 19661]] and TE.assign(cost) == [(1, 0, 9362), (0, 1, 0)]
    # a remembered track from two frames ago is not continuity: the assignment decides, and a switch is counted
    st, m = play([first, ([(A, 0, 0)], []), second])
    assert m[2] == [(0, 2, 0), (1, 1, 9362)] and st["head"][TE.H["switches"]] == 1


def test_a_switch_is_counted_against_a_memory_many_frames_old():
    seen, lost = ([(A, 0, 3)], [(A, 0, 1)]), ([(A, 0, 3)], [])
    st, _ = play([seen] + [lost] * 5 + [([(A, 0, 3)], [(A, 0, 2)])])
    r, _ = scores(st)
    assert (r["num_switches"], r["num_misses"], r["num_matches"], r["num_fragmentations"]) == (1, 5, 2, 1)
    st, _ = play([seen] + [lost] * 5 + [seen])                               # the same track again: no switch
    assert scores(st)[0]["num_switches"] == 0 and st["mem"][3] == 2 and st["last"][3] == 7


def test_a_fragmentation_spans_frames_in_which_the_identity_is_absent():
    seen, lost, absent = ([(A, 0, 0)], [(A, 0, 1)]), ([(A, 0, 0)], []), ([], [])
    st, _ = play([seen, lost, absent, absent, seen])
    assert scores(st)[0]["num_fragmentations"] == 1 and st["present"][0] == 3 and st["matched"][0] == 2
    st, _ = play([seen, absent, absent, seen])                                # absent is not unmatched
    assert scores(st)[0]["num_fragmentations"] == 0
    st, _ = play([lost, lost, seen, lost, seen, lost, seen])                  # not before the first match
    assert scores(st)[0]["num_fragmentations"] == 2


@pytest.mark.parametrize("present,matched,want", [(5, 4, "mostly_tracked"), (10, 8, "mostly_tracked"), (10, 7, "partially_tracked"),
                                                  (5, 1, "partially_tracked"), (10, 2, "partially_tracked"), (10, 1, "mostly_lost"),
                                                  (5, 0, "mostly_lost"), (1, 1, "mostly_tracked")])
def test_the_boundaries_of_mostly_tracked_and_mostly_lost(present, matched, want):
    seen, lost = ([(A, 0, 0)], [(A, 0, 1)]), ([(A, 0, 0)], [])
    st, _ = play([seen] * matched + [lost] * (present - matched))
    r, _ = scores(st)
    assert {k: r[k] for k in ("mostly_tracked", "partially_tracked", "mostly_lost")} == {
        k: int(k == want) for k in ("mostly_tracked", "partially_tracked", "mostly_lost")}


def test_a_frame_without_ground_truth_and_a_frame_without_rows():
    st, m = play([([], [(A, 0, 1), (FAR, 0, 2)]), ([(A, 0, 0), (FAR, 0, 1)], []), ([], [])])
    r, f = scores(st)
    assert m == [[], [], []] and not any(f.values())
    assert (r["num_frames"], r["num_false_positives"], r["num_misses"], r["num_matches"], r["num_objects"], r["num_hypotheses"]) == (3, 2, 2, 0, 2, 2)
    assert r["mota"] == -1.0 and np.isnan(r["motp"]) and (r["idtp"], r["idfp"], r["idfn"]) == (0, 2, 2) and r["idf1"] == 0.0
    assert np.isnan(scores(TE.new_state(4, 4))[0]["mota"])
    # rows with id -1 are not tracker output
    st, m = play([([(A, 0, 0)], [(A, 0, -1), (A, 0, 5)])])
    assert m == [[(0, 5, 0)]] and scores(st)[0]["num_hypotheses"] == 1


def test_class_gating_and_class_agnostic():
    frame = ([(A, 1, 0)], [(A, 2, 7)])
    st, m = play([frame])
    assert m == [[]] and st["c"].sum() == 0 and scores(st)[0]["num_misses"] == 1 and scores(st)[0]["num_false_positives"] == 1
    st, m = play([frame], class_agnostic=True)
    assert m == [[(0, 7, 0)]] and st["c"][0, 7] == 1
    # the gate: IoU 0.5 passes at the default, and a lower one does not
    st, m = play([([(A, 0, 0)], [([0, 0, 100, 50], 0, 1)]), ([(A, 0, 1)], [([0, 0, 100, 49], 0, 2)])])
    assert m == [[(0, 1, 32768)], []]
    st, m = play([([(A, 0, 1)], [([0, 0, 100, 49], 0, 2)])], iou=0.49)
    assert m == [[(1, 2, 33423)]]


def test_every_flag():
    def flags_after(truths, hyps, **kw):
        st, _ = play([(truths, hyps)], **kw)
        r, f = scores(st)
        return f, r
    none = dict.fromkeys(("nan", "dup_row", "dup_gt", "identity", "track", "frame", "excess"), 0)
    f, r = flags_after([(A, 0, 0)], [([0, NAN, 100, 100], 0, 1), (A, 0, 2)])
    assert f == {**none, "nan": 1} and (r["num_matches"], r["num_hypotheses"]) == (1, 1)
    f, r = flags_after([([NAN, 0, 100, 100], 0, 0), (A, 0, 1)], [(A, 0, 2)])
    assert f == {**none, "nan": 1} and (r["num_matches"], r["num_objects"]) == (1, 1)
    f, r = flags_after([(A, 0, 0), (FAR, 0, 1)], [(A, 0, 4), (FAR, 0, 4), (FAR, 0, 4)])      # the first row with the id stays
    assert f == {**none, "dup_row": 2} and (r["num_matches"], r["num_hypotheses"], r["num_misses"]) == (1, 1, 1)
    f, r = flags_after([(A, 0, 2), (FAR, 0, 2)], [(A, 0, 4), (FAR, 0, 5)])
    assert f == {**none, "dup_gt": 1} and (r["num_matches"], r["num_objects"], r["num_false_positives"]) == (1, 1, 1)
    f, r = flags_after([(A, 0, 16), (A, 0, -1), (A, 0, 1.5), (A, 0, NAN), (A, 0, 15)], [(A, 0, 4)])     # max_gt_ids is 16 here
    assert f == {**none, "identity": 4} and (r["num_matches"], r["num_objects"]) == (1, 1)
    f, r = flags_after([(A, 0, 0)], [(FAR, 0, 32), (A, 0, 31)])                                          # max_track_ids is 32 here
    assert f == {**none, "track": 1} and (r["num_matches"], r["num_hypotheses"]) == (1, 1)
    # a NaN row with a repeated id is a NaN, and does not make the next one a duplicate
    f, r = flags_after([(A, 0, 0)], [([NAN, 0, 1, 1], 0, 3), (A, 0, 3)])
    assert f == {**none, "nan": 1} and r["num_matches"] == 1
    # bad counts and streams skip the frame whole
    states, prm = [TE.new_state(16, 32), TE.new_state(16, 32)], TE.params()
    rows, n, ids, gt, g = arrays([(A, 0, 0)], [(A, 0, 1)])
    B = 6
    TE.run(states, np.stack([rows] * B), [1, -1, 9, 1, 1, 1], np.stack([ids] * B), np.stack([gt] * B), [1, 1, 1, 9, -2, 1], prm,
           frame_stream=[0, 0, 1, 1, 2, 1])
    t = TE.summary(states)
    assert TE.flags(t[0])["frame"] == 2 and TE.flags(t[1])["frame"] == 2 and TE.flags(t[2]) == {**none, "frame": 4}
    assert TE.results(t[0])["num_frames"] == 1 and TE.results(t[1])["num_frames"] == 1 and TE.results(t[2])["num_matches"] == 2
    # more than 1024 hypotheses in a frame
    K = 1030
    rows, ids = np.zeros((K, 6), np.float32), np.arange(K, dtype=np.int32)
    rows[:, 0], rows[:, 2], rows[:, 3] = np.arange(K) * 20, np.arange(K) * 20 + 10, 10
    st = TE.new_state(4, 4096)
    TE.step(st, rows, K, ids, np.zeros((1, 6), np.float32), 0, prm)
    assert TE.flags(TE.summary_row(st)) == {**none, "excess": 6} and st["head"][TE.H["hypotheses"]] == 1024


# ---- the solver against scipy -------------------------------------------------------------------------------------------------------------
def scipy_optimum(cost):
    """(pairs, total) of the assignment with the most allowed pairs and the least sum among those"""
    big = np.where(cost < 0, TE.BIG, cost)
    r, c = linear_sum_assignment(big)
    ok = cost[r, c] >= 0
    return int(ok.sum()), int(cost[r, c][ok].sum())


def random_cost(rng, a, b, forbidden, duplicates, top=65536):
    cost = rng.randint(0, top + 1, (a, b)).astype(np.int64)
    if duplicates:                                           # duplicate rows and columns: ties everywhere
        cost[rng.randint(0, a, a // 2 + 1)] = cost[rng.randint(0, a)]
        cost[:, rng.randint(0, b, b // 2 + 1)] = cost[:, [rng.randint(0, b)]]
    cost[rng.uniform(size=(a, b)) < forbidden] = -1
    return cost


SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (7, 3), (8, 8), (17, 17), (30, 45), (45, 30), (64, 65), (70, 90), (90, 70)]


@pytest.mark.parametrize("shape", SHAPES)
def test_the_solver_equals_scipy_in_pairs_and_total(shape):
    rng = np.random.RandomState(shape[0] * 100 + shape[1])
    for forbidden in (0.0, 0.3, 0.8, 0.97, 1.0):
        for duplicates in (False, True):
            for top in (65536, 3):
                cost = random_cost(rng, *shape, forbidden, duplicates, top)
                pairs = TE.assign(cost)
                assert len({i for i, _, _ in pairs}) == len(pairs) == len({j for _, j, _ in pairs})          # one to one
                assert all(cost[i, j] == c >= 0 for i, j, c in pairs)
                assert (len(pairs), sum(c for _, _, c in pairs)) == scipy_optimum(cost), (shape, forbidden, duplicates, top)


def test_the_solver_by_hand():
    assert TE.assign(np.array([[4, 1, 3], [2, 0, 5], [3, 2, 2]])) == [(1, 0, 2), (0, 1, 1), (2, 2, 2)]
    # cardinality before cost: the cheap pair (0, 0) would leave row 1 without a partner
    assert TE.assign(np.array([[0, 50], [7, -1]])) == [(1, 0, 7), (0, 1, 50)]
    # an exact tie: row 0 takes the lowest column
    assert TE.assign(np.array([[5, 5], [5, 5]])) == [(0, 0, 5), (1, 1, 5)]
    assert TE.assign(np.array([[-1, -1], [-1, -1]])) == [] and TE.assign(np.zeros((0, 3))) == [] and TE.assign(np.zeros((3, 0))) == []
    # the smaller side drives: 3 x 2 is solved as 2 x 3, the answer is in the matrix's own coordinates
    assert sorted(TE.assign(np.array([[9, 1], [1, 9], [0, 0]]))) == [(0, 1, 1), (2, 0, 0)]
    assert TE.solve(np.array([[3, 1, 2]])).tolist() == [-1, 0, -1]


# ---- IDTP against the dummy-node formulation ----------------------------------------------------------------------------------------------
def lanes(seed, nobj=12, frames=25, swap=0.1, drop=0.15, clutter=2):
    """a seeded scene with planted id swaps: [(truths, hypotheses)] with integer boxes"""
    rng = np.random.RandomState(seed)
    x0, vx = rng.randint(0, 300, nobj), rng.randint(-6, 7, nobj)
    track, nxt, out = list(range(nobj)), nobj, []
    for f in range(frames):
        truths, hyps = [], []
        for o in range(nobj):
            if (f + o) % 9 == 0:
                continue                                     # the identity is absent
            x, y = int(x0[o] + vx[o] * f), 40 * o
            truths.append(([x, y, x + 40, y + 30], o % 2, o))
            if rng.uniform() < swap:
                track[o], nxt = nxt, nxt + 1                 # a new track id
            if rng.uniform() >= drop:
                dx = int(rng.randint(-6, 7))
                hyps.append(([x + dx, y, x + 40 + dx, y + 30], o % 2, track[o]))
        for _ in range(clutter):
            x = int(rng.randint(0, 300))
            hyps.append(([x, 600, x + 30, 630], 0, nxt))
            nxt += 1
        out.append((truths, hyps))
    return out


@pytest.mark.parametrize("seed", range(4))
def test_idtp_equals_the_minimum_of_fn_plus_fp_on_the_dummy_node_graph(seed):
    scene = lanes(seed)
    st = TE.new_state(16, 128)
    prm = TE.params()
    n_o, n_h = np.zeros(16, np.int64), np.zeros(128, np.int64)
    for truths, hyps in scene:
        TE.step(st, *arrays(truths, hyps, K=16, G=16), prm)
        for _, _, o in truths:
            n_o[o] += 1
        for _, _, h in hyps:
            n_h[h] += 1
    r, f = scores(st)
    assert not any(f.values()) and r["num_switches"] > 0 and np.array_equal(st["present"], n_o) and r["num_hypotheses"] == n_h.sum()
    os_, hs = np.flatnonzero(n_o), np.flatnonzero(n_h)
    c = st["c"][np.ix_(os_, hs)].astype(np.int64)
    no, nh, inf = len(os_), len(hs), 10 ** 9
    graph = np.full((no + nh, no + nh), inf, np.int64)
    graph[:no, :nh] = (n_o[os_][:, None] - c) + (n_h[hs][None, :] - c)        # identity o explained by track h: its FN plus its FP
    graph[:no, nh:][np.eye(no, dtype=bool)] = n_o[os_]                         # identity o unexplained: all of it FN
    graph[no:, :nh][np.eye(nh, dtype=bool)] = n_h[hs]                          # track h explains nobody: all of it FP
    graph[no:, nh:] = 0
    rr, cc = linear_sum_assignment(graph)
    total = int(graph[rr, cc].sum())
    assert total == n_o.sum() + n_h.sum() - 2 * r["idtp"] == r["idfn"] + r["idfp"]
    print(f"seed {seed}: IDTP {r['idtp']} of {r['num_objects']} objects and {r['num_hypotheses']} hypotheses, IDF1 {r['idf1']:.4f}, "
          f"MOTA {r['mota']:.4f}, {r['num_switches']} switches")


def test_state_block_round_trip():
    st, _ = play(lanes(0, nobj=6, frames=5), state=TE.new_state(7, 40))        # an odd max_gt_ids: the block is padded to 8 bytes
    block = TE.pack(st)
    assert block.size == TE.state_bytes(7, 40) == V.state_bytes(7, 40) == 8 * 16 + 20 * 7 + 4 * 7 * 40 + 4
    back = TE.unpack(block, 7, 40)
    assert all(np.array_equal(back[k], st[k]) for k in st) and not TE.pack(TE.new_state(7, 40)).any()


# ---- ABI and surface ----------------------------------------------------------------------------------------------------------------------
NEW = ("cvx_mot_state_bytes", "cvx_mot_workspace_bytes", "cvx_mot_frames", "cvx_mot_summary")


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name in NEW:
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
    assert [len(L.PROTOTYPES[n][1]) for n in NEW] == [3, 1, 15, 6]
    assert "#define CVX_ABI_VERSION 6" in header and L.ABI_VERSION == 6
    for text in ("cvx_mot_stream_header", "cvx_mot_params", "#define CVX_MOT_FRAME_CAP 1024", "#define CVX_MOT_MAX_GT_IDS 1024",
                 "#define CVX_MOT_MAX_TRACK_IDS 4096", "#define CVX_MOT_HEADER_WORDS 16", "#define CVX_MOT_TABLE_WORDS 24"):
        assert text in header
    assert ctypes.sizeof(V.MotParams) == 24 and (V.HEADER_WORDS, V.TABLE_WORDS) == (len(TE.HEAD), TE.TABLE_WORDS) == (16, 24)
    assert (V.FRAME_CAP, V.MAX_GT_IDS, V.MAX_TRACK_IDS) == (TE.FRAME_CAP, TE.MAX_GT_IDS, TE.MAX_TRACK_IDS) == (1024, 1024, 4096)
    assert V.TABLE[:22] == TE.TABLE[:22]
    assert "track_eval.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    if lib is not None:
        lib.cvx_mot_state_bytes.restype = lib.cvx_mot_workspace_bytes.restype = ctypes.c_int64
        assert lib.cvx_mot_state_bytes(3, 1024, 4096) == 3 * V.state_bytes(1024, 4096) == 3 * (128 + 20 * 1024 + 4 * 1024 * 4096)
        assert lib.cvx_mot_state_bytes(2, 7, 40) == 2 * TE.state_bytes(7, 40)
        assert lib.cvx_mot_state_bytes(1, 1025, 4096) == 0 and lib.cvx_mot_state_bytes(1, 1024, 4097) == 0 and lib.cvx_mot_state_bytes(0, 4, 4) == 0
        assert lib.cvx_mot_workspace_bytes(2) == 2 * 4 * 1024 * 1024 and lib.cvx_mot_workspace_bytes(0) == 0
    assert T.DEFAULTS == dict(high=0.5, new_score=0.6, iou_high=0.2, iou_low=0.5, alpha=0.75, beta=0.25, min_hits=3, max_age=30,
                              class_agnostic=False)                          # the tracker's defaults are not this change's to move


def test_results_and_report_from_a_table_row():
    st, _ = play([([(A, 0, 0)], [(A, 0, 1)])] * 4 + [([(A, 0, 0)], [(A, 0, 2)])] * 6)
    table = TE.summary([st])
    assert V.results_of(table[0]) == TE.results(table[0]) == V.results_of(table[1]) and V.flags_of(table[0]) == TE.flags(table[0])
    for key in ("mota", "motp", "idf1", "idp", "idr", "num_objects", "num_matches", "num_misses", "num_false_positives", "num_switches",
                "num_fragmentations", "mostly_tracked", "partially_tracked", "mostly_lost", "idtp", "idfp", "idfn"):
        assert key in V.results_of(table[0])
    text = V.format_report({"streams": [V.results_of(table[0])], "overall": V.results_of(table[1])})
    lines = text.splitlines()
    assert lines[2].split()[:6] == ["stream", "mota", "motp", "idf1", "idp", "idr"] and lines[3].split()[:4] == ["0", "0.900000", "1.000000", "0.600000"]
    assert lines[4].split()[0] == "overall" and len(lines) == 5


def test_evaluator_refuses_bad_parameters_and_the_cpu():
    for bad in (dict(streams=0), dict(streams=1.5), dict(iou=1.5), dict(iou=-0.1), dict(iou=NAN), dict(max_gt_ids=0), dict(max_gt_ids=1025),
                dict(max_track_ids=4097), dict(max_track_ids=0), dict(max_track_ids=2.5)):
        with pytest.raises(ValueError):
            V.TrackingEvaluator("cpu", **bad)
    with pytest.raises(CvxError):
        V.TrackingEvaluator("cpu")
    sig = inspect.signature(V.TrackingEvaluator.__init__).parameters
    assert [(k, p.default) for k, p in list(sig.items())[2:]] == [("streams", 1), ("iou", 0.5), ("class_agnostic", False), ("max_gt_ids", 1024),
                                                                  ("max_track_ids", 4096)]
    assert list(inspect.signature(V.TrackingEvaluator.add_frames).parameters)[1:] == ["rows", "counts", "ids", "gt", "gt_counts", "frame_stream"]
    for name in ("reset", "get_results", "write_report"):
        assert callable(getattr(V.TrackingEvaluator, name))


def test_evaluate_tracking_on_the_four_detectors_and_not_on_deeplab():
    from configs import CenternetConfig, DeeplabV3PlusConfig, SsdConfig, Yolo7Config, Yolo8DetConfig
    from core.algorithms.base import Detector
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from core.algorithms.ssd import Ssd
    from core.algorithms.yolo_v7 import YOLOv7
    from core.algorithms.yolo_v8 import YOLOv8
    sig = inspect.signature(Detector.evaluate_tracking).parameters
    assert [(k, p.default) for k, p in sig.items()][1:] == [("model", inspect.Parameter.empty), ("sequence", inspect.Parameter.empty),
                                                           ("out_root", inspect.Parameter.empty), ("tracker", None), ("batch_size", 8), ("tiled", None)]
    frame_ = torch.zeros(200, 300, 3, dtype=torch.uint8)
    for cls, cfg in ((YOLOv8, Yolo8DetConfig), (YOLOv7, Yolo7Config), (Ssd, SsdConfig), (CenterNetA, CenternetConfig)):
        with pytest.raises(CvxError):                                         # no CPU path
            cls(cfg(), "cpu").evaluate_tracking(None, [(frame_, torch.zeros(0, 6))], "unused")
    cfg = DeeplabV3PlusConfig()
    cfg.arch.backbone_pretrained = False
    with pytest.raises(CvxError, match="no detections to track"):
        DeeplabV3PlusA(cfg, "cpu").evaluate_tracking(None, [(frame_, torch.zeros(0, 6))], "unused")
