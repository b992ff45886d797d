"""CPU: the optional tracker rules as tests/track_model_restatement.py states them -- the Kalman motion model and the
minimum-cost association -- against hand-derived answers, against scipy's assignment and against tests/track_restatement.py where the two
must agree; the new symbols; the surface that needs no GPU.  No quality threshold is asserted: quality is a figure in the profile."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_eval_restatement as ER
import track_model_restatement as TM
import track_restatement as TS
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import track as T
from test_track_cpu import feed as feed_plain
from test_track_cpu import frame, lanes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# a model whose numbers come out by hand on a box 16 high: (r_pos s)^2 = (q_pos s)^2 = (q_vel s)^2 = 1, birth at Pxx = Pvv = 1
HAND = dict(motion="kalman", q_pos=1 / 16, q_vel=1 / 16, r_pos=1 / 16, init_pos=1.0, init_vel=1.0)


def feed(state, frames, mdl, **kw):
    prm = TM.params(**kw)
    return [TM.step(state, rows, n, prm, mdl)[0][:max(n, 0)].tolist() for rows, n in frames]


def gains_of(monkeypatch):
    """records (frame, kx) of every gain the restatement works out"""
    seen, plain = [], TM.kalman_gains

    def recording(k, mdl):
        kx, kv = plain(k, mdl)
        seen.append(float(kx))
        return kx, kv

    monkeypatch.setattr(TM, "kalman_gains", recording)
    return seen


# ---- the Kalman model by hand ---------------------------------------------------------------------------------------------------------------
def test_kalman_a_birth_and_two_updates_by_hand():
    mdl = TM.model(**HAND)
    st = TM.new_state()
    assert feed(st, [frame(([10, 10, 50, 26], 0.9, 1))], mdl) == [[0]]
    (k,) = st["tracks"]
    assert k["cov"].tolist() == [1, 0, 1] and k["cov"].dtype == np.float32 and k["v"].tolist() == [0, 0, 0, 0]
    # frame 2, predict: Pxx = 1 + (0 + 0 + 1 + 1) = 3, Pxv = 0 + 1, Pvv = 1 + 1; e = 3 + 1: kx = 3/4, kv = 1/4; the box moved 4 to the right
    assert feed(st, [frame(([14, 10, 54, 26], 0.9, 1))], mdl) == [[0]]
    (k,) = st["tracks"]
    assert k["p"].tolist() == [13, 10, 53, 26] and k["v"].tolist() == [1, 0, 1, 0]
    # Pvv = 2 - 1/4 * 1, Pxv = 1 - 3/4 * 1, Pxx = 3 - 3/4 * 3
    assert k["cov"].tolist() == [0.75, 0.25, 1.75]
    # frame 3, predict: a = 0.25 + 0.25 + 1.75 + 1 = 3.25: Pxx = 4, Pxv = 0.25 + 1.75 = 2, Pvv = 2.75; e = 5; seen 4 to the right of [14, 54]
    assert feed(st, [frame(([18, 10, 58, 26], 0.9, 1))], mdl) == [[0]]
    (k,) = st["tracks"]
    kx, kv = F(4) / F(5), F(2) / F(5)
    assert k["p"].tolist() == [F(14) + kx * F(4), 10, F(54) + kx * F(4), 26] and k["v"].tolist() == [F(1) + kv * F(4), 0, F(1) + kv * F(4), 0]
    assert k["cov"].tolist() == [F(4) - kx * F(4), F(2) - kx * F(2), F(2.75) - kv * F(2)]
    assert (k["id"], k["hits"], k["miss"]) == (0, 3, 0) and k["p"].dtype == k["v"].dtype == k["cov"].dtype == np.float32


def test_kalman_gain_falls_while_matched_and_rises_over_a_gap(monkeypatch):
    seen = gains_of(monkeypatch)
    mdl = TM.model(motion="kalman")                                          # ByteTrack's weights
    st = TM.new_state()
    box = frame(([10, 10, 50, 90], 0.9, 0))
    feed(st, [box] * 12, mdl)
    assert len(seen) == 11 and seen[0] > seen[10] and all(a >= b for a, b in zip(seen, seen[1:]))      # first match after the birth: the highest
    settled = seen[10]
    # Pxx after the birth 0.01 h^2, Pvv (10 / 160)^2 h^2, q 0.0025 h^2: kx = 0.01640625 / 0.01890625
    assert abs(seen[0] - 0.01640625 / 0.01890625) < 1e-6
    feed(st, [frame()] * 10 + [box], mdl)                                    # ten frames unseen, then back
    assert len(seen) == 12 and st["tracks"][0]["id"] == 0 and st["tracks"][0]["hits"] == 13
    print(f"kx after the birth {seen[0]:.4f}, settled {settled:.4f}, after a gap of 10 frames {seen[11]:.4f}")
    assert seen[11] > settled


def test_kalman_a_box_of_zero_height_takes_min_scale():
    mdl = TM.model(motion="kalman", min_scale=2.0)
    assert TM.noise_scale([10, 10, 50, 10], mdl) == 2 and TM.noise_scale([10, 10, 50, 5], mdl) == 2 and TM.noise_scale([0, 1, 0, 9], mdl) == 8
    assert TM.noise_scale([10, float("inf"), 50, float("inf")], mdl) == 2      # inf - inf: fmaxf gives the other operand
    st = TM.new_state()
    feed(st, [frame(([10, 10, 50, 10], 0.9, 0))], mdl)
    a, b = F(2.0) * F(1 / 20) * F(2), F(10.0) * F(1 / 160) * F(2)
    assert st["tracks"][0]["cov"].tolist() == [a * a, 0, b * b]


def test_kalman_ignores_alpha_and_beta():
    mdl = TM.model(motion="kalman")
    a, b = TM.new_state(), TM.new_state()
    frames = [frame(([10 + 3 * f, 10, 50 + 3 * f, 60], 0.9, 0)) for f in range(5)]
    assert feed(a, frames, mdl) == feed(b, frames, mdl, alpha=0.1, beta=0.9)
    assert all(np.array_equal(x["p"], y["p"]) and np.array_equal(x["v"], y["v"]) for x, y in zip(a["tracks"], b["tracks"]))


# ---- the optimal association by hand --------------------------------------------------------------------------------------------------------
def shifted(x):
    return [x, 0, x + 40, 40]                                                # two such boxes d apart: IoU (40 - d) / (40 + d)


def test_optimal_gives_two_pairs_where_greedy_gives_one():
    # tracks at 0 and 10, rows at 4 and -8: IoU 36/44 = 0.82, 32/48 = 0.67 (track 0), 34/46 = 0.74, 22/58 = 0.38 < 0.4 (track 1)
    first = frame((shifted(0), 0.9, 0), (shifted(10), 0.9, 0))
    second = frame((shifted(4), 0.9, 0), (shifted(-8), 0.9, 0))
    st = TM.new_state()
    assert feed(st, [first, second], TM.model(), iou_high=0.4) == [[0, 1], [0, 2]]      # greedy: 0.82 first, track 1 is left with nothing
    assert [k["id"] for k in st["tracks"]] == [0, 2]
    assert feed_plain(TS.new_state(), [first, second], iou_high=0.4) == [[0, 1], [0, 2]]
    st = TM.new_state()
    assert feed(st, [first, second], TM.model(assign="optimal"), iou_high=0.4) == [[0, 1], [1, 0]]
    assert [(k["id"], k["hits"]) for k in st["tracks"]] == [(0, 2), (1, 2)] and st["next_id"] == 2


def test_optimal_rule_on_cost_matrices_by_hand():
    # the same count, the lesser sum: 20 + 15 < 10 + 40
    assert TM.assign_cost([[10, 20], [15, 40]]) == ([], [(1, 0), (0, 1)])
    # an exact tie: tracks inserted in ascending id, the lowest row wins
    assert TM.assign_cost([[5, 5], [5, 5]]) == ([], [(0, 0), (1, 1)])
    assert TM.assign_cost([[5, 5, 5]] * 2) == ([], [(0, 0), (1, 1)]) and sorted(TM.assign_cost([[5, 5]] * 3)[1]) == [(0, 0), (1, 1)]
    # (a) a pair alone on both sides is taken without the solver; the rest goes to it
    assert TM.assign_cost([[7, -1, -1], [-1, 3, 4], [-1, 5, 6]]) == ([(0, 0)], [(1, 1), (2, 2)])
    assert TM.assign_cost([[7, -1], [-1, 9]]) == ([(0, 0), (1, 1)], [])
    # ... not when its row has another track: count first (two pairs), then the sum
    assert TM.assign_cost([[7, -1], [1, 9]]) == ([], [(0, 0), (1, 1)])
    # (b) candidates without an allowed pair
    assert TM.assign_cost([[-1, -1], [-1, -1]]) == ([], []) and TM.assign_cost([[-1, 4, -1], [-1, -1, -1]]) == ([(0, 1)], [])
    assert TM.assign_cost(np.zeros((0, 3))) == ([], []) and TM.assign_cost(np.zeros((3, 0))) == ([], [])
    # more tracks than rows: the rows drive
    assert sorted(TM.assign_cost([[9, 9], [1, 9], [9, 1]])[1]) == [(1, 0), (2, 1)]


def test_optimal_class_gate_and_nan_boxes():
    opt = TM.model(assign="optimal")
    st = TM.new_state()
    assert feed(st, [frame((shifted(0), 0.9, 1)), frame((shifted(2), 0.9, 2), (shifted(6), 0.9, 1))], opt) == [[0], [1, 0]]
    st = TM.new_state()                                                      # class-agnostic: the closer row, whatever its class
    assert feed(st, [frame((shifted(0), 0.9, 1)), frame((shifted(2), 0.9, 2), (shifted(6), 0.9, 1))], opt, class_agnostic=True) == [[0], [0, 1]]
    assert st["tracks"][0]["cls"] == 2
    nan = float("nan")
    st = TM.new_state()                                                      # a NaN row is no candidate; a NaN track box allows no pair
    assert feed(st, [frame((shifted(0), 0.9, 0)), frame(([nan, 0, 40, 40], 0.9, 0), (shifted(1), 0.9, 0))], opt) == [[0], [-1, 0]]
    st["tracks"][0]["p"][0] = nan
    assert feed(st, [frame((shifted(1), 0.9, 0))], opt) == [[1]] and [k["id"] for k in st["tracks"]] == [1]


# ---- against scipy --------------------------------------------------------------------------------------------------------------------------
def seeded_cost(rng, a, b, kind):
    cost = rng.randint(0, 65537, (a, b)).astype(np.int64)
    if kind == "ties":
        cost = rng.randint(0, 4, (a, b)).astype(np.int64) * 1000
    forbid = rng.uniform(size=(a, b)) < (1.0 if kind == "none" else rng.choice([0.0, 0.3, 0.7, 0.95, 0.98]))
    cost[forbid] = -1
    if kind == "dup" and a > 1 and b > 1:
        cost[rng.randint(a)] = cost[rng.randint(a)]
        cost[:, rng.randint(b)] = cost[:, rng.randint(b)]
    return cost


def test_optimal_rule_has_the_count_and_the_sum_of_scipys_optimum():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.RandomState(7)
    shapes = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (7, 3), (16, 16), (33, 20), (40, 64), (90, 70), (70, 90)]
    skipped = 0
    for a, b in shapes:
        for kind in ("plain", "dup", "ties", "none", "plain"):
            cost = seeded_cost(rng, a, b, kind)
            alone, solved = TM.assign_cost(cost)
            pairs = alone + solved
            assert len({i for i, _ in pairs}) == len({j for _, j in pairs}) == len(pairs) and all(cost[i, j] >= 0 for i, j in pairs)
            ri, ci = linear_sum_assignment(np.where(cost < 0, ER.BIG, cost))
            keep = cost[ri, ci] >= 0
            assert len(pairs) == int(keep.sum()), (a, b, kind)
            assert sum(int(cost[i, j]) for i, j in pairs) == int(cost[ri, ci][keep].sum()), (a, b, kind)
            skipped += len(alone)
    assert skipped > 10                                                      # step (a) was exercised


# ---- against the plain restatement, and invariants ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_default_model_equals_the_plain_restatement_bit_for_bit(seed):
    a, b, prm, mdl = TS.new_state(), TM.new_state(), TS.params(), TM.model()
    for rows, n, _ in lanes(seed):
        ia, oa = TS.step(a, rows, n, prm)
        ib, ob = TM.step(b, rows, n, prm, mdl)
        assert np.array_equal(ia, ib) and oa == ob
    ta, tb = TS.tracks_by_id(a), TM.tracks_by_id(b, mdl)
    assert set(ta) == set(tb) and a["frame"] == b["frame"] and a["next_id"] == b["next_id"]
    for key in ta:
        assert np.array_equal(ta[key].view(np.uint32) if ta[key].dtype == np.float32 else ta[key], tb[key].view(np.uint32) if tb[key].dtype == np.float32 else tb[key]), key


@pytest.mark.parametrize("motion,assign", TM.COMBINATIONS)
def test_invariants_on_the_lane_scene(motion, assign):
    st, prm, mdl = TM.new_state(), TM.params(), TM.model(motion=motion, assign=assign)
    labelled = 0
    for rows, n, _ in lanes(1):
        ids, ov = TM.step(st, rows, n, prm, mdl)
        got = ids[ids >= 0]
        labelled += len(got)
        assert ov == 0 and (ids[n:] == -1).all()
        assert len(set(got.tolist())) == len(got)                            # an id labels at most one row of a frame
        assert (got < st["next_id"]).all()
        slot_ids = [k["id"] for k in st["tracks"]]
        assert slot_ids == sorted(slot_ids) and len(set(slot_ids)) == len(slot_ids)      # slots are sorted by id: compaction keeps, births append
        assert all(("cov" in k) == (motion == "kalman") for k in st["tracks"])
    assert labelled > 150


# ---- ABI and surface ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name in ("cvx_track_ext_bytes", "cvx_track_update_model"):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
    assert len(L.PROTOTYPES["cvx_track_ext_bytes"][1]) == 1 and len(L.PROTOTYPES["cvx_track_update_model"][1]) == 13
    assert len(L.PROTOTYPES["cvx_track_update"][1]) == 11                    # the old entry is as it was
    assert "#define CVX_ABI_VERSION 6" in header and "typedef struct cvx_track_model" in header
    for name, value in (("CVX_TRACK_MOTION_ALPHA_BETA", 0), ("CVX_TRACK_MOTION_KALMAN", 1), ("CVX_TRACK_ASSIGN_GREEDY", 0),
                        ("CVX_TRACK_ASSIGN_OPTIMAL", 1), ("CVX_TRACK_OPTIMAL_MAX_DET", 4096)):
        assert f"#define {name} {value}\n" in header
    assert ctypes.sizeof(T.TrackModelStruct) == 32 and ctypes.sizeof(T.TrackParams) == 40
    assert [f[0] for f in T.TrackModelStruct._fields_] == list(TM.MODEL_DEFAULTS)
    assert T.MOTIONS == {"alpha_beta": 0, "kalman": 1} and T.ASSIGNS == {"greedy": 0, "optimal": 1}
    assert T.EXT_BYTES == 16 * T.TRACK_CAP and T.OPTIMAL_MAX_DET == TM.OPTIMAL_MAX_DET == 4096
    if lib is not None:
        lib.cvx_track_ext_bytes.restype, lib.cvx_track_ext_bytes.argtypes = ctypes.c_int64, [ctypes.c_int32]
        assert [lib.cvx_track_ext_bytes(s) for s in (0, 1, 3)] == [0, 16384, 3 * 16384]
        assert lib.cvx_abi_version() == 6
    csrc = os.path.join(ROOT, "computervision.pytorch_amd", "csrc")
    assert "solve(" in open(os.path.join(csrc, "assign_solver.h")).read()
    for name in ("track.hip", "track_eval.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "assign_solver.h"' in text and "struct Solver" not in text


def test_the_old_defaults_and_the_model_defaults():
    assert T.DEFAULTS == dict(high=0.5, new_score=0.6, iou_high=0.2, iou_low=0.5, alpha=0.75, beta=0.25, min_hits=3, max_age=30,
                              class_agnostic=False) == TS.DEFAULTS
    assert T.check_params() == T.DEFAULTS
    m = T.TrackModel()
    assert {k: getattr(m, k) for k in TM.MODEL_DEFAULTS} == TM.MODEL_DEFAULTS
    s = T.TrackModel(motion="kalman", assign="optimal", min_scale=4).struct()
    assert (s.motion, s.assign, s.q_pos, s.q_vel, s.min_scale) == (1, 1, F(1 / 20), F(1 / 160), 4)
    assert T.TrackModel.of(None) is None and T.TrackModel.of(m) is m and T.TrackModel.of({"motion": "kalman"}).motion == "kalman"
    assert "kalman" in repr(T.TrackModel(motion="kalman"))


def test_bad_model_values_raise_before_the_device_check():
    nan, inf = float("nan"), float("inf")
    bad = [dict(motion="ekf"), dict(assign="hungarian"), dict(motion=1), dict(q_pos=-0.1), dict(q_vel=nan), dict(r_pos=inf), dict(init_pos=-1),
           dict(init_vel=nan), dict(min_scale=0), dict(min_scale=-1.0), dict(min_scale=nan), dict(q_pos="1"), dict(gain=1)]
    for kw in bad:
        with pytest.raises((ValueError, TypeError)) as e:
            T.TrackModel(**kw)
        assert e.type is (TypeError if "gain" in kw else ValueError), kw
        if "gain" not in kw:
            with pytest.raises(ValueError):
                T.Tracker("cpu", model=kw)                                   # a dict of the keywords, before the device check
    with pytest.raises(ValueError):
        T.Tracker("cpu", model="kalman")
    with pytest.raises(ValueError):
        T.Tracker("cpu", model=T.TrackModel(), speed=1)                      # the old parameters are still checked
    with pytest.raises(CvxError):
        T.Tracker("cpu", model=T.TrackModel(motion="kalman"))               # no CPU path
    T.TrackModel(q_pos=0, q_vel=0, r_pos=0, init_pos=0, init_vel=0)           # zero is a weight
    # K > 4096 under the optimal association: a shape check
    with pytest.raises(ValueError, match="4096"):
        T.TrackModel(assign="optimal").check_rows(4097)
    T.TrackModel(assign="optimal").check_rows(4096)
    T.TrackModel(motion="kalman").check_rows(100000)
