"""numpy restatement of the optional rules of csrc/track.hip (include/cvx_engine.h): the Kalman motion model and the
minimum-cost association of ``cvx_track_update_model``.  Plain fp32, one rounded operation per line, over the parts of
tests/track_restatement.py (the frame rules, the IoU, the greedy walk) and tests/track_eval_restatement.py (the solver) that do not change.
A track is ``track_restatement``'s dict plus ``cov``: (Pxx, Pxv, Pvv) float32 under the Kalman model, absent otherwise."""
import numpy as np

import track_eval_restatement as ER
import track_restatement as TS

F = np.float32
TRACK_CAP = TS.TRACK_CAP
OPTIMAL_MAX_DET = 4096
MODEL_DEFAULTS = dict(motion="alpha_beta", assign="greedy", q_pos=1 / 20, q_vel=1 / 160, r_pos=1 / 20, init_pos=2.0, init_vel=10.0, min_scale=1.0)
COMBINATIONS = [(m, a) for m in ("alpha_beta", "kalman") for a in ("greedy", "optimal")]

params, new_state = TS.params, TS.new_state


def model(**kw):
    unknown = set(kw) - set(MODEL_DEFAULTS)
    assert not unknown, unknown
    m = {**MODEL_DEFAULTS, **kw}
    assert m["motion"] in ("alpha_beta", "kalman") and m["assign"] in ("greedy", "optimal")
    return m


# ---- the Kalman model ---------------------------------------------------------------------------------------------------------------------
def noise_scale(box, mdl):
    """s = max(y2 - y1, min_scale): the height of the box, min_scale at the least (fmaxf: min_scale for a NaN)"""
    with np.errstate(all="ignore"):
        h = F(box[3]) - F(box[1])
        return np.fmax(h, F(mdl["min_scale"]))


def kalman_birth(box, mdl):
    s = noise_scale(box, mdl)
    with np.errstate(all="ignore"):
        a = F(mdl["init_pos"]) * F(mdl["r_pos"])
        a = a * s
        pxx = a * a
        b = F(mdl["init_vel"]) * F(mdl["q_vel"])
        b = b * s
        pvv = b * b
    return np.array([pxx, F(0), pvv], F)


def kalman_predict(k, mdl):
    """the covariance one frame on, at the scale of the box BEFORE the move (the caller moves the box)"""
    s = noise_scale(k["p"], mdl)
    pxx, pxv, pvv = k["cov"]
    with np.errstate(all="ignore"):
        a = pxv + pxv
        a = a + pvv
        b = F(mdl["q_pos"]) * s
        b = b * b
        a = a + b
        pxx = pxx + a
        pxv = pxv + pvv
        c = F(mdl["q_vel"]) * s
        c = c * c
        pvv = pvv + c
    k["cov"] = np.array([pxx, pxv, pvv], F)


def kalman_gains(k, mdl):
    """(kx, kv) of a matched track, at the scale of the predicted box"""
    s = noise_scale(k["p"], mdl)
    pxx, pxv, _ = k["cov"]
    with np.errstate(all="ignore"):
        e = F(mdl["r_pos"]) * s
        e = e * e
        e = pxx + e
        kx = pxx / e
        kv = pxv / e
    assert kx.dtype == kv.dtype == F
    return kx, kv


def kalman_shrink(k, kx, kv):
    pxx, pxv, pvv = k["cov"]
    with np.errstate(all="ignore"):
        t = kv * pxv
        pvv = pvv - t
        t = kx * pxv
        pxv = pxv - t
        t = kx * pxx
        pxx = pxx - t
    k["cov"] = np.array([pxx, pxv, pvv], F)


# ---- the optimal association --------------------------------------------------------------------------------------------------------------
def allowed_costs(tracks, cand_tracks, rows, cand_rows, threshold, agnostic):
    """(T, D) int64 over the candidates as given: section 7ac's integer cost of every allowed pair, -1 where the pair is forbidden"""
    iou = TS.iou_matrix([tracks[t]["p"] for t in cand_tracks], rows[cand_rows, :4])
    with np.errstate(invalid="ignore"):
        ok = iou > F(threshold)                                  # strict; a NaN never passes
    if not agnostic:
        ok &= np.array([tracks[t]["cls"] for t in cand_tracks], F)[:, None] == rows[cand_rows, 5][None, :]
    away = F(1) - iou
    scaled = away * F(65536)
    assert scaled.dtype == F
    cost = np.full(iou.shape, -1, np.int64)
    cost[ok] = np.rint(scaled[ok]).astype(np.int64)
    return cost


def assign_cost(cost):
    """the rule on a cost matrix (tracks in ascending id, rows in ascending index; -1 forbidden) -> (pairs (i, j) of (a), pairs of (c))"""
    cost = np.asarray(cost, np.int64)
    ok = cost >= 0
    tdeg, rdeg = ok.sum(1), ok.sum(0)
    # (a) an allowed pair that is the only one of its track and of its row
    alone = [(int(i), int(j)) for i, j in zip(*np.nonzero(ok)) if tdeg[i] == 1 and rdeg[j] == 1]
    gone_t, gone_r = {i for i, _ in alone}, {j for _, j in alone}
    # (b) candidates without an allowed pair are set aside; (c) the rest, each side in order, to the solver
    rest_t = [i for i in range(cost.shape[0]) if tdeg[i] > 0 and i not in gone_t]
    rest_r = [j for j in range(cost.shape[1]) if rdeg[j] > 0 and j not in gone_r]
    solved = [(rest_t[i], rest_r[j]) for i, j, _ in ER.assign(cost[np.ix_(rest_t, rest_r)])] if rest_t and rest_r else []
    return alone, solved


def optimal(tracks, cand_tracks, rows, cand_rows, threshold, agnostic):
    """``track_restatement.greedy``'s arguments and result, by the minimum-cost assignment"""
    cand_tracks = sorted(cand_tracks, key=lambda t: tracks[t]["id"])
    cand_rows = sorted(cand_rows)
    if not cand_tracks or not cand_rows:
        return []
    alone, solved = assign_cost(allowed_costs(tracks, cand_tracks, rows, cand_rows, threshold, agnostic))
    return [(cand_tracks[i], cand_rows[j]) for i, j in alone + solved]


# ---- a frame ------------------------------------------------------------------------------------------------------------------------------
def step(state, rows, n, prm, mdl):
    """``track_restatement.step`` with the model's choices: one frame of one stream -> (ids (K) int32, overflow count)"""
    rows = np.asarray(rows, F).reshape(-1, 6)
    K = len(rows)
    kalman = mdl["motion"] == "kalman"
    match = optimal if mdl["assign"] == "optimal" else TS.greedy
    assert not (mdl["assign"] == "optimal" and K > OPTIMAL_MAX_DET)
    overflow = 0
    n = int(n)
    if n < 0 or n > K:
        overflow, n = 1, 0
    alpha, beta, min_hits = F(prm["alpha"]), F(prm["beta"]), int(prm["min_hits"])
    # 1. count and clear
    state["frame"] += 1
    frame = state["frame"]
    ids = np.full(K, -1, np.int32)
    tracks = state["tracks"]
    # 2. predict
    with np.errstate(all="ignore"):
        for t in tracks:
            if kalman:
                kalman_predict(t, mdl)
            t["p"] = (t["p"] + t["v"]).astype(F)
    # 3. split
    valid = [d for d in range(n) if not np.isnan(rows[d, :4]).any()]
    high = [d for d in valid if rows[d, 4] >= F(prm["high"])]
    low = [d for d in valid if not rows[d, 4] >= F(prm["high"])]
    # 4. stage 1, 5. stage 2
    first = match(tracks, range(len(tracks)), rows, high, prm["iou_high"], prm["class_agnostic"])
    matched = {t for t, _ in first}
    rest = [t for t in range(len(tracks)) if t not in matched and tracks[t]["hits"] >= min_hits and tracks[t]["miss"] == 0]
    second = match(tracks, rest, rows, low, prm["iou_low"], prm["class_agnostic"])
    # 6. update
    with np.errstate(all="ignore"):
        for t, d in first + second:
            k = tracks[t]
            kx, kv = kalman_gains(k, mdl) if kalman else (alpha, beta)
            r = (rows[d, :4] - k["p"]).astype(F)
            k["p"] = (k["p"] + (kx * r).astype(F)).astype(F)
            k["v"] = (k["v"] + (kv * r).astype(F)).astype(F)
            if kalman:
                kalman_shrink(k, kx, kv)
            k["hits"] += 1
            k["miss"] = 0
            k["cls"] = F(rows[d, 5])
            if k["hits"] >= min_hits or frame <= min_hits:
                ids[d] = k["id"]
    # 7. unmatched tracks
    matched |= {t for t, _ in second}
    kept = []
    for i, k in enumerate(tracks):
        if i not in matched:
            if k["hits"] < min_hits:
                continue
            k["miss"] += 1
            if k["miss"] > int(prm["max_age"]):
                continue
        kept.append(k)
    # 8. births
    taken_rows = {d for _, d in first}
    for d in high:
        if d in taken_rows or not rows[d, 4] >= F(prm["new_score"]):
            continue
        if len(kept) >= TRACK_CAP:
            overflow += 1
            continue
        born = {"id": state["next_id"], "hits": 1, "miss": 0, "cls": F(rows[d, 5]), "p": rows[d, :4].copy(), "v": np.zeros(4, F)}
        if kalman:
            born["cov"] = kalman_birth(rows[d, :4], mdl)
        kept.append(born)
        if 1 >= min_hits or frame <= min_hits:
            ids[d] = state["next_id"]
        state["next_id"] += 1
    state["tracks"] = kept
    return ids, overflow


def run(states, rows, counts, prm, mdl, frame_stream=None):
    """``cvx_track_update_model`` over a batch: states is the list of the streams' states -> (ids (B, K) int32, overflow count)"""
    rows = np.asarray(rows, F)
    B, K = rows.shape[:2]
    ids = np.full((B, K), -1, np.int32)
    overflow = 0
    for b in range(B):
        s = 0 if frame_stream is None else int(frame_stream[b])
        if s < 0 or s >= len(states):
            overflow += 1
            continue
        ids[b], ov = step(states[s], rows[b], counts[b], prm, mdl)
        overflow += ov
    return ids, overflow


def tracks_by_id(state, mdl):
    """the live tracks sorted by id, as ``Tracker.tracks`` returns them under the model"""
    out = TS.tracks_by_id(state)
    if mdl["motion"] == "kalman":
        ts = sorted(state["tracks"], key=lambda k: k["id"])
        out["cov"] = np.array([k["cov"] for k in ts], F).reshape(-1, 3)
    return out
