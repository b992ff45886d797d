"""numpy restatement of the tracking-evaluation rules of csrc/track_eval.hip (include/cvx_engine.h): CLEAR-MOT per
frame and the identity measures at the end, sequential, with the literal assignment solver in the kernel's order (rows inserted one by
one, the lowest column on a tie in every arg min; numpy only spans the columns, where the kernel has one lane each).  The state of a
stream is held in the arrays of the device's state block, so ``pack`` gives the block's bytes and ``unpack`` reads one."""
import numpy as np

import track_restatement as TS

F = np.float32
FRAME_CAP, MAX_GT_IDS, MAX_TRACK_IDS, MAT_LDS = 1024, 1024, 4096, 16384
BIG = 1 << 27
INF = (2 ** 63 - 1) // 4
HEAD = ("frames", "objects", "hypotheses", "matches", "misses", "false_positives", "switches", "fragmentations", "cost", "flag_nan",
        "flag_dup_row", "flag_dup_gt", "flag_identity", "flag_track", "flag_frame", "flag_excess")
H = {name: k for k, name in enumerate(HEAD)}
TABLE = HEAD[:9] + ("mostly_tracked", "partially_tracked", "mostly_lost", "idtp") + HEAD[9:] + ("identities", "tracks", "zero0", "zero1")
TABLE_WORDS = 24
assert len(TABLE) == TABLE_WORDS
PER_IDENTITY = ("mem", "last", "present", "matched", "gap")


def params(iou=0.5, class_agnostic=False):
    return {"iou": F(iou), "class_agnostic": bool(class_agnostic)}


def new_state(max_gt_ids=MAX_GT_IDS, max_track_ids=MAX_TRACK_IDS):
    """one stream: nothing seen"""
    st = {"head": np.zeros(len(HEAD), np.int64), "c": np.zeros((max_gt_ids, max_track_ids), np.int32)}
    for name in PER_IDENTITY:
        st[name] = np.zeros(max_gt_ids, np.int32)
    return st


def state_bytes(max_gt_ids, max_track_ids):
    return (8 * len(HEAD) + 20 * max_gt_ids + 4 * max_gt_ids * max_track_ids + 7) & ~7


def pack(state):
    """the stream's state block as the device holds it"""
    gi, ti = state["c"].shape
    raw = b"".join([state["head"].astype("<i8").tobytes()] + [state[k].astype("<i4").tobytes() for k in PER_IDENTITY] + [state["c"].astype("<i4").tobytes()])
    out = np.zeros(state_bytes(gi, ti), np.uint8)
    out[:len(raw)] = np.frombuffer(raw, np.uint8)
    return out


def unpack(block, max_gt_ids, max_track_ids):
    """reads one stream's state block (uint8 array of state_bytes)"""
    block = np.ascontiguousarray(block, np.uint8)
    assert block.size == state_bytes(max_gt_ids, max_track_ids)
    st = {"head": block[:8 * len(HEAD)].view("<i8").astype(np.int64)}
    off = 8 * len(HEAD)
    for name in PER_IDENTITY:
        st[name] = block[off:off + 4 * max_gt_ids].view("<i4").astype(np.int32)
        off += 4 * max_gt_ids
    st["c"] = block[off:off + 4 * max_gt_ids * max_track_ids].view("<i4").astype(np.int32).reshape(max_gt_ids, max_track_ids)
    return st


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
def solve(cost):
    """Minimum-cost assignment of the n rows of ``cost`` (n, m >= n) int64 to n of the columns, by shortest augmenting paths with potentials,
    rows inserted in order, the lowest column on a tie.  Returns p (m): the row of each column, -1 free."""
    cost = np.asarray(cost, np.int64)
    n, m = cost.shape
    assert n <= m
    u, v, p = np.zeros(n, np.int64), np.zeros(m, np.int64), np.full(m, -1, np.int64)
    for i in range(n):
        minv, used, way = np.full(m, INF, np.int64), np.zeros(m, bool), np.full(m, -1, np.int64)
        j0, i0 = -1, i
        while True:
            cur = cost[i0] - u[i0] - v
            better = ~used & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            slack = np.where(used, INF, minv)
            j1 = int(np.argmin(slack))                       # the first of the minima
            delta = slack[j1]
            assert delta < INF
            u[p[used]] += delta                              # distinct rows, none of them row i
            v[used] -= delta
            minv[~used] -= delta
            u[i] += delta
            used[j1] = True
            j0 = j1
            if p[j0] < 0:
                break
            i0 = p[j0]
        while j0 >= 0:
            jp = way[j0]
            p[j0] = i if jp < 0 else p[jp]
            j0 = jp
    return p


def assign(cost):
    """``cost`` (a, b) integers, -1 forbidden: the pairs (row, column, cost) of the assignment with the most allowed pairs and, among those,
    the least sum, as the solver finds it: the smaller side drives (the rows when both are equal), forbidden cells cost BIG and their pairs
    are dropped.  The pairs come in column order of the solver."""
    cost = np.asarray(cost, np.int64)
    assert cost.ndim == 2
    a, b = cost.shape
    if a == 0 or b == 0:
        return []
    flip = a > b
    mat = cost.T if flip else cost
    p = solve(np.where(mat < 0, BIG, mat))
    pairs = []
    for j in range(mat.shape[1]):
        i = int(p[j])
        if i >= 0 and mat[i, j] >= 0:
            pairs.append((j, i, int(mat[i, j])) if flip else (i, j, int(mat[i, j])))
    return pairs


# ---- a frame ------------------------------------------------------------------------------------------------------------------------------
def pair_costs(gbox, gcls, hbox, hcls, prm):
    """(G, H) int64: the cost of every allowed pair, -1 where the gate forbids it"""
    if len(gbox) == 0 or len(hbox) == 0:
        return np.zeros((len(gbox), len(hbox)), np.int64)
    iou = TS.iou_matrix(gbox, hbox)
    with np.errstate(invalid="ignore"):
        allowed = iou >= prm["iou"]                          # a NaN never passes
    if not prm["class_agnostic"]:
        allowed &= np.asarray(gcls, F).reshape(-1, 1) == np.asarray(hcls, F).reshape(1, -1)
    away = F(1) - iou
    scaled = away * F(65536)
    assert scaled.dtype == F
    cost = np.full(iou.shape, -1, np.int64)
    cost[allowed] = np.rint(scaled[allowed]).astype(np.int64)
    return cost


def step(state, rows, count, ids, gt, gt_count, prm):
    """one frame of a stream: rows (K, 6), ids (K), gt (G, 6).  Returns the matches [(identity, track id, cost)] in ground-truth order."""
    head = state["head"]
    gi, ti = state["c"].shape
    rows, gt, ids = np.asarray(rows, F), np.asarray(gt, F), np.asarray(ids)
    if not (0 <= count <= len(rows) and 0 <= gt_count <= len(gt)):
        head[H["flag_frame"]] += 1
        return []
    head[H["frames"]] += 1
    frame = int(head[H["frames"]])
    # the hypotheses
    cand = [d for d in range(count) if ids[d] >= 0]
    if len(cand) > FRAME_CAP:
        head[H["flag_excess"]] += len(cand) - FRAME_CAP
        cand = cand[:FRAME_CAP]
    hyp, seen = [], set()
    for d in cand:
        if np.isnan(rows[d, :4]).any():
            head[H["flag_nan"]] += 1
        elif ids[d] >= ti:
            head[H["flag_track"]] += 1
        elif int(ids[d]) in seen:
            head[H["flag_dup_row"]] += 1
        else:
            seen.add(int(ids[d]))
            hyp.append(d)
    # the ground truths
    tru, seen = [], set()
    for g in range(gt_count):
        fi = gt[g, 5]
        if np.isnan(gt[g, :4]).any():
            head[H["flag_nan"]] += 1
        elif not (fi >= 0 and fi < gi and fi == np.trunc(fi)):
            head[H["flag_identity"]] += 1
        elif int(fi) in seen:
            head[H["flag_dup_gt"]] += 1
        else:
            seen.add(int(fi))
            tru.append(g)
    gid, hid = [int(gt[g, 5]) for g in tru], [int(ids[d]) for d in hyp]
    cost = pair_costs(gt[tru, :4], gt[tru, 4], rows[hyp, :4], rows[hyp, 5], prm)
    for t, s in zip(*np.nonzero(cost >= 0)):
        state["c"][gid[t], hid[s]] += 1
    # 1. continuity
    gmatch, hmatch, gcost, gnew = [-1] * len(tru), [-1] * len(hyp), [0] * len(tru), [False] * len(tru)
    remembered = [int(state["mem"][o]) for o in gid]
    for t, o in enumerate(gid):
        state["present"][o] += 1
        if remembered[t] > 0 and state["last"][o] == frame - 1 and remembered[t] - 1 in hid:
            s = hid.index(remembered[t] - 1)
            if cost[t, s] >= 0:
                gmatch[t], hmatch[s], gcost[t] = s, t, int(cost[t, s])
    # 2. the assignment of the rest
    rest_g = [t for t in range(len(tru)) if gmatch[t] < 0]
    rest_h = [s for s in range(len(hyp)) if hmatch[s] < 0]
    for i, j, c in assign(cost[np.ix_(rest_g, rest_h)] if rest_g and rest_h else np.zeros((len(rest_g), len(rest_h)))):
        t, s = rest_g[i], rest_h[j]
        gmatch[t], hmatch[s], gcost[t], gnew[t] = s, t, c, True
    # 3, 4. the counters
    out, hits = [], 0
    for t, o in enumerate(gid):
        s = gmatch[t]
        if s < 0:
            state["gap"][o] = 1
            continue
        hits += 1
        head[H["cost"]] += gcost[t]
        if gnew[t] and remembered[t] > 0 and remembered[t] != hid[s] + 1:
            head[H["switches"]] += 1
        state["mem"][o], state["last"][o] = hid[s] + 1, frame
        if state["matched"][o] > 0 and state["gap"][o] != 0:
            head[H["fragmentations"]] += 1
        state["matched"][o] += 1
        state["gap"][o] = 0
        out.append((o, hid[s], gcost[t]))
    head[H["objects"]] += len(tru)
    head[H["hypotheses"]] += len(hyp)
    head[H["matches"]] += hits
    head[H["misses"]] += len(tru) - hits
    head[H["false_positives"]] += len(hyp) - hits
    return out


def run(states, rows, counts, ids, gt, gt_counts, prm, frame_stream=None):
    """``cvx_mot_frames`` on a batch over ``states`` (a list, one per stream)"""
    for b in range(len(rows)):
        s = 0 if frame_stream is None else int(frame_stream[b])
        if not 0 <= s < len(states):
            states[0]["head"][H["flag_frame"]] += 1
            continue
        step(states[s], rows[b], int(counts[b]), ids[b], gt[b], int(gt_counts[b]), prm)


# ---- the summary --------------------------------------------------------------------------------------------------------------------------
def idtp_of(c):
    """the maximum of sum c[o, h] over the partial one-to-one matchings, with the solver on the non-empty rows and columns"""
    c = np.asarray(c, np.int64)
    r, k = np.flatnonzero((c > 0).any(1)), np.flatnonzero((c > 0).any(0))
    if len(r) == 0:
        return 0, 0
    sub = c[np.ix_(r, k)]
    sub = sub if len(r) <= len(k) else sub.T
    p = solve(-sub)
    return int(sum(sub[int(p[j]), j] for j in range(sub.shape[1]) if p[j] >= 0)), len(k)


def summary_row(state):
    """one row of ``cvx_mot_summary``'s table, (24) int64"""
    row = np.zeros(TABLE_WORDS, np.int64)
    row[:9] = state["head"][:9]
    n, k = state["present"].astype(np.int64), state["matched"].astype(np.int64)
    seen = n > 0
    mt = seen & (5 * k >= 4 * n)
    ml = seen & ~mt & (5 * k < n)
    row[9], row[10], row[11] = mt.sum(), (seen & ~mt & ~ml).sum(), ml.sum()
    row[12], row[21] = idtp_of(state["c"])
    row[13:20] = state["head"][9:16]
    row[20] = seen.sum()
    return row


def summary(states):
    """the whole table (streams + 1, 24): the last row is the sum"""
    rows = [summary_row(s) for s in states]
    return np.stack(rows + [np.sum(rows, axis=0)])


def ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def results(row):
    """the scores of one table row, in double from the integers"""
    r = {name: int(v) for name, v in zip(TABLE, row)}
    obj, hyp, tp = r["objects"], r["hypotheses"], r["idtp"]
    out = {"mota": 1.0 - ratio(r["misses"] + r["false_positives"] + r["switches"], obj), "motp": 1.0 - ratio(r["cost"], 65536 * r["matches"]),
           "idf1": ratio(2 * tp, obj + hyp), "idp": ratio(tp, hyp), "idr": ratio(tp, obj),
           "num_frames": r["frames"], "num_objects": obj, "num_hypotheses": hyp, "num_matches": r["matches"], "num_misses": r["misses"],
           "num_false_positives": r["false_positives"], "num_switches": r["switches"], "num_fragmentations": r["fragmentations"],
           "mostly_tracked": r["mostly_tracked"], "partially_tracked": r["partially_tracked"], "mostly_lost": r["mostly_lost"],
           "idtp": tp, "idfp": hyp - tp, "idfn": obj - tp}
    return out


def flags(row):
    return {name[5:]: int(v) for name, v in zip(TABLE, row) if name.startswith("flag_")}
