"""numpy restatement of the tracking rules of csrc/track.hip (include/cvx_engine.h): plain fp32, one rounded operation
per line.  The association is the literal greedy walk over the sorted pairs, where the kernel runs rounds of mutual best matches -- the
restatement is independent of that structure.  ``draw_tracks`` restates ``cvx_draw_tracks`` over the shared parts of
tests/render_restatement.py."""
import numpy as np

import render_restatement as RS
from computervision.pytorch_amd import render as R

TRACK_CAP = 1024
F = np.float32
DEFAULTS = dict(high=0.5, new_score=0.6, iou_high=0.2, iou_low=0.5, alpha=0.75, beta=0.25, min_hits=3, max_age=30, class_agnostic=False)


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return {**DEFAULTS, **kw}


def new_state():
    """one stream: no tracks, frame 0, next id 0.  A track is a dict(id, hits, miss, cls, p, v)."""
    return {"frame": 0, "next_id": 0, "tracks": []}


def iou_matrix(a, b):
    """box_overlap.h:iou_value of every box of a (T, 4) with every box of b (D, 4): fp32, every operation rounded on its own (0 / 0 is
    NaN, which passes no threshold)"""
    a, b = np.asarray(a, F).reshape(-1, 1, 4), np.asarray(b, F).reshape(1, -1, 4)
    with np.errstate(all="ignore"):
        w = np.fmin(a[..., 2], b[..., 2]) - np.fmax(a[..., 0], b[..., 0])
        w = np.fmax(F(0), w)
        h = np.fmin(a[..., 3], b[..., 3]) - np.fmax(a[..., 1], b[..., 1])
        h = np.fmax(F(0), h)
        inter = w * h
        area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        total = area_a + area_b
        union = total - inter
        out = inter / union
    assert out.dtype == F
    return out


def iou_value(a, b):
    return iou_matrix(a, b)[0, 0]


def greedy(tracks, cand_tracks, rows, cand_rows, threshold, agnostic):
    """the pairs (index into tracks, row index) the greedy walk takes over the candidate pairs sorted by (IoU descending, track id
    ascending, row index ascending)"""
    cand_tracks, cand_rows = list(cand_tracks), list(cand_rows)
    if not cand_tracks or not cand_rows:
        return []
    iou = iou_matrix([tracks[t]["p"] for t in cand_tracks], rows[cand_rows, :4])
    ok = iou > F(threshold)
    if not agnostic:
        ok &= np.array([tracks[t]["cls"] for t in cand_tracks], F)[:, None] == rows[cand_rows, 5][None, :]
    pairs = sorted((-float(iou[i, j]), tracks[cand_tracks[i]]["id"], cand_rows[j], cand_tracks[i]) for i, j in zip(*np.nonzero(ok)))
    used_t, used_d, taken = set(), set(), []
    for _, _, d, t in pairs:
        if t not in used_t and d not in used_d:
            used_t.add(t)
            used_d.add(d)
            taken.append((t, d))
    return taken


def step(state, rows, n, prm):
    """one frame of one stream: changes ``state`` in place and returns (ids (K) int32, overflow count)"""
    rows = np.asarray(rows, F).reshape(-1, 6)
    K = len(rows)
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
            t["p"] = (t["p"] + t["v"]).astype(F)
    # 3. split
    valid = [d for d in range(n) if not np.isnan(rows[d, :4]).any()]
    high = [d for d in valid if rows[d, 4] >= F(prm["high"])]
    low = [d for d in valid if not rows[d, 4] >= F(prm["high"])]
    # 4. stage 1, 5. stage 2
    first = greedy(tracks, range(len(tracks)), rows, high, prm["iou_high"], prm["class_agnostic"])
    matched = {t for t, _ in first}
    rest = [t for t in range(len(tracks)) if t not in matched and tracks[t]["hits"] >= min_hits and tracks[t]["miss"] == 0]
    second = greedy(tracks, rest, rows, low, prm["iou_low"], prm["class_agnostic"])
    # 6. update
    with np.errstate(all="ignore"):
        for t, d in first + second:
            k = tracks[t]
            r = (rows[d, :4] - k["p"]).astype(F)
            k["p"] = (k["p"] + (alpha * r).astype(F)).astype(F)
            k["v"] = (k["v"] + (beta * r).astype(F)).astype(F)
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
        kept.append({"id": state["next_id"], "hits": 1, "miss": 0, "cls": F(rows[d, 5]), "p": rows[d, :4].copy(), "v": np.zeros(4, F)})
        if 1 >= min_hits or frame <= min_hits:
            ids[d] = state["next_id"]
        state["next_id"] += 1
    state["tracks"] = kept
    return ids, overflow


def run(states, rows, counts, prm, frame_stream=None):
    """``cvx_track_update`` over a batch: states is the list of the streams' states -> (ids (B, K) int32, overflow count)"""
    rows = np.asarray(rows, F)
    B, K = rows.shape[:2]
    ids = np.full((B, K), -1, np.int32)
    overflow = 0
    for b in range(B):
        s = 0 if frame_stream is None else int(frame_stream[b])
        if s < 0 or s >= len(states):
            overflow += 1
            continue
        ids[b], ov = step(states[s], rows[b], counts[b], prm)
        overflow += ov
    return ids, overflow


def tracks_by_id(state):
    """the live tracks sorted by id, as ``Tracker.tracks`` returns them"""
    ts = sorted(state["tracks"], key=lambda k: k["id"])
    return {"id": np.array([k["id"] for k in ts], np.int32), "box": np.array([k["p"] for k in ts], F).reshape(-1, 4),
            "velocity": np.array([k["v"] for k in ts], F).reshape(-1, 4), "cls": np.array([k["cls"] for k in ts], F),
            "hits": np.array([k["hits"] for k in ts], np.int32), "miss": np.array([k["miss"] for k in ts], np.int32)}


# ---- drawing ------------------------------------------------------------------------------------------------------------------------------
def track_label(track_id, cls):
    return f"{int(track_id) % 1000000}:{int(cls)}"


def track_layers(h, w, row, label, thickness=2, font_scale=2):
    """``render_restatement.box_layers`` with the label given: (outline mask, tag mask, text mask) or None"""
    if any(F(v) != F(v) for v in row[:4]):
        return None
    x0, y0, x1, y1 = (RS.trunc_coord(v) for v in row[:4])
    if x1 < x0 or y1 < y0:
        return None
    yy, xx = np.mgrid[0:h, 0:w]
    g, s = thickness // 2, (thickness + 1) // 2
    outer = (xx >= x0 - g) & (xx <= x1 + g) & (yy >= y0 - g) & (yy <= y1 + g)
    inner = (xx >= x0 + s) & (xx <= x1 - s) & (yy >= y0 + s) & (yy <= y1 - s)
    fs = font_scale
    tag_w, tag_h = (6 * len(label) + 1) * fs, 9 * fs
    tx, ty = x0, (y0 - tag_h if y0 - tag_h >= 0 else y0)
    tag = (xx >= tx) & (xx < tx + tag_w) & (yy >= ty) & (yy < ty + tag_h)
    text = np.zeros((h, w), bool)
    for k, ch in enumerate(label):
        for gy, bits in enumerate(R.FONT[ch]):
            for gx in range(5):
                if bits >> (4 - gx) & 1:
                    px, py = tx + fs + k * 6 * fs + gx * fs, ty + fs + gy * fs
                    text |= (xx >= px) & (xx < px + fs) & (yy >= py) & (yy < py + fs)
    return outer & ~inner, tag, text


def draw_tracks(frame, rows, ids, count, lut=None, thickness=2, font_scale=2):
    """frame (h, w, 3) uint8 with the rows[:count] whose id is not negative painted, as a new array; also the mask of painted pixels"""
    lut = R.palette(256) if lut is None else np.asarray(lut, np.uint8)
    out = np.array(frame, copy=True)
    h, w = out.shape[:2]
    painted = np.zeros((h, w), bool)
    rows = np.asarray(rows, F).reshape(-1, 6)
    for d in range(max(int(count), 0)):
        if int(ids[d]) < 0:
            continue
        cls = min(max(RS.trunc_coord(rows[d, 5]), 0), R.MAX_CLASS)
        layers = track_layers(h, w, rows[d], track_label(ids[d], cls), thickness, font_scale)
        if layers is None:
            continue
        outline, tag, text = layers
        colour = lut[(int(ids[d]) + 1) % len(lut)].astype(np.int64)
        out[outline] = colour
        out[tag] = colour * 7 // 10
        out[text] = 0 if int(colour.sum()) > 382 else 255
        painted |= outline | tag | text
    return out, painted
