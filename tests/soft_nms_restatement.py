"""``cvx_soft_nms`` (include/cvx_engine.h, csrc/soft_nms.hip) restated in plain numpy float32, one rounding per operation, and the seeded
cases tests/test_soft_nms_cpu.py and tests/test_soft_nms_gpu.py share.  No GPU dependency.  The candidate front end -- the rule, the
order, the boxes -- is ``eval_tail_cases._candidates``, the one the hard-NMS sweeps use.

``soft_nms_restated`` is the specification the kernel is compared with bit for bit.  Its switches are ways a kernel could be subtly wrong;
test_soft_nms_cpu.py shows that each of them changes the expected output of a named case.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import eval_tail_cases as T

F32 = np.float32
CAP = 16384
METHODS = ("hard", "linear", "gaussian")


def exp_neg(x):
    """E(x), the library's exp(-x): the operations of snms_exp_neg in their order, each one rounded to fp32"""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):                      # x >= 80 (an infinite x among them) is replaced below
        t = -x
        k = np.rint(t * F32(1.44269504088896341))
        r = t - k * F32(0.693359375)
        r = r - k * F32(-2.12194440e-4)
        p = np.full_like(r, F32(1) / F32(720))
        for c in (F32(1) / F32(120), F32(1) / F32(24), F32(1) / F32(6), F32(0.5), F32(1), F32(1)):
            p = p * r + c
        out = np.ldexp(p, np.clip(np.nan_to_num(k), -200, 200).astype(np.int32)).astype(F32)
    return np.where(x >= F32(80), F32(0), out).astype(F32)


def iou_value(box, area, m, others):
    """box_overlap.h:iou_value of candidate m against ``others``"""
    x1, y1, x2, y2 = (box[:, i] for i in range(4))
    w = np.maximum(F32(0), np.minimum(x2[m], x2[others]) - np.maximum(x1[m], x1[others]))
    h = np.maximum(F32(0), np.minimum(y2[m], y2[others]) - np.maximum(y1[m], y1[others]))
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / ((area[m] + area[others]) - inter)


def walk_segment(box, area, sc, pos, method, iou, sigma, min_score, tie_high=False, ge_iou=False, ge_min=False, twice=False):
    """One segment: ``pos`` are its positions, ascending.  Returns (emitted positions, final scores, decays per candidate of ``pos``, live
    candidates left when the segment stopped)."""
    s = sc[pos].astype(F32).copy()
    live = np.ones(len(pos), bool)
    decays = np.zeros(len(pos), np.int64)
    out_pos, out_s = [], []
    while True:
        ok = np.nonzero(live & (s >= 0))[0]
        if ok.size == 0:
            break
        best = ok[s[ok] == s[ok].max()]
        m = best[-1] if tie_high else best[0]
        sm = s[m]
        if method != "hard" and not (sm >= min_score if ge_min else sm > min_score):
            break
        out_pos.append(pos[m])
        out_s.append(sm)
        live[m] = False
        rest = np.nonzero(live & (s >= 0))[0]
        if rest.size == 0:
            continue
        o = iou_value(box, area, pos[m], pos[rest])
        for _ in range(2 if twice else 1):
            if method == "gaussian":
                hit = o > F32(0)
                s[rest[hit]] = s[rest[hit]] * exp_neg((o[hit] * o[hit]) / sigma)
            else:
                hit = (o >= iou) if ge_iou else (o > iou)
                if method == "hard":
                    live[rest[hit]] = False
                else:
                    s[rest[hit]] = s[rest[hit]] * (F32(1.0) - o[hit])
        decays[rest[hit]] += 1
    return np.asarray(out_pos, np.int64), np.asarray(out_s, F32), decays, int((live & (s >= 0)).sum())


def soft_nms_image(x, conf, iou, max_det, method, sigma=0.5, min_score=0.001, class_agnostic=False, xyxy=False, tie_high=False, ge_iou=False,
                   cross_class=False, no_merge=False, ge_min=False, twice=False, stats=None):
    """One block y (4 + nc, A) -> (rows (k, 6) [box, final score, cls], anchors (k,)).  Switches (the mutants): ``tie_high`` the highest
    position among equal scores; ``ge_iou`` ``>=`` at the IoU threshold; ``cross_class`` decay across classes; ``no_merge`` the segments
    concatenated in class order instead of merged; ``ge_min`` ``>=`` at ``min_score``; ``twice`` every decay applied twice."""
    assert method in METHODS
    iou, sigma, min_score = F32(iou), F32(sigma), F32(min_score)
    box, sc, cls, cand = T._candidates(np.asarray(x, F32), conf, xyxy)
    n = len(cand)
    box = box.astype(F32).reshape(n, 4)
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    one = class_agnostic or cross_class
    segments = [np.arange(n)] if one else [np.nonzero(cls == c)[0] for c in np.unique(cls)]
    pos, fin = [], []
    for seg in segments:
        if len(seg) == 0:
            continue
        p, s, decays, left = walk_segment(box, area, sc, seg, method, iou, sigma, min_score, tie_high, ge_iou, ge_min, twice)
        pos.append(p)
        fin.append(s)
        if stats is not None:
            stats.append(dict(length=len(seg), emitted=len(p), left=left, decays=decays, finals=s))
    pos = np.concatenate(pos) if pos else np.zeros(0, np.int64)
    fin = np.concatenate(fin) if fin else np.zeros(0, F32)
    if not no_merge:
        order = np.lexsort((pos, -fin.astype(np.float64)))
        pos, fin = pos[order], fin[order]
    pos, fin = pos[:max_det], fin[:max_det]
    rows = np.concatenate((box[pos], fin[:, None], cls[pos, None].astype(F32)), 1).astype(F32).reshape(-1, 6)
    return rows, cand[pos].astype(np.int64)


def soft_nms_restated(pred, conf, iou, max_det, method, overflow=(), **kw):
    """Per block of ``pred`` (B, 4 + nc, A) what ``soft_nms_image`` returns; None for a block of ``overflow`` (count -1)."""
    return tuple(None if b in overflow else soft_nms_image(x, conf, iou, max_det, method, **kw) for b, x in enumerate(np.asarray(pred, F32)))


# ----------------------------------------------------------------------------------------------------------------------------------------
# the seeded cases
# ----------------------------------------------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class SoftCase:
    name: str
    pred: np.ndarray
    n: tuple
    conf: float = 0.25
    iou: float = 0.3                 # well below the hard-NMS default: inside a cluster most pairs lie above it, so linear decays often
    max_det: int = 4096
    sigma: float = 0.5
    min_score: float = 0.001
    agnostic: tuple = (False, True)  # the class_agnostic settings the GPU sweep runs the case under
    tags: tuple = field(default_factory=tuple)

    def __hash__(self):
        return hash(self.name)


def spread_classes(pred, seed, classes):
    """``clustered`` plants its candidates in the first six classes: move each planted score to one of ``classes``"""
    pred = pred.copy()
    rng = np.random.default_rng(seed)
    for x in pred:
        for a in np.nonzero(x[4:].max(0) > 0.25)[0]:
            old, new = int(x[4:, a].argmax()), int(rng.choice(classes))
            x[4 + old, a], x[4 + new, a] = x[4 + new, a], x[4 + old, a]
    return pred


def with_duplicate(pred):
    """the second candidate becomes an exact copy of the first, same class, a lower score: IoU == 1 exactly"""
    pred = pred.copy()
    i0, i1 = np.nonzero(pred[0, 4:].max(0) > 0.25)[0][:2]
    pred[0, :, i1] = pred[0, :, i0]
    pred[0, 4 + pred[0, 4:, i0].argmax(), i1] = 0.29
    return pred, int(i0), int(i1)


def three_boxes():
    """A = [0, 0, 100, 100] with 0.9, B = [0, 0, 100, 50] with 0.8, C = [0, 25, 100, 75] with 0.7, one class of two, as (cx, cy, w, h):
    IoU(A, B) = IoU(A, C) = 0.5 exactly, IoU(B, C) = 1/3.  Linear at iou 0.4 decays B to 0.8f * 0.5f exactly (test_soft_nms_cpu.py)."""
    pred = np.zeros((1, 6, 3), F32)
    pred[0, :4] = np.array([[50, 50, 100, 100], [50, 25, 100, 50], [50, 50, 100, 50]], F32).T
    pred[0, 5] = (0.9, 0.8, 0.7)
    return pred


def _case(name, pred, n, **kw):
    n = (n,) * pred.shape[0] if isinstance(n, int) else tuple(n)
    got = T.candidate_counts(pred, kw.get("conf", 0.25))
    assert got == n, (name, got, n)
    return SoftCase(name, pred, n, **kw)


MIXED = (0, 1, 64, 700, 65)
SPREAD_CLASSES = tuple(range(0, 80, 2))          # 40 of 80 classes, an empty class between every two


@functools.lru_cache(maxsize=None)
def soft_cases() -> tuple:
    cases = []
    for k, n in enumerate((0, 1, 63, 64, 65, 129)):                      # lane and word edges of one segment (class-agnostic) and of three
        cases.append(_case(f"edge_n{n}", T.clustered(500 + k, 130, 3, n), n, tags=("edge",)))
    cases.append(_case("long_segments_700x3", T.clustered(510, 1500, 3, 700), 700, tags=("long",)))
    cases.append(_case("classes_300x40_of_80", spread_classes(T.clustered(511, 700, 80, 300), 512, SPREAD_CLASSES), 300, tags=("classes",)))
    cases.append(_case("mixed_batch", T.clustered(513, 1500, 3, MIXED), MIXED, tags=("mixed",)))
    cases.append(_case("mass_ties", T.clustered(514, 1500, 3, 900, decimals=1), 900, tags=("ties",)))
    cases.append(_case("duplicate_box", with_duplicate(T.clustered(515, 130, 3, 100))[0], 100, tags=("duplicate",)))
    cases.append(_case("duplicate_box_iou_1", with_duplicate(T.clustered(515, 130, 3, 100))[0], 100, iou=1.0, tags=("duplicate",)))
    cases.append(_case("min_score_exact", three_boxes(), 3, iou=0.4, min_score=float(F32(0.8) * F32(0.5)), tags=("min_score",)))
    cases.append(_case("min_score_0.3", T.clustered(516, 1500, 6, 700), 700, min_score=0.3, tags=("min_score",)))
    cases.append(_case("sigma_0.05", T.clustered(517, 400, 3, 300), 300, sigma=0.05, tags=("sigma",)))
    cases.append(_case("sigma_10", T.clustered(517, 400, 3, 300), 300, sigma=10.0, tags=("sigma",)))
    cases.append(_case("agnostic_3000", T.clustered(518, 4000, 3, 3000), 3000, agnostic=(True,), tags=("large",)))
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def soft_case(name: str) -> SoftCase:
    return next(c for c in soft_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def soft_reference(case: SoftCase, method: str, agnostic: bool, max_det: int = None) -> tuple:
    return soft_nms_restated(case.pred, case.conf, case.iou, case.max_det if max_det is None else max_det, method, sigma=case.sigma,
                             min_score=case.min_score, class_agnostic=agnostic)


def same(a, b) -> bool:
    """two results of ``soft_nms_restated``: anchors equal, rows equal bit for bit"""
    return all((p is None and q is None) or (p is not None and q is not None and np.array_equal(p[1], q[1]) and
                                             np.array_equal(p[0].view(np.uint32), q[0].view(np.uint32))) for p, q in zip(a, b))
