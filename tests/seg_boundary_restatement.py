"""Boundary metrics of label maps, restated in plain numpy: the specification of ``cvx_seg_boundary``
(csrc/seg_boundary.hip).  Written straight from the definitions -- every distance is a scan of the square window around the pixel, ring
by ring, with no separable trick -- so that it shares no idea with the kernels.  Every count is an integer; the kernels are held to this
file bit for bit.  ``RULES`` names the decisions a reader could take the other way; the mutants of tests/test_seg_boundary_cpu.py flip
them one at a time."""
import math

import numpy as np

VOID = 255
OUTSIDE = -1
MAX_WIDTH, MAX_WIDTHS = 64, 8

RULES = dict(trimap_edge=False,     # the picture border does not count in the trimap band
             biou_edge=True,        # ... and does in the Boundary IoU bands
             strict=False,          # a pixel at distance exactly d_k is inside the band (<=)
             void_is_class0=False,  # a void target pixel is no class
             contour4=False,        # the contour looks at all 8 neighbours
             void_pred=True,        # a prediction under a void target is void too
             cityblock=False)       # distances are Chebyshev


def ring(d, cityblock=False):
    """the offsets (dy, dx) at distance exactly ``d`` from the centre"""
    if d == 0:
        return [(0, 0)]
    if cityblock:
        return [(dy, dx) for dy in range(-d, d + 1) for dx in {d - abs(dy), abs(dy) - d}]
    return [(dy, dx) for dy in range(-d, d + 1) for dx in range(-d, d + 1) if max(abs(dy), abs(dx)) == d]


def voided(pred, target, nc, rules=RULES):
    """(G', P') int16, VOID where the rules say so"""
    g, p = target.astype(np.int16), pred.astype(np.int16)
    if rules["void_is_class0"]:
        g = np.where(g < nc, g, 0)
    gv = np.where(g < nc, g, VOID)
    pv = np.where(p < nc, p, VOID)
    if rules["void_pred"]:
        pv = np.where(gv != VOID, pv, VOID)
    return gv.astype(np.int16), pv.astype(np.int16)


def shifted(padded, pad, dy, dx, h, w):
    return padded[pad + dy:pad + dy + h, pad + dx:pad + dx + w]


def distance(m, dmax, edge, cityblock=False):
    """D_M^e: (h, w) int64, 0 on VOID pixels, else the smallest d in 1 .. dmax whose window holds another label (or, with ``edge``, leaves
    the picture), dmax + 1 when none does"""
    h, w = m.shape
    padded = np.full((h + 2 * dmax, w + 2 * dmax), OUTSIDE, np.int16)
    padded[dmax:dmax + h, dmax:dmax + w] = m
    out = np.where(m == VOID, 0, dmax + 1).astype(np.int64)
    for d in range(1, dmax + 1):
        hit = np.zeros((h, w), bool)
        for dy, dx in ring(d, cityblock):
            q = shifted(padded, dmax, dy, dx, h, w)
            hit |= ((q != OUTSIDE) & (q != m)) | (edge & (q == OUTSIDE))
        out[(out == dmax + 1) & hit] = d
    return out


def contour(m, rules=RULES):
    """the class of the pixels of K_M, VOID elsewhere"""
    if rules["contour4"]:
        d = distance(m, 1, False, cityblock=True)
    else:
        d = distance(m, 1, False, rules["cityblock"])
    return np.where((m != VOID) & (d == 1), m, VOID).astype(np.int16)


def nearest(ka, kb, dmax, cityblock=False):
    """N_{A->B}: (h, w) int64, -1 off the contour ``ka``, else the distance to the nearest pixel of ``kb`` of the same class, dmax + 1 when
    none lies within dmax"""
    h, w = ka.shape
    padded = np.full((h + 2 * dmax, w + 2 * dmax), VOID, np.int16)
    padded[dmax:dmax + h, dmax:dmax + w] = kb
    on = ka != VOID
    out = np.where(on, dmax + 1, -1).astype(np.int64)
    for d in range(0, dmax + 1):
        hit = np.zeros((h, w), bool)
        for dy, dx in ring(d, cityblock):
            hit |= on & (shifted(padded, dmax, dy, dx, h, w) == ka)
        out[(out == dmax + 1) & hit] = d
    return out


def counts(pred, target, nc, widths, rules=RULES):
    """One frame: ``pred`` / ``target`` (h, w) uint8, ``widths`` the K widths.  Returns ``trimap`` (K, nc, nc), ``biou`` (K, nc, 3) (I, Gb,
    Pb), ``bf`` (K, nc, 4) (mp, cp, mg, cg), all int64, and ``planes`` (6, h, w) uint8."""
    widths = [int(d) for d in widths]
    assert 1 <= nc <= 255 and 1 <= len(widths) <= MAX_WIDTHS and all(1 <= d <= MAX_WIDTH for d in widths)
    assert pred.shape == target.shape and pred.dtype == target.dtype == np.uint8
    K, dmax, cb = len(widths), max(widths), rules["cityblock"]
    gv, pv = voided(pred, target, nc, rules)
    dge, dgn = distance(gv, dmax, True, cb), distance(gv, dmax, False, cb)
    dpe, dpn = distance(pv, dmax, True, cb), distance(pv, dmax, False, cb)
    kg, kp = contour(gv, rules), contour(pv, rules)
    npg, ngp = nearest(kp, kg, dmax, cb), nearest(kg, kp, dmax, cb)
    within = (lambda a, d: a < d) if rules["strict"] else (lambda a, d: a <= d)
    trimap = np.zeros((K, nc, nc), np.int64)
    biou = np.zeros((K, nc, 3), np.int64)
    bf = np.zeros((K, nc, 4), np.int64)
    both = (gv != VOID) & (pv != VOID)
    for k, d in enumerate(widths):
        band = both & within(dge if rules["trimap_edge"] else dgn, d)
        np.add.at(trimap[k], (gv[band], pv[band]), 1)
        gband = (gv != VOID) & within(dge if rules["biou_edge"] else dgn, d)
        pband = (pv != VOID) & within(dpe if rules["biou_edge"] else dpn, d)
        for c in range(nc):
            gb, pb = gband & (gv == c), pband & (pv == c)
            biou[k, c] = (int((gb & pb).sum()), int(gb.sum()), int(pb.sum()))
            onp, ong = kp == c, kg == c
            bf[k, c] = (int((onp & within(npg, d)).sum()), int(onp.sum()), int((ong & within(ngp, d)).sum()), int(ong.sum()))
    planes = np.stack([dge, dgn, dpe, dpn, npg + 1, ngp + 1]).astype(np.uint8)
    return dict(trimap=trimap, biou=biou, bf=bf, planes=planes)


def batch_counts(preds, targets, nc, widths_per_frame, rules=RULES):
    """the three tables summed over the frames; ``widths_per_frame``: one list of K widths per frame"""
    total = None
    for p, g, wd in zip(preds, targets, widths_per_frame):
        c = counts(p, g, nc, wd, rules)
        if total is None:
            total = {k: c[k].copy() for k in ("trimap", "biou", "bf")}
        else:
            for k in total:
                total[k] += c[k]
    return total


def ratio_width(ratio, h, w):
    """the width of a band given as a fraction of the frame diagonal"""
    return min(max(int(math.floor(ratio * math.hypot(h, w) + 0.5)), 1), MAX_WIDTH)


def fold(trimap, biou, bf):
    """The metrics of one width from its (nc, nc), (nc, 3) and (nc, 4) tables, in double: ``(trimap mIoU, Boundary IoU, BF)`` and the
    per-class arrays (NaN where a class does not enter the mean)."""
    hist = trimap.astype(np.float64)
    diag = np.diag(hist)
    with np.errstate(divide="ignore", invalid="ignore"):
        iu = diag / (hist.sum(1) + hist.sum(0) - diag)
        i, gb, pb = (biou[:, j].astype(np.float64) for j in range(3))
        b = np.where(gb + pb > 0, i / (gb + pb - i), np.nan)
        mp, cp, mg, cg = (bf[:, j].astype(np.float64) for j in range(4))
        prec, rec = mp / cp, mg / cg
        f = np.where((mp == 0) | (mg == 0), 0.0, 2 * prec * rec / (prec + rec))
        f = np.where(cp + cg > 0, f, np.nan)

    def mean(a):
        return float(np.nanmean(a)) if np.isfinite(a).any() else float("nan")

    return (mean(iu), mean(b), mean(f)), (iu, b, f)


# ---- seeded maps ----------------------------------------------------------------------------------------------------------------------------
def blobby(h, w, seed, classes=3, void=True, cell=9):
    """a coarse random class grid blown up to (h, w); with ``void`` a one-pixel 255 outline wherever two cells of different classes meet
    along x or y, and a void rectangle"""
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, classes, ((h + cell - 1) // cell + 1, (w + cell - 1) // cell + 1))
    oy, ox = rng.randint(0, cell, 2)
    m = np.kron(coarse, np.ones((cell, cell), np.int64))[oy:oy + h, ox:ox + w].astype(np.uint8)
    if void:
        edge = np.zeros((h, w), bool)
        edge[:, 1:] |= m[:, 1:] != m[:, :-1]
        edge[1:, :] |= m[1:, :] != m[:-1, :]
        m = m.copy()
        m[edge & (rng.rand(h, w) < 0.7)] = VOID
        if h > 6 and w > 6:
            m[h // 3:h // 3 + 3, w // 4:w // 4 + 5] = VOID
    return m


def jitter(m, seed, classes, share=0.1, wild=False):
    """a prediction for the target ``m``: the map moved by one pixel with a share of the pixels redrawn; with ``wild`` a few values >= the
    class count as well.  Void target pixels become a class (a network predicts no void)."""
    rng = np.random.RandomState(seed)
    p = np.roll(m, (1, -1), (0, 1)).copy()
    p[p == VOID] = rng.randint(0, classes, int((p == VOID).sum()))
    redraw = rng.rand(*m.shape) < share
    p[redraw] = rng.randint(0, classes, int(redraw.sum()))
    if wild:
        odd = rng.rand(*m.shape) < 0.02
        p[odd] = rng.randint(classes, 256, int(odd.sum()))
    return p.astype(np.uint8)


def checkerboard(h, w, a=0, b=1):
    yy, xx = np.mgrid[:h, :w]
    return np.where((yy + xx) % 2 == 0, a, b).astype(np.uint8)


def stripes(h, w, classes=3, vertical=True):
    yy, xx = np.mgrid[:h, :w]
    return ((xx if vertical else yy) % classes).astype(np.uint8)
