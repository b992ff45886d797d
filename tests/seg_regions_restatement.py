"""Connected-component regions of a label map, restated in plain numpy: the specification of ``cvx_seg_regions``
(csrc/seg_regions.hip).  No scipy: a raster scan with a union-find whose links always point to the lower linear index, so a region's root
is its seed.  Every quantity is an integer or one rounded division of integers; the kernel is held to this file bit for bit."""
import numpy as np

CAPACITY = 8192


def class_mask(classes):
    """(256) bool: ``"foreground"`` (all but 0 and 255), ``"all"``, or an iterable of labels"""
    m = np.zeros(256, bool)
    if isinstance(classes, str):
        if classes == "all":
            m[:] = True
        elif classes == "foreground":
            m[1:255] = True
        else:
            raise ValueError(classes)
    else:
        m[[int(c) for c in classes]] = True
    return m


def roots_of(labels, selected, connectivity):
    """(h, w) int64: the seed (smallest linear index) of every selected pixel's region, -1 for the others"""
    assert connectivity in (4, 8)
    h, w = labels.shape
    lab, sel = labels.reshape(-1).tolist(), selected.reshape(-1).tolist()
    parent = list(range(h * w))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for y in range(h):
        for x in range(w):
            p = y * w + x
            if not sel[p]:
                continue
            near = []
            if x > 0:
                near.append(p - 1)
            if y > 0:
                near.append(p - w)
                if connectivity == 8:
                    if x > 0:
                        near.append(p - w - 1)
                    if x + 1 < w:
                        near.append(p - w + 1)
            for q in near:
                if sel[q] and lab[q] == lab[p]:
                    a, b = find(p), find(q)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    out = np.full(h * w, -1, np.int64)
    for p in range(h * w):
        if sel[p]:
            out[p] = find(p)
    return out.reshape(h, w)


def quantise(conf):
    """q per pixel: (uint32) rintf(fminf(fmaxf(c, 0), 1) * 65535), a NaN gives 0 (fmax / fmin return the other operand)"""
    c = np.asarray(conf, np.float32)
    return np.rint(np.fmin(np.fmax(c, np.float32(0.0)), np.float32(1.0)) * np.float32(65535.0)).astype(np.int64)


def regions(labels, classes="foreground", connectivity=8, min_area=64, max_det=300, conf=None, fill=None):
    """One frame.  Returns a dict: rows (max_det, 6) float32, count, total, areas / seeds (max_det) int32, region_map (h, w) int32, clean_map
    (h, w) uint8 or None, and ``roots`` (h, w) int64, the partition itself (the seed of every selected pixel, -1 elsewhere)."""
    labels = np.asarray(labels)
    assert labels.dtype == np.uint8 and labels.ndim == 2
    h, w = labels.shape
    rows = np.zeros((max_det, 6), np.float32)
    areas, seeds = np.full(max_det, -1, np.int32), np.full(max_det, -1, np.int32)
    mask = class_mask(classes)
    selected = mask[labels]
    roots = roots_of(labels, selected, connectivity)
    flat = roots.reshape(-1)
    pix = np.nonzero(flat >= 0)[0]
    seed_list, inverse, area = np.unique(flat[pix], return_inverse=True, return_counts=True)
    ys, xs = pix // w, pix % w
    n = len(seed_list)
    min_x, max_x, max_y = np.full(n, w, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    np.minimum.at(min_x, inverse, xs)
    np.maximum.at(max_x, inverse, xs)
    np.maximum.at(max_y, inverse, ys)
    min_y = seed_list // w
    if conf is not None:
        S = np.zeros(n, np.int64)
        np.add.at(S, inverse, quantise(conf).reshape(-1)[pix])
        score = (S.astype(np.float64) / (area.astype(np.float64) * 65535.0)).astype(np.float32)
    else:
        score = np.ones(n, np.float32)
    cand = np.nonzero(area >= min_area)[0]
    total = len(cand)
    order = cand[np.lexsort((seed_list[cand], -area[cand]))]          # area descending, then seed ascending
    region_map = np.full((h, w), -1, np.int32)
    clean = None
    if fill is not None:
        clean = labels.copy()
        small = np.zeros(n, bool)
        small[area < min_area] = True
        clean.reshape(-1)[pix[small[inverse]]] = fill
    if total > CAPACITY:
        return dict(rows=rows, count=-1, total=total, areas=areas, seeds=seeds, region_map=region_map, clean_map=clean, roots=roots)
    kept = order[:max_det]
    k = len(kept)
    rows[:k, 0], rows[:k, 1] = min_x[kept], min_y[kept]
    rows[:k, 2], rows[:k, 3] = max_x[kept] + 1, max_y[kept] + 1
    rows[:k, 4] = score[kept]
    rows[:k, 5] = labels.reshape(-1)[seed_list[kept]]
    areas[:k], seeds[:k] = area[kept], seed_list[kept]
    stamp = np.full(n, -1, np.int32)
    stamp[kept] = np.arange(k, dtype=np.int32)
    region_map.reshape(-1)[pix] = stamp[inverse]
    return dict(rows=rows, count=k, total=total, areas=areas, seeds=seeds, region_map=region_map, clean_map=clean, roots=roots)


# ---- the seeded maps the tests share -------------------------------------------------------------------------------------------------------
def blobby(h, w, seed, classes=3, blur=3):
    """A seeded (h, w) uint8 map of ``classes`` labels 0 .. classes - 1 in blobs: the arg max of box-blurred noise planes"""
    rng = np.random.RandomState(seed)
    z = rng.rand(classes, h + 2 * blur, w + 2 * blur)
    c = np.cumsum(np.cumsum(np.pad(z, ((0, 0), (1, 0), (1, 0))), 1), 2)
    k = 2 * blur + 1
    s = c[:, k:, k:] - c[:, :-k, k:] - c[:, k:, :-k] + c[:, :-k, :-k]
    return np.argmax(s, 0).astype(np.uint8)


def serpentine(h, w, value=1):
    """A one-pixel-wide path through the frame: every other row is full, joined alternately at the right and the left end"""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = value
    for i, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if i % 2 == 0 else 0] = value
    return m


def spiral(h, w, value=1):
    """A one-pixel-wide rectangular spiral from the top-left corner towards the centre, one unset pixel between its turns: a walker
    goes straight while the pixel after the next is free, and turns right when it is not"""
    m = np.zeros((h, w), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = value

    def free(yy, xx):
        return 0 <= yy < h and 0 <= xx < w and m[yy, xx] == 0

    def open_ahead(dy, dx):
        ny, nx = y + dy, x + dx
        beyond = (ny + dy, nx + dx)
        return free(ny, nx) and (not (0 <= beyond[0] < h and 0 <= beyond[1] < w) or m[beyond] == 0)

    while True:
        if not open_ahead(dy, dx):
            dy, dx = dx, -dy                                          # right, down, left, up
            if not open_ahead(dy, dx):
                return m
        y, x = y + dy, x + dx
        m[y, x] = value


def comb(h, w, value=1, pitch=2, offset=0):
    """Vertical teeth every ``pitch`` columns from ``offset``, joined only along the last row"""
    m = np.zeros((h, w), np.uint8)
    m[:h - 1, offset::pitch] = value
    m[h - 1, offset:] = value
    return m


def two_combs(h, w):
    """Two interleaved combs: class 1 has its teeth in the even columns and is joined along the last row, class 2 has them in the odd
    columns and is joined along the first row"""
    m = np.zeros((h, w), np.uint8)
    m[1:h, 0::2] = 1
    m[h - 1, :] = 1
    m[0:h - 2, 1::2] = 2
    m[0, :] = 2
    return m


def checkerboard(h, w, value=1):
    m = np.zeros((h, w), np.uint8)
    m[0::2, 0::2] = value
    m[1::2, 1::2] = value
    return m
