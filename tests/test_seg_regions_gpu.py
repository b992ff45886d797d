"""MI355X: connected-component regions.  ``cvx_seg_regions`` (csrc/seg_regions.hip) against the numpy restatement
(tests/seg_regions_restatement.py): rows and scores as fp32 bit patterns, counts, totals, areas, seeds, region maps and clean maps as
integers -- no tolerance exists in this feature.  The shapes are the smallest that break each mechanism of a tiled union-find with 64 x 32
tiles: paths that cross every tile border many times, a comb that top-down propagation gets wrong, every size around one and two tiles,
a frame that is one region (one hot root), the capacity of the sort and one past it.  Then ``DeeplabV3PlusA.predict_regions`` and
``segment_frames(regions=, track=)`` end to end."""
import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import render as R
from computervision.pytorch_amd import seg_regions as G
import seg_regions_restatement as SR

pytestmark = pytest.mark.gpu

T_H, T_W = 32, 64                        # the tile of csrc/seg_regions.hip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def padded(dev, host, extra, fill):
    """``host`` (h, w) on the device as a view whose rows are ``extra`` elements longer"""
    h, w = host.shape
    store = torch.full((h, w + extra), fill, dtype=torch.from_numpy(host).dtype, device=dev)
    view = store[:, :w]
    view.copy_(torch.from_numpy(host))
    assert view.stride(0) == w + extra and not view.is_contiguous()
    return view, store


def want_of(maps, regions, confs=None):
    return [SR.regions(m, regions.classes, regions.connectivity, regions.min_area, regions.max_det, None if confs is None else confs[f], regions.fill)
            for f, m in enumerate(maps)]


def assert_frame(got, f, want, what=""):
    """every output of frame ``f`` of the RegionBatch ``got`` against the restatement's dict ``want``"""
    rows, areas, seeds = got.rows[f].cpu().numpy(), got.areas[f].cpu().numpy(), got.seeds[f].cpu().numpy()
    count, total = int(got.counts[f]), int(got.total[f])
    print(f"{what} frame {f}: count {count} (want {want['count']}), total {total} (want {want['total']}), "
          f"{int((bits(rows) != bits(want['rows'])).sum())} row words differ, largest area {int(areas[0])}")
    assert (count, total) == (want["count"], want["total"]), what
    assert np.array_equal(areas, want["areas"]) and np.array_equal(seeds, want["seeds"]), what
    assert np.array_equal(bits(rows), bits(want["rows"])), what
    if got.region_maps is not None and got.region_maps[f] is not None:
        assert np.array_equal(got.region_maps[f].cpu().numpy(), want["region_map"]), what
    if got.clean_maps is not None and got.clean_maps[f] is not None:
        assert np.array_equal(got.clean_maps[f].cpu().numpy(), want["clean_map"]), what


# ---- 1. paths and combs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_paths_and_combs(dev, connectivity):
    """97 x 131 is 4 x 3 tiles, none of them whole at the far edges.  The serpentine and the spiral are single one-pixel-wide regions that
    cross the tile borders hundreds of times (the seed in the first row, the spiral's end in the centre); the comb's teeth meet only in
    the last row; the two interleaved combs are two classes that meet at opposite ends."""
    maps = [SR.serpentine(97, 131), SR.spiral(97, 131, 5), SR.comb(97, 131, 2), SR.two_combs(97, 131)]
    regions = G.SegRegions(connectivity, 1, "foreground", 16, fill=0)
    want = want_of(maps, regions)
    assert [w["total"] for w in want] == [1, 1, 1, 2] and want[0]["seeds"][0] == 0 and want[3]["areas"][:2].tolist() == [6401, 6241]
    got = G.label_regions([on(dev, m) for m in maps], regions, region_maps=True)
    for f in range(4):
        assert_frame(got, f, want[f], f"connectivity {connectivity}")
    assert int(got.overflow) == 0
    found = got.read()
    assert found[3][0].tolist() == [[0.0, 1.0, 131.0, 97.0], [0.0, 0.0, 131.0, 95.0]] and found[3][2].tolist() == [1, 2]


# ---- 2. every size around one and two tiles -------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 300), (300, 1)] + [(h, w) for h in (T_H - 1, T_H, T_H + 1, 2 * T_H + 1) for w in (T_W - 1, T_W, T_W + 1, 2 * T_W + 1)]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_sizes_around_the_tile(dev, connectivity):
    """one seeded blobby map per size, all 19 in one batch: labels 0, 1, 2 all selected, a confidence plane, both maps, a max_det that cuts
    the larger frames"""
    maps = [SR.blobby(h, w, 100 + i) for i, (h, w) in enumerate(SIZES)]
    rng = np.random.RandomState(7)
    confs = [rng.rand(h, w).astype(np.float32) for h, w in SIZES]
    regions = G.SegRegions(connectivity, 3, "all", 64, fill=9)
    want = want_of(maps, regions, confs)
    assert sum(w["total"] > 64 for w in want) >= 3 and sum(0 < w["total"] <= 64 for w in want) >= 8 and want[0]["total"] == 0
    got = G.label_regions([on(dev, m) for m in maps], regions, conf=[on(dev, c) for c in confs], region_maps=True)
    for f, hw in enumerate(SIZES):
        assert_frame(got, f, want[f], f"{hw} connectivity {connectivity}")
    assert int(got.overflow) == 0


# ---- 3. a batch of different frames, a padded view, maps for one frame only ------------------------------------------------------------------
def test_batch_of_three_with_a_padded_view_and_optional_maps(dev):
    sizes = [(70, 101), (33, 200), (90, 64)]
    maps = [SR.blobby(h, w, 200 + i, classes=4) for i, (h, w) in enumerate(sizes)]
    maps[2][40:50, 10:30] = 255
    rng = np.random.RandomState(8)
    confs = [rng.rand(h, w).astype(np.float32) for h, w in sizes]
    regions = G.SegRegions(8, 20, "foreground", 50, fill=0)
    want = want_of(maps, regions, confs)
    labels = [on(dev, m) for m in maps]
    labels[0], keep_l = padded(dev, maps[0], 3, 1)               # pitch 104: the padding holds label 1 and must connect nothing
    planes = [on(dev, c) for c in confs]
    planes[0], keep_c = padded(dev, confs[0], 5, 1.0)
    got = G.label_regions(labels, regions, conf=planes, region_maps=[False, True, False], clean_maps=[False, True, False])
    assert [m is not None for m in got.region_maps] == [False, True, False] == [m is not None for m in got.clean_maps]
    for f in range(3):
        assert_frame(got, f, want[f])
    assert (keep_l[:, 101:] == 1).all() and int(got.overflow) == 0
    # one (B, H, W) tensor is the same call
    stack = torch.stack([on(dev, maps[1]), on(dev, maps[1])])
    again = G.label_regions(stack, regions, conf=torch.stack([planes[1], planes[1]]))
    assert again.region_maps is None and len(again.clean_maps) == 2
    for f in range(2):
        assert_frame(again, f, want[1])


# ---- 4. one region over the whole frame: one hot root -------------------------------------------------------------------------------------------
def test_one_region_over_a_whole_frame(dev):
    """257 x 259 of class 1: 5 x 9 tiles whose 45 tile roots all add to pixel 0.  q = rint(1e-5 * 65535) = 1 per pixel, so S = area and the
    score is the fp32 nearest to 1 / 65535, exactly"""
    m = np.ones((257, 259), np.uint8)
    conf = np.full((257, 259), 1e-5, np.float32)
    got = G.label_regions([on(dev, m)], G.SegRegions(8, 64, "foreground", 4), conf=[on(dev, conf)], region_maps=True)
    rows = got.rows[0].cpu().numpy()
    assert int(got.counts[0]) == 1 and int(got.total[0]) == 1 and got.areas[0].tolist() == [66563, -1, -1, -1] and got.seeds[0].tolist() == [0, -1, -1, -1]
    assert np.array_equal(bits(rows[0]), bits([0.0, 0.0, 259.0, 257.0, np.float32(66563.0 / (66563.0 * 65535.0)), 1.0])) and not rows[1:].any()
    assert rows[0, 4] == np.float32(1.0 / 65535.0) and not got.region_maps[0].any()
    assert_frame(got, 0, SR.regions(m, "foreground", 8, 64, 4, conf))


# ---- 5. the capacity --------------------------------------------------------------------------------------------------------------------------
def test_exactly_the_capacity_comes_back_complete(dev):
    m = SR.checkerboard(128, 128)
    regions = G.SegRegions(4, 1, "foreground", 8192)
    got = G.label_regions([on(dev, m)], regions, region_maps=True)
    assert int(got.counts[0]) == 8192 and int(got.total[0]) == 8192 and int(got.overflow) == 0
    assert_frame(got, 0, want_of([m], regions)[0])
    assert np.array_equal(got.seeds[0].cpu().numpy(), np.flatnonzero(m))           # equal areas: by seed


def test_one_past_the_capacity_flags_the_frame_alone(dev):
    over, normal = SR.checkerboard(128, 130), SR.blobby(60, 90, 5)
    regions = G.SegRegions(4, 1, "foreground", 8192, fill=3)
    want = want_of([over, normal], regions)
    assert want[0]["count"] == -1 and want[0]["total"] == 8320 and 5 < want[1]["count"] < 500
    got = G.label_regions([on(dev, over), on(dev, normal)], regions, region_maps=True)
    assert int(got.counts[0]) == -1 and int(got.total[0]) == 8320 and int(got.overflow) == 1
    assert not got.rows[0].any() and (got.region_maps[0] == -1).all() and (got.seeds[0] == -1).all() and (got.areas[0] == -1).all()
    for f in range(2):
        assert_frame(got, f, want[f])
    with pytest.raises(CvxError):
        got.read()


def test_bad_frames_are_no_ops(dev):
    regions = G.SegRegions(8, 1, "all", 4)
    normal = SR.blobby(20, 30, 6)
    got = G.label_regions([torch.empty(0, 7, dtype=torch.uint8, device=dev), on(dev, normal)], regions)
    assert int(got.counts[0]) == 0 and int(got.total[0]) == 0 and int(got.overflow) == 1 and not got.rows[0].any()
    assert_frame(got, 1, want_of([normal], regions)[0])


# ---- 6. two calls, the same bytes --------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(dev):
    rng = np.random.RandomState(9)
    noise = (rng.rand(150, 210) < 0.5).astype(np.uint8) * rng.randint(1, 3, (150, 210)).astype(np.uint8)
    maps = [noise, SR.blobby(129, 257, 10), np.ones((100, 130), np.uint8)]
    confs = [rng.rand(*m.shape).astype(np.float32) for m in maps]
    labels, planes = [on(dev, m) for m in maps], [on(dev, c) for c in confs]
    regions = G.SegRegions(8, 2, "foreground", 300, fill=0)
    a = G.label_regions(labels, regions, conf=planes, region_maps=True)
    a_out = [t.clone() for t in (a.rows, a.counts, a.total, a.areas, a.seeds, a.overflow, *a.region_maps, *a.clean_maps)]
    b = G.label_regions(labels, regions, conf=planes, region_maps=True)
    b_out = [b.rows, b.counts, b.total, b.areas, b.seeds, b.overflow, *b.region_maps, *b.clean_maps]
    for x, y in zip(a_out, b_out):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    want = want_of(maps, regions, confs)
    assert want[0]["total"] > 300
    for f in range(3):
        assert_frame(b, f, want[f])


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deeplab(dev):
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    cfg = DeeplabV3PlusConfig()
    cfg.arch.input_size, cfg.arch.backbone_pretrained = (3, 97, 129), False       # the smallest input of tests/test_segment_tiled_gpu.py
    algo = DeeplabV3PlusA(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    return algo, model


MODEL_FRAMES = [(150, 300), (97, 129), (60, 200)]


def pictures(dev, seed):
    rng = np.random.RandomState(seed)
    host = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in MODEL_FRAMES]
    return host, [on(dev, a) for a in host]


def test_predict_regions_equals_the_restatement_on_its_label_maps(dev, deeplab):
    algo, model = deeplab
    regions = G.SegRegions(8, 4, "all", 40)
    host, frames = pictures(dev, 51)
    got = algo.predict_regions(model, frames, regions=regions, overlap=0.2, batch_size=4, sync=True)
    assert all(torch.equal(f, on(dev, a)) for f, a in zip(frames, host))           # draw=False leaves the frames alone
    labels = algo.segment_tiled(model, [on(dev, a) for a in host], overlap=0.2, batch_size=4, draw=False)
    totals = []
    for f in range(3):
        assert torch.equal(got.labels[f], labels[f])
        want = SR.regions(labels[f].cpu().numpy(), "all", 8, 4, 40)
        totals.append(want["total"])
        assert_frame(got, f, want)
    assert max(totals) >= 2, totals                                                # the random network does draw regions
    assert len(got.read()) == 3
    # draw=True: segment_tiled's overlay, then the boxes
    _, drawn = pictures(dev, 51)
    algo.predict_regions(model, drawn, regions=regions, overlap=0.2, batch_size=4, draw=True)
    _, expect = pictures(dev, 51)
    algo.segment_tiled(model, expect, overlap=0.2, batch_size=4, draw=True)
    R.draw_detections(expect, got.rows, got.counts)
    for f in range(3):
        assert torch.equal(drawn[f], expect[f]) and not torch.equal(drawn[f], on(dev, host[f])), f


def test_a_tracker_keeps_one_id_on_a_moving_blob(dev, deeplab, monkeypatch):
    """``predict_regions`` with a tracker, three calls: the label maps are a 30 x 40 blob that moves by two pixels per frame (the random
    network draws no such thing, so ``segment_tiled`` is replaced by the maps; the labelling, the tracker and the painting are real)"""
    from computervision.pytorch_amd.track import Tracker
    algo, model = deeplab
    maps = []
    for t in range(3):
        m = np.zeros((120, 160), np.uint8)
        m[40:70, 50 + 2 * t:90 + 2 * t] = 3
        m[5, 5 + t] = 4                                                            # a speckle below min_area
        maps.append(m)
    feed = iter(maps)
    monkeypatch.setattr(algo, "segment_tiled", lambda model, frames, **kw: [on(dev, next(feed))])
    tracker = Tracker(dev)
    seen = []
    for t in range(3):
        frame = torch.zeros(120, 160, 3, dtype=torch.uint8, device=dev)
        got = algo.predict_regions(model, [frame], regions=G.SegRegions(8, 16), draw=True, tracker=tracker)
        boxes, scores, classes, ids = got.read()[0]
        assert boxes.tolist() == [[50.0 + 2 * t, 40.0, 90.0 + 2 * t, 70.0]] and scores.tolist() == [1.0] and classes.tolist() == [3]
        seen.append(int(ids[0]))
        expect = torch.zeros(120, 160, 3, dtype=torch.uint8, device=dev)
        R.draw_tracks([expect], got.rows, got.ids, got.counts)
        assert torch.equal(frame, expect) and bool(frame.any())
    assert seen == [0, 0, 0] and tracker.overflowed() == 0


def test_segment_frames_with_regions_equals_predict_regions_batch_by_batch(dev, deeplab):
    from computervision.pytorch_amd.track import Tracker
    from scripts import detect
    algo, model = deeplab
    regions = G.SegRegions(8, 4, "all", 40)
    _, video = pictures(dev, 52)
    batches = list(detect.segment_frames(algo, model, iter(video), 2, regions=regions, track={"min_hits": 1}, overlap=0.2))
    assert [len(b) for b in batches] == [2, 1] and all(f is v for f, v in zip([f for b in batches for f in b], video))
    _, again = pictures(dev, 52)
    tracker = Tracker(dev, min_hits=1)
    algo.predict_regions(model, again[:2], regions=regions, draw=True, tracker=tracker, overlap=0.2)
    algo.predict_regions(model, again[2:], regions=regions, draw=True, tracker=tracker, overlap=0.2)
    _, plain = pictures(dev, 52)
    for _ in algo.segment_frames(model, iter(plain), 2, overlap=0.2):
        pass
    for f in range(3):
        assert torch.equal(video[f], again[f]), f
    assert any(not torch.equal(video[f], plain[f]) for f in range(3))              # the boxes were painted


def test_without_the_keywords_nothing_new_is_launched(dev, deeplab, monkeypatch):
    from scripts import detect
    algo, model = deeplab
    calls = []
    real = G.label_regions
    monkeypatch.setattr(G, "label_regions", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    _, frames = pictures(dev, 53)
    algo.segment_tiled(model, frames, overlap=0.2, batch_size=4)
    for _ in detect.segment_frames(algo, model, iter(frames), 2, overlap=0.2):
        pass
    for _ in algo.segment_frames(model, iter(frames), 2, regions=None, track=None):
        pass
    assert calls == []
    algo.predict_regions(model, frames[:1])
    assert calls == [1]                                                            # the wrapper does count


def test_label_regions_and_predict_regions_do_not_synchronise(dev, deeplab):
    algo, model = deeplab
    regions = G.SegRegions(8, 4, "all", 40, fill=0)
    _, frames = pictures(dev, 54)
    algo.predict_regions(model, frames, regions=regions, draw=True, overlap=0.2)          # first use: code objects, palette, workspace
    labels = [on(dev, SR.blobby(70, 90, 11)), on(dev, SR.blobby(40, 200, 12))]
    conf = [torch.rand(70, 90, device=dev), torch.rand(40, 200, device=dev)]
    G.label_regions(labels, regions, conf=conf, region_maps=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            flags = False
        except RuntimeError:
            flags = True
        print(f"set_sync_debug_mode('error') flags a read-back on this build: {flags}")
        got = G.label_regions(labels, regions, conf=conf, region_maps=True)
        found = algo.predict_regions(model, frames, regions=regions, draw=True, overlap=0.2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for f in range(2):
        assert_frame(got, f, SR.regions(labels[f].cpu().numpy(), "all", 8, 4, 40, conf[f].cpu().numpy(), 0))
    assert len(found.read()) == 3
