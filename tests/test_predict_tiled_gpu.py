"""MI355X: tiled prediction for large frames.  The two launches of csrc/tiles.hip (``cvx_tiles_u8_to_nchw``, ``cvx_det_merge_tiles``) against
the numpy restatement (tests/tiled_restatement.py), and ``predict_tiled`` / ``detect_frames(tiled=...)`` of the four detectors end to end
against the same composition with the restatement's merge on the host.  Every comparison is bit-exact: the tile kernel resamples nothing
and the merge is single rounded fp32 operations."""
import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import render as R
import render_restatement as RS
import tiled_restatement as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def pictures(shapes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def on(dev, arrays):
    return [torch.from_numpy(a).to(dev) for a in arrays]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the tile kernel -------------------------------------------------------------------------------------------------------------------
TILE_FRAMES = [(37, 53), (96, 80), (20, 30)]


def tile_frames(dev):
    """37 x 53 contiguous; 96 x 80 as a view with row pitch 3 * 80 + 12; 20 x 30, smaller than the tile"""
    host = pictures(TILE_FRAMES, 21)
    frames = on(dev, host)
    padded = torch.full((96, 3 * 80 + 12), 77, dtype=torch.uint8, device=dev)
    frames[1] = padded[:, :3 * 80].view(96, 80, 3)
    frames[1].copy_(torch.from_numpy(host[1]))
    assert frames[1].stride(0) == 3 * 80 + 12 and not frames[1].is_contiguous()
    return host, frames


@pytest.mark.parametrize("swap_rb", [False, True])
@pytest.mark.parametrize("input_hw", [(32, 48), (31, 50)])          # 16-byte stores, and a width that allows none
def test_tile_kernel_equals_the_restatement(dev, input_hw, swap_rb):
    H, W = input_hw
    host, frames = tile_frames(dev)
    grids = [R.tile_grid(h, w, (H, W), 0.25) for h, w in TILE_FRAMES]
    assert len(grids[0]) == 4 and len(grids[1]) > 4 and grids[2] == [(0, 0, 20, 30)]
    flat = [(f, t) for f, g in enumerate(grids) for t in g]
    flat.append((0, (30, 40, H, W)))                                 # a job that runs over its frame's edge: what lies outside reads as padding
    n = len(flat)
    slots = n + 1                                                    # one slot no job names stays as it was
    order = list(range(n))[::-1]                                     # a slot order that is not the job order
    assert sorted(order) != order and len(set(order)) == n
    table = np.array([(frames[f].data_ptr(), TILE_FRAMES[f][0], TILE_FRAMES[f][1], frames[f].stride(0), y0, x0, th, tw, order[j])
                      for j, (f, (y0, x0, th, tw)) in enumerate(flat)], dtype=R.TILE_JOB_DTYPE)
    jobs = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    out = torch.full((slots, 3, H, W), -7.0, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().cvx_tiles_u8_to_nchw(L.ptr(jobs), n, int(swap_rb), L.ptr(out), H, W, L.stream_ptr(dev)), "cvx_tiles_u8_to_nchw")
    got = out.cpu().numpy()
    want = TR.tiles([(host[f], y0, x0, th, tw, order[j]) for j, (f, (y0, x0, th, tw)) in enumerate(flat)], slots, H, W, swap_rb)
    untouched = [s for s in range(slots) if s not in order]
    assert len(untouched) == 1 and (got[untouched[0]] == -7.0).all()
    for s in order:
        assert same_bits(got[s], want[s]), s
    assert (want[order[-1]][:, -1, -1] == TR.PAD).all()              # the corner of the job past the edge


@pytest.mark.parametrize("full_frame", [False, True])
def test_tile_batch_input_equals_the_restatement(dev, full_frame):
    H, W = 32, 48
    host, frames = tile_frames(dev)
    tb = R.TileBatch(frames, (H, W), 0.25, full_frame, True)
    got = tb.network_input().cpu().numpy()
    jobs, slot, full = [], 0, []
    for f, (h, w) in enumerate(TILE_FRAMES):
        for y0, x0, th, tw in R.tile_grid(h, w, (H, W), 0.25):
            jobs.append((host[f], y0, x0, th, tw, slot))
            slot += 1
        if full_frame:
            full.append(slot)
            slot += 1
    assert tb.slots == slot == got.shape[0] and tb.n_tiles == len(jobs)
    want = TR.tiles(jobs, slot, H, W)
    for j in jobs:
        assert same_bits(got[j[5]], want[j[5]]), j[1:]
    if full_frame:
        whole = R.letterbox_batch(frames, (H, W)).cpu().numpy()
        for f, s in enumerate(full):
            assert same_bits(got[s], whole[f]), f
    sm, hw = tb.slot_map.cpu().numpy(), tb.image_hw.cpu().numpy()
    assert tb.frame_hw.cpu().numpy().tolist() == [list(s) for s in TILE_FRAMES]
    assert sm[:, 0].tolist() == tb.slot_frame and [sm[j[5], 1:3].tolist() for j in jobs] == [[j[2], j[1]] for j in jobs]
    assert all(hw[j[5]].tolist() == [H, W] for j in jobs) and all(hw[s].tolist() == list(TILE_FRAMES[f]) and sm[s, 1:].tolist() == [0, 0, 0]
                                                                   for f, s in enumerate(full))


# ---- 2. the merge kernel ------------------------------------------------------------------------------------------------------------------
MERGE_SEED = 3
SLOT_MAP = np.array([[0, 0, 0, 0], [0, 40, 0, 0], [0, 0, 30, 0], [2, 0, 0, 0], [2, 50, 0, 0], [2, 0, 45, 0], [2, 50, 45, 0]], np.int32)
MERGE_FRAME_HW = np.array([[120, 150], [64, 64], [140, 160]], np.int32)          # frame 1 has no slot: no candidates
K_IN = 16


def draw_rows(rng, slot_map, counts, k_in):
    """jittered copies of a few base boxes (in the slots' own pixels), scores from a small set so that ties occur, three classes"""
    base = np.array([[20, 20, 70, 80], [60, 30, 120, 90], [10, 70, 60, 118], [90, 60, 150, 125]], np.float32)
    rows = np.zeros((len(counts), k_in, 6), np.float32)
    for s in range(len(counts)):
        for r in range(counts[s]):
            box = base[rng.randint(4)] + rng.randint(-6, 7, 4).astype(np.float32) * np.float32(0.75)
            if rng.rand() < 0.3:                                     # the part of the box a tile border leaves
                box[2] = box[0] + (box[2] - box[0]) * np.float32(0.4)
            box[[0, 2]] -= slot_map[s, 1]
            box[[1, 3]] -= slot_map[s, 2]
            rows[s, r] = [*box, rng.choice([0.9, 0.75, 0.5, 0.25]), rng.randint(3)]
    return rows


def merge_case(seed):
    """7 slots over 3 frames, slot 5 with count 0"""
    counts = np.array([16, 11, 9, 13, 16, 0, 7], np.int32)
    rows = draw_rows(np.random.RandomState(seed), SLOT_MAP, counts, K_IN)
    rows[5, :3] = rows[0, :3]                                        # rows past a count are not candidates
    return rows, counts


@pytest.fixture(scope="module")
def merge_inputs(dev):
    rows, counts = merge_case(MERGE_SEED)
    return rows, counts, on(dev, [rows, counts, SLOT_MAP, MERGE_FRAME_HW])


def check_merge(got, want):
    rows, counts, source, overflow = (t.cpu().numpy() for t in got)
    assert counts.tolist() == want[1].tolist() and overflow.tolist() == [want[3]]
    assert np.array_equal(source, want[2]) and same_bits(rows, want[0])


@pytest.mark.parametrize("max_det", [5, 300])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("metric", ["iou", "ios"])
def test_merge_kernel_equals_the_restatement(dev, merge_inputs, metric, agnostic, max_det):
    rows, counts, (d_rows, d_counts, d_map, d_hw) = merge_inputs
    want = TR.merge(rows, counts, SLOT_MAP, MERGE_FRAME_HW, metric, 0.5, agnostic, max_det)
    everything = TR.merge(rows, counts, SLOT_MAP, MERGE_FRAME_HW, metric, 0.5, agnostic, 300)[1]
    candidates = [int(counts[SLOT_MAP[:, 0] == f].sum()) for f in range(3)]
    assert candidates[1] == 0 and want[1][1] == 0
    for f in (0, 2):                                                 # the case bites: every non-empty frame suppresses and keeps
        assert 2 <= want[1][f] and everything[f] < candidates[f], (f, want[1], everything, candidates)
    check_merge(R.merge_tiles(d_rows, d_counts, d_map, d_hw, metric, 0.5, agnostic, max_det), want)


WORD_SLOT_MAP = np.array([[0, 0, 0, 0], [0, 40, 0, 0], [0, 0, 30, 0]], np.int32)
WORD_FRAME_HW = np.array([[140, 200]], np.int32)
WORD_K, WORD_SEED = 64, 11


@pytest.mark.parametrize("metric", ["iou", "ios"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_merge_kernel_across_a_mask_word_edge(dev, n, metric):
    """n candidates of one frame, filled slot by slot into three slots of 64: the suppression matrix has one, two and three 64-bit words per
    row, and a kept candidate of word 0 has to remove a candidate of word 1"""
    counts = np.array([min(WORD_K, max(0, n - WORD_K * s)) for s in range(3)], np.int32)
    rows = draw_rows(np.random.RandomState(WORD_SEED), WORD_SLOT_MAP, counts, WORD_K)
    want = TR.merge(rows, counts, WORD_SLOT_MAP, WORD_FRAME_HW, metric, 0.5, False, 300)
    ordinals = np.concatenate([s * WORD_K + np.arange(counts[s]) for s in range(3)]).astype(np.uint64)
    score_bits = rows.reshape(-1, 6)[ordinals.astype(np.int64), 4].view(np.uint32).astype(np.uint64)
    order = np.argsort(((np.uint64(0xFFFFFFFF) - score_bits) << np.uint64(32)) | ordinals, kind="stable")
    position = {int(ordinals[o]): i for i, o in enumerate(order)}    # ordinal -> place under (score desc, ordinal asc)
    kept = sorted(position[int(o)] for o in want[2][0, :want[1][0]])
    assert want[3] == 0 and 1 <= len(kept) <= n
    if n == 65:                                                      # the one candidate of word 1 falls to a kept candidate of word 0
        assert max(kept) < 64, kept
    if n == 129 and metric == "iou":                                 # and the walk keeps candidates beyond word 0
        assert max(kept) >= 64, kept
    check_merge(R.merge_tiles(*on(dev, [rows, counts, WORD_SLOT_MAP, WORD_FRAME_HW]), metric, 0.5, False, 300), want)


def test_merge_kernel_flags_a_bad_count(dev, merge_inputs):
    rows, counts, (d_rows, _, d_map, d_hw) = merge_inputs
    for bad in (-1, K_IN + 1):
        c = counts.copy()
        c[4] = bad
        want = TR.merge(rows, c, SLOT_MAP, MERGE_FRAME_HW, "ios", 0.5, False, 300)
        assert want[3] == 1 and not np.isin(want[2][2], np.arange(4 * K_IN, 5 * K_IN)).any() and want[1][2] >= 2
        check_merge(R.merge_tiles(d_rows, torch.from_numpy(c).to(dev), d_map, d_hw, "ios", 0.5, False, 300), want)
    before = torch.full((1,), 5, dtype=torch.int32, device=dev)      # a word the caller hands in is added to
    assert R.merge_tiles(d_rows, torch.from_numpy(c).to(dev), d_map, d_hw, overflow=before)[3].tolist() == [6]


@pytest.mark.parametrize("extra", [0, 1])
def test_merge_kernel_capacity(dev, extra):
    """exactly 8192 disjoint candidates in a frame pass; 8193 give count -1 and overflow 1 -- flagged, never truncated"""
    K, rng = 1024, np.random.RandomState(5)
    k = np.arange(9 * K)
    boxes = np.stack([(k % 128) * 4, (k // 128) * 4, (k % 128) * 4 + 2, (k // 128) * 4 + 2], 1).astype(np.float32)
    rows = np.concatenate([boxes, rng.choice([0.9, 0.6, 0.3], (9 * K, 1)), np.zeros((9 * K, 1))], 1).astype(np.float32).reshape(9, K, 6)
    counts = np.array([K] * 8 + [extra], np.int32)
    slot_map = np.zeros((9, 4), np.int32)
    slot_map[:, 0] = 1                                               # frame 0 of 2 stays empty
    frame_hw = np.array([[10, 10], [400, 600]], np.int32)
    assert counts.sum() == R.MERGE_CAP + extra
    want = TR.merge(rows, counts, slot_map, frame_hw, "ios", 0.5, False, 300)
    assert want[1].tolist() == [0, -1 if extra else 300] and want[3] == extra
    check_merge(R.merge_tiles(*on(dev, [rows, counts, slot_map, frame_hw]), "ios", 0.5, False, 300), want)
    if extra:
        r, c, _, ov = R.merge_tiles(*on(dev, [rows, counts, slot_map, frame_hw]))
        with pytest.raises(CvxError):                                # the one host read refuses a dropped frame
            R.read_detections(r, c, ov)


def test_merge_tiles_validates_its_arguments(dev):
    rows, counts, sm, hw = on(dev, [np.zeros((2, 4, 6), np.float32), np.zeros(2, np.int32), np.zeros((2, 4), np.int32), np.ones((1, 2), np.int32)])
    for bad in (dict(metric="giou"), dict(threshold=1.5), dict(max_det=0), dict(max_det=R.MERGE_CAP + 1)):
        with pytest.raises(ValueError):
            R.merge_tiles(rows, counts, sm, hw, **bad)
    for args in ((rows[..., :5], counts, sm, hw), (rows, counts.long(), sm, hw), (rows, counts, sm[:1], hw), (rows, counts, sm, hw.float())):
        with pytest.raises(ValueError):
            R.merge_tiles(*args)
    assert R.merge_tiles(rows, counts, sm, hw)[1].tolist() == [0]


# ---- 3. YOLOv8 end to end -----------------------------------------------------------------------------------------------------------------
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
    return cfg, algo, model


FRAME_SHAPES = [(200, 300), (97, 128), (128, 128)]


def composition(algo, model, frames, conf, overlap, full_frame, batch_size, **merge):
    """the expectation: the same ``TileBatch`` input through the class's ``_evaluation_rows`` in the same chunks, ``det_to_image``, and the
    restatement's merge on the host.  Returns (rows, counts, source, overflow) and the per-slot counts."""
    input_hw, letterbox = algo._predict_input()
    tb = R.TileBatch(frames, input_hw, overlap, full_frame, letterbox)
    x = tb.network_input()
    rows_of = algo._evaluation_rows(model)
    parts, dropped = [], 0
    for c0 in range(0, tb.slots, batch_size):
        c1 = min(c0 + batch_size, tb.slots)
        rows, counts, box_map = rows_of(x[c0:c1], {"image_hw": tb.image_hw[c0:c1]}, conf)
        rows, counts, overflow = R.det_to_image(rows, counts, box_map)
        parts.append((rows.cpu().numpy(), counts.cpu().numpy()))
        dropped += int(overflow)
    K = max(p[0].shape[1] for p in parts)
    rows = np.zeros((tb.slots, K, 6), np.float32)
    c0 = 0
    for r, _ in parts:
        rows[c0:c0 + len(r), :r.shape[1]] = r
        c0 += len(r)
    counts = np.concatenate([p[1] for p in parts])
    out = TR.merge(rows, counts, tb.slot_map.cpu().numpy(), tb.frame_hw.cpu().numpy(), **merge)
    return (out[0], out[1], out[2], out[3] + dropped), counts, tb


def triples_of(want):
    rows, counts = want[0], want[1]
    return [(rows[f, :n, :4], rows[f, :n, 4], rows[f, :n, 5].astype(np.int64)) for f, n in enumerate(counts)]


def triples_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert same_bits(g[0], w[0]) and same_bits(g[1], w[1]) and np.array_equal(g[2], w[2]) and g[2].dtype == np.int64


MERGES = [dict(metric="ios", threshold=0.5, class_agnostic=False, max_det=300),          # predict_tiled's defaults
          dict(metric="iou", threshold=0.7, class_agnostic=True, max_det=7)]


@pytest.mark.parametrize("merge", MERGES, ids=["ios", "iou"])
@pytest.mark.parametrize("full_frame", [True, False])
def test_yolov8_predict_tiled_equals_the_composition(dev, yolov8, full_frame, merge):
    _, algo, model = yolov8
    frames = on(dev, pictures(FRAME_SHAPES, 31))
    want, slot_counts, tb = composition(algo, model, frames, 0.001, 0.2, full_frame, 4, **merge)
    assert tb.slots == 8 + 3 * full_frame and len(tb.tiles[0]) == 6            # chunks of 4, 4 and, with the whole pictures, 3
    print("YOLOv8-n tiled: rows per slot", slot_counts.tolist(), "merged per frame", want[1].tolist())
    assert want[3] == 0 and want[1].min() > 0
    per_frame = [sum(1 for s, f in enumerate(tb.slot_frame) if f == g and slot_counts[s] > 0) for g in range(3)]
    assert max(per_frame) >= 2                                                   # some frame has candidates from more than one slot
    keywords = dict(overlap=0.2, full_frame=full_frame, match=merge["metric"], match_threshold=merge["threshold"],
                    class_agnostic=merge["class_agnostic"], max_det=merge["max_det"], conf_threshold=0.001, batch_size=4)
    triples_equal(algo.predict_tiled(model, frames, sync=True, **keywords), triples_of(want))
    rows, counts = algo.predict_tiled(model, frames, sync=False, **keywords)
    assert rows.is_cuda and rows.shape == (3, merge["max_det"], 6) and counts.tolist() == want[1].tolist()
    assert same_bits(rows.cpu().numpy(), want[0])


# ---- 4. the other detectors ---------------------------------------------------------------------------------------------------------------
def other_detector(name, dev):
    if name == "yolo7":
        from configs import Yolo7Config
        from core.algorithms.yolo_v7 import YOLOv7
        cfg = Yolo7Config()
        cfg.arch.input_size, cfg.train.pretrained = (3, 160, 224), False
        return YOLOv7(cfg, dev), 0.2
    if name == "ssd":
        from configs import SsdConfig
        from core.algorithms.ssd import Ssd
        cfg = SsdConfig()
        cfg.train.pretrained = False
        return Ssd(cfg, dev), 0.05
    from configs import CenternetConfig
    from core.algorithms.centernet import CenterNetA
    cfg = CenternetConfig()
    cfg.arch.input_size = (3, 128, 128)
    return CenterNetA(cfg, dev), 0.3


# random-init SSD leaves about 4400 rows per slot above 0.05 -- a frame of five slots is beyond the merge's capacity and must come back
# flagged -- and about 440 above 0.07
@pytest.mark.parametrize("name,conf", [("yolo7", None), ("ssd", None), ("ssd", 0.07), ("centernet", None)])
def test_predict_tiled_equals_the_composition(dev, name, conf):
    algo, default_conf = other_detector(name, dev)
    conf = default_conf if conf is None else conf
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    (H, W), _ = algo._predict_input()
    shapes = [(H * 7 // 5, W * 7 // 5), (H // 2 + 5, W // 2 + 7)]               # about 1.4 x the network size: four tiles; and a small frame
    frames = on(dev, pictures(shapes, 32))
    want, slot_counts, tb = composition(algo, model, frames, conf, 0.2, True, 4, metric="ios", threshold=0.5, class_agnostic=False, max_det=300)
    assert len(tb.tiles[0]) == 4 and len(tb.tiles[1]) == 1 and tb.slots == 7
    print(f"{name} tiled: rows per slot above {conf}: {slot_counts.tolist()}, merged per frame {want[1].tolist()}, overflow {want[3]}")
    rows, counts = algo.predict_tiled(model, frames, conf_threshold=conf, batch_size=4, sync=False)
    assert counts.tolist() == want[1].tolist() and same_bits(rows.cpu().numpy(), want[0])
    if want[3] == 0:
        triples_equal(algo.predict_tiled(model, frames, conf_threshold=conf, batch_size=4, sync=True), triples_of(want))
    else:                                                                        # a frame beyond the merge's capacity: the host read refuses
        with pytest.raises(CvxError):
            algo.predict_tiled(model, frames, conf_threshold=conf, batch_size=4, sync=True)


# ---- 5. drawing ---------------------------------------------------------------------------------------------------------------------------
def test_predict_tiled_draws_the_merged_rows(dev, yolov8):
    _, algo, model = yolov8
    host = pictures(FRAME_SHAPES, 33)
    frames = on(dev, host)
    rows, counts = algo.predict_tiled(model, frames, conf_threshold=0.001, batch_size=4, max_det=40, draw=True, sync=False)
    torch.cuda.synchronize()
    clean = algo.predict_tiled(model, on(dev, host), conf_threshold=0.001, batch_size=4, max_det=40, sync=False)
    assert torch.equal(rows.view(torch.int32), clean[0].view(torch.int32)) and torch.equal(counts, clean[1])     # the rows come from the clean pixels
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    assert counts.sum() > 0
    for b in range(3):
        want, painted = RS.draw(host[b], rows[b], counts[b])
        assert painted.any() and np.array_equal(frames[b].cpu().numpy(), want), b


# ---- 6. no host wait ----------------------------------------------------------------------------------------------------------------------
def test_predict_tiled_and_detect_frames_do_not_synchronise(dev, yolov8):
    from scripts import detect
    _, algo, model = yolov8
    tiled = dict(overlap=0.2, conf_threshold=0.001, batch_size=4, max_det=40)
    host = pictures(FRAME_SHAPES + [(64, 90), (150, 140)], 34)
    algo.predict_tiled(model, on(dev, host[:3]), draw=True, sync=False, **tiled)      # first use: code objects, palette, engines, workspace
    algo.predict_tiled(model, on(dev, host[3:]), draw=True, sync=False, **tiled)
    once, video = on(dev, host[:3]), on(dev, host)
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
        rows, counts = algo.predict_tiled(model, once, draw=True, sync=False, **tiled)
        batches = list(detect.detect_frames(algo, model, iter(video), 3, tiled=tiled))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert [len(b) for b in batches] == [3, 2] and all(f is v for f, v in zip([f for b in batches for f in b], video))
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    assert counts.sum() > 0
    for b in range(3):
        want, _ = RS.draw(host[b], rows[b], counts[b])
        assert np.array_equal(once[b].cpu().numpy(), want), b
        assert np.array_equal(video[b].cpu().numpy(), want), b         # the same pictures through detect_frames
    r2, c2 = algo.predict_tiled(model, on(dev, host[3:]), sync=False, **tiled)
    for b in range(2):
        want, _ = RS.draw(host[3 + b], r2[b].cpu().numpy(), int(c2[b]))
        assert np.array_equal(video[3 + b].cpu().numpy(), want), b
