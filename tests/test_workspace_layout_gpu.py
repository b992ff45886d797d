"""MI355X: the entries of the suppression family that carve a caller's workspace (cvx_carver, csrc/cvx_common.h), held to their own
size query.  Each entry runs twice on one buffer of ``need + 8 + 4096`` bytes filled with 0xAB: once on the buffer's own pointer, once on
the pointer advanced by 8 bytes with ``workspace_bytes = need`` exactly -- a base that is not 256-byte aligned and not a byte to spare.
Both calls give the same bytes, those the entry's restatement expects, and the last 4096 bytes of the buffer still hold 0xAB: the
layout the launcher places is the one the query measured.  Inputs: 2 blocks or frames, 129 candidates in the first (a mask-word edge
is crossed) and 65 in the second, 3 classes; for the regions two 33 x 65 maps."""
import numpy as np
import pytest
import torch

import box_fusion_restatement as BR
import det_tta_restatement as DR
import eval_tail_cases as T
import seg_regions_restatement as SR
import soft_nms_restatement as S
import tiled_restatement as TR
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import box_fusion as BF
from computervision.pytorch_amd import det_tta as DT
from computervision.pytorch_amd import engine as E
from computervision.pytorch_amd import render as R
from computervision.pytorch_amd import seg_regions as G
from computervision.pytorch_amd import soft_nms as SN
from oracle import nms_ref
from test_predict_tiled_gpu import draw_rows

pytestmark = pytest.mark.gpu

GUARD = 4096
SLOT_COUNTS = np.array([64, 64, 64, 1, 1, 0], np.int32)            # slot k * 2 + f of three sources: frame 0 has 129 rows, frame 1 has 65


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_nms(got, want):
    """(rows, index, counts) against the per-block (rows, anchors); what lies past a count is zero"""
    rows, index, counts = got
    assert counts.tolist() == [len(ref[1]) for ref in want]
    for b, ref in enumerate(want):
        k = len(ref[1])
        assert np.array_equal(index[b, :k].astype(np.int64), ref[1]) and np.array_equal(bits(rows[b, :k]), bits(ref[0])), b
        assert not rows[b, k:].any() and not index[b, k:].any(), b


def nms_entry(dev):
    pred = T.clustered(900, 130, 3, (129, 65))
    y = torch.from_numpy(pred).to(dev)
    need = lambda lib: lib.cvx_nms_workspace_bytes(2, 130)
    call = lambda: E.nms(y, 0.25, 0.7, 300)
    return need, call, lambda got: check_nms(got, nms_ref.non_max_suppression(pred, 0.25, 0.7, 300, variant="tv0141_cuda"))


def soft_nms_entry(dev):
    pred = T.clustered(900, 130, 3, (129, 65))
    y = torch.from_numpy(pred).to(dev)
    need = lambda lib: lib.cvx_soft_nms_workspace_bytes(2, 130)
    call = lambda: SN.soft_nms(y, 0.25, SN.SoftNMS("gaussian"), 0.3, 300)
    return need, call, lambda got: check_nms(got, S.soft_nms_restated(pred, 0.25, 0.3, 300, "gaussian"))


def merge_entry(dev):
    slot_map = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 40, 0, 0], [1, 40, 0, 0], [0, 0, 30, 0], [1, 0, 30, 0]], np.int32)
    frame_hw = np.array([[140, 200], [140, 200]], np.int32)
    rows = draw_rows(np.random.RandomState(11), slot_map, SLOT_COUNTS, 64)
    device = on(dev, [rows, SLOT_COUNTS, slot_map, frame_hw])
    want = TR.merge(rows, SLOT_COUNTS, slot_map, frame_hw, "iou", 0.5, False, 300)

    def check(got):
        out_rows, counts, source, overflow = got
        assert counts.tolist() == want[1].tolist() and overflow.tolist() == [want[3]]
        assert np.array_equal(source, want[2]) and np.array_equal(bits(out_rows), bits(want[0]))

    return (lambda lib: lib.cvx_det_merge_workspace_bytes(2)), (lambda: R.merge_tiles(*device, "iou", 0.5, False, 300)), check


def check_fused(got, want):
    rows, counts, source, members, overflow = got
    assert counts.tolist() == want[1].tolist() and overflow.tolist() == [want[4]]
    assert np.array_equal(source, want[2]) and np.array_equal(members, want[3]) and np.array_equal(bits(rows), bits(want[0]))


def fuse_views_entry(dev):
    rows, _, vmap = DR.fuse_case(2, 3, seed=11, k_in=64, empty_frame=False)
    hw = DR.FRAME_HW[:2]
    device = on(dev, [rows, SLOT_COUNTS, vmap, hw])
    want = DR.fuse_views(rows, SLOT_COUNTS, vmap, hw, 0.5, False, "vote", "views", 300)
    return ((lambda lib: lib.cvx_det_merge_workspace_bytes(2)), (lambda: DT.fuse_views(*device, 0.5, False, "vote", "views", 300)),
            lambda got: check_fused(got, want))


def wbf_entry(dev):
    rows, _, vmap, hw, weights = BR.wbf_case(2, 3, k_in=64)
    device = on(dev, [rows, SLOT_COUNTS, vmap, hw])
    want = BR.fuse_wbf(rows, SLOT_COUNTS, vmap, hw, weights, BR.WBF_IOU)
    return ((lambda lib: lib.cvx_det_wbf_workspace_bytes(2)), (lambda: BF.fuse_wbf(*device, weights=weights, iou=BR.WBF_IOU)),
            lambda got: check_fused(got, want))


def regions_entry(dev):
    maps = [SR.blobby(33, 65, 300 + f) for f in range(2)]
    regions = G.SegRegions(8, 3, "all", 64, fill=9)
    want = [SR.regions(m, regions.classes, regions.connectivity, regions.min_area, regions.max_det, None, regions.fill) for m in maps]
    device = on(dev, maps)

    def call():
        got = G.label_regions(device, regions, region_maps=True)
        return [got.rows, got.counts, got.total, got.areas, got.seeds, got.overflow, *got.region_maps, *got.clean_maps]

    def check(got):
        rows, counts, total, areas, seeds, overflow = got[:6]
        assert overflow.tolist() == [0] and min(w["count"] for w in want) >= 2
        for f, w in enumerate(want):
            assert (int(counts[f]), int(total[f])) == (w["count"], w["total"]), f
            assert np.array_equal(areas[f], w["areas"]) and np.array_equal(seeds[f], w["seeds"]) and np.array_equal(bits(rows[f]), bits(w["rows"])), f
            assert np.array_equal(got[6 + f], w["region_map"]) and np.array_equal(got[8 + f], w["clean_map"]), f

    return (lambda lib: lib.cvx_seg_regions_workspace_bytes(2, 33, 65)), call, check


def centernet_entry(dev):
    c = next(k for k in T.centernet_cases() if k.name == "cn_1x40x3_k50")
    x = T.centernet_device_input(c).to(dev)
    ld, reg_col, wh_col = c.cols
    keys = ("boxes", "scores", "classes", "topk_index", "keep", "counts")

    def call():
        out = E.centernet_decode(x, c.H, c.W, c.nc, reg_col, wh_col, c.K, c.conf, c.nms_thr, c.use_nms)
        return [out[k] for k in keys]

    def check(got):   # the comparisons of test_eval_tail_gpu.test_centernet_decode_sweep: indices, classes and survivors exact
        out = dict(zip(keys, got))
        for b, ref in enumerate(T.centernet_reference(c)):
            nz = int((ref["scores"] > 0).sum())
            assert np.array_equal(out["topk_index"][b, :nz].astype(np.int64), ref["index"][:nz].numpy()), b
            assert np.array_equal(out["classes"][b, :nz].astype(np.int64), ref["classes"][:nz].numpy()), b
            n = int(out["counts"][b])
            assert n == len(ref["keep"]) and np.array_equal(out["keep"][b, :n].astype(np.int64), ref["keep"].numpy()), b
            ulp = np.abs(bits(out["scores"][b, :nz]).astype(np.int64) - bits(ref["scores"][:nz].numpy()).astype(np.int64))
            assert ulp.max() <= 1, (b, int(ulp.max()))
            np.testing.assert_allclose(out["boxes"][b, :nz], ref["boxes"][:nz].numpy(), rtol=1e-6, atol=1e-5)

    return (lambda lib: lib.cvx_centernet_decode_workspace_bytes(c.B, c.H, c.W, c.nc)), call, check


ENTRIES = {"nms_variant": nms_entry, "soft_nms": soft_nms_entry, "merge_tiles": merge_entry, "fuse_views": fuse_views_entry, "fuse_wbf": wbf_entry,
           "seg_regions": regions_entry, "centernet_decode": centernet_entry}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_exactly_the_queried_bytes_at_an_unaligned_base(dev, monkeypatch, entry):
    need_of, call, check = ENTRIES[entry](dev)
    need = int(need_of(L.load()))
    assert need > 0
    buf = torch.full((need + 8 + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    outs = []
    for view in (buf, buf[8:8 + need]):
        asked = []
        monkeypatch.setattr(L, "workspace", lambda name, device, n, view=view: (asked.append(n), view)[1])
        outs.append([t.cpu().numpy() for t in call()])
        assert asked == [need] and view.numel() >= need
    torch.cuda.synchronize(dev)
    tail = buf[need + 8:].cpu().numpy()
    print(f"{entry}: need {need} bytes, {int((tail != 0xAB).sum())} guard bytes touched")
    assert tail.size == GUARD and bool((tail == 0xAB).all())
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    check(outs[0])
