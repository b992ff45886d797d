"""The cases of tests/eval_tail_cases.py can tell a wrong eval-tail kernel from a right one -- shown from the references alone, no GPU.

Every generator's intended property is asserted from the oracle (exact candidate counts, the library's strategy switch on both sides of
both limits, ties that straddle the top-K boundary and the slices, no pair within 1e-5 of a suppression threshold), and seven deliberately
wrong restatements ("mutants") must each change the expected output of at least one case.  tests/test_eval_tail_gpu.py then holds the
kernels to these expected outputs."""
import numpy as np
import pytest
import torch

import eval_tail_cases as T
from oracle import centernet_ref as C
from oracle import nms_ref

MARGIN = 1e-5


def by_tag(tag):
    return [c for c in T.nms_cases() if tag in c.tags]


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------------
def test_nms_cases_have_the_candidate_counts_they_were_built_for():
    cases = T.nms_cases()
    for c in cases:
        assert T.candidate_counts(c.pred, c.conf) == c.n, c.name
        assert c.pred.dtype == np.float32 and (c.pred.shape[2] % 64 != 0 or "switch" in c.tags), c.name
    edges = by_tag("edge")
    assert sorted({c.n[0] for c in edges}) == [1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]
    assert {c.pred.shape[1] - 4 for c in edges} == {1, 3, 80} and {c.pred.shape[2] for c in edges} == {65, 130, 1500, 3000}
    assert T.nms_case("mixed_batch").n == (0, 1, 64, 700, 65)
    assert [c.n[0] for c in by_tag("switch")] == [1000, 1001, 5000, 5001]
    big = T.nms_case("large_a_25200")
    cand = np.nonzero(big.pred[0, 4:].max(0) > np.float32(big.conf))[0]
    assert big.pred.shape[2] == 25200 and (cand > 16384).sum() == 450 and (cand < 16384).sum() == 50
    over = T.nms_case("large_a_overflow")
    assert over.n[0] == 16500 > T.NMS_CAP and over.overflow == (0,) and over.n[1] == 300
    zero = T.nms_case("conf_thres_0")
    assert zero.n[0] == int((zero.pred[0, 4:].max(0) > 0).sum()) < zero.pred.shape[2]            # exact zeros stay out


def test_nms_strategy_switch_sits_between_the_cases():
    """tv0141_cpu: coordinate offsets up to 1000 candidates (boxes.numel() <= 4000), per class from 1001; tv0141_cuda: 5000 / 5001.  On these
    borderline pairs the two strategies keep different sets, so a switch moved by one candidate shows."""
    kept = {}
    for c in by_tag("switch"):
        n = c.n[0]
        off, van = T.nms_reference(c, "offset"), T.nms_reference(c, "vanilla")
        kept[n] = (len(off[0][1]), len(van[0][1]))
        assert not T.same_nms(off, van), n
        assert max(kept[n]) <= c.max_det
        for variant, limit in (("tv0141_cpu", 1000), ("tv0141_cuda", 5000)):
            assert T.same_nms(T.nms_reference(c, variant), van if n > limit else off), (n, variant)
    print("kept (offset, vanilla):", kept)
    assert kept == {1000: (766, 758), 1001: (767, 759), 5000: (3741, 3692), 5001: (3742, 3693)}


def test_nms_cases_keep_clear_of_the_threshold():
    for c in T.nms_cases():
        if not c.borderline:
            m = T.nms_iou_margin(c)
            assert m >= MARGIN, (c.name, m)


def test_nms_case_properties():
    ties = T.nms_case("mass_ties")
    sc = ties.pred[0, 4:].max(0)
    values, counts = np.unique(sc[sc > np.float32(0.25)], return_counts=True)
    assert len(values) <= 8 and counts.max() >= 100                         # hundreds of candidates share a score
    md = by_tag("max_det")
    s = len(T.nms_reference(T.nms_case(md[3].name), "vanilla")[0][1])
    assert [c.max_det for c in md] == [1, 7, s - 1, s, s + 1] and s > 8
    for c in md:
        for v in T.VARIANTS:
            assert len(T.nms_reference(c, v)[0][1]) == min(c.max_det, s), (c.name, v)
    for v in T.VARIANTS:
        assert len(T.nms_reference(T.nms_case("iou_thres_1"), v)[0][1]) == 100          # IoU > 1 never holds
        assert len(T.nms_reference(T.nms_case("iou_thres_0"), v)[0][1]) < 60
    x = T.nms_case("xyxy_clipped")
    box, _, cls, cand = T._candidates(x.pred[0], x.conf, True)
    flat = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1]) == 0
    assert box.min() == 0 and box.max() == 1 and flat.sum() >= 8 and len({tuple(r) for r in box[flat]}) < flat.sum()
    for v in T.VARIANTS:                                                       # 0 / 0 is not > thr: a box without area neither suppresses nor dies
        rows, keep = T.nms_reference(x, v)[0]
        assert set(cand[flat]) <= set(keep) and len(keep) < len(cand)
    mixed = T.nms_reference(T.nms_case("mixed_batch"), "tv0141_cuda")
    assert len(mixed[0][1]) == 0 and len(mixed[1][1]) == 1
    # suppression reaches across the 64-bit words of the mask: most dead boxes died by a keeper that sorts in an earlier word
    c = T.nms_case("edge_n1025_a3000_nc1")
    box, _, cls, cand = T._candidates(c.pred[0], c.conf, False)
    keep = nms_ref.batched_nms(box, cls, c.iou, "vanilla")
    dead = np.setdiff1d(np.arange(len(box)), keep)
    b64 = box.astype(np.float64)
    area = (b64[:, 2] - b64[:, 0]) * (b64[:, 3] - b64[:, 1])
    far = 0
    for j in dead:
        k = keep[keep < j]
        inter = (np.maximum(0, np.minimum(b64[k, 2], b64[j, 2]) - np.maximum(b64[k, 0], b64[j, 0])) *
                 np.maximum(0, np.minimum(b64[k, 3], b64[j, 3]) - np.maximum(b64[k, 1], b64[j, 1])))
        killer = k[inter / (area[k] + area[j] - inter) > c.iou][0]
        far += killer // 64 < j // 64
    assert len(dead) > 100 and far > len(dead) // 2, (len(dead), far)


def test_nms_restatement_is_the_oracle():
    for c in T.nms_cases():
        for v in T.VARIANTS:
            if c.n[-1] >= 5000 and v in ("offset", "vanilla"):
                continue                                                      # the two big greedy passes are compared through the switch
            assert T.same_nms(T.nms_restated(c, v), T.nms_reference(c, v)), (c.name, v)


def changed(mutant, cases, variants=T.VARIANTS):
    return [(c.name, v) for c in cases for v in variants if not T.same_nms(T.nms_restated(c, v, **mutant), T.nms_reference(c, v))]


def test_nms_mutants_change_the_expected_output():
    small = [c for c in T.nms_cases() if max(c.n) <= 1100 or c.overflow]
    hits = changed(dict(tie_desc=True), by_tag("ties") + by_tag("edge"), ("vanilla",))
    assert hits, "tie order by descending index"
    print("tie order:", len(hits))
    hits = changed(dict(ge=True), [T.nms_case("iou_thres_0"), T.nms_case("iou_thres_1")], ("vanilla", "offset"))
    assert len(hits) == 4, "'>=' in the suppression test"      # IoU == 0 for disjoint boxes, IoU == 1 never exceeded: both ends notice
    hits = changed(dict(word_exempt=True), [c for c in small if max(c.n) > 64], ("vanilla",))
    assert hits, "first box of each 64-box word exempt"
    print("word exempt:", len(hits))
    for shift in (-1, 1):
        hits = changed(dict(switch_shift=shift), by_tag("switch"), ("tv0141_cuda", "tv0141_cpu"))
        assert len(hits) == 2, ("strategy switch moved by one candidate", shift, hits)
    for shift in (-1, 1):
        hits = changed(dict(max_det_shift=shift), by_tag("max_det"), ("vanilla",))
        assert hits, ("max_det off by one", shift)
        print("max_det", shift, [h[0] for h in hits])


# ---- CenterNet ---------------------------------------------------------------------------------------------------------------------------
def test_centernet_cases_tie_across_the_list_end_and_the_slices():
    seen_empty_slice = seen_short = False
    for c in T.centernet_cases():
        pred = T.centernet_pred(c)
        logits = pred[..., :c.nc]
        assert pred.shape == (c.B, c.H * c.W, c.nc + 4) and bool(torch.isfinite(pred).all())
        grid = logits * c.s
        ok = (grid == grid.round()) & (grid >= -6 * c.s) & (grid <= 3 * c.s)
        assert bool(ok.all()) or c.saturated or c.overflow, c.name
        for b in range(c.B):
            st = T.centernet_tie_stats(c, b)
            print(c.name, b, st)
            if b in c.overflow:
                assert st["most_per_slice"] == st["per"] == 5120 > T.CAND_CAP       # every score of a slice ties
                continue
            assert st["most_per_slice"] <= T.CAND_CAP, (c.name, b)
            assert st["repeats"] > 0 or c.K == 1, (c.name, b)                       # equal scores inside the list: index order decides
            if c.boundary_tie:
                assert st["n_tie"] > st["n_inside"] >= 1 and len(st["slices"]) > 1, (c.name, b, st)
            seen_short |= st["nonzero"] < c.K
            seen_empty_slice |= st["per"] * (st["S"] - 1) >= c.H * c.W * c.nc
    assert seen_short and seen_empty_slice
    # 16-byte loads need the slice's first score aligned: image base b N and slice offset s per, in floats, both multiples of 4
    geo = {c.name: (c.H * c.W * c.nc, -(-c.H * c.W * c.nc // T.slices_for(c.K))) for c in T.centernet_cases()}
    assert geo["cn_12x12x7_k100"] == (1008, 63) and geo["cn_9x13x3_k256"] == (351, 44) and geo["cn_5x5x4_k100"] == (100, 7)
    assert geo["cn_32x32x80_k100"] == (81920, 5120) and geo["cn_23x1x5_k64"][0] % 2 == 1
    big = T.centernet_tie_stats(next(c for c in T.centernet_cases() if c.name == "cn_32x32x80_k100"), 0)
    assert big["n_tie"] > 900 and big["n_inside"] == 100
    sat = next(c for c in T.centernet_cases() if c.name == "cn_saturated")
    assert all(int((r["scores"] == 1.0).sum()) >= 20 for r in T.centernet_reference(sat))
    assert {T.slices_for(c.K) for c in T.centernet_cases()} == {8, 16}


def test_centernet_cases_keep_clear_of_the_thresholds():
    for c in T.centernet_cases():
        if c.use_nms:
            m = T.centernet_diou_margin(c)
            assert m >= MARGIN, (c.name, m)
        for r in T.centernet_reference(c):
            if r is not None:                                   # conf is no grid score: the mask cannot sit within an ulp of one
                assert float((r["scores"] - c.conf).abs().min()) > 1e-3, c.name
                assert 0 < len(r["keep"]) <= int(r["mask"].sum()), c.name
                assert c.use_nms or len(r["keep"]) == int(r["mask"].sum())
    assert any(len(r["keep"]) < int(r["mask"].sum()) for c in T.centernet_cases() for r in T.centernet_reference(c) if r is not None)
    assert {c.conf for c in T.centernet_cases()} == {0.3, 0.6}


def test_centernet_restatement_is_the_oracle_and_its_mutants_are_not():
    hits = {"tie_desc": 0, "per_slice": 0, "yx": 0}
    for c in T.centernet_cases():
        pred = T.centernet_pred(c)
        scores, inds = C.suppress_and_topk(pred.reshape(c.B, c.H, c.W, c.nc + 4), c.nc, c.K)
        flat = T.peak_map(pred, c.H, c.W, c.nc)
        wrong = T.peak_map(pred, c.H, c.W, c.nc, window="yx")
        for b in range(c.B):
            if b in c.overflow:
                continue
            ref = T.centernet_reference(c)[b]
            assert torch.equal(ref["index"], inds[b]) and torch.equal(ref["scores"], scores[b])
            assert torch.equal(T.topk_restated(flat[b], c.K), inds[b]), c.name
            nz = int((scores[b] > 0).sum())                    # the kernel is compared on the prefix with a score
            hits["tie_desc"] += not torch.equal(T.topk_restated(flat[b], c.K, tie_desc=True)[:nz], inds[b, :nz])
            hits["per_slice"] += not torch.equal(T.topk_restated(flat[b], c.K, per_slice=True)[:nz], inds[b, :nz])
            hits["yx"] += not torch.equal(T.topk_restated(wrong[b], c.K)[:nz], inds[b, :nz])
    print(hits)
    assert all(v > 0 for v in hits.values()), hits


# ---- YOLOv7 decode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", T.Y7_NC)
def test_yolo7_cases(nc):
    preds, rows, want = T.yolo7_case(nc, 0)
    _, rows_slack, want_slack = T.yolo7_case(nc, 2)
    R = sum(h * w for h, w in T.Y7_LEVELS)
    assert rows.shape == (T.Y7_B, R, 3 * (5 + nc)) and rows_slack.shape == (T.Y7_B, R, 3 * (5 + nc) + 2)
    assert bool(torch.isnan(rows_slack[..., -2:]).all()) and torch.equal(rows_slack[..., :-2], rows) and torch.equal(want, want_slack)
    assert want.shape == (T.Y7_B, 3 * R, 5 + nc) and bool(torch.isfinite(want).all())
    assert (3 * R) % 32 and (T.Y7_B * 3 * R) % 32                  # 32-anchor workgroups straddle anchors, levels and images
    # the rows are the head outputs: column a (5 + nc) + k of pixel (y, x) of level l
    p1 = preds[1]
    assert float(rows[2, 4 + 1 * 4 + 2, 2 * (5 + nc) + 3]) == float(p1[2, 2 * (5 + nc) + 3, 1, 2])
    assert sorted(5 + n for n in T.Y7_NC) == [6, 25, 64, 65, 85]
