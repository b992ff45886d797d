"""The cases of tests/loss_sweep_cases.py can tell a wrong loss / target kernel from a right one -- shown from the oracles alone, no GPU.

Every case's stated property is asserted from the oracle; every YOLOv7 case satisfies the admissibility condition of the SimOTA margins
(float32 and float64 assign identically, every margin >= 100 x the largest float32-vs-float64 difference; duplicate pairs that straddle a
k are decided by the lower-index rule, oracle ``ties="lower"``); and sixteen deliberately wrong restatements ("mutants") must each change
the expected output of at least one case.  tests/test_loss_sweep_gpu.py then holds the kernels to these expected outputs."""
import ctypes

import numpy as np
import pytest
import torch

import loss_sweep_cases as T
from oracle import yolov7_ref as Y

Y7_NAMES = [c.name for c in T.Y7_CASES]


@pytest.fixture(scope="module")
def margins():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = T.y7_margins(T.y7_case(name))
        return cache[name]

    return get


# ---- YOLOv7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Y7_NAMES)
def test_yolo7_case_is_admissible(margins, name):
    """float32 == float64 assignment, every margin >= 100 x the measured float32-vs-float64 difference, and the restatements equal the
    oracle: candidates; the assignment with ties="lower" in both precisions, and with the reference's torch.topk wherever no duplicate
    pair straddles a k (with such a pair torch.topk's choice is unspecified and reaches the loss: module docstring of the cases)."""
    c = T.y7_case(name)
    outs, targets = T.y7_inputs(c)
    r = margins(name)
    print(f"{name}: margin {r['margin']:.3e}, float32-vs-float64 difference {r['diff']:.3e}, ratio {r['margin'] / max(r['diff'], 1e-300):.0f}, "
          f"straddling duplicate pairs {r['straddles']}, candidates per image {[a['C'] for a in r['info'].values()]}")
    assert r["same"]
    assert r["margin"] >= T.MARGIN_FACTOR * r["diff"], (r["margin"], r["diff"])
    cands = Y.loss_candidates(targets, c.levels)
    assert T.y7_candidates(targets, c.levels) == cands
    for dtype in (torch.float32, torch.float64):
        assert Y.simota_assign(T.y7_preds(outs, dtype), targets, cands, c.img_size, c.nc, dtype, "lower") == r["matched"], dtype
        if r["straddles"] == 0:
            assert r["topk_agrees"] and Y.simota_assign(T.y7_preds(outs, dtype), targets, cands, c.img_size, c.nc, dtype) == r["matched"], dtype
    assert T.y7_reference(name)["matched"] == r["matched"]
    for a in r["info"].values():
        assert a["G"] <= T.Y7_GMAX and a["C"] <= T.Y7_CMAX


def test_yolo7_float32_oracle_is_unchanged_by_the_dtype_argument():
    c = T.y7_case("smoothing")
    outs, targets = T.y7_inputs(c)
    a = Y.yolo7_loss(outs, targets, c.img_size, c.nc, c.input_hw, c.smoothing)
    b = Y.yolo7_loss(outs, targets, c.img_size, c.nc, c.input_hw, c.smoothing, dtype=torch.float32)
    assert all(u.dtype == torch.float32 and torch.equal(u, v) for u, v in zip(a, b))
    d = T.y7_reference("smoothing")["items"]
    assert d.dtype == torch.float64 and float((d - torch.stack([v.reshape(()) for v in a]).double()).abs().max()) < 1e-5 * float(d[0])


def test_yolo7_case_properties(margins):
    crowd, r = T.y7_case("crowd"), margins("crowd")
    _, t = T.y7_inputs(crowd)
    img = t[:, 0].long()
    per = [int((img == b).sum()) for b in range(3)]
    assert per == [40, 0, 30] and t.shape[0] >= 69 and 15 * t.shape[0] > 1024              # the candidate kernel carries across a 1024-slot chunk
    assert bool((img[1:] < img[:-1]).any()) and bool((img[1:] > img[:-1]).any())          # not grouped by image
    assert r["info"][0]["C"] >= 513 and r["info"][0]["G"] > 8 and 1 not in r["info"]       # three 256-chunks in the gather and the compaction
    assert sum(len(m) for m in r["matched"]) > 100                                        # (both loops run over the image's C candidates)

    cap, r = T.y7_case("capacity64"), margins("capacity64")
    _, t = T.y7_inputs(cap)
    assert int((t[:, 0] == 1).sum()) == 64 == r["info"][1]["G"] and r["info"][1]["C"] <= T.Y7_CMAX

    cl, r = T.y7_case("clusters"), margins("clusters")
    outs, t = T.y7_inputs(cl)
    assert sum(len(a["contested"]) for a in r["info"].values()) >= 10
    dups = T.y7_duplicates(r["matched"])
    vals = T.y7_entry_ious(cl, outs, t, r["matched"])
    later = [k for k, pos in dups.items() if float(vals[k[0]][pos[-1]]) != float(vals[k[0]][pos[0]])]
    print(f"clusters: contested {sum(len(a['contested']) for a in r['info'].values())}, cells matched twice {len(dups)}, with a different later value {len(later)}")
    assert len(dups) >= 3 and len(later) >= 1
    lv, b, a, gj, gi = later[0]
    assert float(T.y7_reference("clusters")["tobj"][lv][b, a, gj, gi]) == float(vals[lv][dups[later[0]][-1]])
    groups = {}
    for row in t.tolist():
        groups.setdefault((row[0], row[2], row[3]), []).append(row)
    assert all(3 <= len(v) <= 4 and len({x[1] for x in v}) == len(v) and len({x[4] for x in v}) == len(v) for v in groups.values())

    bd = T.y7_case("borders")
    _, t = T.y7_inputs(bd)
    gx, gy = t[:, 2] * 16, t[:, 3] * 16
    assert bool((gx < 1).any() and (gx > 15).any() and (gy < 1).any() and (gy > 15).any())
    assert bool(((gx % 1 == 0) & (gy % 1 == 0)).any()) and bool(((gx % 1 == 0.5) & (gy % 1 == 0.5)).any())
    assert bool((gx == 1).any() and (gx == 15).any() and (gy == 1).any() and (gy == 15).any())
    anc = Y._level_anchors(2)[0]
    assert bool((t[:, 4] * 16 / anc[0] == 4.0).any()) and bool((t[:, 5] * 16 / anc[1] == 4.0).any())
    cands = Y.loss_candidates(t, bd.levels)
    wide = int(torch.nonzero(t[:, 4] * 16 / anc[0] == 4.0)[0])
    assert not any(e[1] == 0 and e[4] == wide for e in cands[2]) and any(e[4] == wide for e in cands[2])
    assert any(e[2] == 0 for lvl in cands for e in lvl) and any(e[3] == 0 for lvl in cands for e in lvl)
    assert any(e[2] == 15 for e in cands[2]) and any(e[3] == 15 for e in cands[2])

    ns = T.y7_case("nonsquare")
    assert ns.levels == ((5, 7), (10, 14), (20, 28)) and ns.input_hw == (160, 224) and ns.img_size == 160.0
    assert (T.y7_case("nc1").nc, T.y7_case("nc1").ld) == (1, 18) and 3 * (5 + 1) == 18                  # the smallest ld the entry accepts
    assert (T.y7_case("nc80").nc, T.y7_case("nc80").ld) == (80, 256) and T.y7_case("smoothing").smoothing == 0.1

    sat, r = T.y7_case("saturated"), margins("saturated")
    assert sat.gain == 6.0
    clamped = sum(int((a["sums"] < 1).sum()) for a in r["info"].values())
    disjoint = sum(1 for a in r["info"].values() for cidx in range(a["C"]) if int(a["gt_of"][cidx]) >= 0 and float(a["iou"][int(a["gt_of"][cidx]), cidx]) == 0.0)
    zero = float(torch.cat([(a["iou"] < 1e-3).flatten() for a in r["info"].values()]).float().mean())
    print(f"saturated: {zero:.2f} of the IoUs below 1e-3, dynamic k clamped for {clamped} ground truths, {disjoint} matched pairs without overlap")
    assert zero > 0.5 and clamped >= 1 and disjoint >= 1


def _assign_differs(name, margins, **mutant):
    c = T.y7_case(name)
    outs, targets = T.y7_inputs(c)
    r = margins(name)
    got, _ = T.y7_assign(T.y7_preds(outs, torch.float64), targets, r["cands"], mutant.pop("img_size", c.img_size), c.nc, torch.float64, **mutant)
    return got != r["matched"]


def test_yolo7_mutants_change_an_expected_output(margins):
    # 1: objectness target from the first duplicate
    c = T.y7_case("clusters")
    outs, t = T.y7_inputs(c)
    ref = T.y7_reference("clusters")
    first = T.y7_objectness_targets(c, outs, t, ref["matched"], first_wins=True)
    assert any(not torch.equal(a, b) for a, b in zip(first, ref["tobj"]))
    # 2: conflict argmin over the claimants only; 3: dynamic k rounded; 4: top-10
    assert any(_assign_differs(n, margins, claimants_only=True) for n in ("clusters", "crowd", "capacity64"))
    assert any(_assign_differs(n, margins, round_k=True) for n in Y7_NAMES)
    assert any(_assign_differs(n, margins, topn=10) for n in Y7_NAMES)
    # 5: ratio <= 4; 6: half cell <= 0.5; 7: gx >= 1 -- the exact-threshold rows of the borders case; 8: anchor-major order -- every case
    bt = T.y7_inputs(T.y7_case("borders"))[1]
    want = Y.loss_candidates(bt, T.y7_case("borders").levels)
    for mutant in ("ratio_le", "half_le", "border_ge"):
        assert T.y7_candidates(bt, T.y7_case("borders").levels, **{mutant: True}) != want, mutant
    for name in Y7_NAMES:
        c = T.y7_case(name)
        assert T.y7_candidates(T.y7_inputs(c)[1], c.levels, anchor_major=True) != margins(name)["cands"], name
    # 9: img_size from the width
    assert _assign_differs("nonsquare", margins, img_size=float(T.y7_case("nonsquare").input_hw[1]))


def test_yolo7_layout_entry_is_host_code():
    """cvx_debug_yolo7_loss_layout needs no GPU: ascending offsets inside the workspace, from the launcher's own layout function."""
    from computervision.pytorch_amd import _lib as L
    lib = L.load()
    for B, A, ld, N in ((3, 336, 80, 70), (2, 336, 18, 0), (2, 875, 256, 10)):
        out = (ctypes.c_int64 * 6)()
        L.check(lib.cvx_debug_yolo7_loss_layout(B, A, ld, N, out), "layout")
        cand, matched, mcount, state, cap, cmax = list(out)
        total = int(lib.cvx_yolo7_loss_workspace_bytes(B, A, ld, N))
        assert state == 0 and cap == max(15 * N, 1) and cmax == T.Y7_CMAX
        assert state < cand and cand + 3 * cap * 5 * 4 <= matched and matched + 3 * B * cmax * 16 <= mcount and mcount + B * 12 <= total
        assert all(v % 256 == 0 for v in (cand, matched, mcount))
    assert lib.cvx_debug_yolo7_loss_layout(0, 336, 80, 1, out) != 0


# ---- CenterNet loss ----------------------------------------------------------------------------------------------------------------------
def test_centernet_loss_case_properties():
    assert {(c.h, c.w) for c in T.CN_CASES} >= {(5, 7), (16, 16), (32, 24)} and {c.nc for c in T.CN_CASES} == {1, 3, 20, 80}
    assert {c.K for c in T.CN_CASES} == {1, 30} and T.cn_case("32x24_nc20_k30").nc_pad == 24
    span = {c.name: (c.B * c.h * c.w * c.nc, c.B * c.h * c.w * c.ld) for c in T.CN_CASES}
    assert [n for n, v in span.items() if v[0] > T.CN_REDUCE_SPAN] == ["32x24_nc80_k30", "64x64_nc80_k30"]
    assert span["32x24_nc80_k30"][0] // 2 < T.CN_REDUCE_SPAN                     # one image less and the second iteration is gone
    assert [n for n, v in span.items() if v[1] > T.CN_GRAD_SPAN] == ["64x64_nc80_k30"] and span["64x64_nc80_k30"][1] * 3 // 4 > T.CN_GRAD_SPAN - 4 * 64 * 96
    assert max(v[1] for v in span.values()) * 4 <= 6.5e6                           # the largest tensor: 6 MB
    pred, (heat, reg, wh, mask, idx) = T.cn_inputs("16x16_nc3_k30")
    below = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert int((heat == 1.0).sum()) >= 3 and int((heat == float(below)).sum()) == 3 and float(below) < 1.0
    A = 16 * 16
    on = idx[0][mask[0] == 1]
    assert int((on == 77).sum()) >= 3 and 0 in on.tolist() and A - 1 in on.tolist()
    m0 = mask[0].tolist()
    assert any(m0[k] == 1 and m0[k + 1] == 0 and 1 in m0[k + 2:] for k in range(len(m0) - 2))
    assert float(mask[1].sum()) == 0 and float(mask[2].sum()) == 30 and len(set(idx[2].tolist())) < 30
    for name in ("16x16_nc3_k30", "32x24_nc20_k30"):
        c = T.cn_case(name)
        pred, (heat, *_rest) = T.cn_inputs(name)
        _, grad = T.cn_reference(name)
        logit, g = pred[..., :c.nc], grad.reshape(c.B, c.h, c.w, c.ld)[..., :c.nc]
        for v in T.CLAMP_LOGITS:
            at = logit == v
            assert bool((at & (heat == 1.0)).any()) and bool((at & (heat < 1.0)).any()), (name, v)
            assert bool((g[at] == 0).all()) == (abs(v) >= 9.3), (name, v)                      # zero gradient outside the clamp, not inside
    p = torch.sigmoid(torch.tensor([9.3, -9.3, 9.2, -9.2], dtype=torch.float64))
    assert p[0] > 1 - 1e-4 > p[2] and p[1] < 1e-4 < p[3]


def test_centernet_loss_mutants_change_an_expected_output():
    for name in [c.name for c in T.CN_CASES]:
        c = T.cn_case(name)
        pred, targets = T.cn_inputs(name)
        items, grad = T.cn_reference(name)
        t64 = [t.double() if t.dtype != torch.long else t for t in targets]
        mine = T.cn_loss(pred.double(), t64, c.nc)
        assert all(float(a) == float(b) for a, b in zip(mine, items)), name
    g = T.cn_groups(T.cn_case("16x16_nc3_k30"))
    items, grad = T.cn_reference("16x16_nc3_k30")
    i10, g10 = T.cn_reference("16x16_nc3_k30", single_den=True)                      # 10: L1 denominator sum(mask)
    assert abs(float(i10[2]) / float(items[2]) - 2.0) < 1e-3 and T.rel(g10[..., g["a"]], grad[..., g["a"]]) > 0.9
    assert T.rel(g10, grad) < 0.2                                                     # ... which the whole-gradient L2 all but hides
    i11, g11 = T.cn_reference("16x16_nc3_k30", clamp_passes=True)                    # 11: gradient passed outside the clamp
    assert torch.equal(i11, items) and T.rel(g11[..., g["heat"]], grad[..., g["heat"]]) > 1e-2
    i12, g12 = T.cn_reference("16x16_nc3_k30", scatter_once=True)                    # 12: shared centre scattered once
    assert T.rel(g12[..., g["a"]], grad[..., g["a"]]) > 1e-2 and T.rel(g12[..., g["b"]], grad[..., g["b"]]) > 1e-2


# ---- CenterNet target drawing ------------------------------------------------------------------------------------------------------------
def test_draw_case_properties():
    assert {(c.H, c.W, c.nc) for c in T.DRAW_CASES} == {(24, 40, 80), (8, 8, 1)}
    for c in T.DRAW_CASES:
        lab, counts = T.draw_inputs(c.name)
        ref = T.draw_reference(c.name)
        mine = T.draw_reference(c.name, round_radius=False)
        assert all(np.array_equal(a, b) for r, m in zip(ref, mine) for a, b in zip(r, m)), c.name
        assert int(counts[0]) == c.K == lab.shape[1] and int(counts[3]) == 0                   # a full table, an empty one
        x, y, r, h, w = T.draw_geometry(c, lab[1, 0].numpy())
        assert h > c.H and w > c.W and r > x and r + 1 > c.W - x and r > y and r + 1 > c.H - y  # clipped on all four sides
        assert T.draw_geometry(c, lab[1, 1].numpy())[4] == 0 and T.draw_geometry(c, lab[1, 2].numpy())[3] == 0
        assert T.draw_geometry(c, lab[1, 3].numpy())[3:] == (0, 0)
        assert T.draw_geometry(c, lab[1, 4].numpy())[:2] == (c.W - 1, c.H - 1)
        assert float(ref[1][4][4]) == c.H * c.W - 1 and float(ref[1][0][c.H - 1, c.W - 1, 0]) == 1.0
        assert c.nc - 1 in lab[1, :6, 0].tolist() and float(ref[1][0][..., c.nc - 1].max()) == 1.0
        radii = [T.draw_geometry(c, lab[0, k].numpy())[2] for k in range(c.K)]
        assert len({int(v) for v in lab[0, :, 0].tolist()}) == 1 and len(set(radii)) >= 2
        assert np.array_equal(ref[0][0], ref[4][0]) and not np.array_equal(ref[0][1], ref[4][1])     # same heat map, the table reversed
    c = T.draw_case("24x40_nc80")
    lab, _ = T.draw_inputs(c.name)
    assert len({T.draw_geometry(c, lab[0, k].numpy())[2] for k in range(c.K)}) >= 6


def test_draw_mutants_change_an_expected_output():
    for mutant in (dict(round_radius=True), dict(sum_merge=True)):                     # 13, 14
        assert any(not np.array_equal(r[0], m[0]) for c in T.DRAW_CASES for r, m in zip(T.draw_reference(c.name), T.draw_reference(c.name, **mutant))), mutant


# ---- SSD target encoding -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", T.SSD_PRIOR_SETS)
def test_ssd_case_properties_and_mutants(which):
    pri = T.ssd_priors(which)
    lab, counts, notes = T.ssd_inputs(which)
    ref = T.ssd_reference(which)
    assert np.array_equal(ref, T.ssd_reference(which, force_always=False))
    assert len(pri) in (8732, 300) and (len(counts) * len(pri)) % 256 != 0 and list(counts[:3]) == [0, 1, T.SSD_NMAX]
    pos = ref[..., -1].sum(1)
    print(which, "positives per image", pos.tolist(), notes)
    assert pos[0] == 0 and np.array_equal(ref[0, :, 4], np.ones(len(pri), np.float32)) and pos[2] >= T.SSD_NMAX
    whole = T._iou64(pri, lab[3, 0])
    assert np.allclose(whole, (pri[:, 2] - pri[:, 0]) * (pri[:, 3] - pri[:, 1]), rtol=1e-6) and pos[3] == max(int((whole > T.SSD_THR).sum()), 1)     # IoU = the prior's area
    ia, ib = T._iou64(pri, lab[4, 0]), T._iou64(pri, lab[4, 1])
    p = notes["sliver_prior"]
    assert ia.max() <= T.SSD_THR and ib.max() <= T.SSD_THR and ia.argmax() == ib.argmax() == p and pos[4] == 1
    assert ref[4, p, 5 + int(lab[4, 0 if ia[p] > ib[p] else 1, 0])] == 1.0
    ia, ib = T._iou64(pri, lab[5, 0]), T._iou64(pri, lab[5, 1])
    p = notes["mirror_prior"]
    assert ia[p] == ib[p] > T.SSD_THR and not np.array_equal(lab[5, 0], lab[5, 1]) and ref[5, p, 5 + int(lab[5, 0, 0])] == 1.0      # the first wins
    out = T._iou64(pri, lab[6, 0])
    assert out.max() == 0.0 and pos[6] == 0 and np.array_equal(ref[6], ref[0])            # forced at IoU 0: not positive
    forced, last = T.ssd_reference(which, force_always=True), T.ssd_reference(which, last_on_ties=True)           # 15, 16
    assert not np.array_equal(forced, ref) and not np.array_equal(last[5], ref[5]) and np.array_equal(np.delete(last, 5, 0), np.delete(ref, 5, 0))
