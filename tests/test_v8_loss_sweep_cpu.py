"""CPU side of the YOLOv8 loss sweep (tests/v8_loss_cases.py): from the oracle alone -- every case is admissible (float32 and float64
assign identically, every margin >= 100 x the float32-vs-float64 difference of the same quantity), has the property it was built for,
the restatement equals oracle/yolov8_ref.py in both precisions, the filler rule differs from ``torch.topk`` exactly where stated, every
mutant changes the expected output of a named case by more than the GPU test's bounds, and the fp16 rounding of the scaled float64
gradient stays below 2.5e-4 in every group (which is what leaves the GPU test's 5e-4 per group meaningful)."""
import numpy as np
import pytest
import torch

import v8_loss_cases as T
from oracle import yolov8_ref as O

# the cases in which fillers="topk" (the oracle) and fillers="none" (the kernel's rule, the expected output) assign differently
FILLER_CASES = ("fillers",)


def assert_same(r, o, dtype, what):
    assert torch.equal(r["a"]["gt_index"], o["gt_index"]), what
    assert torch.equal(r["a"]["norm"], o["norm"]), what
    tol = 1e-6 if dtype == torch.float32 else 1e-13
    np.testing.assert_allclose(r["items"].numpy(), o["items"].numpy(), rtol=tol, atol=0, err_msg=what)
    assert float((r["grad"] - o["grad"]).abs().max()) <= tol * float(o["grad"].abs().max()), what


@pytest.mark.parametrize("name", T.V8_NAMES)
def test_v8_case_is_admissible(name):
    """float32 == float64 assignment; the four margins (inside-the-box, positive-vs-zero metric, tenth-vs-eleventh metric, the two largest
    overlaps of a multiply claimed anchor) each >= 100 x the float32-vs-float64 difference of that quantity; no positive metric anywhere
    near float32 underflow; and the restatement equals the oracle in both precisions -- with fillers="topk" everywhere, with
    fillers="none" (the expected output) everywhere but in FILLER_CASES."""
    m = T.v8_margins(name)
    print(f"{name}: " + ", ".join(f"{k} margin {v[0]:.3e} difference {v[1]:.3e}" for k, v in m["kinds"].items())
          + f"; centres on an edge {m['edge_ties']}, tied overlaps {m['overlap_ties']}, smallest positive metric {m['min_metric']:.3e}")
    assert m["same"]
    assert m["min_metric"] >= T.MIN_POSITIVE_METRIC
    for kind, (margin, diff) in m["kinds"].items():
        assert margin >= T.MARGIN_FACTOR * diff, (kind, margin, diff)
    assert m["admissible"]
    for dtype in (torch.float32, torch.float64):
        o = T.v8_oracle(name, dtype)
        assert o["items"].dtype == dtype and o["grad"].dtype == dtype
        assert_same(T.v8_run(name, dtype, fillers="topk"), o, dtype, (name, dtype, "topk"))
        if name not in FILLER_CASES:
            assert_same(T.v8_run(name, dtype), o, dtype, (name, dtype, "none"))
    ref, o = T.v8_reference(name), T.v8_oracle(name, torch.float32)
    assert ref["items"].dtype == torch.float64
    if name not in FILLER_CASES:                                        # float64 against the reference's own precision: round-off only
        np.testing.assert_allclose(o["items"].double().numpy(), ref["items"].numpy(), rtol=1e-5)


def test_v8_float32_oracle_is_unchanged_by_the_dtype_argument():
    c = T.v8_case("nonsquare")
    pred, batch = T.v8_inputs(c)
    strides = tuple(float(s) for s in c.strides)
    out = []
    for kw in ({}, {"dtype": torch.float32}):
        p = pred.clone().requires_grad_(True)
        aux = {}
        loss, items = O.v8_loss(T.v8_feats(c, p), batch, c.nc, strides, T.GAINS, aux, **kw)
        loss.backward()
        out.append([loss.detach(), items, p.grad, aux["target_scores"], aux["target_bboxes"], aux["target_gt_idx"]])
    assert all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(*out)) and out[0][0].dtype == torch.float32
    a, b = O.build_targets(batch, c.B, *map(float, c.hw)), O.build_targets(batch, c.B, *map(float, c.hw), dtype=torch.float32)
    assert a.dtype == torch.float32 and torch.equal(a, b)
    assert O.build_targets(batch, c.B, *map(float, c.hw), dtype=torch.float64).dtype == torch.float64
    d = T.v8_oracle("nonsquare", torch.float64)["items"]
    assert d.dtype == torch.float64 and float((d - out[0][1].double()).abs().max()) < 1e-5 * float(d.sum())


@pytest.mark.parametrize("name", T.V8_NAMES)
def test_v8_case_properties(name):
    """the property each case was built for (V8_PROPERTY), from the float64 expected output, which test_v8_case_is_admissible ties to the
    oracle"""
    f = T.v8_facts(name)
    print(name, {k: v for k, v in f.items() if k not in ("valid", "pos_align", "kept_per_level")})
    assert T.V8_PROPERTY[name](f), f
    c = T.v8_case(name)
    assert c.A == {"crowd": 336, "duplicates": 84, "huge": 1344, "nonsquare": 315, "levels4": 340}.get(name, c.A)
    if name == "nonsquare":
        assert all(h != w for h, w in c.levels) and c.hw[0] != c.hw[1] and c.ld == 88 > c.no and c.nc == 20
    if name in ("levels1", "levels2", "levels4"):
        assert len(c.strides) == int(name[-1])
    if name in ("nc1", "nc3"):
        assert c.nc == int(name[-1]) and c.nc & 3 and -1 in f["labels"]                                # (a label below the range: clamped to class 0)
    if name == "edge_on":
        a = T.v8_reference(name)["a"]
        H, W = c.hw
        b = a["gtbox"][a["valid"]]
        assert bool((b[:, 0] < 0).any() and (b[:, 1] < 0).any() and (b[:, 2] > W).any() and (b[:, 3] > H).any())
        assert float(a["gtbox"][~a["valid"]].sum()) == 0.0             # the corner sum is exactly 0, not a rounding


def test_v8_filler_rule():
    """Only in FILLER_CASES do torch.topk's zero-metric fillers reach the assignment.  There, in both precisions: anchors 226 and 228 (inside
    row 0's box, metric 0 for it, claimed by nobody else) are zero-weight foreground for the oracle and background for the kernel's
    rule; anchor 227 has ONE claimant by a positive metric, row 0, which the kernel's rule keeps -- the oracle counts row 1's filler as
    a second claim and the overlap arg-max over all rows hands the anchor to row 2, which never selected it."""
    for name in T.V8_NAMES:
        for dtype in (torch.float64, torch.float32):
            d = T.filler_difference(name, dtype)
            if name not in FILLER_CASES:
                assert not any(d.values()), (name, d)
                continue
            assert d == dict(zero_weight=[(0, 226, 0), (0, 228, 0)], reassigned=[(0, 227, 2, 0, [0])], other=[]), d
    a, o = T.v8_reference("fillers")["a"], T.v8_oracle("fillers")
    for _, k, row in [(0, 226, 0), (0, 228, 0)]:
        assert float(o["norm"][0, k]) == 0.0 and int(o["gt_index"][0, k]) == row and bool(a["inbox"][row, k]) and float(a["metric"][row, k]) == 0.0
        assert int(a["claims"][0, k]) == 0
    assert float(a["metric"][0, 227]) > 0 and float(a["metric"][1, 227]) == 0.0 and bool(a["inbox"][1, 227]) and not bool(a["mask"][2, 227])
    assert int(a["ov"][:, 227].argmax()) == 2
    # the zero-weight anchors leave the loss alone; the reassigned one does not
    assert float((o["items"] - T.v8_reference("fillers")["items"]).abs().max()) > 1e-3


# mutant -> (switches of the restatement, the cases that must notice)
MUTANTS = {
    "top-9": (dict(topk=9), ("crowd", "huge", "levels4")),
    "claims resolved by metric": (dict(resolve="metric"), ("crowd", "duplicates")),
    "arg-max over the claimants only": (dict(claimants_only=True), ("crowd", "fillers")),
    "`>=` in the box test": (dict(box_ge=True), ("edge_on",)),
    "zero metrics selectable": (dict(fillers="inbox"), ("tiny", "fillers")),
    "DFL clamp at 15": (dict(dfl_clamp=15.0), ("huge",)),
    "gradient through alpha": (dict(alpha_grad=True), ("crowd", "low_score")),
    "eps on the widths too": (dict(eps_w=True), ("low_score",)),
    "no clamp of the score sum": (dict(clamp_sum=False), ("low_score",)),
    "pos_align before the resolution": (dict(pos_before=True), ("crowd",)),
    "last row wins ties": (dict(last_wins=True), ("duplicates",)),
    "validity by area": (dict(valid_area=True), ("edge_on",)),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_v8_mutant_changes_the_expected_output(mutant):
    """each wrong restatement changes the assignment, a loss item by more than 2e-5 or a gradient group by more than 5e-4 (the GPU test's
    bounds) in every case listed for it"""
    sw, cases = MUTANTS[mutant]
    for name in cases:
        c, ref, r = T.v8_case(name), T.v8_reference(name), T.v8_run(name, **sw)
        moved = int((r["a"]["gt_index"] != ref["a"]["gt_index"]).sum())
        items = float(((r["items"] - ref["items"]).abs() / ref["items"].abs()).max())
        groups = T.group_errors(c, ref["a"]["gt_index"], r["grad"], ref["grad"])
        worst = max([v for v in groups.values() if v is not None], default=0.0)
        print(f"{mutant} on {name}: {moved} anchors assigned differently, items {items:.2e}, worst gradient group {worst:.2e}")
        assert moved > 0 or items > T.ITEM_RTOL or worst > T.GRAD_BOUND, (mutant, name)


@pytest.mark.parametrize("name", T.V8_NAMES)
def test_v8_fp16_floor(name):
    """the float64 gradient times the case's loss scale, rounded to fp16: no group (level x DFL / class columns x foreground / background)
    is off by more than 2.5e-4 relative L2, none overflows, and the DFL columns of the background anchors are exactly zero"""
    c = T.v8_case(name)
    floor = T.v8_fp16_floor(name)
    print(name, "scale", c.scale, {k: (None if v is None else float(f"{v:.3e}")) for k, v in floor.items()})
    for (lv, cols, kind), v in floor.items():
        if (cols, kind) == ("dfl", "bg"):
            assert v is None
        else:
            assert v is not None and v <= T.FP16_FLOOR, ((lv, cols, kind), v)
