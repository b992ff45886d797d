"""MI355X: the seeded sweep of the YOLOv8 loss chain -- ``V8LossOp`` (csrc/loss_v8.hip: task-aligned assigner, CIoU, DFL, BCE, eight
kernels) on the cases of tests/v8_loss_cases.py against the float64 expected output (the project's oracle with the kernel's filler rule;
tests/test_v8_loss_sweep_cpu.py shows from the oracle alone what each case was built to catch, that the assigner's discrete decisions keep
clear of float32 round-off and that the fp16 rounding of the scaled gradient costs at most 2.5e-4 per group).

Bounds: the target row of every anchor exact; normalised scores rtol 2e-5 / atol 1e-7 and loss items rtol 2e-5 (the existing bounds of
tests/test_gpu_parity.py); the gradient 5e-4 relative L2 (the project's bound) -- but separately per level, per column group (DFL 0:64,
classes 64:64+nc) and per anchor kind (foreground, background), not over the whole tensor; a group that is zero in the reference exactly
zero (the DFL columns of every background anchor); no NaN in the 64 + nc columns of a NaN-filled gradient buffer and nothing but NaN in its
padding.  Two runs on fresh ops are bit-identical, and so is every case on one op whose workspace still holds a larger earlier call.

Measured on the MI355X over the fifteen cases: every target row exact; normalised scores at most 6.9e-6 relative in fourteen cases and
4.0e-5 on one score of the fillers case (inside rtol + atol); loss items 8.7e-7; gradient groups DFL foreground 2.38e-4, classes foreground 2.37e-4, classes
background 2.36e-4 (the fp16 rounding of the scaled gradient: the CPU test's floor is 2.4e-4), the micro box's group 2.25e-4; all runs
bit-identical; 0.3 s for the crowd (which loads the library), 0.01 s for each of the others."""
import numpy as np
import pytest
import torch

import v8_loss_cases as T
from computervision.pytorch_amd import engine as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def run_case(dev, op, name):
    """one call of `op` on a case: (items (3,), dpred (B, A, ld) fp16, target row (B, A), normalised score (B, A)), on the host.  The
    targets go in as a device-resident collate dict in the case's own row order (the wrapper regroups them); where the case has a row
    pitch the prediction is the [..., :64 + nc] view of a buffer whose padding is NaN; the gradient buffer is NaN everywhere."""
    from computervision.pytorch_amd.train import flatten_targets
    c = T.v8_case(name)
    pred, batch = T.v8_inputs(c)
    rows = flatten_targets({k: v.to(dev) for k, v in batch.items()}, dev)
    assert torch.equal(rows.cpu(), T.v8_rows(batch))
    ld = c.ld or ((c.no + 3) & ~3)
    if c.ld:
        buf = torch.full((c.B, c.A, ld), float("nan"), dtype=torch.float32, device=dev)
        buf[..., :c.no] = pred.to(dev)
        x = buf[..., :c.no]
    else:
        x = pred.to(dev)
    dpred = torch.full((c.B, c.A, ld), float("nan"), dtype=torch.float16, device=dev)
    op.nc = c.nc
    items, dp = op(x, rows, list(c.levels), [float(s) for s in c.strides], c.scale, dpred)
    idx, norm = op.assignment(c.B, c.A, rows.shape[0])
    torch.cuda.synchronize()
    return items.cpu(), dp.cpu(), idx.cpu(), norm.cpu()


def same_bits(a, b):
    return all(torch.equal(u.view(torch.int16) if u.dtype == torch.float16 else u.view(torch.int32) if u.dtype == torch.float32 else u,
                           v.view(torch.int16) if v.dtype == torch.float16 else v.view(torch.int32) if v.dtype == torch.float32 else v)
               for u, v in zip(a, b))


@pytest.fixture(scope="module")
def fresh(dev):
    """the result of every case on an op of its own, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_case(dev, E.V8LossOp(T.v8_case(name).nc), name)
        return cache[name]

    return get


@pytest.mark.parametrize("name", T.V8_NAMES)
def test_v8_loss_sweep(dev, fresh, name):
    c = T.v8_case(name)
    ref = T.v8_reference(name)
    items, dp, idx, norm = fresh(name)
    # the assignment
    want_idx = ref["a"]["gt_index"]
    assert torch.equal(idx, want_idx), f"{int((idx != want_idx).sum())} anchors assigned differently: {torch.nonzero(idx != want_idx)[:8].tolist()}"
    want_norm = ref["a"]["norm"].numpy()
    nz = want_norm > 0
    norm_err = float((np.abs(norm.numpy()[nz] - want_norm[nz]) / want_norm[nz]).max()) if nz.any() else 0.0
    # the items
    got_items = items.double().numpy()
    want_items = ref["items"].numpy()
    item_err = float(np.abs(got_items / np.where(want_items == 0, 1.0, want_items) - 1)[want_items != 0].max())
    # the gradient
    assert not bool(torch.isnan(dp[..., :c.no]).any())
    assert bool(torch.isnan(dp[..., c.no:]).all())
    got = dp[..., :c.no].double() / c.scale
    errs = T.group_errors(c, want_idx, got, ref["grad"])
    shown = {f"L{lv} {cols} {kind}": float(f"{v:.3e}") for (lv, cols, kind), v in errs.items() if v is not None}
    print(f"{name}: norm {norm_err:.3e}, items {got_items.tolist()} error {item_err:.3e}, gradient groups {shown}")
    np.testing.assert_allclose(norm.numpy(), want_norm, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(got_items, want_items, rtol=2e-5, atol=0)
    for key, (m, cs) in T.v8_groups(c, want_idx).items():
        if errs[key] is None:
            assert float(got[m][:, cs].abs().max()) == 0.0, key
        else:
            assert errs[key] < T.GRAD_BOUND, (key, errs[key])
    for lv, sl in enumerate(c.level_slices()):                          # (stated on its own: every background anchor's DFL columns)
        assert float(got[:, sl][want_idx[:, sl] < 0][:, :64].abs().max() if bool((want_idx[:, sl] < 0).any()) else 0.0) == 0.0, lv


def test_v8_loss_is_bit_reproducible_and_ignores_stale_workspace(dev, fresh):
    """every case twice on fresh ops: bit-identical; then all cases in decreasing workspace size on ONE op, so that each call finds the
    overlap / metric / mask / target-index arrays of a larger call in its workspace (the empty case behind the 64 x 64 cases of two images
    with targets): bit-identical to the fresh-op result"""
    lib = E.L.load()
    for name in T.V8_NAMES:
        assert same_bits(run_case(dev, E.V8LossOp(T.v8_case(name).nc), name), fresh(name)), name

    def size(name):
        c = T.v8_case(name)
        return int(lib.cvx_loss_v8_workspace_bytes(c.B, c.A, c.nc, max(T.v8_inputs(c)[1]["batch_idx"].numel(), 1)))

    order = sorted(T.V8_NAMES, key=size, reverse=True)
    assert order.index("duplicates") < order.index("empty") and size(order[0]) > 10 * size("empty")     # same B and A, with targets, before it
    op = E.V8LossOp(80)
    for name in order:
        assert same_bits(run_case(dev, op, name), fresh(name)), name
    assert op._ws.numel() == size(order[0])                             # one allocation served them all
