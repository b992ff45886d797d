"""GPU (MI355X): the BatchNorm backward pair -- bn_bwd_reduce + bn_bwd_apply (csrc/bn_act.hip) -- around the hand-off of the per-channel
sums: the reduce pass scatters them over replica slabs, every workgroup of the apply pass folds the slabs (fold_replicas, bn_common.h)
before it touches a row.

Called through ``cvx_debug_bn_bwd_views`` (the two passes as the engine calls them: strided gradient / residual views, kept xhat or kept
raw fp16 output) against the fp64 formula on the CPU, evaluated on the SAME fp16 operands:

    xhat = kept                       or (kept - mean) * invstd for a raw-fp16 layer
    dz   = g * act'(gamma * xhat + beta [+ residual value])      (ReLU: the mask is the lowest bit of the kept xhat)
    dy   = gamma * invstd * (dz - mean(dz) - xhat * mean(dz * xhat)),   dgamma += sum(dz * xhat),   dbeta += sum(dz)
    gres = g (residual behind the activation) or dz (residual inside it)  [+ what gres held]

Bounds: those of the existing units of these passes (test_gpu_parity.py: test_bn_silu_train_and_backward_unit /
test_bn_act_train_and_backward_unit): dy 2e-3, dgamma / dbeta 1e-3, residual gradient 5e-4 relative L2.

Sizes come from ``cvx_debug_bn_bwd_plan`` (rows per workgroup, rows of one trip), batch 2 unless noted:
  short   one workgroup shorter than a first trip (row by row only),
  trip    one workgroup of exactly one trip,
  ragged  three workgroups, the last one a trip and six rows (a trip, then the row-by-row tail),
  partial batch 1: two workgroups, the last one just short of a trip -- only its first row slots have a whole trip.
Every case runs twice from the same inputs: bit-identical.  Outputs start as NaN with a NaN guard band behind them (and NaN around a
channel slice): afterwards the band is still NaN and the output holds none.
"""
import ctypes as C

import pytest
import torch

from computervision.pytorch_amd import _lib as L
from test_conv_dma_gpu import _rel

pytestmark = pytest.mark.gpu

TOL_DY, TOL_COEF, TOL_GRES = 2e-3, 1e-3, 5e-4   # the existing units' bounds (module docstring)
GUARD = 256
KINDS = {  # act (0 SiLU, 1 ReLU, 2 none), residual inside the activation, kept tensor is the raw fp16 output
    "silu": (0, 0, False), "silu_raw16": (0, 0, True), "relu": (1, 0, False), "none": (2, 0, False),
    "silu_respre": (0, 1, False), "relu_respre": (1, 1, False), "none_respre": (2, 1, False),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _plan(M, c):
    out = (C.c_int32 * 4)()
    L.check(L.load().cvx_debug_bn_bwd_plan(M, c, out), "cvx_debug_bn_bwd_plan")
    return tuple(out)   # rows per workgroup, rows per step, rows of a trip, workgroups


def _sizes(c):
    """(name, batch, hw, workgroups) -- see the module docstring"""
    rows, rp, trip, _ = _plan(1 << 12, c)
    assert trip % 2 == 0 and rows >= trip and rows % rp == 0
    return [("short", 2, trip // 2 - 1, 1), ("trip", 2, trip // 2, 1), ("ragged", 2, rows + trip // 2 + 3, 3),
            ("partial", 1, rows + trip - max(1, rp // 2), 2)]


def _modes(act, res_pre):
    """residual gradient: None (no residual branch), 0 (written), 1 (accumulated)"""
    if res_pre:
        return [0, 1]
    return [None] if act == 1 else [None, 0, 1]   # ReLU with a residual behind the activation is refused


class _View:
    """a (B, hw, c) fp16 operand: dense, or channels [8, 8 + c) of a wider buffer whose images do not follow each other directly
    (bstride != hw * ld: view_off's division path); NaN everywhere outside the operand and in a guard band behind it"""

    def __init__(self, B, hw, c, sliced, dev, values=None):
        self.ld = c + 24 if sliced else c
        self.bstride = hw * self.ld + (40 if sliced else 0)
        self.off = 8 if sliced else 0
        self.flat = torch.full((B * self.bstride + GUARD,), float("nan"), dtype=torch.float16, device=dev)
        self.B, self.hw, self.c = B, hw, c
        if values is not None:
            self.view().copy_(values.to(dev).view(B, hw, c))

    def view(self):
        return torch.as_strided(self.flat, (self.B, self.hw, self.c), (self.bstride, self.ld, 1), self.off)

    def ptr(self):
        return C.c_void_p(self.flat.data_ptr() + 2 * self.off)

    def outside_is_nan(self):
        mask = torch.ones_like(self.flat, dtype=torch.bool)
        torch.as_strided(mask, (self.B, self.hw, self.c), (self.bstride, self.ld, 1), self.off).fill_(False)
        return bool(torch.isnan(self.flat[mask]).all())


def _reference(kept, g, fo, old, gamma, beta, mean, invstd, act, res_pre, raw, inv_scale, mode, d0):
    """fp64, on the fp16 operands (M, c) -> dy, dgamma, dbeta, gres"""
    k64 = kept.double()
    xh = (k64 - mean.double()) * invstd.double() if raw else k64
    g64 = g.double()
    if act == 1:
        dz = g64 * (kept.view(torch.int16) & 1).double()
    elif act == 0:
        pre = xh * gamma.double() + beta.double() + (fo.double() if res_pre else 0.0)
        s = torch.sigmoid(pre)
        dz = g64 * s * (1.0 + pre * (1.0 - s))
    else:
        dz = g64
    M = kept.shape[0]
    s0, s1 = dz.sum(0), (dz * xh).sum(0)
    dy = gamma.double() * invstd.double() * (dz - s0 / M - xh * (s1 / M))
    gres = None
    if mode is not None:
        gres = (dz if res_pre else g64) + (old.double() if mode else 0.0)
    return dy, d0 + s1 * inv_scale, d0 + s0 * inv_scale, gres


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("c", [16, 32, 80, 144, 256])   # 80 and 144: the channel groups do not divide a wave (the column walk of the sums)
def test_bn_backward_pair_handoff(dev, c, kind):
    lib = L.load()
    st = L.stream_ptr(dev)
    act, res_pre, raw = KINDS[kind]
    inv_scale, d0 = 0.5, 0.25
    for name, B, hw, blocks in _sizes(c):
        M = B * hw
        assert _plan(M, c)[3] == blocks, (name, "the size no longer meets the path it was chosen for")
        gen = torch.Generator().manual_seed(1000 * c + 10 * hw + act + 3 * res_pre)
        gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.3
        if raw:
            y = (torch.randn(M, c, generator=gen) * (torch.rand(c, generator=gen) * 3 + 0.2) + torch.randn(c, generator=gen) * 2).half()
            mean = y.double().mean(0).float()
            invstd = (y.double().var(0, unbiased=False) + 1e-3).rsqrt().float()
            kept = y
        else:
            kept, mean, invstd = torch.randn(M, c, generator=gen).half(), None, torch.rand(c, generator=gen) + 0.5
        g = torch.randn(M, c, generator=gen).half()
        fo = torch.randn(M, c, generator=gen).half() if (act == 0 and res_pre) else None
        old = torch.randn(M, c, generator=gen).half()
        keptd, gammad, betad, invstdd = kept.to(dev), gamma.to(dev), beta.to(dev), invstd.to(dev)
        meand = mean.to(dev) if raw else None
        for mode in _modes(act, res_pre):
            want = _reference(kept, g, fo, old, gamma, beta, mean, invstd, act, res_pre, raw, inv_scale, mode, d0)
            for sliced in (False, True):
                tag = (kind, c, name, B, hw, "gres", mode, "slice" if sliced else "dense")
                gv = _View(B, hw, c, sliced, dev, g)
                fv = _View(B, hw, c, sliced, dev, fo) if fo is not None else None
                runs = []
                for _ in range(2):
                    dy = torch.full((M * c + GUARD,), float("nan"), dtype=torch.float16, device=dev)
                    rv = None if mode is None else _View(B, hw, c, sliced, dev, old if mode else None)
                    dgam, dbet = torch.full((c,), d0, device=dev), torch.full((c,), d0, device=dev)
                    L.check(lib.cvx_debug_bn_bwd_views(
                        L.ptr(keptd), B, hw, c, L.ptr(gammad), L.ptr(betad), L.ptr(invstdd), L.ptr(meand), act, res_pre, inv_scale,
                        gv.ptr(), gv.bstride, gv.ld, fv.ptr() if fv else None, fv.bstride if fv else 0, fv.ld if fv else 0,
                        rv.ptr() if rv else None, rv.bstride if rv else 0, rv.ld if rv else 0, 1 if mode else 0,
                        L.ptr(dgam), L.ptr(dbet), L.ptr(dy), st), "cvx_debug_bn_bwd_views")
                    assert bool(torch.isnan(dy[M * c:]).all()), (tag, "dy: guard band overwritten")
                    assert not bool(torch.isnan(dy[:M * c]).any()), (tag, "dy: rows left unwritten")
                    assert gv.outside_is_nan() and (fv is None or fv.outside_is_nan()), (tag, "an input view was written")
                    gr = None
                    if rv is not None:
                        assert rv.outside_is_nan(), (tag, "gres: written outside its view")
                        gr = rv.view().reshape(M, c).cpu()
                        assert not bool(torch.isnan(gr).any()), (tag, "gres: rows left unwritten")
                    runs.append((dy[:M * c].view(M, c).cpu(), dgam.cpu(), dbet.cpu(), gr))
                a, b = runs
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (tag, "two runs differ")
                assert a[3] is None or torch.equal(a[3], b[3]), (tag, "two runs differ (gres)")
                e = [_rel(a[0], want[0]), _rel(a[1], want[1]), _rel(a[2], want[2]), _rel(a[3], want[3]) if a[3] is not None else 0.0]
                print(f"[bn handoff] {tag}: dy {e[0]:.2e} dgamma {e[1]:.2e} dbeta {e[2]:.2e} gres {e[3]:.2e}")
                assert e[0] < TOL_DY and e[1] < TOL_COEF and e[2] < TOL_COEF and e[3] < TOL_GRES, (tag, e)
