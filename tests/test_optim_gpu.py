"""GPU (MI355X): ``cvx_optim_step`` / ``cvx_grad_norm``, ``FlatSGD`` / ``FlatAdamW``, the train steps and a trainer on top of them.

The kernel comparisons are bit-exact (``torch.equal``): SGD, the decay multiply and the clip coefficient against tests/optim_restatement.py
(numpy fp32, one rounding per operation; tests/test_optim_cpu.py pins it against torch), the ADAM kind against ``cvx_adam_step_dev`` --
the ungrouped instantiation of the same kernel body; the Adam core is csrc/optim_core.h's, and every Adam entry point replays
tests/golden/adam_trace.npz, recorded on the device before the kernels were folded into one --, the fused average against the two-launch
form.  Clipped steps are fed the norm the
device measured, so the reduction order is not part of the bit-exact claim; the norm itself is held to 1e-5 of the fp64 norm (a tree sum
of n <= 2^22 fp32 squares is bounded by about log2(n) 2^-24 = 1.3e-6; the rest is room for the square root and the partition)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import optim_restatement as R  # noqa: E402
from computervision.pytorch_amd import _lib as L  # noqa: E402
from computervision.pytorch_amd import engine as E  # noqa: E402
from computervision.pytorch_amd import optim as O  # noqa: E402
from computervision.pytorch_amd.ema import ModelEMA  # noqa: E402
from oracle import synth  # noqa: E402

F = np.float32
GUARD = 64
PLAN = [dict(inf=0, zg=True), dict(inf=0, zg=False), dict(inf=1, zg=True), dict(inf=0, zg=False), dict(inf=0, zg=True)]   # test_ema_gpu.py's
LENGTHS = [3, 21, 64, 255, 576, 4099, 30001]
BETAS, EPS = (0.9, 0.999), 1e-8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def make_map(n, n_groups=4, holes=True):
    """Segments of logical lengths 3, 21, 64, 255, 576 ... on 4-aligned offsets, groups in turn, an unmapped chunk after every second one:
    last chunks carry padding lanes, and for n >= 1020 all of groups 0..3 and unmapped chunks occur."""
    gmap = np.full((n + 3) // 4, R.UNMAPPED, np.uint8)
    off = j = 0
    while off < n:
        length = min(LENGTHS[j % len(LENGTHS)], n - off)
        c1 = (off + length + 3) // 4
        gmap[off // 4:c1] = j % n_groups
        off = c1 * 4 + (4 if holes and j % 2 == 1 else 0)
        j += 1
    return gmap


def rows_for(mode):
    mu, nes = dict(plain=(0.0, 0.0), momentum=(0.9, 0.0), nesterov=(0.937, 1.0))[mode]
    base = [dict(lr=1e-2, wd=5e-4, frozen=0.0), dict(lr=3e-3, wd=0.0, frozen=0.0), dict(lr=2e-2, wd=1e-3, frozen=0.0),
            dict(lr=1e-2, wd=5e-4, frozen=1.0)]
    return [dict(r, mu=mu, nesterov=nes) for r in base]


def table(rows, kind, dev):
    if kind == E.OPTIM_SGD:
        t = [[r["lr"], r["wd"], 1.0, r["frozen"], r["mu"], r["nesterov"], 0.0, 0.0] for r in rows]
    else:
        t = [[r["lr"], 0.0, O.decay_factor(r["lr"], r["wd"]), r["frozen"], 0.0, 0.0, 0.0, 0.0] for r in rows]
    return torch.tensor(t, dtype=torch.float32, device=dev)


def element_groups(gmap, n):
    return np.repeat(gmap, 4)[:n]


def live_mask(gid, rows):
    frozen = np.array([r["frozen"] for r in rows] + [1.0] * (256 - len(rows)), F)
    return frozen[gid] == 0


def host_sgd(p, b, g, gid, rows, gscale, coef, skip):
    k = np.where(gid == R.UNMAPPED, 0, gid)
    col = lambda name: np.array([r[name] for r in rows], F)[k]   # noqa: E731
    g2 = R.scaled_grad(g, gscale, coef)
    pa, ba = R.sgd_step(p, b, g2, col("lr"), col("wd"), col("mu"), False)
    pb, bb = R.sgd_step(p, b, g2, col("lr"), col("wd"), col("mu"), True)
    nes = col("nesterov") != 0
    live = live_mask(gid, rows) & (not skip)
    return np.where(live, np.where(nes, pb, pa), p), np.where(live, np.where(nes, bb, ba), b)


class Arenas:
    """n values in front of a guard region, 16-byte aligned"""

    def __init__(self, n, dev, seed, names=("p", "g", "a", "b", "e")):
        gen = torch.Generator().manual_seed(seed)
        self.n = n
        self.full = {k: torch.randn(n + GUARD, generator=gen).to(dev) for k in names}
        for k in ("a", "b"):
            if k in self.full:
                self.full[k][:n] = 0
        self.guard0 = {k: v[n:].clone() for k, v in self.full.items()}
        self.grads = [torch.randn(n, generator=gen) * (10.0 ** (i - 2)) for i in range(5)]

    def __getattr__(self, k):
        return self.full[k][:self.n]

    def guards_intact(self):
        return all(torch.equal(v[self.n:], self.guard0[k]) for k, v in self.full.items())


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- 1. SGD against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "momentum", "nesterov"])
@pytest.mark.parametrize("n", [3, 4, 12, 1020, 1024, 1027, 1028, 4100, 262148])
def test_sgd_kernel_is_bit_identical_to_the_restatement(dev, n, mode):
    """Three live groups of different lr and lambda, a frozen group, unmapped chunks, a guard behind n; 5 steps, one skipped by found_inf,
    zero_grad both ways, grad_scale 0.5.  n = 3 and 1027 run the scalar tail."""
    rows, gmap = rows_for(mode), make_map(n)
    gid = element_groups(gmap, n)
    if n >= 1020:
        assert set(np.unique(gmap)) == {0, 1, 2, 3, R.UNMAPPED}
    A = Arenas(n, dev, n, names=("p", "g", "a"))
    gs, dmap = table(rows, E.OPTIM_SGD, dev), torch.from_numpy(gmap).to(dev)
    state = torch.zeros(4, device=dev)
    found = torch.zeros(1, dtype=torch.int32, device=dev)
    p, b = A.p.cpu().numpy().copy(), np.zeros(n, F)
    still = ~live_mask(gid, rows)
    for i, st in enumerate(PLAN):
        A.g.copy_(A.grads[i].to(dev))
        found.fill_(st["inf"])
        count = float(state[1])
        E.optim_step(E.OPTIM_SGD, A.p, A.g, A.a, None, dmap, gs, state, found_inf=found, zero_grad=st["zg"], grad_scale=0.5)
        torch.cuda.synchronize()
        p_new, b_new = host_sgd(p, b, A.grads[i].numpy(), gid, rows, 0.5, None, bool(st["inf"]))
        assert np.array_equal(p_new[still].view(np.uint32), p[still].view(np.uint32)) and np.array_equal(b_new[still], b[still])
        p, b = p_new, b_new
        assert np.array_equal(bits(A.p), p.view(np.uint32)), f"step {i}: p"
        assert np.array_equal(bits(A.a), b.view(np.uint32)), f"step {i}: momentum buffer"
        assert torch.equal(A.g.cpu(), torch.zeros(n) if st["zg"] else A.grads[i]), f"step {i}: gradients (frozen and unmapped chunks included)"
        assert float(state[1]) == count + (0 if st["inf"] else 1)
        assert A.guards_intact()


# ---- 2. the ADAM kind against the existing kernel -------------------------------------------------------------------------------------
def adam_reference(n, dev, seed, lr, wd=0.0, pre=None):
    """cvx_adam_step_dev over the plan; with wd the decay as torch's own multiply of the device tensor by the fp32 factor first"""
    A = Arenas(n, dev, seed, names=("p", "g", "a", "b"))
    state = torch.tensor([lr, 0.0, 0.0, 0.0], device=dev)
    found = torch.zeros(1, dtype=torch.int32, device=dev)
    trace = []
    for i, st in enumerate(PLAN):
        A.g.copy_(A.grads[i].to(dev))
        found.fill_(st["inf"])
        if wd and not st["inf"]:
            A.p.mul_(O.decay_factor(lr, wd))
        E.adam_step_dev(A.p, A.g, A.a, A.b, BETAS, EPS, state, found, st["zg"], 0.5)
        torch.cuda.synchronize()
        trace.append([t.clone().cpu() for t in (A.p, A.a, A.b, A.g, state)])
    return trace


def adam_grouped(n, dev, seed, rows, gmap):
    A = Arenas(n, dev, seed, names=("p", "g", "a", "b"))
    gs, dmap = table(rows, E.OPTIM_ADAM, dev), torch.from_numpy(gmap).to(dev)
    state = torch.tensor([rows[0]["lr"], 0.0, 0.0, 0.0], device=dev)
    found = torch.zeros(1, dtype=torch.int32, device=dev)
    trace = []
    for i, st in enumerate(PLAN):
        A.g.copy_(A.grads[i].to(dev))
        found.fill_(st["inf"])
        E.optim_step(E.OPTIM_ADAM, A.p, A.g, A.a, A.b, dmap, gs, state, BETAS, EPS, found, st["zg"], 0.5)
        torch.cuda.synchronize()
        assert A.guards_intact()
        trace.append([t.clone().cpu() for t in (A.p, A.a, A.b, A.g, state)])
    return trace


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("n", [3, 1027, 4100, 262148])
def test_adam_kind_equals_the_existing_adam_kernel(dev, n, wd):
    """One group, no clip, no freeze, a map without holes: p, m, v, g and the whole state equal cvx_adam_step_dev's over the 5-step plan --
    with lambda > 0 after torch's multiply by the fp32 factor."""
    rows = [dict(lr=1e-2, wd=wd, frozen=0.0)]
    want = adam_reference(n, dev, n, 1e-2, wd)
    got = adam_grouped(n, dev, n, rows, np.zeros((n + 3) // 4, np.uint8))
    for i, (a, b) in enumerate(zip(got, want)):
        for name, x, y in zip(("p", "m", "v", "g", "state"), a, b):
            assert np.array_equal(bits(x), bits(y)), f"step {i}: {name}"


@pytest.mark.parametrize("n", [1027, 4100])
def test_adam_kind_two_groups_equal_one_group_runs(dev, n):
    rows = [dict(lr=1e-2, wd=0.0, frozen=0.0), dict(lr=3e-3, wd=0.02, frozen=0.0)]
    gmap = make_map(n, n_groups=2, holes=False)
    gid = torch.from_numpy(element_groups(gmap, n).astype(np.int64))
    got = adam_grouped(n, dev, n, rows, gmap)
    singles = [adam_reference(n, dev, n, r["lr"], r["wd"]) for r in rows]
    assert set(gid.tolist()) == {0, 1}
    for i in range(len(PLAN)):
        for j, name in enumerate(("p", "m", "v", "g")):
            want = torch.where(gid == 0, singles[0][i][j], singles[1][i][j])
            assert np.array_equal(bits(got[i][j]), bits(want)), f"step {i}: {name}"
        assert float(got[i][4][1]) == float(singles[0][i][4][1])


# ---- 2b. the Adam bits against the recorded trace -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adam_trace(gold):
    return gold("adam_trace.npz")


@pytest.mark.parametrize("path", ["dev", "ema", "host", "grouped"])
@pytest.mark.parametrize("n", [3, 4, 1027, 1028])
def test_adam_entry_points_replay_the_recorded_trace(dev, adam_trace, n, path):
    """tests/golden/adam_trace.npz (tools/make_adam_golden.py) holds what cvx_adam_step_dev, cvx_adam_ema_step_dev and cvx_adam_step left
    behind over PLAN on the build its ``commit`` names.  Every entry point, and cvx_optim_step(ADAM, one group, a map without holes, no
    decay) against the ``dev`` leg, leaves the same bits in p, m, v, g, the state and the average after every step, and the guards alone."""
    T = adam_trace
    leg = "dev" if path == "grouped" else path
    lr, betas, eps, gscale, d = float(T["lr"]), tuple(float(x) for x in T["betas"]), float(T["eps"]), float(T["grad_scale"]), float(T["d"])
    A = Arenas(n, dev, 0)
    A.p.copy_(torch.from_numpy(T[f"n{n}_p0"]))
    A.e.copy_(torch.from_numpy(T[f"n{n}_e0"]))
    grads = T[f"n{n}_grads"]
    state0 = torch.tensor([lr, 0.0, 0.0, 0.0], device=dev)
    state = state0.clone()
    found = torch.zeros(1, dtype=torch.int32, device=dev)
    gs = table([dict(lr=lr, wd=0.0, frozen=0.0)], E.OPTIM_ADAM, dev)
    dmap = torch.zeros((n + 3) // 4, dtype=torch.uint8, device=dev)
    arenas = dict(p=A.p, m=A.a, v=A.b, g=A.g, state=state, **({"e": A.e} if path == "ema" else {}))
    for i, st in enumerate(PLAN):
        A.g.copy_(torch.from_numpy(grads[i]))
        found.fill_(st["inf"])
        if path == "dev":
            E.adam_step_dev(A.p, A.g, A.a, A.b, betas, eps, state, found, st["zg"], gscale)
        elif path == "ema":
            E.adam_ema_step_dev(A.p, A.g, A.a, A.b, betas, eps, state, A.e, d, 1.0 - d, found, st["zg"], gscale)
        elif path == "host":
            E.adam_step(A.p, A.g, A.a, A.b, lr, betas, eps, i + 1, found, st["zg"])
        else:
            E.optim_step(E.OPTIM_ADAM, A.p, A.g, A.a, A.b, dmap, gs, state, betas, eps, found, st["zg"], gscale)
        torch.cuda.synchronize()
        for name, t in arenas.items():
            key = f"n{n}_{leg}_{name}"
            if key in T.files:
                assert np.array_equal(bits(t), T[key][i].view(np.uint32)), f"step {i}: {name}"
        assert A.guards_intact()
    if path != "ema":
        assert np.array_equal(bits(A.e), T[f"n{n}_e0"].view(np.uint32))
    if path == "host":
        assert torch.equal(state, state0)


# ---- 3. the fused average -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [E.OPTIM_SGD, E.OPTIM_ADAM])
@pytest.mark.parametrize("n", [1027, 4100])
def test_fused_average_equals_step_then_ema_update_on_the_mapped_chunks(dev, n, kind):
    rows, gmap = rows_for("nesterov"), make_map(n)
    mapped = torch.from_numpy(element_groups(gmap, n) != R.UNMAPPED).to(dev)
    runs = []
    for fused in (True, False):
        A = Arenas(n, dev, n)
        gs, dmap = table(rows, kind, dev), torch.from_numpy(gmap).to(dev)
        state = torch.zeros(4, device=dev)
        found = torch.zeros(1, dtype=torch.int32, device=dev)
        trace = []
        for i, st in enumerate(PLAN):
            A.g.copy_(A.grads[i].to(dev))
            found.fill_(st["inf"])
            d = 0.9 + 0.01 * i
            omd = 1 - d
            before = (A.p.clone(), A.e.clone())
            buf2 = A.b if kind == E.OPTIM_ADAM else None
            if fused:
                E.optim_step(kind, A.p, A.g, A.a, buf2, dmap, gs, state, BETAS, EPS, found, st["zg"], 0.5, None, A.e, d, omd)
            else:
                E.optim_step(kind, A.p, A.g, A.a, buf2, dmap, gs, state, BETAS, EPS, found, st["zg"], 0.5)
                whole = A.e.clone()
                E.ema_update(whole, A.p.clone(), d, omd)
                A.e.copy_(torch.where(mapped, whole, A.e))
            torch.cuda.synchronize()
            assert A.guards_intact()
            if st["inf"]:
                assert torch.equal(A.p, before[0]) and not torch.equal(A.e[mapped], before[1][mapped])       # the average moves on a skipped step
            assert torch.equal(A.e[~mapped], before[1][~mapped])
            trace.append([t.clone().cpu() for t in (A.p, A.a, A.b, A.g, A.e, state)])
        runs.append(trace)
    for i, (a, b) in enumerate(zip(*runs)):
        for name, x, y in zip(("p", "buf1", "buf2", "g", "ema", "state"), a, b):
            assert np.array_equal(bits(x), bits(y)), f"step {i}: {name} differs between the fused and the two-launch step"


# ---- 4. the norm and clipping ---------------------------------------------------------------------------------------------------------
def norm_setup(n, dev, rows, gmap, seed=0):
    gen = torch.Generator().manual_seed(seed)
    g = (torch.randn(n, generator=gen) * 3.0).to(dev)
    return g, table(rows, E.OPTIM_SGD, dev), torch.from_numpy(gmap).to(dev), torch.zeros(4, device=dev), torch.zeros(E.grad_norm_workspace(n), device=dev)


@pytest.mark.parametrize("n", [1027, 1028, 262148])
def test_grad_norm_is_deterministic_accurate_and_ignores_what_stands_still(dev, n):
    """n = 262148 gives cvx_grad_norm_workspace(n) = 65 first-stage partials, so a real second stage exists."""
    rows, gmap = rows_for("plain"), make_map(n)
    live = torch.from_numpy(live_mask(element_groups(gmap, n), rows)).to(dev)
    g, gs, dmap, clip, ws = norm_setup(n, dev, rows, gmap)
    assert E.grad_norm_workspace(n) == (65 if n == 262148 else 1) and E.grad_norm_workspace(1 << 26) == 1024
    E.grad_norm(g, dmap, gs, 1.0, clip, ws, 0.5)
    first = clip.clone()
    clip.zero_()
    ws.fill_(7.0)
    E.grad_norm(g, dmap, gs, 1.0, clip, ws, 0.5)
    torch.cuda.synchronize()
    assert np.array_equal(bits(first), bits(clip))
    want = float(np.sqrt(((g[live].double().cpu().numpy() * 0.5) ** 2).sum()))
    assert abs(float(clip[0]) - want) <= 1e-5 * want
    assert float(clip[1]) == float(R.clip_coef(float(clip[0]), 1.0)) < 1 and float(clip[2]) == 0
    g2 = torch.where(live, g, torch.full_like(g, 1e30))                       # frozen and unmapped gradients set to huge values
    E.grad_norm(g2, dmap, gs, 1.0, clip, ws, 0.5)
    torch.cuda.synchronize()
    assert np.array_equal(bits(first), bits(clip))
    E.grad_norm(g, dmap, gs, 1e9, clip, ws, 0.5)                              # a max norm above the norm: the coefficient is exactly 1
    assert float(clip[1]) == 1.0 and float(clip[0]) == float(first[0])
    lib = L.load()
    args = lambda grads, ws_floats, G=4: (L.ptr(grads), n, L.ptr(dmap), L.ptr(gs), G, 0.5, 1.0, L.ptr(clip), None, L.ptr(ws), ws_floats,   # noqa: E731
                                          L.stream_ptr(dev))
    assert lib.cvx_grad_norm(*args(g, ws.numel() - 1)) != 0 and b"workspace" in lib.cvx_last_error()
    assert lib.cvx_grad_norm(*args(g, ws.numel(), 17)) != 0
    assert lib.cvx_grad_norm(*args(torch.zeros(n + 4, device=dev)[1:], ws.numel())) != 0 and b"align" in lib.cvx_last_error()
    assert lib.cvx_grad_norm(*args(g, ws.numel())) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_norm_skips_the_step_and_raises_found_inf(dev, bad):
    n = 4100
    rows, gmap = rows_for("momentum"), make_map(n)
    gid = element_groups(gmap, n)
    live = live_mask(gid, rows)
    g, gs, dmap, clip, ws = norm_setup(n, dev, rows, gmap)
    found = torch.zeros(1, dtype=torch.int32, device=dev)
    frozen_at, live_at = int(np.flatnonzero(gid == 3)[5]), int(np.flatnonzero(live)[-1])
    A = Arenas(n, dev, 1, names=("p", "a"))
    state = torch.zeros(4, device=dev)
    # the value in a frozen chunk: no marker, no found_inf, the step runs
    g[frozen_at] = bad
    E.grad_norm(g, dmap, gs, 1.0, clip, ws, 1.0, found)
    p0 = A.p.clone()
    E.optim_step(E.OPTIM_SGD, A.p, g.clone(), A.a, None, dmap, gs, state, found_inf=found, zero_grad=False, clip_state=clip)
    torch.cuda.synchronize()
    assert float(clip[2]) == 0 and int(found) == 0 and float(state[1]) == 1 and not torch.equal(A.p, p0) and bool(torch.isfinite(A.p).all())
    # the same value in a live chunk: marker and found_inf; the following step leaves p and the buffer alone, with or without found_inf
    g[frozen_at] = 0.0
    g[live_at] = bad
    E.grad_norm(g, dmap, gs, 1.0, clip, ws, 1.0, found)
    p1, a1 = A.p.clone(), A.a.clone()
    for flag in (found, None):
        gg = g.clone()
        E.optim_step(E.OPTIM_SGD, A.p, gg, A.a, None, dmap, gs, state, found_inf=flag, zero_grad=True, clip_state=clip)
        torch.cuda.synchronize()
        assert float(clip[2]) == 1 and int(found) == 1 and float(state[1]) == 1
        assert np.array_equal(bits(A.p), bits(p1)) and np.array_equal(bits(A.a), bits(a1)) and float(gg.abs().sum()) == 0 and A.guards_intact()


@pytest.mark.parametrize("kind", [E.OPTIM_SGD, E.OPTIM_ADAM])
@pytest.mark.parametrize("n", [1027, 262148])
def test_clipped_steps_against_the_restatement_fed_the_devices_norm(dev, n, kind):
    """max_norm alternates between half and twice the fp64 norm, so clipped and unclipped steps both occur.  SGD: the restatement; the
    ADAM kind: cvx_adam_step_dev on the gradient torch scaled by grad_scale and by the restated coefficient."""
    rows, gmap = rows_for("nesterov"), make_map(n)
    gid = element_groups(gmap, n)
    live = live_mask(gid, rows)
    tlive = torch.from_numpy(live).to(dev)
    A = Arenas(n, dev, n, names=("p", "g", "a", "b"))
    ref = Arenas(n, dev, n, names=("p", "g", "a", "b"))
    gs, dmap = table([dict(rows[0], wd=0.0)] if kind == E.OPTIM_ADAM else rows, kind, dev), torch.from_numpy(gmap).to(dev)
    if kind == E.OPTIM_ADAM:                                                   # one live group at the reference's lr, no decay; the rest stands still
        gmap = np.where(gmap == 0, 0, R.UNMAPPED).astype(np.uint8)
        dmap, live = torch.from_numpy(gmap).to(dev), gmap[np.arange(n) // 4] == 0
        tlive = torch.from_numpy(live).to(dev)
    clip, ws = torch.zeros(4, device=dev), torch.zeros(E.grad_norm_workspace(n), device=dev)
    state, ref_state = torch.zeros(4, device=dev), torch.tensor([rows[0]["lr"], 0.0, 0.0, 0.0], device=dev)
    p, b = A.p.cpu().numpy().copy(), np.zeros(n, F)
    seen = set()
    for i in range(4):
        A.g.copy_(A.grads[i].to(dev))
        norm64 = float(np.sqrt(((A.grads[i].numpy()[live].astype(np.float64) * 0.5) ** 2).sum()))
        max_norm = norm64 * (0.5 if i % 2 == 0 else 2.0)
        E.grad_norm(A.g, dmap, gs, max_norm, clip, ws, 0.5)
        E.optim_step(kind, A.p, A.g, A.a, A.b if kind == E.OPTIM_ADAM else None, dmap, gs, state, BETAS, EPS, None, True, 0.5, clip)
        torch.cuda.synchronize()
        norm = float(clip[0])
        coef = R.clip_coef(norm, max_norm)
        seen.add(bool(coef < 1))
        assert abs(norm - norm64) <= 1e-5 * norm64 and float(clip[1]) == float(coef) and (coef < 1) == (i % 2 == 0)
        if kind == E.OPTIM_SGD:
            p, b = host_sgd(p, b, A.grads[i].numpy(), gid, rows, 0.5, coef, False)
            assert np.array_equal(bits(A.p), p.view(np.uint32)) and np.array_equal(bits(A.a), b.view(np.uint32)), f"step {i}"
        else:
            ref.g.copy_(torch.from_numpy(R.scaled_grad(A.grads[i].numpy(), 0.5, coef)).to(dev))
            E.adam_step_dev(ref.p, ref.g, ref.a, ref.b, BETAS, EPS, ref_state, None, True, 1.0)
            torch.cuda.synchronize()
            for name, x, y in (("p", A.p, ref.p), ("m", A.a, ref.a), ("v", A.b, ref.b)):
                assert np.array_equal(bits(x[tlive]), bits(y[tlive])), f"step {i}: {name}"
            assert float((A.a[~tlive]).abs().sum()) == 0 and float(state[1]) == float(ref_state[1]) == i + 1
    assert seen == {True, False} and A.guards_intact()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_optim_step_refusals(dev):
    lib = L.load()
    st = L.stream_ptr(dev)
    t = lambda: torch.zeros(16, device=dev)   # noqa: E731
    p, g, a, b, e, state = t(), t(), t(), t(), t(), torch.zeros(4, device=dev)
    gs = torch.zeros(17, 8, device=dev)
    gmap = torch.zeros(4, dtype=torch.uint8, device=dev)

    def call(kind=E.OPTIM_ADAM, p=p, g=g, a=a, b=b, G=1, ema=None, n=16):
        return lib.cvx_optim_step(kind, L.ptr(p), L.ptr(g), L.ptr(a), L.ptr(b), n, L.ptr(gmap), L.ptr(gs), G, L.ptr(state), 0.9, 0.999, 1e-8, None, 1, 1.0,
                                  None, L.ptr(ema), 0.5, 0.5, st)

    big = torch.zeros(20, device=dev)
    for kw in (dict(p=big[1:17]), dict(g=big[1:17]), dict(a=big[1:17]), dict(b=big[1:17]), dict(ema=big[1:17])):
        assert call(**kw) != 0 and b"align" in lib.cvx_last_error(), kw
    assert call(ema=p) != 0 and b"average" in lib.cvx_last_error()
    assert call(G=17) != 0 and b"n_groups" in lib.cvx_last_error()
    assert call(G=0) != 0
    assert call(b=None) != 0 and b"buf2" in lib.cvx_last_error()
    assert call(kind=2) != 0 and call(n=0) != 0
    torch.cuda.synchronize()
    assert all(float(x.abs().sum()) == 0 for x in (p, g, a, b, e, state))
    assert call(kind=E.OPTIM_SGD, b=None) == 0 and call() == 0                # SGD needs no buf2
    with pytest.raises(L.CvxError):
        E.optim_step(E.OPTIM_SGD, p, g, a, None, gmap[:3], gs[:1], state)     # a map of the wrong length
    with pytest.raises(L.CvxError):
        E.optim_step(E.OPTIM_SGD, p, g, a, None, gmap, gs[:1, :4], state)
    # an id the caller failed to refuse (>= n_groups, not 255) is left alone by the kernel; FlatOptimizer's builder refuses it on the host
    p.fill_(1.0)
    g.fill_(1.0)
    gs[0, 0] = 0.1
    E.optim_step(E.OPTIM_SGD, p, g, a, None, torch.tensor([0, 1, 200, 255], dtype=torch.uint8, device=dev), gs[:1].contiguous(), state, zero_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), torch.tensor([0.9] * 4 + [1.0] * 12))
    from types import SimpleNamespace as NS
    with pytest.raises(L.CvxError):
        O.build_group_map(NS(n_params=4, slots={"w": NS(arena="param", trainable=True, offset=0, shape=(4,), strides=(1,))}), {"w": 1}, 1)


# ---- 6. the real layout -----------------------------------------------------------------------------------------------------------------
def test_flat_sgd_on_the_real_yolov8_layout(dev):
    """FlatSGD with groups, a frozen stem and clipping on YOLOv8-n (20 classes: the class head's last convolutions are padded from 20 to 24
    rows).  Gradients are written through the p.grad views, garbage into the padding rows of the gradient arena; every parameter equals
    the restatement applied per parameter with the device's norm, and the garbage changed neither the norm nor anything else."""
    from computervision.pytorch_amd.model import Yolo8
    torch.manual_seed(0)
    m = Yolo8("n", 20).to(dev).train()
    opt = O.FlatSGD(m, lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4, groups=O.NO_DECAY_NORM_BIAS, bias_lr_scale=2.0, freeze=("model.0.",),
                    clip_grad_norm=10.0)
    gmap = opt.plan.gmap
    pad = torch.from_numpy(np.repeat(gmap == R.UNMAPPED, 4)).to(dev)
    assert int(pad.sum()) > 0 and len(opt.param_groups) == 4
    m.attach_grads()
    named = dict(m.named_parameters())
    group_of = {k: g for g, keys in zip(opt.param_groups, opt.plan.keys) for k in keys}
    host = {k: (p.detach().cpu().numpy().copy(), np.zeros(tuple(p.shape), F)) for k, p in named.items()}
    params0 = m.flat_params.clone()
    gen = torch.Generator().manual_seed(9)
    for step in range(3):
        grads = {}
        for k, p in named.items():
            if p.grad is None:
                continue                                                       # the DFL projection lives outside the arenas
            grads[k] = torch.randn(tuple(p.shape), generator=gen)
            p.grad.copy_(grads[k].to(dev))
        m.flat_grads[pad] = 1e30 if step < 2 else float("inf")                # deliberate garbage in the padding rows
        opt.step(zero_grad=False)
        torch.cuda.synchronize()
        norm = float(opt.last_grad_norm)
        norm64 = float(np.sqrt(sum((g.double() ** 2).sum().item() for k, g in grads.items() if not group_of[k]["frozen"])))
        assert abs(norm - norm64) <= 1e-5 * norm64 and float(opt._clip[2]) == 0
        clean = m.flat_grads.clone()
        clean[pad] = 0
        clip2 = torch.zeros(4, device=dev)
        E.grad_norm(clean, opt._map, opt._gs, 10.0, clip2, opt._ws)
        assert np.array_equal(bits(clip2), bits(opt._clip))                   # the garbage changed nothing of the norm
        coef = R.clip_coef(norm, 10.0)
        assert coef < 1
        for k, p in named.items():
            g = group_of[k]
            if not g["frozen"]:
                host[k] = R.sgd_step(*host[k], R.scaled_grad(grads[k].numpy(), 1.0, coef), g["lr"], g["weight_decay"], g["momentum"], g["nesterov"])
            assert np.array_equal(bits(p), host[k][0].view(np.uint32)), (step, k)
    assert opt.device_step() == 3 and torch.equal(m.flat_params[pad], params0[pad])
    frozen = torch.from_numpy(np.repeat(gmap == 3, 4)).to(dev)
    assert int(frozen.sum()) > 0 and torch.equal(m.flat_params[frozen], params0[frozen]) and not torch.equal(m.flat_params, params0)
    assert float(opt._buf1[frozen | pad].abs().sum()) == 0
    assert [k for k in named if k.startswith("model.0.")] == [k for k in opt.plan.keys[3] if k.startswith("model.0.")] and len(opt.plan.keys[3]) == 4


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------
def _yolo8_run(dev, make_opt, scaler, steps=3):
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.train import DynamicLossScale, FusedTrainStep, V8DetectionLoss
    from configs import Yolo8DetConfig
    x, batch = synth.images(2, 128, 128, seed=1).to(dev), {k: v.to(dev) for k, v in synth.targets(2, seed=2).items()}
    torch.manual_seed(0)
    m = Yolo8("n", 80).to(dev).train()
    opt = make_opt(m)
    p0 = m.flat_params.clone()
    step = FusedTrainStep(m, V8DetectionLoss(Yolo8DetConfig(), m), opt, n_buckets=4, scaler=DynamicLossScale(dev, init_scale=1024.0) if scaler else None)
    losses = torch.stack([step(x, batch).clone() for _ in range(steps)])
    torch.cuda.synchronize()
    return m, opt, p0, losses


@pytest.mark.parametrize("recipe", ["sgd", "adamw"])
def test_yolov8_fused_train_step_with_the_new_optimisers(dev, recipe):
    """SGD + groups + clip + freeze, and AdamW + freeze under a DynamicLossScale: 3 steps at 2x128x128, twice."""
    make = {"sgd": lambda m: O.FlatSGD(m, lr=0.01, momentum=0.937, nesterov=True, weight_decay=5e-4, groups=O.NO_DECAY_NORM_BIAS, freeze=("model.0.",),
                                       clip_grad_norm=10.0),
            "adamw": lambda m: O.FlatAdamW(m, lr=1e-3, weight_decay=0.05, freeze=("model.0.", "model.1."))}[recipe]
    runs = [_yolo8_run(dev, make, scaler=recipe == "adamw") for _ in range(2)]
    m, opt, p0, losses = runs[0]
    assert bool(torch.isfinite(losses).all()) and opt.device_step() == 3
    frozen = torch.from_numpy(np.repeat(opt.plan.gmap == opt.plan.frozen, 4)).to(dev)
    live = torch.from_numpy(np.repeat(opt.plan.gmap < opt.plan.frozen, 4)).to(dev)
    assert int(frozen.sum()) > 0 and torch.equal(m.flat_params[frozen], p0[frozen])
    assert float((m.flat_params[live] != p0[live]).float().mean()) > 0.5
    assert torch.equal(m.flat_params[~(frozen | live)], p0[~(frozen | live)])
    assert torch.equal(runs[1][0].flat_params, m.flat_params) and torch.equal(runs[1][3], losses)
    assert float(m.flat_grads.abs().sum()) == 0                                # zeroed by the step, frozen and padding chunks included
    if recipe == "sgd":
        assert float(opt.last_grad_norm) > 0 and float(opt._clip[2]) == 0


@pytest.mark.parametrize("family", ["deeplab", "centernet", "ssd", "yolov7"])
def test_other_families_step_with_flat_sgd(dev, gold, family):
    """One fused train step each, at the shapes tests/test_ema_gpu.py uses, with groups, clipping and the fused average."""
    from test_ema_gpu import _family_cases
    from computervision.pytorch_amd.train import DynamicLossScale
    make, crit, step_cls, get_batch = _family_cases(dev, gold)[family]
    images, targets = get_batch()
    torch.manual_seed(0)
    m = make().to(dev).train()
    opt = O.FlatSGD(m, lr=1e-3, momentum=0.9, nesterov=True, weight_decay=5e-4, groups=O.NO_DECAY_NORM_BIAS, clip_grad_norm=10.0)
    gmap = opt.plan.gmap
    assert set(np.unique(gmap)) == {0, 1, 2, R.UNMAPPED} and opt.plan.frozen is None
    step = step_cls(m, crit(m), opt, scaler=DynamicLossScale(dev, init_scale=4096.0) if family == "deeplab" else None)
    ema = ModelEMA(m, decay=0.999, tau=50, updates=20)
    e0 = ema.ema.flat_params.clone()
    opt.attach_ema(ema)
    p0 = m.flat_params.clone()
    loss = step(images, targets)
    torch.cuda.synchronize()
    mapped = torch.from_numpy(np.repeat(gmap != R.UNMAPPED, 4)).to(dev)
    assert bool(torch.isfinite(loss).all()) and opt.device_step() == 1 and ema.updates == 21
    assert float((m.flat_params[mapped] != p0[mapped]).float().mean()) > 0.5 and torch.equal(m.flat_params[~mapped], p0[~mapped])
    d, omd = ema.factors()
    want = (e0.cpu().numpy() * F(d)).astype(F) + (F(omd) * m.flat_params.cpu().numpy()).astype(F)
    assert np.array_equal(bits(ema.ema.flat_params[mapped]), want.view(np.uint32)[mapped.cpu().numpy()])
    assert bool(torch.isfinite(opt.last_grad_norm)) and float(opt.last_grad_norm) > 0


def test_trainer_with_sgd_runs_two_iterations(dev, tmp_path):
    """The stock trainers keep the reference's call (Adam only: tests/test_plugin_layer_cpu.py pins that "sgd" raises there); a trainer opts
    in by handing its config to ``get_optimizer``.  Such a trainer trains, schedules, saves and evaluates with FlatSGD."""
    import builder
    from core.trainer.engine_trainer import get_optimizer
    from core.trainer.yolo8_train import SyntheticDetectionLoader
    cfg, _, stock_cls = builder.export_from_registry("yolo8_det")

    class trainer_cls(stock_cls):
        def set_optimizer(self):
            self.optimizer = get_optimizer(self.optimizer_name, self.model, self.initial_lr, self.cfg)

    cfg.arch.input_size = (3, 128, 128)
    cfg.engine.init_loss_scale = 1024.0
    cfg.train.batch_size, cfg.train.epoch, cfg.train.save_interval, cfg.train.eval_interval = 2, 1, 1, 1
    cfg.train.save_path = str(tmp_path / "saves")
    cfg.train.freeze = ("model.0.",)
    cfg.optimizer.name, cfg.optimizer.groups, cfg.optimizer.weight_decay, cfg.optimizer.clip_grad_norm = "sgd", "no_decay_norm_bias", 5e-4, 10.0
    cfg.log.print_interval = 1
    torch.manual_seed(0)
    tr = trainer_cls(cfg, dev, dataloader=SyntheticDetectionLoader(2, (128, 128), cfg.dataset.num_classes, length=2, seed=5))
    assert type(tr.optimizer) is O.FlatSGD and tr.optimizer.param_groups[0]["momentum"] == 0.937 and tr.optimizer.param_groups[0]["nesterov"]
    p0 = tr.model.flat_params.clone()
    tr.train()
    torch.cuda.synchronize()
    assert 1 <= tr.optimizer.device_step() <= 2                               # (a step the loss scale skipped is not counted)
    frozen = torch.from_numpy(np.repeat(tr.optimizer.plan.gmap == 3, 4)).to(dev)
    assert torch.equal(tr.model.flat_params[frozen], p0[frozen]) and not torch.equal(tr.model.flat_params, p0)
    assert bool(torch.isfinite(tr.model.flat_params).all())
