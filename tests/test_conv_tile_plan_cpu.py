"""The launcher of the row-band convolution kernel (csrc/conv_tile.hip) makes, for every case of tests/conv_tile_cases.py under that case's
forced (TR, NTW), the plan the table states -- and the table reaches every (MT, NTW, ring regime) the planner can produce by itself: 24
instantiations, 68 triples.  The reachable set is established here, with the force at (0, 0), by sweeping ``cvx_debug_conv_tile_ring`` (host
code: the function runs the launcher's own plan_tile) over every batch 1 .. 64, maps at both sides of 20 / 40 / 80 pixels per side and ragged
ones, cin 32 .. 512 and cout 8 .. 512 in steps of 8, and compared with the table and with the hand count.  This is the lock of
tests/test_conv_tile_gpu.py: when a threshold of the planner moves, the failure names the configuration that lost or gained a case.

Two limits cannot be asserted from here, because cvx_conv_tile_supported is not exported: the dispatcher gives this kernel maps of at most
40 x 40 (``p.IW > max_w || p.IH > max_w``, max_w = 40) with at most 144 gathered channels (``p.Cin > max_c``), csrc/conv_tile.hip,
cvx_conv_tile_supported.  The kernel itself (cvx_conv_tile_shape_ok, what ``mode | 0x2000`` and the query functions ask) goes to cin 512 and to
any map a plan exists for; those edges are asserted below."""
import ctypes
import functools

import pytest

import conv_tile_cases as T
from computervision.pytorch_amd import _lib as L

CASES = list(T.TABLE.items()) + list(T.FORCED_ONLY.items())


def _id(key, want):
    return f"MT{want[0]}-NTW{want[1]}-R{want[5]}-cin{key[0]}-TR{key[4]}"


@pytest.mark.parametrize("key,want", CASES, ids=[_id(k, w) for k, w in CASES])
def test_forced_plan_is_the_one_the_table_states(key, want):
    cin, B, (H, W), cout, tr, ntw = key
    with T.forced(tr, ntw):
        plan = T.tile_plan(B, H, W, cin, cout)
        assert plan is not None and plan[0] == tr and T.launch_key(B, H, W, cin, cout) == want
    mt, _, nb = want[:3]
    assert mt == ((tr * W + 15) // 16 + T.WAVES - 1) // T.WAVES
    # the last 16-channel tile is 8 wide; several channel blocks: the last one is ragged
    assert cout % 16 == 8 and (nb - 1) * 16 * ntw < cout < nb * 16 * ntw and (ntw > 1 or nb == 2)
    assert B == T.REF_BATCH[(H, W)] and (B * ((H + tr - 1) // tr)) % 8 != 0      # tiles: no multiple of 8 (workgroups that return early)


@functools.lru_cache(maxsize=None)
def _sweep():
    """{(MT, NTW, R): count}, the largest first wait, and the number of plans, with the force at (0, 0).  plan_tile reads Cout once, as
    ceil(Cout / 16) channel tiles, so cout = 16 n - 8 and 16 n have one plan: that is ASSERTED for every shape of batch 1, 2 and 64 (cout in
    steps of 8), and the other batches run cout in steps of 16 -- half the calls of a sweep that takes most of the CPU suite's time."""
    lib = L.load()
    assert lib.cvx_debug_conv_tile_force(0, 0) == 0
    fn, out = lib.cvx_debug_conv_tile_ring, (ctypes.c_int32 * 8)()
    seen, worst_wait, plans = {}, 0, 0
    for B in T.SWEEP_BATCHES:
        every_cout = B in (1, 2, 64)
        for H, W in T.SWEEP_MAPS:
            for cin in T.SWEEP_CINS:
                prev = None
                for cout in T.SWEEP_COUTS:
                    if cout % 16 and not every_cout:
                        continue
                    if fn(B, H, W, cin, cout, out) != 0:
                        prev = None
                        continue
                    ksc, nch, R, spt, pw, pp, mt, ntw = out
                    if every_cout:
                        if cout % 16 == 0:
                            assert prev == (ksc, nch, R, mt, ntw), (B, H, W, cin, cout, "cout and cout - 8 have different plans")
                        prev = (ksc, nch, R, mt, ntw)
                    assert spt == (cin + 31) // 32 and ksc * nch == 9 * spt and (R == 2) == (nch == 1) and R in (2, 3, 4), (B, H, W, cin, cout)
                    assert (ksc == spt or spt % ksc == 0) if R > 2 else ksc == 9 * spt, (B, H, W, cin, cout)
                    key = (mt, ntw, R)
                    seen[key] = seen.get(key, 0) + 1
                    plans += 1
                    wait = (min(nch, R - 1) - 1) * pw
                    if wait > worst_wait:
                        worst_wait = wait
    return seen, worst_wait, plans


def test_the_table_reaches_every_configuration_the_planner_can_produce():
    sweep = set(_sweep()[0])
    table = {}
    for key, (mt, ntw, nb, ksc, nch, R) in T.TABLE.items():
        assert (mt, ntw, R) not in table, f"two table entries for (MT, NTW, R) = {(mt, ntw, R)}"
        table[(mt, ntw, R)] = key
    for triple, reason in T.EXCEPTIONS.items():
        assert triple not in table and reason, triple
    covered = set(table) | set(T.EXCEPTIONS)
    missing = sorted(sweep - covered)
    assert not missing, f"no table entry runs (MT, NTW, R) = {missing}"
    assert covered == sweep, f"table entries the planner does not produce by itself: {sorted(covered - sweep)}"
    # what the force adds beyond the reachable set is listed as such
    forced_only = {(mt, ntw, R) for mt, ntw, _, _, _, R in T.FORCED_ONLY.values()}
    assert not (forced_only & sweep) and len(forced_only) == len(T.FORCED_ONLY)


def test_the_configuration_count_matches_the_hand_count():
    seen, worst_wait, plans = _sweep()
    sweep = {}
    for mt, ntw, R in seen:
        sweep.setdefault((mt, ntw), set()).add(R)
    lost = sorted((p, r) for p, rs in T.CONFIGS.items() for r in rs - sweep.get(p, set()))
    new = sorted((p, r) for p, rs in sweep.items() for r in rs - T.CONFIGS.get(p, set()))
    assert not lost and not new, f"(MT, NTW), R no longer reachable {lost}, newly reachable {new}"
    assert len(T.CONFIGS) == T.PAIR_COUNT == 24 and sum(len(v) for v in T.CONFIGS.values()) == T.CONFIG_COUNT == 68 == len(seen)
    assert set(T.CONFIGS) == {(mt, ntw) for mt in (1, 2, 3, 4) for ntw in T.NTW_MENU} - {(3, 9), (4, 5), (4, 6), (4, 9)}
    assert plans > 500000, plans
    # The kernel's first wait is wait_vmcnt_dyn((npre - 1) * PW), which drains everything above 20.  No plan gets there: a ring needs three slots
    # in under 160 KiB, so a chunk has at most 53 pieces, PW <= 7, and npre - 1 = 2 needs four slots, PW <= 5 -- the fallback is dead code for
    # every plan the planner makes (and the in-loop wait, (issued - chunk - 2) * PW with issued - chunk <= R - 1, stays below it a fortiori).
    # The sweep's largest is 8 (a ring of 4 with PW = 4).
    assert worst_wait == 8, worst_wait


def _rings():
    """[(key, want, ring)] of the table, under each case's force"""
    got = []
    for key, want in T.TABLE.items():
        cin, B, (H, W), cout, tr, ntw = key
        with T.forced(tr, ntw):
            got.append((key, want, T.tile_ring(B, H, W, cin, cout)))
    return got


def test_the_table_holds_every_class_the_kernel_distinguishes():
    rings = _rings()
    cins = {key[0] for key, _, _ in rings}
    # the swizzle classes: P = cin / 8 = 4, 8, 16, 32 (16 and above share one mask); no swizzle: a ragged last K-step (40, 72, 144 = the
    # dispatcher's maximum: the chunk index is clamped) and every step full (96)
    assert {32, 64, 128, 256, 40, 72, 144, 96} <= cins and 512 in cins
    for ragged in (40, 72, 144):
        assert ragged % 32 != 0 and (ragged // 8) & (ragged // 8 - 1)
    assert 96 % 32 == 0 and (96 // 8) & (96 // 8 - 1)
    ring_cases = [(key, want, r) for key, want, r in rings if r[2] > 2]
    # chunks of a whole tap, of a divisor of a tap's steps, of one step (of several)
    assert any(r[0] == r[3] and r[3] > 1 for _, _, r in ring_cases)
    assert any(1 < r[0] < r[3] for _, _, r in ring_cases)
    assert any(r[0] == 1 and r[3] > 1 for _, _, r in ring_cases)
    # the first wait: wait_vmcnt<0> (one chunk requested), and counted waits from 1 piece up to 8, the largest any plan of the sweep has.  The
    # other path of wait_vmcnt_dyn (above 20: a full drain) is not reachable: test_the_configuration_count_matches_the_hand_count says why.
    waits = {T.first_wait(r, want[1]) for _, want, r in rings}
    assert {0, 1, 2, 3, 4, 5, 6, 8} <= waits and max(waits) == 8, sorted(waits)
    # surplus DMA pieces (a wave's share beyond the last piece repeats the last one): patch and chunk
    assert any(r[5] % T.WAVES for _, _, r in rings) and any((r[0] * want[1]) % T.WAVES for _, want, r in rings)
    assert any(r[5] % T.WAVES == 0 for _, _, r in rings) and any((r[0] * want[1]) % T.WAVES == 0 for _, want, r in rings)
    # the staged epilogue with idle lanes and several trips: BN / 8 = 2 NTW does not divide 64
    for ntw in (3, 5, 6, 9):
        assert 64 % (2 * ntw) != 0 and any(want[0] >= 2 and want[1] == ntw for _, want, _ in rings), ntw
    # a last band of one row (TR 4, 9, 12 on 37 rows; TR 1 trivially), several channel blocks
    assert {4, 9, 12} <= {key[4] for key, _, _ in rings if key[2] == T.MAIN and T.MAIN[0] % key[4] == 1}
    assert any(want[2] > 1 and want[1] > 1 for _, want, _ in rings)


def test_the_main_map_has_the_tails_the_cases_rely_on():
    H, W = T.MAIN
    assert W % 16 != 0 and [(tr, ((tr * W + 15) // 16 + 7) // 8) for tr in (1, 4, 7, 10)] == [(1, 1), (4, 2), (7, 3), (10, 4)] == [(tr, mt) for mt, tr in sorted(T.TR_OF_MT.items())]
    assert [T.REF_BATCH[T.MAIN] * ((H + tr - 1) // tr) for tr in (1, 4, 7, 10)] == [111, 30, 18, 12]
    assert [H % tr for tr in (4, 7, 10)] == [1, 2, 7]


def test_the_default_leaves_every_plan_unchanged():
    """(0, 0) is free: the plans before a set / restore and after it are the same, and the force in between is honoured or has no plan"""
    lib = L.load()
    shapes = [(2, 40, 40, 64, 64), (3, 20, 20, 128, 128), (2, 80, 80, 32, 32), (1, 40, 40, 128, 144), (2, 20, 20, 256, 144), (2, 40, 40, 80, 80),
              (1, 20, 20, 144, 256), (2, 13, 17, 32, 40), (1, 7, 5, 96, 24), (3, 33, 9, 48, 200), (1, 80, 80, 64, 144), (2, 2, 2, 64, 16), (1, 3, 50, 40, 8),
              (32, 20, 20, 128, 128), (32, 40, 40, 64, 64), (16, 40, 40, 128, 144), (3, 37, 39, 512, 24), (1, 2, 512, 32, 16)]
    before = [(T.tile_plan(*s), T.tile_ring(*s)) for s in shapes]
    assert all(p is not None for p, _ in before[:-2]) and lib.cvx_debug_conv_tile_force(0, 0) == 0
    for tr, ntw in ((4, 0), (0, 3), (2, 9), (1, 1)):
        with T.forced(tr, ntw):
            for s in shapes:
                p = T.tile_plan(*s)
                assert p is None or ((tr == 0 or p[0] == tr) and (ntw == 0 or p[2] == ntw)), (tr, ntw, s, p)
        assert [(T.tile_plan(*s), T.tile_ring(*s)) for s in shapes] == before, (tr, ntw)


def test_the_force_is_set_and_restored():
    lib = L.load()
    assert lib.cvx_debug_conv_tile_force(0, 0) == 0          # the default
    try:
        assert lib.cvx_debug_conv_tile_force(7, 5) == 0 and lib.cvx_debug_conv_tile_force(10, 0) == (7 << 8) | 5
        for bad in ((-1, 0), (0, -1), (0, 7), (0, 8), (0, 10), (4001, 1)):     # rejected, nothing changes
            assert lib.cvx_debug_conv_tile_force(*bad) == -1, bad
        assert lib.cvx_debug_conv_tile_force(10, 0) == 10 << 8
    finally:
        assert lib.cvx_debug_conv_tile_force(0, 0) >= 0
    assert lib.cvx_debug_conv_tile_force(0, 0) == 0


def test_thresholds_and_refusals():
    # the widest row the kernel plans: 512 pixels are 32 pixel groups = 4 per wave, in one row
    assert T.tile_plan(1, 2, 512, 32, 16)[:3] == (1, 4, 1)
    for shape, why in (((1, 2, 513, 32, 16), "33 pixel groups in a row: MT 5"), ((1, 8, 1, 32, 16), "a 1-wide map: the magic division needs a divisor >= 2"),
                       ((1, 12, 20, 24, 16), "cin 24 < 32"), ((1, 12, 20, 36, 16), "cin 36: no multiple of 8"),
                       ((1, 12, 20, 32, 36), "cout 36: the staged epilogue stores 8 channels per lane"), ((1, 12, 20, 520, 16), "cin 520 > 512")):
        assert T.tile_plan(*shape) is None and T.tile_ring(*shape) is None, why
    assert T.tile_plan(1, 12, 20, 32, 16) is not None and T.tile_plan(1, 12, 20, 512, 16) is not None
    # a forced pair that does not fit: 10 rows of 39 pixels with 5, 6 or 9 channel tiles (registers / staged rows), 7 rows with 9; more rows than the
    # map has; cin 512 beyond TR 1 on 37 x 39 (the patch exceeds the LDS); more channel tiles than the layer has while a smaller block holds them
    for tr, ntw, shape in ((10, 5, (3, 37, 39, 32, 72)), (10, 6, (3, 37, 39, 32, 88)), (10, 9, (3, 37, 39, 32, 136)), (7, 9, (3, 37, 39, 32, 136)),
                           (38, 1, (3, 37, 39, 32, 24)), (4, 1, (3, 37, 39, 512, 24)), (1, 9, (3, 37, 39, 32, 24))):
        with T.forced(tr, ntw):
            assert T.tile_plan(*shape) is None and T.tile_ring(*shape) is None, (tr, ntw, shape)
        assert T.tile_plan(*shape) is not None, shape
    with T.forced(1, 1):
        assert T.tile_plan(3, 37, 39, 512, 24) is not None


def test_the_other_gpu_cases_have_the_plans_they_were_written_for():
    for (B, H, W, cin, cout, tr, ntw), (mt, n) in T.EXTREMES.items():
        with T.forced(tr, ntw):
            p = T.tile_plan(B, H, W, cin, cout)
        assert p is not None and (p[1], p[2]) == (mt, n), ((B, H, W, cin, cout), p)
    H, W = T.MAIN
    with T.forced(4, 3):
        assert T.tile_plan(2, 5, 23, 72, 40)[0] == 4 and 5 % 4 == 1
    # the data gradients run a plan under the dispatcher's limits, and the forced ones one MT each
    for dy in T.DG_GATHERED:
        for dx in T.DG_DX:
            assert T.tile_plan(T.REF_BATCH[T.MAIN], H, W, dy, dx) is not None and max(H, W) <= 40 and dy <= 144 and dx % 8 == 0
    mts = []
    for dy, dx, tr, ntw in T.DG_FORCED:
        with T.forced(tr, ntw):
            mts.append(T.tile_plan(T.REF_BATCH[T.MAIN], H, W, dy, dx)[1])
    assert mts == [1, 2, 3, 4]
