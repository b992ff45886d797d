"""The launchers of the two convolution kernels with LDS-resident weights (csrc/conv_halo.hip, csrc/conv_pw.hip) pick, for every case of
tests/conv_resident_cases.py, the compiled instantiation the table states -- and the table reaches every instantiation the planners can
produce: 56 of the halo kernel, 51 of the pointwise kernel.  The set of reachable instantiations is established here, by sweeping
``cvx_debug_conv_halo_plan`` / ``cvx_debug_conv_pw_plan`` (the functions the launchers call themselves; host code, no GPU needed) over every
output channel count on maps at both sides of every threshold, and compared with the table and with the hand count.  This is the lock of
tests/test_conv_resident_gpu.py: when a threshold moves or a ``case`` is dropped, the failure names the configuration that lost its case."""
import functools

import pytest

import conv_resident_cases as T
from computervision.pytorch_amd import _lib as L

HALO_CASES = list(T.HALO_TABLE.items())
PW_CASES = list(T.PW_TABLE.items())


@pytest.mark.parametrize("key,want", HALO_CASES, ids=[f"cin{k[0]}-{k[1]}x{k[2][0]}x{k[2][1]}-cout{k[3]}" for k, _ in HALO_CASES])
def test_halo_launcher_picks_the_configuration_the_table_states(key, want):
    cin, B, (H, W), cout = key
    assert T.halo_plan(B, H, W, cin, cout) == want


@pytest.mark.parametrize("key,want", PW_CASES, ids=[f"cin{k[0]}-cout{k[1]}" for k, _ in PW_CASES])
def test_pw_launcher_picks_the_configuration_the_table_states(key, want):
    cin, cout = key
    B, H, W = T.PW_MAP
    assert T.pw_plan(B * H * W, cin, cout) == want


@functools.lru_cache(maxsize=None)
def _halo_sweep():
    """{cin: {(TH, NT, HV)}} over cout = 4 .. 512 step 4 on maps at both sides of h * w = 1600, 6400 and B * h * w = 128 K.  A plan whose
    single-stream workgroup does not fit the 160 KiB of LDS is an error of the debug function (a launcher bug), so the sweep would raise."""
    got = {}
    for cin in T.HALO_CINS:
        for B, H, W in T.HALO_SWEEP_MAPS:
            for cout in range(4, 516, 4):
                th, nt, gy, hv = T.halo_plan(B, H, W, cin, cout)
                wm, bn = (2, 32 * nt) if th == 2 else (4, 16 * nt)
                assert T.halo_lds(th, wm, bn, cin, 1) <= 160 * 1024 and (hv == 1 or T.halo_lds(th, wm, bn, cin, 2) <= 160 * 1024), (cin, B, H, W, cout)
                assert gy * bn >= cout > (gy - 1) * bn, (cin, B, H, W, cout, "the channel blocks do not cover the output channels exactly")
                got.setdefault(cin, set()).add((th, nt, hv))
    return got


@functools.lru_cache(maxsize=None)
def _pw_sweep():
    got = set()
    for cin in range(8, 520, 8):
        for cout in range(4, 516, 4):
            ns, nt, gy, mt = T.pw_plan(2886, cin, cout)
            assert ns == min(a for a in (1, 2, 3, 4, 6, 8, 12, 16) if a * 32 >= cin) and mt == (2 if ns <= 8 else 1), (cin, cout)
            assert gy * nt * 16 >= cout > (gy - 1) * nt * 16, (cin, cout)
            assert 1024 + ns * nt * 16 * 64 + 4 * nt * 16 * 8 <= 160 * 1024, (cin, cout, "LDS")
            got.add((ns, nt, mt))
    return got


def test_the_halo_table_reaches_every_configuration_the_planner_can_produce():
    sweep = _halo_sweep()
    table = {}
    for (cin, B, (H, W), cout), (th, nt, gy, hv) in T.HALO_TABLE.items():
        assert (th, nt, hv) not in table.setdefault(cin, set()), f"cin {cin}: two table entries for (TH, NT, HV) = {(th, nt, hv)}"
        table[cin].add((th, nt, hv))
    for cin in T.HALO_CINS:
        missing = sorted(sweep[cin] - table.get(cin, set()))
        assert not missing, f"cin {cin}: no table entry runs (TH, NT, HV) = {missing}"
        assert table[cin] == sweep[cin], (cin, sorted(table[cin] - sweep[cin]))
    assert len(T.HALO_TABLE) == sum(len(v) for v in sweep.values())


def test_the_halo_configuration_count_matches_the_hand_count():
    sweep = _halo_sweep()
    for cin in T.HALO_CINS:
        lost, new = sorted(T.HALO_CONFIGS[cin] - sweep[cin]), sorted(sweep[cin] - T.HALO_CONFIGS[cin])
        assert not lost and not new, f"cin {cin}: (TH, NT, HV) no longer reachable {lost}, newly reachable {new}"
    assert sum(len(v) for v in T.HALO_CONFIGS.values()) == T.HALO_COUNT == 56 and sum(len(v) for v in sweep.values()) == 56


def test_the_pw_table_reaches_every_configuration_the_planner_can_produce():
    sweep = _pw_sweep()
    table = {(ns, nt, mt) for ns, nt, _, mt in T.PW_TABLE.values()}
    assert len(table) == len(T.PW_TABLE), "two table entries for one configuration"
    missing = sorted(sweep - table)
    assert not missing, f"no table entry runs (NS, NT, MT) = {missing}"
    assert table == sweep, sorted(table - sweep)
    # every K-step count has a case with a ragged or absent last K-step and one that fills every step
    for ns, (ragged, full) in T.PW_CINS.items():
        cins = {cin for (cin, _), plan in T.PW_TABLE.items() if plan[0] == ns}
        assert cins == {ragged, full} and ragged % 32 != 0 and full == ns * 32, ns


def test_the_pw_configuration_count_matches_the_hand_count():
    sweep = _pw_sweep()
    lost, new = sorted(T.PW_CONFIGS - sweep), sorted(sweep - T.PW_CONFIGS)
    assert not lost and not new, f"(NS, NT, MT) no longer reachable {lost}, newly reachable {new}"
    assert len(T.PW_CONFIGS) == T.PW_COUNT == 51 and len(sweep) == 51


def test_thresholds_of_the_halo_launcher():
    """the edges themselves: 40 x 40 and 80 x 80 pixels per image, 128 K pixels per launch, and the 160 KiB that send wide layers to 4 rows"""
    th = lambda *a: T.halo_plan(*a)[0]  # noqa: E731
    assert th(1, 39, 41, 16, 16) == 2 and th(1, 40, 40, 16, 16) == 4
    assert th(1, 79, 81, 16, 16) == 4 and th(1, 80, 80, 16, 16) == 8
    assert th(81, 39, 41, 16, 16) == 2 and th(82, 39, 41, 16, 16) == 8        # 81 * 1599 = 129519 < 131072 <= 82 * 1599
    assert th(1, 39, 41, 144, 16) == 2 and th(1, 80, 80, 144, 16) == 4 and th(1, 80, 80, 128, 16) == 4   # cap 2: the 10-row patches do not fit twice
    assert T.halo_plan(1, 80, 80, 64, 64) == (4, 4, 1, 2)                     # one 8-row stream per CU -> two 4-row streams
    assert T.halo_plan(1, 80, 80, 64, 16) == (8, 1, 1, 1)


def test_the_debug_functions_reject_shapes_the_kernels_do_not_take():
    for cin in (8, 24, 48, 96, 256):
        with pytest.raises(L.CvxError):
            T.halo_plan(1, 41, 43, cin, 16)
    for cin in (0, 4, 36, 520, 1024):
        with pytest.raises(L.CvxError):
            T.pw_plan(2886, cin, 16)
    with pytest.raises(L.CvxError):
        T.pw_plan(0, 32, 16)


def test_the_grid_divisor_is_set_and_restored():
    lib = L.load()
    assert lib.cvx_debug_conv_grid_div(1) == 1          # the default
    try:
        assert lib.cvx_debug_conv_grid_div(64) == 1 and lib.cvx_debug_conv_grid_div(8) == 64
        assert lib.cvx_debug_conv_grid_div(0) == -1 and lib.cvx_debug_conv_grid_div(-3) == -1   # rejected, nothing changes
        assert lib.cvx_debug_conv_grid_div(8) == 8
    finally:
        assert lib.cvx_debug_conv_grid_div(1) >= 1
    assert lib.cvx_debug_conv_grid_div(1) == 1


def test_the_persistent_walks_run_table_configurations():
    """the walk cases of the GPU file are table configurations on more images, and their grids have 2 .. 8 workgroups per channel block"""
    for cin, B, (H, W), cout, div in T.HALO_WALKS:
        plan = T.halo_plan(B, H, W, cin, cout)
        assert (plan[0], plan[1], plan[3]) in T.HALO_CONFIGS[cin]
        assert 2 <= T.halo_grid_x(plan, cin, T.halo_tiles(B, H, W, plan[0]), div) <= 8, (cin, B, H, W, cout)
    assert {(T.halo_plan(B, H, W, cin, cout)[0], T.halo_plan(B, H, W, cin, cout)[3]) for cin, B, (H, W), cout, _ in T.HALO_WALKS} == \
        {(th, hv) for th in (2, 4, 8) for hv in (1, 2)}
    B, H, W = T.PW_MAP
    assert [T.pw_plan(B * H * W, cin, cout)[3] for cin, cout, _ in T.PW_WALKS] == [2, 1]
