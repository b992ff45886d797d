"""The launcher of the LDS-DMA ring convolution kernel (csrc/conv_igemm_dma.hip) picks, for every case of tests/conv_dma_cases.py, the tile
configuration the table states -- and the table reaches all 18 compiled configurations, each family (128, 64, 32 rows) at least once with a
partial last DMA pass.  ``cvx_debug_conv_dma_plan`` is the function the launcher itself calls; it is host code, no GPU needed.  This is the
lock of tests/test_conv_dma_gpu.py: when a threshold of the launcher moves, the failure names the configuration that lost its case there."""
import pytest

import conv_dma_cases as T
from computervision.pytorch_amd import _lib as L

CASES = T.plan_cases()


@pytest.mark.parametrize("label,pixels,cin,cout,ntaps,want", CASES, ids=[c[0] for c in CASES])
def test_launcher_picks_the_configuration_the_table_states(label, pixels, cin, cout, ntaps, want):
    assert T.launcher_plan(pixels, cin, cout, ntaps) == want


def test_the_table_reaches_all_18_configurations_and_a_partial_pass_in_every_family():
    got = {}     # (tile rows, channel tiles per workgroup) -> [(label, channel blocks)]
    for label, pixels, cin, cout, ntaps, _ in CASES:
        rows, nt, gy, npass = T.launcher_plan(pixels, cin, cout, ntaps)
        assert npass == T.passes(rows, nt), label
        got.setdefault((rows, nt), []).append((label, gy))
    assert len(T.ALL_CONFIGS) == 18
    missing = sorted(T.ALL_CONFIGS - set(got))
    assert not missing, f"no case runs (tile rows, channel tiles per workgroup) = {missing}"
    assert set(got) == T.ALL_CONFIGS, sorted(set(got) - T.ALL_CONFIGS)
    for rows in (128, 64, 32):
        assert any(T.partial_last_pass(r, nt) for r, nt in got if r == rows), f"{rows}-row family: no case with a partial last DMA pass"
        assert any(gy == 2 for (r, _), cases in got.items() if r == rows for _, gy in cases), f"{rows}-row family: no case with two channel blocks"
    # the heavy rule: 64-row tiles below 64 K pixels
    heavy = [c for c in CASES if c[0].startswith("heavy")]
    assert len(heavy) == 2 and all(pixels < 65536 and want[0] == 64 for _, pixels, _, _, _, want in heavy)


def test_thresholds_of_the_launcher():
    """the edges themselves: 64 K and 128 K pixels, 8 K pixels and 512 K weight elements for the heavy rule"""
    rows = lambda *a: T.launcher_plan(*a)[0]  # noqa: E731
    assert rows(65535, 16, 16, 9) == 32 and rows(65536, 16, 16, 9) == 64
    assert rows(131071, 16, 16, 9) == 64 and rows(131072, 16, 16, 9) == 128
    assert rows(8191, 256, 256, 9) == 32 and rows(8192, 256, 256, 9) == 64
    assert rows(8192, 256, 224, 9) == 32 and rows(8192, 256, 228, 9) == 64          # 9 * 256 * 228 = 525312 >= 524288 > 9 * 256 * 224
    with pytest.raises(L.CvxError):
        T.launcher_plan(0, 16, 16, 9)
