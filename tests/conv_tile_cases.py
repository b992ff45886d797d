"""The shapes on which tests/test_conv_tile_gpu.py runs the row-band convolution kernel (csrc/conv_tile.hip, conv_tile_kernel.inc.h,
conv_tile_k1 / k2.hip: 3x3 / stride 1, the kernel the dispatcher asks first on maps of at most 40 x 40 with at most 144 gathered channels),
and the plan the launcher must make for each.

The kernel is compiled for 28 pairs <MT, NTW> (pixel groups per wave 1 .. 4 x 16-channel tiles per workgroup 1, 2, 3, 4, 5, 6, 9); the
planner's register rule (MT * NTW * 4 + 12 * (MT + NTW) <= 216) and the 160 KiB of staged epilogue rows exclude (3, 9), (4, 5), (4, 6) and
(4, 9), so 24 are reachable.  Each runs in three weight regimes, chosen at run time: ONE chunk (R = 2: all weights requested before the K
loop, no refill), a ring of R = 3 slots and a ring of R = 4, with KSC K-steps per chunk (a whole tap's SPT steps, a divisor of them, or 1).

Most pairs are the cost model's choice at batch 16 .. 32 only (its `rounds` term), so the cases fix the tiling with
``cvx_debug_conv_tile_force(TR, NTW)``: TR rows per tile give MT = ceil(ceil(TR * W / 16) / 8).  tests/test_conv_tile_plan_cpu.py holds the
launcher to this table without a GPU (``cvx_debug_conv_tile_plan`` / ``cvx_debug_conv_tile_ring``: the launcher's own planner),
establishes the reachable (MT, NTW, R) by a sweep of its own with the force at (0, 0), and compares it with the table and with the hand
count below, so a moved threshold names the configuration it lost or gained.

The hand count was first made by reading plan_tile; the sweep over the built library corrected it: 68, not 24 x 3 = 72 -- no shape of the
sweep makes the cost model keep MT = 1 with one chunk for NTW >= 4.  The force still produces those four; FORCED_ONLY runs them as well.
"""
import collections
import contextlib
import ctypes

NTW_MENU = (1, 2, 3, 4, 5, 6, 9)
WAVES = 8                    # kTileWaves
MAIN = (37, 39)              # W = 39 never fills a 16-pixel group; TR = 1 / 4 / 7 / 10 give MT = 1 / 2 / 3 / 4 and 37 / 10 / 6 / 4 bands per image, the
                             # last one short (1, 2, 7 rows); 3 images: 111, 30, 18, 12 tiles, no multiple of 8 (workgroups of the XCD mapping return early)
SMALL = (13, 17)             # where wide gathered channels need it: cin 512 has no plan on 37 x 39 beyond TR = 1 (the patch alone exceeds the LDS)
REF_BATCH = {MAIN: 3, SMALL: 5}   # images of the shared fp64 references: the border frame of 13 x 17 has 56 pixels (4 images would do: 5376 elements); 5: 65 / 10 tiles
TR_OF_MT = {1: 1, 2: 4, 3: 7, 4: 10}                 # on MAIN

# (cin, B, (H, W), cout, TR, NTW) -> (MT, NTW, channel blocks NB, KSC, chunks NCH, R).  cout leaves the last 16-channel tile 8 wide: 16 * NTW - 8
# in one block; NTW = 1: 24 = a second block of 8 (16 * 1 - 8 = 8 channels are too few for the compared subsets); the ring-of-3 cases have
# two blocks, the second with NTW // 2 tiles.  A few ring cases need other TR (the band rows decide what is left for the ring): 2, 8, 9, 11, 12
# -- TR 9 and 12 end the image on a band of ONE row.
TABLE = collections.OrderedDict([
    # MT 1
    ((32, 3, MAIN, 24, 1, 1), (1, 1, 2, 9, 1, 2)), ((384, 3, MAIN, 24, 2, 1), (1, 1, 2, 12, 9, 3)), ((512, 5, SMALL, 24, 1, 1), (1, 1, 2, 16, 9, 4)),
    ((64, 3, MAIN, 24, 1, 2), (1, 2, 1, 18, 1, 2)), ((512, 5, SMALL, 40, 1, 2), (1, 2, 2, 16, 9, 3)), ((256, 3, MAIN, 24, 1, 2), (1, 2, 1, 8, 9, 4)),
    ((128, 3, MAIN, 40, 1, 3), (1, 3, 1, 36, 1, 2)), ((256, 3, MAIN, 56, 1, 3), (1, 3, 2, 8, 9, 3)), ((144, 3, MAIN, 40, 1, 3), (1, 3, 1, 5, 9, 4)),
    ((256, 5, SMALL, 88, 1, 4), (1, 4, 2, 8, 9, 3)), ((128, 3, MAIN, 56, 1, 4), (1, 4, 1, 4, 9, 4)),
    ((256, 5, SMALL, 104, 1, 5), (1, 5, 2, 8, 9, 3)), ((96, 3, MAIN, 72, 1, 5), (1, 5, 1, 3, 9, 4)),
    ((144, 3, MAIN, 136, 1, 6), (1, 6, 2, 5, 9, 3)), ((72, 3, MAIN, 88, 1, 6), (1, 6, 1, 3, 9, 4)),
    ((128, 3, MAIN, 200, 1, 9), (1, 9, 2, 4, 9, 3)), ((144, 3, MAIN, 136, 1, 9), (1, 9, 1, 1, 45, 4)),
    # MT 2
    ((40, 3, MAIN, 24, 4, 1), (2, 1, 2, 18, 1, 2)), ((264, 3, MAIN, 24, 4, 1), (2, 1, 2, 9, 9, 3)), ((256, 3, MAIN, 24, 4, 1), (2, 1, 2, 8, 9, 4)),
    ((96, 3, MAIN, 24, 4, 2), (2, 2, 1, 27, 1, 2)), ((256, 5, SMALL, 40, 8, 2), (2, 2, 2, 8, 9, 3)), ((144, 3, MAIN, 24, 4, 2), (2, 2, 1, 5, 9, 4)),
    ((72, 3, MAIN, 40, 4, 3), (2, 3, 1, 27, 1, 2)), ((192, 3, MAIN, 56, 4, 3), (2, 3, 2, 6, 9, 3)), ((128, 3, MAIN, 40, 4, 3), (2, 3, 1, 4, 9, 4)),
    ((64, 3, MAIN, 56, 4, 4), (2, 4, 1, 18, 1, 2)), ((256, 5, SMALL, 88, 8, 4), (2, 4, 2, 4, 18, 3)), ((144, 3, MAIN, 56, 4, 4), (2, 4, 1, 5, 9, 4)),
    ((32, 3, MAIN, 72, 4, 5), (2, 5, 1, 9, 1, 2)), ((144, 3, MAIN, 104, 4, 5), (2, 5, 2, 5, 9, 3)), ((96, 3, MAIN, 72, 4, 5), (2, 5, 1, 3, 9, 4)),
    ((64, 3, MAIN, 88, 4, 6), (2, 6, 1, 18, 1, 2)), ((128, 3, MAIN, 136, 4, 6), (2, 6, 2, 4, 9, 3)), ((256, 3, MAIN, 88, 4, 6), (2, 6, 1, 1, 72, 4)),
    ((32, 3, MAIN, 136, 4, 9), (2, 9, 1, 9, 1, 2)), ((96, 3, MAIN, 200, 4, 9), (2, 9, 2, 3, 9, 3)), ((72, 3, MAIN, 136, 4, 9), (2, 9, 1, 3, 9, 4)),
    # MT 3
    ((144, 3, MAIN, 24, 7, 1), (3, 1, 2, 45, 1, 2)), ((192, 3, MAIN, 24, 7, 1), (3, 1, 2, 6, 9, 3)), ((144, 3, MAIN, 24, 8, 1), (3, 1, 2, 5, 9, 4)),
    ((72, 3, MAIN, 24, 7, 2), (3, 2, 1, 27, 1, 2)), ((192, 3, MAIN, 40, 7, 2), (3, 2, 2, 3, 18, 3)), ((128, 3, MAIN, 24, 7, 2), (3, 2, 1, 4, 9, 4)),
    ((96, 3, MAIN, 40, 7, 3), (3, 3, 1, 27, 1, 2)), ((144, 3, MAIN, 56, 7, 3), (3, 3, 2, 5, 9, 3)), ((128, 3, MAIN, 40, 7, 3), (3, 3, 1, 4, 9, 4)),
    ((40, 3, MAIN, 56, 7, 4), (3, 4, 1, 18, 1, 2)), ((128, 3, MAIN, 88, 7, 4), (3, 4, 2, 4, 9, 3)), ((72, 3, MAIN, 56, 7, 4), (3, 4, 1, 3, 9, 4)),
    ((64, 3, MAIN, 72, 7, 5), (3, 5, 1, 18, 1, 2)), ((128, 3, MAIN, 104, 7, 5), (3, 5, 2, 4, 9, 3)), ((144, 3, MAIN, 72, 7, 5), (3, 5, 1, 1, 45, 4)),
    ((32, 3, MAIN, 88, 7, 6), (3, 6, 1, 9, 1, 2)), ((128, 3, MAIN, 136, 9, 6), (3, 6, 2, 2, 18, 3)), ((64, 3, MAIN, 88, 7, 6), (3, 6, 1, 2, 9, 4)),
    # MT 4
    ((128, 3, MAIN, 24, 10, 1), (4, 1, 2, 36, 1, 2)), ((128, 3, MAIN, 24, 12, 1), (4, 1, 2, 4, 9, 3)), ((144, 3, MAIN, 24, 10, 1), (4, 1, 2, 5, 9, 4)),
    ((96, 3, MAIN, 24, 10, 2), (4, 2, 1, 27, 1, 2)), ((128, 3, MAIN, 40, 11, 2), (4, 2, 2, 4, 9, 3)), ((144, 3, MAIN, 24, 10, 2), (4, 2, 1, 1, 45, 4)),
    ((64, 3, MAIN, 40, 10, 3), (4, 3, 1, 18, 1, 2)), ((128, 3, MAIN, 56, 11, 3), (4, 3, 2, 2, 18, 3)), ((96, 3, MAIN, 40, 10, 3), (4, 3, 1, 3, 9, 4)),
    ((32, 3, MAIN, 56, 10, 4), (4, 4, 1, 9, 1, 2)), ((128, 3, MAIN, 88, 12, 4), (4, 4, 2, 1, 36, 3)), ((72, 3, MAIN, 56, 10, 4), (4, 4, 1, 3, 9, 4)),
])
# pairs of the reachable set no forced small map produces, with the reason: none -- 37 x 39 and 13 x 17 reach all 68
EXCEPTIONS = {}
# one chunk at MT = 1, NTW >= 4: plans the force produces and the cost model never keeps (module docstring)
FORCED_ONLY = collections.OrderedDict([
    ((32, 3, MAIN, 56, 1, 4), (1, 4, 1, 9, 1, 2)), ((40, 3, MAIN, 72, 1, 5), (1, 5, 1, 18, 1, 2)),
    ((64, 3, MAIN, 88, 1, 6), (1, 6, 1, 18, 1, 2)), ((32, 3, MAIN, 136, 1, 9), (1, 9, 1, 9, 1, 2)),
])

# hand count: (MT, NTW) -> ring slots R (2 = one chunk)
_PAIRS = [(mt, ntw) for mt in (1, 2, 3, 4) for ntw in NTW_MENU if mt * ntw * 4 + 3 * (mt + ntw) * 4 <= 216 and WAVES * mt * 16 * (16 * ntw * 4 + 16) <= 160 * 1024]
CONFIGS = {pair: ({3, 4} if pair[0] == 1 and pair[1] >= 4 else {2, 3, 4}) for pair in _PAIRS}
PAIR_COUNT, CONFIG_COUNT = 24, 68

# the sweep of the CPU test: maps at both sides of 20, 40 and 80 pixels per side, and ragged ones; every batch 1 .. 64, cin 32 .. 512 step 8,
# cout 8 .. 512 step 8
SWEEP_MAPS = ((20, 20), (21, 21), (40, 40), (41, 41), (80, 80), (81, 81), (13, 17), (33, 9), (37, 39))
SWEEP_BATCHES = range(1, 65)
SWEEP_CINS = range(32, 520, 8)
SWEEP_COUTS = range(8, 520, 8)

# ---- data gradient (natural dispatch), extremes, packed-weight cache: cases of test_conv_tile_gpu.py -----------------------------------------
DG_GATHERED = (32, 64, 80, 144)      # dy channels = the forward's cout
DG_DX = (16, 40, 80)                 # dx channels = the forward's cin
DG_FORCED = ((144, 40, 1, 0), (64, 80, 4, 0), (80, 40, 7, 0), (32, 16, 10, 0))   # (dy, dx, TR, NTW): one case per MT under the force
# (B, H, W, cin, cout, TR, NTW) -> (MT, NTW); TR = NTW = 0: the cost model's plan
EXTREMES = collections.OrderedDict([
    ((1, 2, 2, 64, 16, 0, 0), (1, 1)),        # 4 pixels: one pixel group, seven waves without pixels
    ((1, 2, 512, 32, 16, 1, 0), (4, 1)),      # the widest row: 512 pixels = 32 groups, magic-number division by 512 and 514
    ((1, 3, 50, 40, 8, 0, 0), (1, 1)),        # of test_row_band_conv_kernel_all_epilogues
    ((2, 5, 23, 72, 40, 4, 3), (1, 3)),       # 5 = 4 + 1 rows: the last band is one row of 23 pixels; ragged cin
])


def _query(fn, B, H, W, cin, cout):
    from computervision.pytorch_amd import _lib as L
    out = (ctypes.c_int32 * 8)()
    return tuple(out) if getattr(L.load(), fn)(B, H, W, cin, cout, out) == 0 else None


def tile_plan(B, H, W, cin, cout):
    """cvx_debug_conv_tile_plan (host code): (TR, MT, NTW, NB, workgroups, KSC, LDS bytes, cost x 100), or None where the kernel has no plan"""
    return _query("cvx_debug_conv_tile_plan", B, H, W, cin, cout)


def tile_ring(B, H, W, cin, cout):
    """cvx_debug_conv_tile_ring (host code): (KSC, NCH, R, SPT, PW, PP, MT, NTW) of the same plan, or None"""
    return _query("cvx_debug_conv_tile_ring", B, H, W, cin, cout)


def launch_key(B, H, W, cin, cout):
    """(MT, NTW, NB, KSC, NCH, R) of the launch, as TABLE states it, from both query functions; None without a plan"""
    p, r = tile_plan(B, H, W, cin, cout), tile_ring(B, H, W, cin, cout)
    if p is None or r is None:
        assert p is None and r is None, (p, r)
        return None
    assert (p[1], p[2], p[5]) == (r[6], r[7], r[0]), (p, r)
    return (p[1], p[2], p[3], r[0], r[1], r[2])


def first_wait(ring, ntw):
    """the argument of the kernel's wait before the K loop: (npre - 1) * PW DMA pieces may stay in flight (npre = min(NCH, R - 1) chunks requested)"""
    ksc, nch, R, spt, pw = ring[:5]
    assert pw == (ksc * ntw + WAVES - 1) // WAVES
    return (min(nch, R - 1) - 1) * pw


@contextlib.contextmanager
def forced(tr, ntw):
    """cvx_debug_conv_tile_force(tr, ntw) for the block; (0, 0) before and after"""
    from computervision.pytorch_amd import _lib as L
    lib = L.load()
    prev = lib.cvx_debug_conv_tile_force(tr, ntw)
    assert prev == 0, prev
    try:
        yield
    finally:
        assert lib.cvx_debug_conv_tile_force(0, 0) == (tr << 8) | ntw
