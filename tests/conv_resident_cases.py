"""The shapes on which tests/test_conv_resident_gpu.py runs the two convolution kernels with LDS-resident weights, and the compiled
instantiation the launcher must pick for each:

* csrc/conv_halo.hip (3x3 / stride 1): (TH output rows per tile, NT channel tiles per workgroup, HV tile streams) per gathered channel
  count -- 56 configurations;
* csrc/conv_pw.hip (1x1 / stride 1): (NS 32-wide K-steps, NT channel tiles per workgroup), MT = 2 pixel groups per wave tile up to 8
  K-steps and 1 beyond -- 51 configurations.

tests/test_conv_resident_plan_cpu.py holds the launchers (through ``cvx_debug_conv_halo_plan`` / ``cvx_debug_conv_pw_plan``, the functions
they call themselves) to this table without a GPU, establishes the set of reachable configurations by a sweep of its own and compares it with
the table and with the hand counts below, so a moved threshold or a dropped ``case`` names the configuration that lost its case.

The counts (56, 51) and the per-channel-count lists below were first made by reading the launchers; the sweep over the built library
confirmed every one of them, and found no plan whose single-stream LDS exceeds 160 KiB.
"""
import collections

# ---- halo kernel ---------------------------------------------------------------------------------------------------------------------
HALO_CINS = (16, 32, 64, 80, 128, 144)
HALO_MAX_COUT = 176
# the smallest maps that still have every tail: TH = 8 needs h * w >= 80 * 80 (81 = 10 * 8 + 1 rows, 83 = 5 * 16 + 3 columns), TH = 4
# h * w >= 40 * 40, TH = 2 below that
MAP_TH8, MAP_TH4, MAP_TH2 = (81, 83), (41, 43), (37, 39)
MAP_TH8_ODD = (97, 77)      # 13 x 5 = 65 tiles of 8 rows: an odd count (81 x 83 has 66) for the two-stream persistent walk
REF_BATCH = {MAP_TH8: 1, MAP_TH4: 3, MAP_TH2: 3, MAP_TH8_ODD: 1}   # images the shared fp64 references hold; cases run the first B of them

# (cin, B, (H, W), cout) -> (TH, NT, channel blocks, HV).  Output channels from {16, 32, 36, 64, 80, 96, 128, 144, 176}: 36 leaves the last
# 16-channel tile 4 wide, 144 and 176 give several channel blocks with a ragged last one.  B = 2 on 41 x 43 with 16 output channels: the
# one-pixel border frame of one image has 164 pixels, 2624 elements -- below the 4096 a compared subset must hold.  Wide gathered channels
# run 4-row tiles on the 81 x 83 map as well (the launcher's hv1 rule); two cases use that.
HALO_TABLE = collections.OrderedDict([
    # cin 16 (cap 8): 18 configurations, all single-stream
    ((16, 2, MAP_TH2, 16), (2, 1, 1, 1)), ((16, 2, MAP_TH2, 36), (2, 2, 1, 1)), ((16, 2, MAP_TH2, 176), (2, 3, 2, 1)), ((16, 2, MAP_TH2, 128), (2, 4, 1, 1)),
    ((16, 2, MAP_TH4, 16), (4, 1, 1, 1)), ((16, 1, MAP_TH4, 32), (4, 2, 1, 1)), ((16, 1, MAP_TH4, 36), (4, 3, 1, 1)), ((16, 1, MAP_TH4, 64), (4, 4, 1, 1)),
    ((16, 1, MAP_TH4, 144), (4, 5, 2, 1)), ((16, 1, MAP_TH4, 96), (4, 6, 1, 1)), ((16, 1, MAP_TH4, 128), (4, 8, 1, 1)),
    ((16, 1, MAP_TH8, 16), (8, 1, 1, 1)), ((16, 1, MAP_TH8, 32), (8, 2, 1, 1)), ((16, 1, MAP_TH8, 36), (8, 3, 1, 1)), ((16, 1, MAP_TH8, 64), (8, 4, 1, 1)),
    ((16, 1, MAP_TH8, 80), (8, 5, 1, 1)), ((16, 1, MAP_TH8, 176), (8, 6, 2, 1)), ((16, 1, MAP_TH8, 128), (8, 8, 1, 1)),
    # cin 32 (cap 8): 18; four 32-channel pairs on 2-row tiles run two streams
    ((32, 2, MAP_TH2, 32), (2, 1, 1, 1)), ((32, 2, MAP_TH2, 64), (2, 2, 1, 1)), ((32, 2, MAP_TH2, 80), (2, 3, 1, 1)), ((32, 2, MAP_TH2, 128), (2, 4, 1, 2)),
    ((32, 2, MAP_TH4, 16), (4, 1, 1, 1)), ((32, 1, MAP_TH4, 32), (4, 2, 1, 1)), ((32, 1, MAP_TH4, 36), (4, 3, 1, 1)), ((32, 1, MAP_TH4, 64), (4, 4, 1, 1)),
    ((32, 1, MAP_TH4, 80), (4, 5, 1, 1)), ((32, 1, MAP_TH4, 176), (4, 6, 2, 1)), ((32, 1, MAP_TH4, 128), (4, 8, 1, 1)),
    ((32, 1, MAP_TH8, 16), (8, 1, 1, 1)), ((32, 1, MAP_TH8, 32), (8, 2, 1, 1)), ((32, 1, MAP_TH8, 36), (8, 3, 1, 1)), ((32, 1, MAP_TH8, 64), (8, 4, 1, 1)),
    ((32, 1, MAP_TH8, 144), (8, 5, 2, 1)), ((32, 1, MAP_TH8, 96), (8, 6, 1, 1)), ((32, 1, MAP_TH8, 128), (8, 8, 1, 1)),
    # cin 64 (cap 4): 9
    ((64, 2, MAP_TH2, 32), (2, 1, 1, 1)), ((64, 2, MAP_TH2, 176), (2, 2, 3, 2)),
    ((64, 2, MAP_TH4, 16), (4, 1, 1, 1)), ((64, 1, MAP_TH4, 32), (4, 2, 1, 1)), ((64, 1, MAP_TH4, 144), (4, 3, 3, 2)), ((64, 1, MAP_TH4, 64), (4, 4, 1, 2)),
    ((64, 1, MAP_TH8, 16), (8, 1, 1, 1)), ((64, 1, MAP_TH8, 32), (8, 2, 1, 2)), ((64, 1, MAP_TH8, 36), (8, 3, 1, 2)),
    # cin 80 (cap 3): 5
    ((80, 2, MAP_TH2, 36), (2, 1, 2, 1)),
    ((80, 2, MAP_TH4, 16), (4, 1, 1, 1)), ((80, 1, MAP_TH4, 64), (4, 2, 2, 2)), ((80, 1, MAP_TH4, 176), (4, 3, 4, 2)),
    ((80, 1, MAP_TH8, 16), (8, 1, 1, 2)),
    # cin 128 (cap 2): 3; no 8-row tiles
    ((128, 2, MAP_TH2, 36), (2, 1, 2, 2)), ((128, 2, MAP_TH4, 16), (4, 1, 1, 2)), ((128, 1, MAP_TH8, 80), (4, 2, 3, 1)),
    # cin 144 (cap 2): 3
    ((144, 2, MAP_TH2, 32), (2, 1, 1, 1)), ((144, 1, MAP_TH8, 16), (4, 1, 1, 1)), ((144, 1, MAP_TH4, 176), (4, 2, 6, 1)),
])

# hand count, as (TH, NT, HV) per gathered channel count (cap = 16-channel tiles whose weights fit the launcher's 88 KiB budget)
_SINGLE = [(2, n, 1) for n in (1, 2, 3, 4)] + [(th, n, 1) for th in (4, 8) for n in (1, 2, 3, 4, 5, 6, 8)]
HALO_CONFIGS = {
    16: set(_SINGLE),
    32: (set(_SINGLE) - {(2, 4, 1)}) | {(2, 4, 2)},
    64: {(2, 1, 1), (2, 2, 2), (4, 1, 1), (4, 2, 1), (4, 3, 2), (4, 4, 2), (8, 1, 1), (8, 2, 2), (8, 3, 2)},
    80: {(2, 1, 1), (4, 1, 1), (4, 2, 2), (4, 3, 2), (8, 1, 2)},
    128: {(2, 1, 2), (4, 1, 2), (4, 2, 1)},
    144: {(2, 1, 1), (4, 1, 1), (4, 2, 1)},
}
HALO_COUNT = 56
# maps at both sides of every threshold of halo_plan: h * w 1600 and 6400, B * h * w 128 K
HALO_SWEEP_MAPS = ((1, 40, 40), (1, 39, 41), (1, 80, 80), (1, 79, 81), (82, 39, 41), (81, 39, 41), (21, 79, 79), (22, 79, 79))

# ---- pointwise kernel ----------------------------------------------------------------------------------------------------------------
PW_MAP = (2, 37, 39)         # 2886 pixels: no multiple of 32 or 16, the last workgroup has a wave without tiles
PW_MAX_COUT = 176
# NS -> (cin whose last K-step is ragged or absent, cin that fills every step): 136 at NS = 6 has a sixth step with no channels at all
PW_CINS = collections.OrderedDict([(1, (24, 32)), (2, (40, 64)), (3, (72, 96)), (4, (104, 128)), (6, (136, 192)), (8, (200, 256)), (12, (264, 384)),
                                   (16, (392, 512))])
# NT -> (cout, channel blocks) per cap (16-channel tiles whose weights fit the launcher's 64 KiB budget: 8 up to NS = 8, 5 at 12, 4 at 16);
# odd NT take the ragged cin, even NT the full one
_PW_COUTS_A = {1: (16, 1), 2: (32, 1), 3: (36, 1), 4: (64, 1), 5: (144, 2), 6: (96, 1), 8: (128, 1)}    # NS 1, 3, 6
_PW_COUTS_B = {1: (16, 1), 2: (32, 1), 3: (36, 1), 4: (64, 1), 5: (80, 1), 6: (176, 2), 8: (128, 1)}    # NS 2, 4, 8
_PW_COUTS_12 = {1: (16, 1), 2: (32, 1), 3: (36, 1), 4: (128, 2), 5: (80, 1)}
_PW_COUTS_16 = {1: (16, 1), 2: (32, 1), 3: (36, 1), 4: (128, 2)}
_PW_COUTS = {1: _PW_COUTS_A, 2: _PW_COUTS_B, 3: _PW_COUTS_A, 4: _PW_COUTS_B, 6: _PW_COUTS_A, 8: _PW_COUTS_B, 12: _PW_COUTS_12, 16: _PW_COUTS_16}
# (cin, cout) -> (NS, NT, channel blocks, MT)
PW_TABLE = collections.OrderedDict(
    ((PW_CINS[ns][0 if nt % 2 else 1], cout), (ns, nt, gy, 2 if ns <= 8 else 1)) for ns, couts in _PW_COUTS.items() for nt, (cout, gy) in couts.items())
PW_CONFIGS = ({(ns, nt, 2) for ns in (1, 2, 3, 4, 6, 8) for nt in (1, 2, 3, 4, 5, 6, 8)} | {(12, nt, 1) for nt in (1, 2, 3, 4, 5)} |
              {(16, nt, 1) for nt in (1, 2, 3, 4)})
PW_COUNT = 51

# ---- persistent walks (test_conv_resident_gpu.py): cases of the tables above on more images, grid divided -------------------------------
# (cin, B, map, cout, grid divisor): one single-stream and one two-stream configuration per TH family
HALO_WALKS = [
    (64, 3, MAP_TH4, 32, 128), (64, 3, MAP_TH4, 144, 16),       # (4, 2, 1) and (4, 3, 2) x 3 blocks: 99 tiles
    (32, 3, MAP_TH2, 80, 128), (32, 3, MAP_TH2, 128, 64),       # (2, 3, 1) and (2, 4, 2): 171 tiles
    (16, 1, MAP_TH8, 36, 256), (64, 1, MAP_TH8, 36, 64),        # (8, 3, 1) and (8, 3, 2): 66 tiles
    (64, 1, MAP_TH8_ODD, 36, 64),                               # (8, 3, 2) on 65 tiles
]
PW_WALKS = [(72, 36, 256), (264, 36, 256)]                      # (cin, cout, grid divisor): MT = 2 and MT = 1


def halo_lds(th, wm, bn, cin, hv):
    """LDS bytes of a halo workgroup (csrc/conv_halo.hip, halo_lds): patch buffers + dump piece | weights | statistics scratch"""
    pieces = ((th + 2) * 18 * (cin // 8) + 63) // 64
    nsteps = (9 * cin + 31) // 32
    return (2 * hv * pieces + 1) * 1024 + nsteps * bn * 32 * 2 + hv * wm * bn * 2 * 4


def halo_tiles(B, H, W, th):
    return B * ((H + th - 1) // th) * ((W + 15) // 16)


def halo_grid_x(plan, cin, total, div):
    """gridDim.x of the halo launch (launch_halo_hv): workgroups that fit the chip, over the channel blocks and the divisor"""
    th, nt, gy, hv = plan
    lds = halo_lds(th, 2 if th == 2 else 4, (32 if th == 2 else 16) * nt, cin, hv)
    per_cu = max(1, min(4, 160 * 1024 // lds))
    if hv == 2:
        per_cu = min(per_cu, 2)
    gx = max(1, 256 * per_cu // gy // div)
    return min(gx, (total + hv - 1) // hv)


def pw_grid_x(plan, pixels, div):
    """(gridDim.x, wave tiles) of the pointwise launch (launch_pw)"""
    ns, nt, gy, mt = plan
    lds = 1024 + ns * nt * 16 * 32 * 2 + 4 * nt * 16 * 2 * 4
    per_cu = max(1, min(4, 160 * 1024 // lds))
    n_wave_tiles = (pixels + mt * 16 - 1) // (mt * 16)
    gx = 256 * per_cu // gy // div
    return max(1, min(gx, (n_wave_tiles + 3) // 4)), n_wave_tiles


def _plan(fn, *args):
    import ctypes

    from computervision.pytorch_amd import _lib as L
    out = (ctypes.c_int32 * 4)()
    L.check(getattr(L.load(), fn)(*args, out), fn)
    return tuple(out)


def halo_plan(B, H, W, cin, cout):
    """what the halo launcher picks (cvx_debug_conv_halo_plan, host code): (TH, NT, channel blocks, HV)"""
    return _plan("cvx_debug_conv_halo_plan", B, H, W, cin, cout)


def pw_plan(pixels, cin, cout):
    """what the pointwise launcher picks (cvx_debug_conv_pw_plan, host code): (NS, NT, channel blocks, MT)"""
    return _plan("cvx_debug_conv_pw_plan", pixels, cin, cout)
