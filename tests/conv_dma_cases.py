"""The shapes on which tests/test_conv_dma_gpu.py runs the LDS-DMA ring convolution kernel (csrc/conv_igemm_dma.hip), and the tile
configuration its launcher must pick for each: 128-row and 64-row tiles with 1, 2, 3, 4, 5, 6 or 8 16-channel tiles per workgroup, 32-row
tiles with 1 .. 4 32-channel pairs -- 18 compiled configurations.  tests/test_conv_dma_plan_cpu.py holds the launcher (through
``cvx_debug_conv_dma_plan``) to this table without a GPU, so a moved threshold names the configuration that lost its case.
"""
import collections

# ---- forward: 3x3, stride 2, pad 1, 16 input channels, run with mode | 0x8000 --------------------------------------------------------
FWD_CIN, FWD_MAX_COUT = 16, 144
FWD_INPUTS = collections.OrderedDict([     # family -> (B, H, W): odd maps, so the last output row and column see the border taps
    (128, (2, 513, 515)),                  # 257 x 258 -> 132612 pixels, 4 rows past the last full tile
    (64, (1, 513, 515)),                   # 66306 pixels, 2 past
    (32, (1, 257, 259)),                   # 129 x 130 -> 16770 pixels, 2 past
])
FWD_COUTS = (16, 32, 36, 48, 64, 80, 96, 112, 128, 144)
# cout -> (channel tiles per workgroup, channel blocks): 36 leaves the last tile 4 channels wide, 112 has 7 real tiles of 8, 144 is two blocks of
# 5 with the second ragged (32 rows: two blocks of 3 pairs)
TILES_BIG = {16: (1, 1), 32: (2, 1), 36: (3, 1), 48: (3, 1), 64: (4, 1), 80: (5, 1), 96: (6, 1), 112: (8, 1), 128: (8, 1), 144: (5, 2)}
TILES_32 = {16: (1, 1), 32: (1, 1), 36: (2, 1), 48: (2, 1), 64: (2, 1), 80: (3, 1), 96: (3, 1), 112: (4, 1), 128: (4, 1), 144: (3, 2)}
# two heavy cases (taps * cin * cout >= 512 K and >= 8192 pixels): 64 rows / 8 tiles / two channel blocks at 8580 pixels
HEAVY_CASES = [   # B, H, W, cin, cout, k, stride, pad, dil
    (2, 129, 131, 256, 256, 3, 2, 1, 1),
    (2, 65, 66, 256, 256, 3, 1, 2, 2),
]

# ---- merged-phase data gradient of a 3x3 / stride 2 / pad 1 convolution with 16 output channels, natural dispatch ---------------------
DG_COUT_FWD, DG_MAX_CIN = 16, 144
DG_MAP = (513, 515)                        # phases 257x258, 257x257, 256x258, 256x257: the launch is sized for the first
DG_CINS = (16, 48, 80, 128, 144)           # dx channels: 1, 3, 5, 8 tiles and 5 in two blocks; none wide enough for the GEMM-shaped kernel
DG_BATCHES = {128: 2, 64: 1}
DG_SMALL = (2, 33, 35, 144)                # B, H, W, dx channels: phases of 612, 578, 576 and 544 pixels in the 32-row family
DG_TAPS_PHASE0 = 1                         # the launcher sees phase (0, 0)'s tap count: only the centre tap reaches an even / even pixel


def out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def passes(rows, tiles):
    """DMA passes per K-step: 64 stage rows per pass over the tile's pixel rows and channel rows"""
    return (rows + (32 if rows == 32 else 16) * tiles + 63) // 64


def partial_last_pass(rows, tiles):
    return (rows + (32 if rows == 32 else 16) * tiles) % 64 != 0


def plan_cases():
    """-> [(label, pixels, cin, cout, ntaps, (tile rows, channel tiles per workgroup, channel blocks, DMA passes))]"""
    out = []
    for rows, (B, H, W) in FWD_INPUTS.items():
        pixels = B * out_size(H, 3, 2, 1, 1) * out_size(W, 3, 2, 1, 1)
        for cout in FWD_COUTS:
            nt, gy = (TILES_32 if rows == 32 else TILES_BIG)[cout]
            out.append((f"forward {B}x{H}x{W} 16->{cout}", pixels, FWD_CIN, cout, 9, (rows, nt, gy, passes(rows, nt))))
    for B, H, W, ci, co, k, s, pad, dil in HEAVY_CASES:
        pixels = B * out_size(H, k, s, pad, dil) * out_size(W, k, s, pad, dil)
        out.append((f"heavy {B}x{H}x{W} {ci}->{co} k{k} s{s} d{dil}", pixels, ci, co, k * k, (64, 8, 2, passes(64, 8))))
    H, W = DG_MAP
    for rows, B in DG_BATCHES.items():
        for cin in DG_CINS:
            nt, gy = TILES_BIG[cin]
            out.append((f"dgrad {B}x{H}x{W} dx {cin}", B * ((H + 1) // 2) * ((W + 1) // 2), DG_COUT_FWD, cin, DG_TAPS_PHASE0, (rows, nt, gy, passes(rows, nt))))
    B, H, W, cin = DG_SMALL
    nt, gy = TILES_32[cin]
    out.append((f"dgrad {B}x{H}x{W} dx {cin}", B * ((H + 1) // 2) * ((W + 1) // 2), DG_COUT_FWD, cin, DG_TAPS_PHASE0, (32, nt, gy, passes(32, nt))))
    return out


def launcher_plan(pixels, cin, cout, ntaps):
    """what the launcher picks (cvx_debug_conv_dma_plan, host code): (tile rows, channel tiles per workgroup, channel blocks, DMA passes)"""
    import ctypes

    from computervision.pytorch_amd import _lib as L
    out = (ctypes.c_int32 * 4)()
    L.check(L.load().cvx_debug_conv_dma_plan(pixels, cin, cout, ntaps, out), "dma plan")
    return tuple(out)


ALL_CONFIGS = {(rows, nt) for rows in (128, 64) for nt in (1, 2, 3, 4, 5, 6, 8)} | {(32, nt) for nt in (1, 2, 3, 4)}
