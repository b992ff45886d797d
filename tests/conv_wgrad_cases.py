"""The shapes on which tests/test_conv_wgrad_gpu.py runs the five weight-gradient kernels behind ``cvx_conv_wgrad_launch``, and the compiled
instantiation (with the plan fields that change code paths) each of them must reach when its kernel is run directly:

* csrc/conv_wgrad_k3.hip: configuration CfgA .. CfgH (0 .. 7) x ring slots (2, 3, 4) x column blocks (1, or 2 for "several") -- 38 keys; the
  stride-2 phase-plane variant is configurations 6 and 7;
* csrc/conv_wgrad_stream.hip: 1x1 or 3x3 x (CO_T, JW) x wave layout WN x WK x tap blocks (1, or 3 kernel rows) -- 42 keys over the 14
  compiled (CO_T, JW) pairs;
* csrc/conv_wgrad_halo.hip: (CO_T, CI_T), nine taps per workgroup below 8 tile pairs and three from there -- 16;
* csrc/conv_wgrad_gemm.hip: the 128 x 128 and the 256 x 256 tile -- 2;
* the generic kernel of csrc/conv_wgrad.hip: five (co, j) tiles -- 5.

tests/test_conv_wgrad_plan_cpu.py holds the launchers to this table through ``cvx_debug_conv_wgrad_plan`` (host code: it calls k3_plan,
ws_plan, pick_tiles and the two tile functions, as the launchers do), establishes the reachable keys by sweeps of its own and compares them
with the table and with the hand counts below.  Every compiled instantiation is reachable, by the dispatcher or when its kernel is asked for.

The maps are the smallest found (by a search over the plan entry) on which the planner produces the key AND the launch has every tail:
two images, a last row block with fewer rows than the others (k3 / stream 3x3: OH > R and OH no multiple of R; where the planner only
ever yields the key on one-row maps -- CfgB with two ring slots -- OH = 1 and more images), a last column block narrower than the others where there are
several, odd input maps for stride 2, pixel counts per image that are no multiple of the chunk (stream 1x1: Qd; gemm: 32; generic: 128)
or of the 8 x 16 pixel tile (halo).  Channel counts prefer a padded last input tile (8 -> 16, 24 -> 32, 72 -> 80 ...) and an output count
that is no multiple of 16, and keep Cin * Cout >= 256: the elements of one tap, the smallest subset the GPU test compares.
"""
import collections
import ctypes

K3, STREAM, HALO, GEMM, GENERIC = 1, 2, 3, 4, 5
KERNEL_NAMES = {K3: "k3", STREAM: "stream", HALO: "halo", GEMM: "gemm", GENERIC: "generic"}
K3_CFG_NAMES = "ABCDEFGH"

Plan = collections.namedtuple("Plan", "kernel nsplit slab_bytes desc")


def plan(B, H, W, cin, cout, k, stride, kernel=0, nsplit=0, wide=0, dil=1, x_ld=None, dy_ld=None):
    """cvx_debug_conv_wgrad_plan (host code, no GPU) for a k x k / pad dil * (k // 2) layer -> Plan; raises CvxError where the kernel
    cannot run the shape"""
    from computervision.pytorch_amd import _lib as L
    out = (ctypes.c_int32 * 16)()
    L.check(L.load().cvx_debug_conv_wgrad_plan(B, H, W, cin, cout, k, stride, dil * (k // 2), dil, x_ld or cin, dy_ld or cout, kernel, nsplit,
                                               wide, out), "cvx_debug_conv_wgrad_plan")
    return Plan(out[0], out[1], out[2] + (out[3] << 31), tuple(out[4:]))


def try_plan(*a, **kw):
    from computervision.pytorch_amd import _lib as L
    try:
        return plan(*a, **kw)
    except L.CvxError:
        return None


def key_of(p, k):
    """the plan fields that change code paths"""
    d = p.desc
    if p.kernel == K3:          # configuration, ring slots, one / several column blocks   (d: cfg R Wc ncb nslot s2 units units_per_split G)
        return (d[0], d[4], min(d[3], 2))
    if p.kernel == STREAM:      # k, CO_T, JW, WN, WK, tap blocks   (d: CO_T JW WN WK tap_blks R|Qd nslot units units_per_split G CI_T)
        return (k, d[0], d[1], d[2], d[3], d[4])
    if p.kernel == HALO:        # CO_T, CI_T, taps per workgroup   (d: CO_T CI_T taps tiles tiles_per_split G)
        return (d[0], d[1], d[2])
    return (d[0], d[1])         # the (co, j) tile   (d: co_b j_b tiles)


def units_of(p, B, OH, OW):
    """work units the pixel splits divide: chunks (k3, stream), 8 x 16 pixel tiles (halo), 32- / 128-pixel steps (gemm / generic)"""
    if p.kernel == K3:
        return p.desc[6]
    if p.kernel == STREAM:
        return p.desc[7]
    if p.kernel == HALO:
        return p.desc[3]
    step = 32 if p.kernel == GEMM else 128
    return (B * OH * OW + step - 1) // step


def out_size(n, k, stride, dil=1):
    return (n + 2 * (dil * (k // 2)) - dil * (k - 1) - 1) // stride + 1


# ---- k3: (cin, cout, stride, (B, H, W)) -> (configuration, ring slots, column blocks 1 / 2+) ---------------------------------------------
K3_TABLE = collections.OrderedDict([
    # CfgA 16 -> 16: always four slots
    ((16, 16, 1, (2, 33, 6)), (0, 4, 1)), ((16, 16, 1, (2, 13, 53)), (0, 4, 2)),
    # CfgB 32 -> 32: two slots only on one-row maps from 142 columns
    ((32, 32, 1, (5, 1, 142)), (1, 2, 1)), ((24, 24, 1, (3, 1, 283)), (1, 2, 2)), ((32, 32, 1, (2, 14, 49)), (1, 3, 1)),
    ((24, 24, 1, (2, 19, 93)), (1, 3, 2)), ((32, 24, 1, (2, 33, 6)), (1, 4, 1)), ((32, 32, 1, (2, 28, 25)), (1, 4, 2)),
    # CfgC blocks of 64 x 64
    ((64, 64, 1, (2, 2, 125)), (2, 2, 1)), ((64, 64, 1, (2, 2, 993)), (2, 2, 2)), ((56, 64, 1, (2, 13, 22)), (2, 3, 1)),
    ((128, 56, 1, (2, 11, 59)), (2, 3, 2)), ((64, 128, 1, (2, 17, 6)), (2, 4, 1)), ((120, 64, 1, (2, 28, 11)), (2, 4, 2)),
    # CfgD 80 -> 80: two slots and one column block do not meet with a ragged row block
    ((80, 80, 1, (2, 17, 61)), (3, 2, 1)), ((80, 80, 1, (2, 4, 121)), (3, 2, 2)), ((72, 72, 1, (2, 11, 19)), (3, 3, 1)),
    ((72, 80, 1, (2, 11, 37)), (3, 3, 2)), ((80, 80, 1, (2, 17, 6)), (3, 4, 1)), ((72, 72, 1, (2, 28, 11)), (3, 4, 2)),
    # CfgE 48-channel co blocks
    ((64, 48, 1, (2, 2, 125)), (4, 2, 1)), ((64, 48, 1, (2, 2, 993)), (4, 2, 2)), ((56, 40, 1, (2, 11, 39)), (4, 3, 1)),
    ((128, 144, 1, (2, 11, 77)), (4, 3, 2)), ((64, 48, 1, (2, 17, 6)), (4, 4, 1)), ((56, 40, 1, (2, 28, 11)), (4, 4, 2)),
    # CfgF 32-channel co blocks
    ((64, 32, 1, (2, 2, 125)), (5, 2, 1)), ((64, 32, 1, (2, 2, 993)), (5, 2, 2)), ((56, 24, 1, (2, 9, 61)), (5, 3, 1)),
    ((128, 32, 1, (2, 5, 369)), (5, 3, 2)), ((64, 32, 1, (2, 17, 6)), (5, 4, 1)), ((56, 24, 1, (2, 28, 11)), (5, 4, 2)),
    # CfgG / CfgH: stride 2, four phase planes per slot -- never four slots
    ((16, 32, 2, (2, 35, 25)), (6, 2, 1)), ((8, 32, 2, (2, 37, 69)), (6, 2, 2)), ((16, 24, 2, (2, 65, 11)), (6, 3, 1)),
    ((16, 32, 2, (2, 61, 45)), (6, 3, 2)), ((32, 64, 2, (2, 33, 11)), (7, 2, 1)), ((24, 56, 2, (2, 19, 61)), (7, 2, 2)),
])
K3_COUNT = 38
# hand count: ring slots x column blocks per configuration
_ALL6 = {(ns, cb) for ns in (2, 3, 4) for cb in (1, 2)}
K3_KEYS = {0: {(4, 1), (4, 2)}, 1: _ALL6, 2: _ALL6, 3: _ALL6, 4: _ALL6, 5: _ALL6, 6: {(2, 1), (2, 2), (3, 1), (3, 2)}, 7: {(2, 1), (2, 2)}}
K3_REPRESENTATIVE = {0: (16, 16), 1: (32, 32), 2: (64, 64), 3: (80, 80), 4: (64, 48), 5: (64, 32), 6: (16, 32), 7: (32, 64)}   # cfg -> (cin, cout)

# ---- stream: (cin, cout, k, (B, H, W)) -> (k, CO_T, JW, WN, WK, tap blocks) -------------------------------------------------------------
STREAM_TABLE = collections.OrderedDict([
    # 3x3: four column-tile waves; one workgroup holds all nine taps while CO_T * ceil(9 * CI_T / 4) <= 18 tiles, else one kernel row
    ((104, 8, 3, (2, 55, 5)), (3, 1, 3, 4, 1, 1)), ((40, 8, 3, (2, 29, 5)), (3, 1, 3, 4, 1, 3)), ((8, 32, 3, (2, 37, 5)), (3, 2, 1, 4, 1, 3)),
    ((24, 24, 3, (2, 10, 11)), (3, 2, 5, 4, 1, 1)), ((24, 40, 3, (2, 19, 5)), (3, 3, 2, 4, 1, 3)), ((8, 40, 3, (2, 7, 19)), (3, 3, 3, 4, 1, 1)),
    ((40, 40, 3, (2, 19, 5)), (3, 3, 3, 4, 1, 3)), ((24, 56, 3, (2, 19, 5)), (3, 4, 2, 4, 1, 3)), ((8, 56, 3, (2, 19, 5)), (3, 4, 3, 4, 1, 1)),
    ((40, 56, 3, (2, 11, 5)), (3, 4, 3, 4, 1, 3)), ((8, 72, 3, (2, 19, 5)), (3, 5, 1, 4, 1, 3)), ((24, 72, 3, (2, 11, 5)), (3, 5, 2, 4, 1, 3)),
    ((72, 72, 3, (2, 11, 5)), (3, 5, 4, 4, 1, 3)),
    # 1x1: WN column-tile waves x WK K-step waves
    ((168, 8, 1, (2, 37, 7)), (1, 1, 1, 1, 4, 1)), ((32, 8, 1, (2, 37, 7)), (1, 1, 1, 2, 2, 1)), ((40, 8, 1, (2, 15, 13)), (1, 1, 1, 3, 1, 1)),
    ((56, 8, 1, (2, 10, 13)), (1, 1, 1, 4, 1, 1)), ((72, 8, 1, (2, 10, 13)), (1, 1, 3, 2, 2, 1)), ((104, 8, 1, (2, 5, 13)), (1, 1, 3, 3, 1, 1)),
    ((8, 32, 1, (2, 37, 7)), (1, 2, 1, 1, 4, 1)), ((24, 24, 1, (2, 10, 13)), (1, 2, 1, 2, 2, 1)), ((40, 24, 1, (2, 10, 13)), (1, 2, 1, 3, 1, 1)),
    ((56, 24, 1, (2, 10, 13)), (1, 2, 1, 4, 1, 1)), ((104, 24, 1, (2, 5, 13)), (1, 2, 2, 4, 1, 1)), ((136, 24, 1, (2, 10, 13)), (1, 2, 5, 2, 2, 1)),
    ((8, 40, 1, (2, 37, 7)), (1, 3, 1, 1, 4, 1)), ((24, 40, 1, (2, 10, 13)), (1, 3, 1, 2, 2, 1)), ((40, 40, 1, (2, 10, 13)), (1, 3, 1, 3, 1, 1)),
    ((56, 40, 1, (2, 5, 13)), (1, 3, 1, 4, 1, 1)), ((72, 40, 1, (2, 5, 13)), (1, 3, 2, 4, 1, 1)), ((136, 40, 1, (2, 5, 13)), (1, 3, 3, 3, 1, 1)),
    ((8, 56, 1, (2, 37, 7)), (1, 4, 1, 1, 4, 1)), ((24, 56, 1, (2, 10, 13)), (1, 4, 1, 2, 2, 1)), ((40, 56, 1, (2, 5, 13)), (1, 4, 1, 3, 1, 1)),
    ((56, 56, 1, (2, 5, 13)), (1, 4, 1, 4, 1, 1)), ((72, 56, 1, (2, 5, 13)), (1, 4, 2, 4, 1, 1)), ((136, 56, 1, (2, 5, 13)), (1, 4, 3, 3, 1, 1)),
    ((8, 72, 1, (2, 37, 7)), (1, 5, 1, 1, 4, 1)), ((24, 72, 1, (2, 10, 13)), (1, 5, 1, 2, 2, 1)), ((40, 72, 1, (2, 5, 13)), (1, 5, 1, 3, 1, 1)),
    ((56, 72, 1, (2, 5, 13)), (1, 5, 1, 4, 1, 1)), ((72, 72, 1, (2, 5, 13)), (1, 5, 2, 4, 1, 1)),
])
STREAM_COUNT = 42
STREAM_PAIRS = {(1, 3), (2, 5), (4, 3), (5, 4), (3, 3), (2, 1), (4, 1), (4, 2), (5, 2), (3, 1), (1, 1), (3, 2), (5, 1), (2, 2)}   # kCfgs: (CO_T, JW)
# hand count, (CO_T, JW, WN, WK, tap blocks).  3x3: WN x WK = 4 x 1; CI_T in 1 .. 5, nine taps where CO_T * ceil(9 CI_T / 4) <= 18 and the
# pair is compiled, else three: JW = ceil(3 CI_T / 4), compiled pairs only (CO_T 1: JW 3 twice -- CI_T 1 with nine taps, CI_T 3 / 4 with three)
STREAM_KEYS_3X3 = {(1, 3, 4, 1, 1), (1, 3, 4, 1, 3), (2, 1, 4, 1, 3), (2, 5, 4, 1, 1), (3, 2, 4, 1, 3), (3, 3, 4, 1, 1), (3, 3, 4, 1, 3), (4, 2, 4, 1, 3),
                   (4, 3, 4, 1, 1), (4, 3, 4, 1, 3), (5, 1, 4, 1, 3), (5, 2, 4, 1, 3), (5, 4, 4, 1, 3)}
# 1x1: CI_T in 1 .. 5, 7, 8, 9 -> (JW, WN, WK): a WN that divides CI_T first, then the widest that has a compiled pair
_K1 = {1: {(1, 1, 4), (1, 2, 2), (1, 3, 1), (1, 4, 1), (3, 2, 2), (3, 3, 1)},
       2: {(1, 1, 4), (1, 2, 2), (1, 3, 1), (1, 4, 1), (2, 4, 1), (5, 2, 2)},
       3: {(1, 1, 4), (1, 2, 2), (1, 3, 1), (1, 4, 1), (2, 4, 1), (3, 3, 1)},
       4: {(1, 1, 4), (1, 2, 2), (1, 3, 1), (1, 4, 1), (2, 4, 1), (3, 3, 1)},
       5: {(1, 1, 4), (1, 2, 2), (1, 3, 1), (1, 4, 1), (2, 4, 1)}}
STREAM_KEYS_1X1 = {(co_t, jw, wn, wk, 1) for co_t, v in _K1.items() for jw, wn, wk in v}

# ---- halo: (cin, cout, HALO_MAP) -> (CO_T, CI_T, taps per workgroup) ---------------------------------------------------------------------
HALO_MAP = (2, 21, 37)       # 3 x 3 pixel tiles per image, the last row of tiles 5 rows high, the last column 5 wide
HALO_TABLE = collections.OrderedDict([
    ((16, 16), (1, 1, 9)), ((32, 8), (1, 2, 9)), ((40, 8), (1, 4, 9)), ((72, 8), (1, 5, 9)),
    ((16, 24), (2, 1, 9)), ((24, 24), (2, 2, 9)), ((40, 24), (2, 4, 3)), ((72, 24), (2, 5, 3)),
    ((16, 40), (4, 1, 9)), ((24, 40), (4, 2, 3)), ((40, 40), (4, 4, 3)), ((72, 128), (4, 5, 3)),     # two co blocks of 64             
    ((16, 72), (5, 1, 9)), ((24, 72), (5, 2, 3)), ((40, 72), (5, 4, 3)), ((152, 72), (5, 5, 3)),     # 152 = 80 + 72: two ci blocks
])
HALO_COUNT = 16

# ---- gemm / generic: (cin, cout, k, stride, dil) on WIDE_MAP -> (co, j) tile --------------------------------------------------------------
WIDE_MAP = (2, 19, 27)       # output map; 513 pixels per image: no multiple of 32
GEMM_TABLE = collections.OrderedDict([
    ((72, 136, 3, 1, 1), (128, 128)),        # two co blocks, the second 8 channels wide; 720 columns: the sixth j block 80 wide
    ((504, 256, 1, 1, 1), (256, 256)),       # cin padded to 512
])
GEMM_COUNT = 2
GENERIC_TABLE = collections.OrderedDict([
    ((32, 8, 3, 2, 1), (16, 192)),           # cout <= 16
    ((8, 32, 1, 2, 1), (32, 128)),           # cout <= 32; a strided 1x1 (ResNet's downsample)
    ((72, 88, 3, 2, 1), (48, 128)),          # cout % 64 != 0 and cout <= 96
    ((40, 64, 3, 1, 2), (64, 64)),           # the rest; dilated (DeepLab's ASPP)
    ((152, 384, 3, 1, 1), (128, 128)),       # cout % 128 == 0, 512+ columns, 512 K+ elements
])
GENERIC_COUNT = 5


def wide_input_map(k, stride, dil):
    """the input map of a WIDE_MAP output: odd where stride 2"""
    B, OH, OW = WIDE_MAP
    H, W = (OH, OW) if stride == 1 else (2 * OH - 1, 2 * OW - 1)
    assert out_size(H, k, stride, dil) == OH and out_size(W, k, stride, dil) == OW
    return B, H, W


Case = collections.namedtuple("Case", "kernel cin cout k stride dil map key")


def all_cases():
    """every table entry as a Case (map = the INPUT map (B, H, W))"""
    out = [Case(K3, cin, cout, 3, s, 1, m, key) for (cin, cout, s, m), key in K3_TABLE.items()]
    out += [Case(STREAM, cin, cout, k, 1, 1, m, key) for (cin, cout, k, m), key in STREAM_TABLE.items()]
    out += [Case(HALO, cin, cout, 3, 1, 1, HALO_MAP, key) for (cin, cout), key in HALO_TABLE.items()]
    out += [Case(GEMM, cin, cout, k, s, d, wide_input_map(k, s, d), key) for (cin, cout, k, s, d), key in GEMM_TABLE.items()]
    out += [Case(GENERIC, cin, cout, k, s, d, wide_input_map(k, s, d), key) for (cin, cout, k, s, d), key in GENERIC_TABLE.items()]
    return out


def case_id(c):
    B, H, W = c.map
    return f"{KERNEL_NAMES[c.kernel]}-{c.cin}to{c.cout}-k{c.k}s{c.stride}d{c.dil}-{B}x{H}x{W}"


def case_plan(c, nsplit=0, wide=0, **kw):
    return plan(*c.map, c.cin, c.cout, c.k, c.stride, c.kernel, nsplit, wide, c.dil, **kw)


# ---- strided operands (test_conv_wgrad_gpu.py): per kernel, the channel-padding situations it supports -----------------------------------
# (kernel, cin, cout, k, stride, input map): Cin 8 -> 16, Cin 72 -> 80, a Cout that is no multiple of 16, and an unpadded layer.  The halo
# kernel takes Cin >= 16 and the gemm kernel dense dy only (strided x).
_WIDE1 = wide_input_map(3, 1, 1)
STRIDED_CASES = [
    (K3, 8, 32, 3, 2, (2, 37, 69)), (K3, 72, 72, 3, 1, (2, 11, 19)), (K3, 64, 40, 3, 1, (2, 11, 39)), (K3, 64, 64, 3, 1, (2, 13, 22)),
    (STREAM, 8, 32, 3, 1, (2, 37, 5)), (STREAM, 72, 72, 3, 1, (2, 11, 5)), (STREAM, 24, 40, 3, 1, (2, 19, 5)), (STREAM, 32, 32, 3, 1, (2, 10, 11)),
    (STREAM, 8, 32, 1, 1, (2, 37, 7)), (STREAM, 72, 56, 1, 1, (2, 5, 13)), (STREAM, 40, 24, 1, 1, (2, 10, 13)), (STREAM, 64, 64, 1, 1, (2, 5, 13)),
    (HALO, 72, 24, 3, 1, HALO_MAP), (HALO, 24, 40, 3, 1, HALO_MAP), (HALO, 64, 64, 3, 1, HALO_MAP),
    (GEMM, 8, 136, 3, 1, _WIDE1), (GEMM, 72, 136, 3, 1, _WIDE1), (GEMM, 64, 128, 1, 1, _WIDE1),
    (GENERIC, 8, 32, 1, 1, _WIDE1), (GENERIC, 72, 88, 3, 1, _WIDE1), (GENERIC, 40, 24, 3, 1, _WIDE1), (GENERIC, 64, 64, 3, 1, _WIDE1),
]
