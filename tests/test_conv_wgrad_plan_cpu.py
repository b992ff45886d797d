"""The launchers of the five weight-gradient kernels (csrc/conv_wgrad_k3.hip, conv_wgrad_stream.hip, conv_wgrad_halo.hip, conv_wgrad_gemm.hip,
conv_wgrad.hip) pick, for every case of tests/conv_wgrad_cases.py, the instantiation and plan key the table states -- and the table reaches
every key the planners can produce: 38 of the k3 kernel, 42 of the stream kernel, 16 halo, 2 gemm, 5 generic.  The reachable set is
established here by sweeping ``cvx_debug_conv_wgrad_plan`` (the planners the launchers call themselves; host code, no GPU needed) with
``kernel = 0`` (the dispatcher's cascade) and with every kernel forced, over channel counts 8 .. 512 in steps of 8, k in {1, 3}, stride in
{1, 2} on maps at both sides of every threshold, and -- the k3 and stream plans depend on the map -- over every map width for one channel
pair per configuration.  This is the lock of tests/test_conv_wgrad_gpu.py: when a threshold moves or a case is dropped, the failure names
the configuration that lost its case.  The same sweep checks the engine's pixel-split counts (``nsplit = 0``), and further tests hold the
dispatcher to the kernels the cases of tests/test_gpu_parity.py were written for and to table keys on every layer of the five models."""
import functools

import pytest
import torch

import conv_wgrad_cases as T
import test_conv_wgrad_gpu as G
from computervision.pytorch_amd import _lib as L

CASES = T.all_cases()
NAME = T.KERNEL_NAMES
TABLE = {kern: {} for kern in NAME}
for _c in CASES:
    assert _c.key not in TABLE[_c.kernel], f"{NAME[_c.kernel]}: two table entries for {_c.key}"
    TABLE[_c.kernel][_c.key] = _c


def _name(kern, key):
    if kern == T.K3:
        return f"k3 Cfg{T.K3_CFG_NAMES[key[0]]} with {key[1]} ring slots and {'several column blocks' if key[2] == 2 else 'one column block'}"
    if kern == T.STREAM:
        return f"stream {key[0]}x{key[0]} <CO_T {key[1]}, JW {key[2]}> as {key[3]} x {key[4]} waves with {key[5]} tap block(s)"
    if kern == T.HALO:
        return f"halo <CO_T {key[0]}, CI_T {key[1]}> with {key[2]} taps per workgroup"
    return f"{NAME[kern]} tile {key[0]} x {key[1]}"


@pytest.mark.parametrize("c", CASES, ids=[T.case_id(c) for c in CASES])
def test_the_launcher_picks_what_the_table_states(c):
    p = T.case_plan(c)
    assert p.kernel == c.kernel
    assert T.key_of(p, c.k) == c.key, f"{_name(c.kernel, c.key)} lost its case: {T.case_id(c)} now runs {_name(p.kernel, T.key_of(p, c.k))}"


# maps (B, H, W) at both sides of the planners' thresholds: OW 3 / 4 (k3_shape_ok, ws_shape_ok) and 5 / 6 (the narrowest k3 column block), OH
# 250 / 251 and OW 250 / 251 (k3: 8-bit row tags, widest stride-1 column block), OW 124 / 125 at stride 2 (input 247 / 249), OW 1024 / 1025
# (stream 3x3), OW 7 / 8 and OH 3 / 4 (gemm), small and large chunk counts, and 800 000 pixels and one row below (stream's preference)
SWEEP_MAPS = ((2, 3, 4), (2, 4, 3), (2, 5, 6), (2, 7, 9), (1, 13, 8), (1, 21, 23), (1, 81, 83), (1, 37, 250), (1, 37, 251), (1, 250, 8), (1, 251, 8),
              (1, 9, 247), (1, 9, 249), (1, 16, 1024), (1, 16, 1025))
BIG_MAPS = ((20, 200, 200), (20, 200, 199), (8, 320, 320), (8, 320, 312))


def _check_engine_count(p, k, cin, cout, units, what):
    """nsplit = 0: the engine's count for the kernel.  1 <= ns <= units; the k3 and stream planners promise no empty split, and the k3
    planner one round of workgroups from 9 splits up (a workgroup takes a whole CU; the launch rounds the count up to a multiple of 8);
    the slabs are ns * cout * k * k * round_up(cin, 16) floats."""
    ns = p.nsplit
    assert 1 <= ns <= units, (what, ns, units)
    assert p.slab_bytes == ns * cout * k * k * ((cin + 15) // 16 * 16) * 4, what
    if p.kernel in (T.K3, T.STREAM):
        ups, G_ = (p.desc[7], p.desc[8]) if p.kernel == T.K3 else (p.desc[8], p.desc[9])
        assert ups == (units + ns - 1) // ns and (ns - 1) * ups < units, (what, "an empty split", ns, ups, units)
        assert ns == 1 or units >= 2 * ns, (what, "fewer than two chunks per workgroup", ns, units)
        if p.kernel == T.K3 and ns > 8:
            assert (ns + 7) // 8 * 8 * G_ <= 256, (what, "more than one round of workgroups", ns, G_)


@functools.lru_cache(maxsize=None)
def _sweep():
    """{"dispatch" | "forced": {kernel: {key}}}"""
    got = {"dispatch": {k: set() for k in NAME}, "forced": {k: set() for k in NAME}}

    def visit(B, H, W, cin, cout, k, s, kern, wide=0):
        p = T.try_plan(B, H, W, cin, cout, k, s, kern, 0, wide)
        if p is None:
            assert kern != 0 and kern != T.GENERIC, ("the cascade and the generic kernel take every layer", B, H, W, cin, cout, k, s)
            return None
        got["forced" if kern else "dispatch"][p.kernel].add(T.key_of(p, k))
        OH, OW = T.out_size(H, k, s), T.out_size(W, k, s)
        _check_engine_count(p, k, cin, cout, T.units_of(p, B, OH, OW), (B, H, W, cin, cout, k, s, kern, wide))
        return p

    for k in (1, 3):
        for s in (1, 2):
            kerns = [0, T.GEMM, T.GENERIC] + ([T.K3] if k == 3 else []) + ([T.STREAM] if s == 1 else []) + ([T.HALO] if (k, s) == (3, 1) else [])
            for B, H, W in SWEEP_MAPS:
                for cin in range(8, 520, 8):
                    for cout in range(8, 520, 8):
                        for kern in kerns:
                            visit(B, H, W, cin, cout, k, s, kern)
    # the map-dependent plans: every output width for one channel pair per k3 configuration (ring slots and column blocks follow the width),
    # with and without `wide`; a one-row, a few-row and a tall map
    for cfg, (cin, cout) in T.K3_REPRESENTATIVE.items():
        s = 2 if cfg >= 6 else 1
        for OH in (1, 2, 4, 7, 33, 250):
            for OW in range(4, 1200):
                H, W = (OH, OW) if s == 1 else (2 * OH - 1, 2 * OW - 1)
                for wide in (0, 1):
                    p = visit(1, H, W, cin, cout, 3, s, T.K3, wide)
                    assert p is None or p.desc[0] == cfg
    for cin, cout in ((16, 16), (40, 40), (72, 72), (24, 56)):
        for OH in (1, 3, 16, 200):
            for OW in range(4, 1030, 3):
                visit(1, OH, OW, cin, cout, 3, 1, T.STREAM)
    # the dispatcher gives the stream kernel layers of 800 000 pixels and more only
    for B, H, W in BIG_MAPS:
        for k in (1, 3):
            for cin in range(8, 168, 8):
                for cout in range(8, 168, 8):
                    visit(B, H, W, cin, cout, k, 1, 0)
    return got


def test_the_table_has_one_case_per_reachable_key():
    sweep = _sweep()
    for kern in NAME:
        reach = sweep["forced"][kern] | sweep["dispatch"][kern]
        missing = sorted(reach - set(TABLE[kern]))
        assert not missing, "no table entry runs " + "; ".join(_name(kern, key) for key in missing)
        stale = sorted(set(TABLE[kern]) - reach)
        assert not stale, "the sweep no longer reaches " + "; ".join(_name(kern, key) for key in stale)
        assert sweep["dispatch"][kern] <= sweep["forced"][kern], (NAME[kern], "the dispatcher reaches a key the forced kernel does not")


def test_the_key_counts_match_the_hand_counts():
    sweep = _sweep()["forced"]
    k3 = {cfg: {(ns, cb) for c, ns, cb in sweep[T.K3] if c == cfg} for cfg in range(8)}
    for cfg in range(8):
        lost, new = sorted(T.K3_KEYS[cfg] - k3[cfg]), sorted(k3[cfg] - T.K3_KEYS[cfg])
        assert not lost and not new, f"k3 Cfg{T.K3_CFG_NAMES[cfg]}: (ring slots, column blocks) no longer reachable {lost}, newly reachable {new}"
    assert sum(len(v) for v in T.K3_KEYS.values()) == T.K3_COUNT == 38 == len(sweep[T.K3])
    s3, s1 = {key[1:] for key in sweep[T.STREAM] if key[0] == 3}, {key[1:] for key in sweep[T.STREAM] if key[0] == 1}
    assert s3 == T.STREAM_KEYS_3X3, (sorted(T.STREAM_KEYS_3X3 - s3), sorted(s3 - T.STREAM_KEYS_3X3))
    assert s1 == T.STREAM_KEYS_1X1, (sorted(T.STREAM_KEYS_1X1 - s1), sorted(s1 - T.STREAM_KEYS_1X1))
    assert len(s3) + len(s1) == T.STREAM_COUNT == 42 and len(s3) == 13 and len(s1) == 29
    assert len(sweep[T.HALO]) == T.HALO_COUNT == 16 and sweep[T.HALO] == {(a, b, 3 if a * b >= 8 else 9) for a in (1, 2, 4, 5) for b in (1, 2, 4, 5)}
    assert sweep[T.GEMM] == {(128, 128), (256, 256)} and T.GEMM_COUNT == 2
    assert sweep[T.GENERIC] == {(16, 192), (32, 128), (48, 128), (64, 64), (128, 128)} and T.GENERIC_COUNT == 5
    assert len(CASES) == 38 + 42 + 16 + 2 + 5


def test_every_compiled_instantiation_is_reachable():
    """8 k3 configurations, 14 stream (CO_T, JW) pairs (kCfgs / the CVX_WS_CASE list), 4 x 4 halo tiles, 2 + 5 tiles: none is compiled in
    vain.  The dispatcher alone reaches all of them but stream <5, 4> and the 1x1 wave layouts of more than 80 x 80 channels."""
    sweep = _sweep()
    assert {key[0] for key in sweep["forced"][T.K3]} == set(range(8)) == {key[0] for key in sweep["dispatch"][T.K3]}
    assert {(key[1], key[2]) for key in sweep["forced"][T.STREAM]} == T.STREAM_PAIRS and len(T.STREAM_PAIRS) == 14
    assert {(key[1], key[2]) for key in sweep["dispatch"][T.STREAM]} >= T.STREAM_PAIRS - {(5, 4)}
    assert sweep["dispatch"][T.HALO] == sweep["forced"][T.HALO] and sweep["dispatch"][T.GEMM] == sweep["forced"][T.GEMM]
    assert sweep["dispatch"][T.GENERIC] == sweep["forced"][T.GENERIC]
    # the stream kernel's three tap blocks, which the dispatcher reaches only where the k3 kernel, asked first, declines (40 -> 40: no k3 configuration)
    p = T.plan(20, 200, 200, 40, 40, 3, 1)
    assert p.kernel == T.STREAM and T.key_of(p, 3) == (3, 3, 3, 4, 1, 3)


def _kernel(B, H, W, cin, cout, k, s, kern=0, **kw):
    return NAME[T.plan(B, H, W, cin, cout, k, s, kern, **kw).kernel]


def _can(B, H, W, cin, cout, k, s, kern, **kw):
    return T.try_plan(B, H, W, cin, cout, k, s, kern, **kw) is not None


def test_the_thresholds_themselves():
    # k3's preference: Cin * Cout up to 256 * 144; one step above, the kernel still can
    assert _kernel(1, 40, 40, 256, 144, 3, 1) == "k3" and _kernel(1, 40, 40, 256, 152, 3, 1) == "gemm" and _kernel(1, 40, 40, 256, 192, 3, 1) == "gemm"
    assert _can(1, 40, 40, 256, 192, 3, 1, T.K3) and not _can(1, 40, 40, 256, 152, 3, 1, T.K3)      # 152 = 10 tiles: no configuration
    # stream's: 800 000 pixels and 80 x 80 channels (1x1: up to 80 output channels)
    assert _kernel(8, 250, 400, 32, 32, 1, 1) == "stream" and _kernel(8, 250, 399, 32, 32, 1, 1) == "generic"
    assert _kernel(8, 320, 320, 16, 16, 3, 1) == "stream" and _kernel(8, 320, 312, 16, 16, 3, 1) == "halo"       # (OH 320: the k3 kernel declines)
    assert _kernel(40, 320, 64, 80, 80, 3, 1) == "stream" and _kernel(40, 320, 64, 88, 80, 3, 1) == "halo" and _kernel(40, 320, 64, 64, 104, 3, 1) == "halo"
    assert _kernel(20, 200, 200, 40, 40, 3, 1) == "stream" and _kernel(20, 200, 199, 40, 40, 3, 1) == "halo"
    assert _kernel(8, 250, 400, 512, 80, 1, 1) == "stream" and _kernel(8, 250, 400, 88, 88, 1, 1) == "generic"
    assert _can(2, 5, 13, 512, 512, 1, 1, T.STREAM)
    # OH 250 / 251 (k3: 8-bit row tags); OW 3 / 4 (stream 3x3) and 5 / 6 (k3: the narrowest column block)
    assert _kernel(1, 250, 16, 16, 16, 3, 1) == "k3" and _kernel(1, 251, 16, 16, 16, 3, 1) == "halo" and not _can(1, 251, 16, 16, 16, 3, 1, T.K3)
    assert _can(2, 9, 4, 16, 16, 3, 1, T.STREAM) and not _can(2, 9, 3, 16, 16, 3, 1, T.STREAM) and not _can(2, 9, 1025, 16, 16, 3, 1, T.STREAM)
    assert _can(2, 9, 6, 16, 16, 3, 1, T.K3) and not _can(2, 9, 5, 16, 16, 3, 1, T.K3) and not _can(2, 9, 3, 16, 16, 3, 1, T.K3)
    # halo's: Cin * Cout up to 16383, Cin from 16
    assert _kernel(1, 251, 16, 144, 112, 3, 1) == "halo" and _kernel(1, 251, 16, 152, 112, 3, 1) == "generic" and _can(1, 251, 16, 512, 512, 3, 1, T.HALO)
    assert _kernel(1, 251, 16, 128, 120, 3, 1) == "halo" and _kernel(1, 251, 16, 128, 128, 3, 1) == "gemm"       # 16384, and Cout 128
    assert not _can(1, 251, 16, 8, 32, 3, 1, T.HALO) and _can(1, 251, 16, 16, 32, 3, 1, T.HALO)
    # gemm's: Cout 120 / 128, 256 weight columns, maps of 8 x 4, dy dense over the images
    assert _kernel(1, 251, 16, 256, 120, 3, 1) == "generic" and _kernel(1, 251, 16, 256, 128, 3, 1) == "gemm"
    assert _kernel(1, 20, 20, 240, 128, 1, 1) == "generic" and _kernel(1, 20, 20, 248, 128, 1, 1) == "gemm"     # 248 pads to 256 columns
    assert _can(2, 4, 8, 64, 128, 3, 1, T.GEMM) and not _can(2, 4, 7, 64, 128, 3, 1, T.GEMM) and not _can(2, 3, 8, 64, 128, 3, 1, T.GEMM)
    assert _can(2, 9, 13, 8, 8, 1, 1, T.GEMM) and not _can(2, 9, 13, 64, 128, 3, 1, T.GEMM, dy_ld=168)
    assert _kernel(2, 9, 13, 64, 128, 3, 1, x_ld=88, dy_ld=168) == "k3"
    # the five tile rules of cvx_conv_wgrad_tile
    tile = lambda cin, cout, k=3: T.key_of(T.plan(2, 9, 13, cin, cout, k, 1, T.GENERIC), k)  # noqa: E731
    assert tile(16, 16) == (16, 192) and tile(16, 24) == (32, 128) and tile(16, 32) == (32, 128) and tile(16, 40) == (48, 128)
    assert tile(16, 96) == (48, 128) and tile(16, 144) == (48, 128) and tile(16, 64) == (64, 64) and tile(16, 112) == (64, 64) and tile(16, 192) == (64, 64)
    assert tile(456, 128) == (128, 128) and tile(448, 128) == (64, 64)            # 128 * 9 * 464 = 534 528 >= 512 K > 128 * 9 * 448
    assert tile(120, 512) == (128, 128) and tile(104, 512) == (64, 64) and tile(512, 256, 1) == (64, 64)      # 512 * 9 * 128 = 589 824, 512 * 9 * 112 = 516 096
    assert T.key_of(T.plan(2, 9, 13, 64, 256, 3, 1, T.GEMM), 3) == (256, 256) and T.key_of(T.plan(2, 9, 13, 48, 256, 3, 1, T.GEMM), 3) == (128, 128)
    assert T.key_of(T.plan(2, 9, 13, 64, 384, 3, 1, T.GEMM), 3) == (128, 128)


def test_a_callers_split_count_stands():
    """nsplit > 0 is reported back whatever the units, and the chunk ranges follow it"""
    for c in CASES:
        for ns in (1, 3, 13, 200):
            p = T.case_plan(c, nsplit=ns)
            assert p.nsplit == ns and p.slab_bytes == ns * c.cout * c.k * c.k * ((c.cin + 15) // 16 * 16) * 4
            if c.kernel == T.K3:
                assert p.desc[7] == (p.desc[6] + ns - 1) // ns
            if c.kernel == T.STREAM:
                assert p.desc[8] == (p.desc[7] + ns - 1) // ns
    with pytest.raises(L.CvxError):
        T.plan(2, 9, 13, 16, 16, 3, 1, 6)
    with pytest.raises(L.CvxError):
        T.plan(2, 9, 13, 12, 16, 3, 1, 0)
    with pytest.raises(L.CvxError):
        T.plan(2, 9, 13, 16, 16, 3, 1, 0, x_ld=8)


# ---- the dispatcher has not changed --------------------------------------------------------------------------------------------------------
# what cvx_conv_wgrad_launch takes for CONV_CASES of tests/test_gpu_parity.py, in their order
CONV_CASES_KERNELS = ["k3", "generic", "k3", "k3", "generic", "gemm", "k3", "generic", "halo", "generic", "halo", "k3", "k3", "k3", "generic", "gemm",
                      "gemm", "gemm", "gemm", "gemm", "gemm"]


def _params(fn):
    return [m.args[1] for m in fn.pytestmark if m.name == "parametrize"][0]


def test_the_cases_of_the_parity_tests_take_the_kernels_they_were_written_for():
    import test_gpu_parity as P
    got = [_kernel(B, H, W, ci, co, k, s) for B, H, W, ci, co, k, s in P.CONV_CASES]
    assert got == CONV_CASES_KERNELS, [(c, g, w) for c, g, w in zip(P.CONV_CASES, got, CONV_CASES_KERNELS) if g != w]
    # "the shapes the two round-5 kernels take": k3 for the 3x3 layers, stream for the 1x1 layers of 800 000+ pixels
    for B, H, W, ci, co, k in P.WGRAD_R05_CASES:
        assert _kernel(B, H, W, ci, co, k, 1) == ("k3" if k == 3 else "stream"), (B, H, W, ci, co, k)
    # the stride-2 list is the k3 kernel's -- but for its 8 x 8 case ("maps smaller than one chunk"): an output map 4 wide is below the narrowest
    # column block, the generic kernel has always run it.  tests/conv_wgrad_cases.py runs the phase planes on a 6-wide output instead.
    for B, H, W, ci, co in _params(P.test_stride2_weight_gradient_in_phase_planes):
        assert _kernel(B, H, W, ci, co, 3, 2) == ("k3" if (W - 1) // 2 + 1 >= 6 else "generic"), (B, H, W, ci, co)
    # the gemm edges are the gemm kernel's -- but for the 8 x 8 map with 256 -> 128 channels: 256 * 128 is inside the k3 kernel's preference,
    # which is asked first.  tests/test_conv_wgrad_gpu.py runs that shape on the gemm kernel directly.
    edges = _params(P.test_gemm_shaped_weight_gradient_edges)
    for B, H, W, ci, co, k, s in edges:
        assert _kernel(B, H, W, ci, co, k, s) == ("k3" if (ci, co, k, s) == (256, 128, 3, 1) else "gemm"), (B, H, W, ci, co, k, s)
        assert _can(B, H, W, ci, co, k, s, T.GEMM)
    assert {T.key_of(T.plan(B, H, W, ci, co, k, s, T.GEMM), k) for B, H, W, ci, co, k, s in edges} == {(128, 128), (256, 256)}


@functools.lru_cache(maxsize=None)
def _model_layers():
    """(model, op name, B, ih, iw, cin, cout, k, stride, dil, x_ld, dy_ld) of every convolution the engine computes a weight gradient for
    with these kernels, at the benchmark's shapes; the pitches are those of the graph's buffers"""
    from computervision.pytorch_amd import deeplab, dla, graph, ssd, yolov7
    from computervision.pytorch_amd.model import Yolo8
    graphs = {
        "deeplab": (16, deeplab.build_deeplab_graph(deeplab.DeepLabLayout(21), 513, 513)),
        "dla": (16, dla.build_dla_graph(dla.DlaLayout(20), 384, 384)),
        "yolov7": (32, yolov7.build_yolov7_graph(yolov7.Yolo7Layout(20), 640, 640)),
        "ssd": (32, ssd.build_ssd_graph(ssd.SsdLayout(20), 300, 300)),
        "yolov8": (32, graph.build_yolov8_graph(Yolo8("n", 80).layout, 640, 640)),
    }
    out = []
    for name, (B, g) in graphs.items():
        for o in g.ops:
            if o["type"] != L.OP_CONV:
                continue
            k, s, pad, dil = o.get("k", 1), o.get("stride", 1), o.get("pad", 0), o.get("dil", 1)
            if o.get("w_cin", 0) == 3 and k == 3 and s == 2:      # the fp32 stem has a weight gradient of its own (stem.hip)
                continue
            if pad != dil * (k // 2):
                continue
            buf, _, cin, _ = o["in"]
            x_ld = g.bufs[buf][2]
            cout = o["out"][2]
            dy_ld = g.bufs[g.pred_buf][2] if o.get("act", 0) == L.ACT_BIAS and g.pred_buf >= 0 else cout
            out.append((name, o.get("name", "?"), B, o["ih"], o["iw"], cin, cout, k, s, dil, x_ld, dy_ld))
    return out


def test_every_layer_of_the_five_models_runs_a_key_the_table_runs():
    layers = _model_layers()
    assert {layer[0] for layer in layers} == {"deeplab", "dla", "yolov7", "ssd", "yolov8"} and len(layers) > 300
    seen = {kern: set() for kern in NAME}
    for name, op, B, ih, iw, cin, cout, k, s, dil, x_ld, dy_ld in layers:
        for wide in (0, 1):
            p = T.plan(B, ih, iw, cin, cout, k, s, 0, 0, wide, dil, x_ld, dy_ld)
            key = T.key_of(p, k)
            assert key in TABLE[p.kernel], f"{name} {op}: {_name(p.kernel, key)} has no case in the table"
            seen[p.kernel].add(key)
            OH, OW = T.out_size(ih, k, s, dil), T.out_size(iw, k, s, dil)
            _check_engine_count(p, k, cin, cout, T.units_of(p, B, OH, OW), (name, op, wide))
    assert all(seen.values()), "a kernel takes no layer of any model"


# ---- the condition of the GPU test's bound -------------------------------------------------------------------------------------------------
def test_the_fp32_gradient_of_the_cpu_is_well_inside_the_bound_on_every_subset():
    """the inputs of tests/test_conv_wgrad_gpu.py: torch's fp32 weight gradient on the CPU stays under 1e-6 relative L2 against fp64 on the
    whole tensor and on every subset that test compares, each of at least 256 elements -- the 1e-5 bound there judges the kernels, not the
    conditioning of a subset"""
    worst = 0.0
    for (m, k, s, d), (cin, cout) in G._widest().items():
        x16, dy16, ref = G.make_operands(m, k, s, d, cin, cout)
        f32 = torch.nn.grad.conv2d_weight(x16.permute(0, 3, 1, 2).float(), (cout, cin, k, k), dy16.permute(0, 3, 1, 2).float(), s, d * (k // 2), d)
        f32 = f32.permute(0, 2, 3, 1).reshape(cout, k * k, cin)
        shapes = {(c.cin, c.cout) for c in CASES if (c.map, c.k, c.stride, c.dil) == (m, k, s, d)}
        shapes |= {(ci, co) for kern, ci, co, kk, ss, mm in T.STRIDED_CASES if (mm, kk, ss, 1) == (m, k, s, d)}
        for ci, co in shapes:
            for (sub, a), (_, b) in zip(G.subsets(f32[:co, :, :ci]), G.subsets(ref[:co, :, :ci])):
                assert b.numel() >= G.SUBSET_MIN, (m, k, s, ci, co, sub)
                e = G._rel(a, b)
                worst = max(worst, e)
                assert e < 1e-6, (m, k, s, d, ci, co, sub, e)
    print(f"[conv wgrad] fp32 CPU gradient against fp64: largest {worst:.3e} (condition 1e-6)")
