"""GPU (MI355X): every compiled instantiation of the two convolution kernels with LDS-resident weights against fp64 on the CPU --
csrc/conv_halo.hip (3x3 / stride 1: halo patch + weights in LDS, ~75 % of the MACs of the five models) and csrc/conv_pw.hip (1x1 / stride 1).

The halo launcher can select 56 instantiations (tile rows x channel tiles per workgroup x gathered channels x tile streams), the pointwise
launcher 51 (K-steps x channel tiles per workgroup); each has its own LDS geometry, counted vmcnt waits and pixel / channel tails.
tests/conv_resident_cases.py lists shapes that reach all of them (tests/test_conv_resident_plan_cpu.py holds the launchers to that list); here
every one of them runs, directly (``mode | 0x10000`` / ``mode | 0x20000``: the default dispatch gives many of these shapes to other kernels):

* forward, all four epilogues (plain fp16, folded BN + SiLU, bias -> fp32, raw fp32 + per-channel statistics from the replica slabs), on the
  smallest maps that still have every tail: 81 x 83 (8-row tiles: 81 = 10 * 8 + 1, 83 = 5 * 16 + 3), 41 x 43 (4 rows), 2 x 37 x 39 (2 rows;
  2886 pixels for the pointwise kernel: the last workgroup has waves without tiles);
* the persistent walk: both kernels size their grids for the whole chip, so on these maps a workgroup sees one tile.  With
  ``cvx_debug_conv_grid_div`` the grid shrinks to 2 .. 8 workgroups per channel block and every workgroup walks many tiles -- the patch double
  buffer, the first / has_next / next_valid wait counts, the second tile stream running out of tiles before the first (odd tile counts), the
  statistics carried in registers across tiles;
* the pointwise kernel on 15 pixels: one wave tile, three idle waves that still owe the barrier;
* the data gradient through ``cvx_conv2d_dgrad_nhwc``'s natural dispatch (mirrored tap table, transposed weights);
* the force bits refuse shapes outside their kernel without launching.

Operands are fp16-valued; the reference is torch's convolution (its input gradient for the data gradient) in fp64 ON THE CPU, the widest one
(176 filters / 80 dx channels, 3 images on the small maps) computed once per (map, gathered channels) and sliced.  Comparison, bounds and subsets
are those of tests/test_conv_dma_gpu.py, whose helpers are used as they are: 5e-4 relative L2 for fp16 outputs, 1e-5 for fp32 outputs,
statistics per channel (mean within 1e-5 of the channel's rms, mean square within 1e-5 relative), on the whole tensor AND on every image, the
one-pixel border frame, the last 256 pixels, the last 16-channel tile and that tile on the last pixels, each of at least SUBSET_MIN_ELEMS
elements; 64 guard elements of 7.0 behind every output must survive.

Measured on MI355X (pytest -s prints them), largest over all cases and subsets:
  halo forward, 56 configurations: fp16 plain 2.119e-04 (1x41x43 80->176, TH 4 / NT 3 x 4 blocks / HV 2, last channel tile, last pixels), fp16 BN + SiLU
                   2.290e-04 (2x37x39 80->36, TH 2, last channel tile, last pixels), fp32 bias 1.90e-07, fp32 raw 2.31e-07 (both 1x41x43 144->176), mean / rms
                   1.8e-08, mean square 5.9e-08
  halo walk: fp16 BN + SiLU 2.137e-04 (1x97x77 64->36, two streams, 4 workgroups x 65 tiles), fp32 raw 1.58e-07, mean / rms 9.8e-09, mean square 7.6e-08
  pointwise forward, 51 configurations: fp16 plain 2.127e-04 (64->64), fp16 BN + SiLU 2.181e-04 (72->36, last channel tile), fp32 bias 1.12e-07, fp32 raw
                   1.46e-07 (both 512->32), mean / rms 9.5e-09, mean square 3.5e-08
  pointwise walk: fp16 BN + SiLU 2.181e-04, fp32 raw 1.09e-07, mean / rms 8.3e-09, mean square 6.8e-08
  15 pixels: fp16 plain max abs 9.40e-04 (bound 3.00e-03), BN + SiLU 1.22e-03 (bound 4.51e-03), fp32 raw 5.2e-08, mean / rms 6.3e-08, mean square 1.7e-07
  data gradient: 2.149e-04 (3x3 2x41x43 dy 64 -> dx 16, last 256 pixels)

That the tests can fail was shown once with three scratch builds (outside the tree), each with one purely numerical change to a kernel:
  A. halo kernel, HV == 2: tile stream 1 skips the MFMAs of the last K-step.  26 tests failed at their first comparison, rel-L2 0.094 ... 0.234 on
     the whole tensor against 5e-4: all 11 two-stream table configurations of test_halo_every_configuration, the 4 two-stream cases of
     test_halo_persistent_walk, the 11 cases of test_halo_and_pw_data_gradient whose plan has two streams.  The other 136 passed, rightly: single-stream
     instantiations and the pointwise kernel do not contain the change.  (The skip has to test a wave-uniform value -- readfirstlane of the stream
     index.  Written on the plain per-thread value the compiler lowers the `if` to an EXEC mask without a branch when the block is short, and MFMA
     ignores EXEC: the instantiations with at most two MFMAs per K-step computed everything, and only 18 tests failed.)
  B. halo kernel: the second trip of a workgroup reads the other patch buffer.  10 tests failed, rel-L2 0.14 ... 0.75: all 7 cases of
     test_halo_persistent_walk, and the three cases whose undivided grid is already smaller than the tile count (1x81x83 with 4-row tiles in three
     channel blocks, 126 tiles on 85 workgroups: table entry cin 128 / TH 4 / NT 2 and the data gradients dy 128 / 144 -> dx 80).  The other 152 passed,
     rightly: there every workgroup has one tile per stream -- which is why the walk tests exist.
  C. pointwise kernel: the operand load guard reduced to ``s < kfull``, so a ragged last K-step reads zeros for valid channels.  29 tests failed,
     rel-L2 0.106 ... 1.0 (cin 24: no full step at all): the 23 table entries with a ragged cin, both walks, the 15-pixel case (max abs error 1.46
     against 3.0e-3) and the three 1x1 data gradients.  The 28 table entries whose cin fills every K-step passed, rightly, as did every halo test.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_resident_cases as T
import test_conv_dma_gpu as D          # _subsets, _localised, _guarded, _guard_ok, _stat_replicas, _rel: the method, as it is
from computervision.pytorch_amd import _lib as L

pytestmark = pytest.mark.gpu

TOL16, TOL32, SUBSET_MIN_ELEMS = D.TOL16, D.TOL32, D.SUBSET_MIN_ELEMS
HALO, PW = 0x10000, 0x20000     # cvx_conv2d_nhwc: run the halo / the pointwise kernel directly
ALL_EPILOGUES = ("plain", "silu", "bias", "stats")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _print_worst(title, worst):
    for kind, (e, bound, tag, sub) in sorted(worst.items()):
        print(f"[conv resident] {title}: {kind}: largest {e:.3e} (bound {bound:.1e}) at {tag} {sub}")


@functools.lru_cache(maxsize=None)
def _fwd_operands(B, H, W, cin, cout, k):
    """fp16-valued operands and the fp64 CPU convolution (stride 1, pad k // 2) of ALL cout filters on ALL B images -> device tensors
    (x NHWC fp16, w [cout][k][k][cin] fp16, conv NHWC fp64, scale, shift); computed once, never written"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 1000 + H * 7 + W + cin * 13 + cout + k)
    x16 = torch.randn(B, cin, H, W, generator=g).half()
    w16 = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).half()
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    conv = F.conv2d(x16.double(), w16.double(), None, 1, k // 2)   # CPU, fp64
    assert conv.dtype == torch.float64 and conv.device.type == "cpu"
    return (x16.permute(0, 2, 3, 1).contiguous().to(dev), w16.permute(0, 2, 3, 1).contiguous().to(dev),
            conv.permute(0, 2, 3, 1).contiguous().to(dev), sc.to(dev), sh.to(dev))


def _sliced(ops, B, cout):
    xd, wd, conv, sc, sh = ops
    return xd[:B], wd[:cout], conv[:B, :, :, :cout], sc[:cout].contiguous(), sh[:cout].contiguous()


def _halo_operands(H, W, cin, B, cout):
    return _sliced(_fwd_operands(T.REF_BATCH[(H, W)], H, W, cin, T.HALO_MAX_COUT, 3), B, cout)


def _pw_operands(cin, cout):
    B, H, W = T.PW_MAP
    return _sliced(_fwd_operands(B, H, W, cin, T.PW_MAX_COUT, 1), B, cout)


def _check_forward(dev, tag, force, k, xd, wd, conv, sc, sh, worst, epilogues=ALL_EPILOGUES):
    """the epilogues of one launch shape (mode | force; stride 1, pad k // 2) against conv (B, H, W, cout) fp64"""
    lib = L.load()
    st = L.stream_ptr(dev)
    B, H, W, cin = xd.shape
    cout = conv.shape[3]
    assert tuple(conv.shape) == (B, H, W, cout) and tuple(wd.shape) == (cout, k, k, cin) and xd.is_contiguous() and wd.is_contiguous()
    args = (L.ptr(xd), B, H, W, cin, L.ptr(wd), cout, k, 1, k // 2, 1)
    scd, shd = sc.double(), sh.double()

    out, guard = D._guarded((B, H, W, cout), torch.float16, dev)
    if "plain" in epilogues:
        L.check(lib.cvx_conv2d_nhwc(*args, force | 0, None, None, L.ptr(out), st), "plain")
        assert D._guard_ok(guard), (tag, "plain: guard cells overwritten")
        D._localised(tag, out, conv, TOL16, worst, "fp16 plain")
    if "silu" in epilogues:
        out.fill_(D.GUARD_VALUE)
        L.check(lib.cvx_conv2d_nhwc(*args, force | 1, L.ptr(sc), L.ptr(sh), L.ptr(out), st), "affine")
        assert D._guard_ok(guard), (tag, "BN + SiLU: guard cells overwritten")
        v = conv * scd + shd
        D._localised(tag, out, v * torch.sigmoid(v), TOL16, worst, "fp16 BN + SiLU")
    out32, guard32 = D._guarded((B, H, W, cout), torch.float32, dev)
    if "bias" in epilogues:
        L.check(lib.cvx_conv2d_nhwc(*args, force | 2, L.ptr(sh), None, L.ptr(out32), st), "bias")
        assert D._guard_ok(guard32), (tag, "bias: guard cells overwritten")
        D._localised(tag, out32, conv + shd, TOL32, worst, "fp32 bias")
    if "stats" in epilogues:
        out32.fill_(D.GUARD_VALUE)
        R = D._stat_replicas(cout)
        flat = torch.zeros(R * cout * 4 + D.GUARD, dtype=torch.int64, device=dev)  # [replica][channel][sum, sum of squares][coarse 2^-6, fine 2^-40]
        flat[R * cout * 4:] = 7
        L.check(lib.cvx_conv2d_nhwc(*args, force | 3, None, L.ptr(flat), L.ptr(out32), st), "stats")
        assert D._guard_ok(guard32) and D._guard_ok(flat[R * cout * 4:]), (tag, "stats: guard cells overwritten")
        D._localised(tag, out32, conv, TOL32, worst, "fp32 raw")
        tot = flat[:R * cout * 4].view(R, cout, 2, 2).sum(0).double()
        sums = (tot[..., 0] / 64.0 + tot[..., 1] / 2.0 ** 40) / (B * H * W)   # per channel: mean, mean square
        mean, msq = conv.mean((0, 1, 2)), (conv * conv).mean((0, 1, 2))
        e1 = ((sums[:, 0] - mean).abs() / msq.sqrt()).max(0)
        e2 = (sums[:, 1] / msq - 1).abs().max(0)
        for kind, e in (("stat mean / rms", e1), ("stat mean square", e2)):
            if float(e.values) > worst.get(kind, (0.0,))[0]:
                worst[kind] = (float(e.values), TOL32, tag, f"channel {int(e.indices)}")
            assert float(e.values) < TOL32, (tag, kind, int(e.indices), float(e.values))


HALO_CASES = list(T.HALO_TABLE.items())
PW_CASES = list(T.PW_TABLE.items())


@pytest.mark.parametrize("key,want", HALO_CASES, ids=[f"cin{k[0]}-TH{w[0]}-NT{w[1]}-HV{w[3]}" for k, w in HALO_CASES])
def test_halo_every_configuration(dev, key, want):
    """3x3 / stride 1 / pad 1 on 1x81x83 (a ragged last row tile and column tile of the 8-row family), 1 or 2 x 41x43 (4 rows), 2x37x39 (2
    rows); cout picks the channel tiles per workgroup: 36 leaves the last tile 4 channels wide, 144 / 176 give several channel blocks with a
    ragged last one.  Measured maxima: module docstring."""
    cin, B, (H, W), cout = key
    assert T.halo_plan(B, H, W, cin, cout) == want
    th, nt, gy, hv = want
    worst = {}
    try:
        _check_forward(dev, f"{B}x{H}x{W} {cin}->{cout} (TH {th}, NT {nt} x {gy}, HV {hv})", HALO, 3, *_halo_operands(H, W, cin, B, cout), worst)
    finally:
        _print_worst("halo", worst)


@pytest.mark.parametrize("key,want", PW_CASES, ids=[f"NS{w[0]}-NT{w[1]}-cin{k[0]}" for k, w in PW_CASES])
def test_pw_every_configuration(dev, key, want):
    """1x1 / stride 1 on 2x37x39 = 2886 pixels (91 wave tiles of 32 pixels, 181 of 16: the last workgroup has waves without tiles, the last
    wave tile a pixel tail); per K-step count one cin whose last K-step is ragged or absent and one that fills every step."""
    cin, cout = key
    B, H, W = T.PW_MAP
    assert T.pw_plan(B * H * W, cin, cout) == want and (B * H * W) % 16 != 0
    ns, nt, gy, mt = want
    worst = {}
    try:
        _check_forward(dev, f"{B}x{H}x{W} {cin}->{cout} (NS {ns}, NT {nt} x {gy}, MT {mt})", PW, 1, *_pw_operands(cin, cout), worst)
    finally:
        _print_worst("pointwise", worst)


def _with_grid_div(div, fn):
    lib = L.load()
    prev = lib.cvx_debug_conv_grid_div(div)
    assert prev == 1, prev
    try:
        fn()
    finally:
        assert lib.cvx_debug_conv_grid_div(1) == div


@pytest.mark.parametrize("cin,B,hw,cout,div", T.HALO_WALKS, ids=[f"cin{c}-{b}x{m[0]}x{m[1]}-cout{co}" for c, b, m, co, _ in T.HALO_WALKS])
def test_halo_persistent_walk(dev, cin, B, hw, cout, div):
    """2 .. 8 workgroups per channel block: every workgroup walks its tiles for at least three trips (both patch buffers, every wait count of
    the first / a middle / the last trip).  Two-stream cases: with an ODD tile count the last tile is stream 0's, so in one workgroup stream
    1 has no next tile while stream 0 has one -- it issues the dump patch to keep the per-wave DMA count of the counted waits, and skips
    its last trip's stores.  (1x81x83 has 66 tiles of 8 rows, no multiple of 2 * gx: workgroups with unequal trip counts; 1x97x77 has 65.)
    BN + SiLU, and the statistics -- the values carried in registers across tiles."""
    H, W = hw
    plan = T.halo_plan(B, H, W, cin, cout)
    th, nt, gy, hv = plan
    total = T.halo_tiles(B, H, W, th)
    gx = T.halo_grid_x(plan, cin, total, div)
    assert 2 <= gx <= 8 and total >= 3 * gx * hv, (plan, total, gx)
    if hv == 2:
        assert total % 2 == 1 or (total % (2 * gx) != 0 and hw == T.MAP_TH8), (total, gx)
    worst = {}
    try:
        _with_grid_div(div, lambda: _check_forward(dev, f"{B}x{H}x{W} {cin}->{cout} (TH {th}, NT {nt} x {gy}, HV {hv}), {gx} workgroups x {total} tiles",
                                                   HALO, 3, *_halo_operands(H, W, cin, B, cout), worst, epilogues=("silu", "stats")))
    finally:
        _print_worst("halo walk", worst)


@pytest.mark.parametrize("cin,cout,div", T.PW_WALKS, ids=[f"cin{c}-cout{co}" for c, co, _ in T.PW_WALKS])
def test_pw_persistent_walk(dev, cin, cout, div):
    """every wave takes at least 3 wave tiles: MT = 2 (cin 72, ragged third K-step) and MT = 1 (cin 264)"""
    B, H, W = T.PW_MAP
    plan = T.pw_plan(B * H * W, cin, cout)
    gx, n_wave_tiles = T.pw_grid_x(plan, B * H * W, div)
    assert gx >= 1 and n_wave_tiles >= 3 * 4 * gx, (plan, gx, n_wave_tiles)
    worst = {}
    try:
        _with_grid_div(div, lambda: _check_forward(dev, f"{B}x{H}x{W} {cin}->{cout} {plan}, {gx} workgroups x {n_wave_tiles} wave tiles", PW, 1,
                                                   *_pw_operands(cin, cout), worst, epilogues=("silu", "stats")))
    finally:
        _print_worst("pointwise walk", worst)


def test_pw_fewer_tiles_than_waves(dev):
    """1x3x5 = 15 pixels, 40 -> 36 channels: ONE wave tile, three waves without one that still owe the workgroup their weight pieces and the
    barrier.  Too small for the subsets: element-wise, one fp16 rounding as in test_depthwise_transposed_conv_fwd_bwd (max |got - want| <=
    1e-3 * max(1, max |want|)); fp32 outputs 1e-5 relative L2."""
    lib = L.load()
    st = L.stream_ptr(dev)
    B, H, W, cin, cout = 1, 3, 5, 40, 36
    assert T.pw_plan(B * H * W, cin, cout) == (2, 3, 1, 2) and T.pw_grid_x((2, 3, 1, 2), B * H * W, 1) == (1, 1)
    g = torch.Generator().manual_seed(35)
    x16 = torch.randn(B, cin, H, W, generator=g).half()
    w16 = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).half()
    sc, sh = (torch.rand(cout, generator=g) + 0.5).to(dev), torch.randn(cout, generator=g).to(dev)
    conv = F.conv2d(x16.double(), w16.double()).permute(0, 2, 3, 1).contiguous().to(dev)   # CPU, fp64
    xd, wd = x16.permute(0, 2, 3, 1).contiguous().to(dev), w16.permute(0, 2, 3, 1).contiguous().to(dev)
    args = (L.ptr(xd), B, H, W, cin, L.ptr(wd), cout, 1, 1, 0, 1)

    def close16(got, want, what):
        err, bound = float((got.double() - want).abs().max()), 1e-3 * max(1.0, float(want.abs().max()))
        print(f"[conv resident] 15 pixels: {what}: max abs error {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (what, err, bound)

    out, guard = D._guarded((B, H, W, cout), torch.float16, dev)
    L.check(lib.cvx_conv2d_nhwc(*args, PW | 0, None, None, L.ptr(out), st), "plain")
    assert D._guard_ok(guard)
    close16(out, conv, "fp16 plain")
    out.fill_(D.GUARD_VALUE)
    L.check(lib.cvx_conv2d_nhwc(*args, PW | 1, L.ptr(sc), L.ptr(sh), L.ptr(out), st), "affine")
    assert D._guard_ok(guard)
    v = conv * sc.double() + sh.double()
    close16(out, v * torch.sigmoid(v), "fp16 BN + SiLU")
    out32, guard32 = D._guarded((B, H, W, cout), torch.float32, dev)
    L.check(lib.cvx_conv2d_nhwc(*args, PW | 2, L.ptr(sh), None, L.ptr(out32), st), "bias")
    assert D._guard_ok(guard32) and D._rel(out32, conv + sh.double()) < TOL32, D._rel(out32, conv + sh.double())
    out32.fill_(D.GUARD_VALUE)
    R = D._stat_replicas(cout)
    flat = torch.zeros(R * cout * 4 + D.GUARD, dtype=torch.int64, device=dev)
    flat[R * cout * 4:] = 7
    L.check(lib.cvx_conv2d_nhwc(*args, PW | 3, None, L.ptr(flat), L.ptr(out32), st), "stats")
    assert D._guard_ok(guard32) and D._guard_ok(flat[R * cout * 4:]) and D._rel(out32, conv) < TOL32, D._rel(out32, conv)
    tot = flat[:R * cout * 4].view(R, cout, 2, 2).sum(0).double()
    sums = (tot[..., 0] / 64.0 + tot[..., 1] / 2.0 ** 40) / (B * H * W)
    mean, msq = conv.mean((0, 1, 2)), (conv * conv).mean((0, 1, 2))
    e1, e2 = float(((sums[:, 0] - mean).abs() / msq.sqrt()).max()), float((sums[:, 1] / msq - 1).abs().max())
    print(f"[conv resident] 15 pixels: fp32 raw {D._rel(out32, conv):.3e}, stat mean / rms {e1:.3e}, stat mean square {e2:.3e}")
    assert e1 < TOL32 and e2 < TOL32, (e1, e2)


# ---- data gradient, natural dispatch ---------------------------------------------------------------------------------------------------
DG_MAX_DX = 80


@functools.lru_cache(maxsize=None)
def _dgrad_operands(B, H, W, k, gathered, dxc):
    """dy, the weights and the fp64 CPU input gradient of a k x k / stride 1 / pad k // 2 convolution dxc -> gathered channels -> device tensors
    (dy NHWC fp16, w (gathered, dxc, k, k) fp16, dx NHWC fp64); computed once, never written"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 100 + H + W * 3 + gathered * 11 + k)
    dy16 = torch.randn(B, gathered, H, W, generator=g).half()
    w16 = (torch.randn(gathered, dxc, k, k, generator=g) / (gathered * k * k) ** 0.5).half()
    dx = torch.nn.grad.conv2d_input((B, dxc, H, W), w16.double(), dy16.double(), stride=1, padding=k // 2)   # autograd's formula, CPU, fp64
    assert dx.dtype == torch.float64 and dx.device.type == "cpu" and tuple(dx.shape) == (B, dxc, H, W)
    return dy16.permute(0, 2, 3, 1).contiguous().to(dev), w16.to(dev), dx.permute(0, 2, 3, 1).contiguous().to(dev)


def _check_dgrad(dev, tag, k, dyd, w16, want, worst):
    B, H, W, dxc = want.shape
    gathered = dyd.shape[3]
    wtd = w16[:, :dxc].permute(1, 2, 3, 0).contiguous()   # [dx channel][kh][kw][gathered]
    dx, guard = D._guarded((B, H, W, dxc), torch.float16, dev)
    L.check(L.load().cvx_conv2d_dgrad_nhwc(L.ptr(dyd), B, H, W, dxc, L.ptr(wtd), gathered, k, 1, k // 2, 1, L.ptr(dx), L.stream_ptr(dev)), "dgrad")
    assert D._guard_ok(guard), (tag, "guard cells overwritten")
    D._localised(tag, dx, want, TOL16, worst, "fp16 dx")


DG_CASES = ([(3, hw, gathered, dxc) for hw in (T.MAP_TH4, T.MAP_TH8) for gathered in T.HALO_CINS for dxc in (16, 36, 80)] +
            [(1, T.PW_MAP[1:], 40, 36), (1, T.PW_MAP[1:], 136, 80), (1, T.PW_MAP[1:], 264, 16)])   # k, map, gathered channels, dx channels
DG_PW_STEPS = {40: 2, 136: 6, 264: 12}    # gathered channels -> K-steps: three different NS, one of the MT = 1 family


@pytest.mark.parametrize("k,hw,gathered,dxc", DG_CASES, ids=[f"k{k}-{m[0]}x{m[1]}-dy{g}-dx{d}" for k, m, g, d in DG_CASES])
def test_halo_and_pw_data_gradient(dev, k, hw, gathered, dxc):
    """The data gradient of a k x k / stride 1 / pad k // 2 convolution is a convolution of dy with the mirrored tap table and transposed
    weights: gathered channels = the forward's cout, produced channels = the forward's cin.  cvx_conv2d_dgrad_nhwc has no mode argument;
    the launch reaches the halo / pointwise kernel through the dispatcher (cvx_conv_igemm_launch) because the two kernels asked before them
    decline: the row-band kernel takes 3x3 maps of at most 40 x 40 (cvx_conv_tile_supported: IW > max_w || IH > max_w -> false; these are
    41 x 43 and 81 x 83; a 1x1 has one tap, not nine), the GEMM-shaped kernel needs 96 or more produced channels unless K = taps * gathered
    >= 2304 (cvx_conv_gemm_supported: deep || Cout >= cmin; dx has 16, 36 or 80 channels, K is at most 1296).
    3x3: 1x41x43 and 1x81x83 (2 images on 41 x 43 with 16 dx channels: the border frame subset, see HALO_TABLE).  1x1: 2x37x39."""
    H, W = hw
    assert dxc < 96 and k * k * gathered < 2304 and dxc % 4 == 0 and gathered % 8 == 0
    if k == 3:
        B = Bref = 1
        if hw == T.MAP_TH4:
            B, Bref = (2 if dxc == 16 else 1), 2
        assert min(H, W) > 40
        plan = T.halo_plan(B, H, W, gathered, dxc)     # the kernel takes the shape (gathered in 16 .. 144); which instantiation: printed
        dyd, w16, dx = _dgrad_operands(Bref, H, W, 3, gathered, DG_MAX_DX)
    else:
        B = T.PW_MAP[0]
        plan = T.pw_plan(B * H * W, gathered, dxc)
        assert plan[0] == DG_PW_STEPS[gathered]
        dyd, w16, dx = _dgrad_operands(B, H, W, 1, gathered, dxc)
    worst = {}
    try:
        _check_dgrad(dev, f"{k}x{k} {B}x{H}x{W} dy {gathered} -> dx {dxc} plan {plan}", k, dyd[:B], w16, dx[:B, :, :, :dxc], worst)
    finally:
        _print_worst("data gradient", worst)


def _out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


REFUSED = [   # force bit, cin, cout, k, stride, pad, dilation, why
    (HALO, 48, 16, 3, 1, 1, 1, "48 gathered channels"), (HALO, 16, 16, 3, 2, 1, 1, "stride 2"), (HALO, 16, 16, 3, 1, 2, 2, "dilation 2"),
    (HALO, 16, 16, 1, 1, 0, 1, "a 1x1"), (PW, 32, 16, 3, 1, 1, 1, "a 3x3"), (PW, 520, 16, 1, 1, 0, 1, "520 gathered channels"),
]


@pytest.mark.parametrize("force,cin,cout,k,stride,pad,dil,why", REFUSED, ids=[f"{'halo' if r[0] == HALO else 'pw'}-{r[7].replace(' ', '-')}" for r in REFUSED])
def test_force_bits_refuse_foreign_shapes(dev, force, cin, cout, k, stride, pad, dil, why):
    """outside the forced kernel's conditions the call is an error and launches nothing: the 7.0-filled output stays as it is"""
    lib = L.load()
    B, H, W = 1, 12, 20
    oh, ow = _out_size(H, k, stride, pad, dil), _out_size(W, k, stride, pad, dil)
    xd = torch.ones(B, H, W, cin, dtype=torch.float16, device=dev)
    wd = torch.ones(cout, k, k, cin, dtype=torch.float16, device=dev)
    for mode in (0, 1, 2, 3):
        dtype = torch.float16 if mode < 2 else torch.float32
        out, guard = D._guarded((B, oh, ow, cout), dtype, dev)
        aux = torch.zeros(D._stat_replicas(cout) * cout * 4, dtype=torch.int64, device=dev)
        sc = torch.ones(cout, device=dev)
        rc = lib.cvx_conv2d_nhwc(L.ptr(xd), B, H, W, cin, L.ptr(wd), cout, k, stride, pad, dil, force | mode, L.ptr(sc), L.ptr(aux if mode == 3 else sc),
                                 L.ptr(out), L.stream_ptr(dev))
        torch.cuda.synchronize()
        assert rc != 0, (why, mode)
        assert bool((out == D.GUARD_VALUE).all()) and D._guard_ok(guard) and bool((aux == 0).all()), (why, mode, "the refused call wrote")
