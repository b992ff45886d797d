"""GPU (MI355X): every compiled tile configuration of the LDS-DMA ring convolution kernel (csrc/conv_igemm_dma.hip) against fp64 on the CPU.

The kernel of last resort has 18 tile configurations (128 / 64 rows x 1, 2, 3, 4, 5, 6, 8 channel tiles, 32 rows x 1 .. 4 channel pairs),
each with its own LDS geometry, number of DMA passes per K-step (the last one partial when rows + channels is no multiple of 64), statistics
slab and pixel / channel tails.  tests/conv_dma_cases.py lists shapes that reach all of them (tests/test_conv_dma_plan_cpu.py holds the
launcher to that list); here every one of them runs:

* forward, 3x3 / stride 2 / pad 1 on odd maps, run directly with ``mode | 0x8000``, all four epilogues (plain fp16, folded BN + SiLU,
  bias -> fp32, raw fp32 + per-channel statistics), plus two heavy-weight cases (256 -> 256 channels, one strided, one dilated);
* the merged-phase data gradient (blockIdx.z selects the phase, the grid is sized for the largest, the smaller ones return early) through
  ``cvx_conv2d_dgrad_nhwc``'s natural dispatch, on unequal phases (257x258, 257x257, 256x258, 256x257) into a dx pre-filled with 7.0.

Operands are fp16-valued; the reference is torch's convolution (its input gradient for the data gradient) in fp64 ON THE CPU, the widest
one (144 filters / 144 dx channels) computed once per input and sliced: filter n of a convolution and channel c of its input gradient do not
depend on how many others there are.  The 64-row cases run image 0 of the 128-row operands.  Only the element-wise epilogue formulas and
the norms of the comparisons are evaluated on the device, in fp64.

Bounds (tests/test_gpu_parity.py, header): 5e-4 relative L2 for fp16 outputs (one fp16 rounding), 1e-5 for fp32 outputs; statistics per
channel: the mean within 1e-5 of the channel's rms, the mean square within 1e-5 relative.  They hold on the whole tensor AND on every
subset below, each of at least SUBSET_MIN_ELEMS elements -- a wrong tail or channel tile disappears in the norm of 130 k pixels:
every image, the one-pixel border frame, the last 256 output pixels (of every phase, for the data gradient), the last 16-channel tile
(all pixels, and the last ceil(4096 / width) pixels).  64 guard elements of 7.0 behind every output must survive.

Measured on MI355X (pytest -s prints them), largest over all cases and subsets:
  forward 16 -> N: fp16 plain 2.120e-04 (1x257x259 16->36, last channel tile, last pixels), fp16 BN + SiLU 2.218e-04 (1x257x259 16->16, last
                   256 pixels), fp32 bias 7.46e-08, fp32 raw 8.17e-08, mean / rms 3.2e-09, mean square 8.6e-09
  heavy 256 -> 256: fp16 plain 2.106e-04, fp16 BN + SiLU 2.099e-04, fp32 bias 2.22e-07, fp32 raw 3.03e-07, mean / rms 1.1e-08, mean square 3.8e-08
  merged data gradient: 2.136e-04 (1x513x515 dx 80, last channel tile, last pixels), 2.089e-04 (2x33x35)

That the tests can fail was shown once with a scratch build (outside the tree) whose kernel skips the MFMAs of the last K-step in the
workgroups of the last blockIdx.x -- a purely numerical change.  All 11 data-gradient tests failed, at their first comparison:
test_merged_phase_data_gradient 1.50e-03 ... 1.71e-03 on the whole tensor (e.g. [128rows-dx80] 1.591e-03, [64rows-dx80] 1.713e-03 against
5e-4: the 4 / 2 pixels of phase (0, 0) past the last full tile come out as zero), test_merged_phase_data_gradient_on_a_small_map 3.26e-02.
The 32 forward tests passed under that change, and rightly: their last workgroup holds pixels of the last output row only, and for those
the last K-step is the bottom-right tap, which reads the padding row below the map -- skipping it changes nothing.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_dma_cases as T
from computervision.pytorch_amd import _lib as L

pytestmark = pytest.mark.gpu

TOL16, TOL32 = 5e-4, 1e-5   # fp16-storage outputs: one fp16 rounding; fp32 outputs and statistics
SUBSET_MIN_ELEMS = 4096     # as in test_gpu_parity.py: the relative L2 of fp16 rounding over n elements scatters by ~ 1 / sqrt(n)
GUARD, GUARD_VALUE = 64, 7.0
DMA = 0x8000                # cvx_conv2d_nhwc: run the ring kernel directly


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _rel(got, want):
    return float((got.double() - want).norm() / (want.norm() + 1e-30))


def _subsets(t, phases=None):
    """(name, elements) of a (B, h, w, C) tensor: see the module docstring.  phases: stride of the data gradient's output phases."""
    B, h, w, C = t.shape
    yield "whole tensor", t
    if B > 1:
        for b in range(B):
            yield f"image {b}", t[b]
    yield "border frame", torch.cat([t[:, 0].reshape(-1), t[:, -1].reshape(-1), t[:, 1:-1, 0].reshape(-1), t[:, 1:-1, -1].reshape(-1)])
    if phases is None:
        yield "last 256 pixels", t.reshape(-1, C)[-256:]
    else:
        for ph in range(phases):
            for pw in range(phases):
                yield f"last 256 pixels of phase ({ph}, {pw})", t[:, ph::phases, pw::phases].reshape(-1, C)[-256:]
    c0 = 16 * ((C - 1) // 16)
    yield "last channel tile", t[..., c0:]
    npix = (SUBSET_MIN_ELEMS + C - c0 - 1) // (C - c0)
    yield "last channel tile, last pixels", t.reshape(-1, C)[-npix:, c0:]


def _localised(tag, got, want, tol, worst, kind, phases=None):
    """rel-L2(got, want) < tol on the whole tensor and on every subset"""
    for (sub, g), (_, w) in zip(_subsets(got, phases), _subsets(want, phases)):
        assert w.numel() >= SUBSET_MIN_ELEMS, (tag, sub, w.numel())
        e = _rel(g, w)
        if e > worst.get(kind, (0.0,))[0]:
            worst[kind] = (e, tol, tag, sub)
        assert e < tol, (tag, kind, sub, e, tol)


def _print_worst(title, worst):
    for kind, (e, bound, tag, sub) in sorted(worst.items()):
        print(f"[conv dma] {title}: {kind}: largest {e:.3e} (bound {bound:.1e}) at {tag} {sub}")


def _guarded(shape, dtype, dev):
    """a tensor of `shape` filled with 7.0 with 64 guard elements of 7.0 behind it -> (view, guard)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + GUARD,), GUARD_VALUE if dtype.is_floating_point else 7, dtype=dtype, device=dev)
    return flat[:n].view(*shape), flat[n:]


def _guard_ok(guard):
    return bool((guard == 7).all())


def _stat_replicas(cout):   # cvx_stat_replicas (csrc/bn_act.h)
    return 16 if cout <= 32 else 8 if cout <= 64 else 4 if cout <= 128 else 2 if cout <= 256 else 1


_plan = T.launcher_plan


@functools.lru_cache(maxsize=None)
def _fwd_operands(B, H, W, cin, cout, k, stride, pad, dil):
    """fp16-valued operands and the fp64 CPU convolution of ALL cout filters -> device tensors (x NHWC fp16, w [cout][k][k][cin] fp16,
    conv NHWC fp64, scale, shift); computed once, never written"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 1000 + H + W + cin + cout + stride + dil)
    x16 = torch.randn(B, cin, H, W, generator=g).half()
    w16 = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).half()
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    conv = F.conv2d(x16.double(), w16.double(), None, stride, pad, dil)   # CPU, fp64
    assert conv.dtype == torch.float64 and conv.device.type == "cpu"
    return (x16.permute(0, 2, 3, 1).contiguous().to(dev), w16.permute(0, 2, 3, 1).contiguous().to(dev),
            conv.permute(0, 2, 3, 1).contiguous().to(dev), sc.to(dev), sh.to(dev))


def _check_forward(dev, tag, xd, wd, conv, sc, sh, k, stride, pad, dil, worst):
    """the four epilogues of one launch shape (mode | 0x8000) against conv (B, OH, OW, cout) fp64"""
    lib = L.load()
    st = L.stream_ptr(dev)
    B, H, W, cin = xd.shape
    _, OH, OW, cout = conv.shape
    args = (L.ptr(xd), B, H, W, cin, L.ptr(wd), cout, k, stride, pad, dil)
    scd, shd = sc.double(), sh.double()

    out, guard = _guarded((B, OH, OW, cout), torch.float16, dev)
    L.check(lib.cvx_conv2d_nhwc(*args, DMA | 0, None, None, L.ptr(out), st), "plain")
    assert _guard_ok(guard), (tag, "plain: guard cells overwritten")
    _localised(tag, out, conv, TOL16, worst, "fp16 plain")

    out.fill_(GUARD_VALUE)
    L.check(lib.cvx_conv2d_nhwc(*args, DMA | 1, L.ptr(sc), L.ptr(sh), L.ptr(out), st), "affine")
    assert _guard_ok(guard), (tag, "BN + SiLU: guard cells overwritten")
    v = conv * scd + shd
    _localised(tag, out, v * torch.sigmoid(v), TOL16, worst, "fp16 BN + SiLU")

    out32, guard32 = _guarded((B, OH, OW, cout), torch.float32, dev)
    L.check(lib.cvx_conv2d_nhwc(*args, DMA | 2, L.ptr(sh), None, L.ptr(out32), st), "bias")
    assert _guard_ok(guard32), (tag, "bias: guard cells overwritten")
    _localised(tag, out32, conv + shd, TOL32, worst, "fp32 bias")

    out32.fill_(GUARD_VALUE)
    R = _stat_replicas(cout)
    flat = torch.zeros(R * cout * 4 + GUARD, dtype=torch.int64, device=dev)  # [replica][channel][sum, sum of squares][coarse 2^-6, fine 2^-40]
    flat[R * cout * 4:] = 7
    L.check(lib.cvx_conv2d_nhwc(*args, DMA | 3, None, L.ptr(flat), L.ptr(out32), st), "stats")
    assert _guard_ok(guard32) and _guard_ok(flat[R * cout * 4:]), (tag, "stats: guard cells overwritten")
    _localised(tag, out32, conv, TOL32, worst, "fp32 raw")
    tot = flat[:R * cout * 4].view(R, cout, 2, 2).sum(0).double()
    sums = (tot[..., 0] / 64.0 + tot[..., 1] / 2.0 ** 40) / (B * OH * OW)   # per channel: mean, mean square
    mean, msq = conv.mean((0, 1, 2)), (conv * conv).mean((0, 1, 2))
    e1 = ((sums[:, 0] - mean).abs() / msq.sqrt()).max(0)
    e2 = (sums[:, 1] / msq - 1).abs().max(0)
    for kind, e in (("stat mean / rms", e1), ("stat mean square", e2)):
        if float(e.values) > worst.get(kind, (0.0,))[0]:
            worst[kind] = (float(e.values), TOL32, tag, f"channel {int(e.indices)}")
        assert float(e.values) < TOL32, (tag, kind, int(e.indices), float(e.values))


FWD_CASES = [(rows, cout) for rows in T.FWD_INPUTS for cout in T.FWD_COUTS]


@pytest.mark.parametrize("rows,cout", FWD_CASES, ids=[f"{r}rows-cout{c}" for r, c in FWD_CASES])
def test_forward_every_tile_configuration_all_epilogues(dev, rows, cout):
    """3x3 / stride 2 / pad 1, 16 -> cout channels on 2x513x515 (128-row tiles), 1x513x515 (64) and 1x257x259 (32): with cout = 16 ... 144 every
    channel-tile count of the family, 36 with a last tile 4 channels wide, 112 with 7 real tiles of 8, 144 in two channel blocks with the second
    ragged; 4 (128 rows) or 2 pixel rows past the last full tile.  Measured maxima: module docstring."""
    B, H, W = T.FWD_INPUTS[rows]
    OH, OW = T.out_size(H, 3, 2, 1, 1), T.out_size(W, 3, 2, 1, 1)
    nt, gy = (T.TILES_32 if rows == 32 else T.TILES_BIG)[cout]
    assert _plan(B * OH * OW, T.FWD_CIN, cout, 9)[:3] == (rows, nt, gy) and (B * OH * OW) % rows in (2, 4)
    big = rows != 32   # the 64-row case is image 0 of the 128-row operands
    xd, wd, conv, sc, sh = _fwd_operands(2 if big else B, H, W, T.FWD_CIN, T.FWD_MAX_COUT, 3, 2, 1, 1)
    worst = {}
    try:
        _check_forward(dev, f"{B}x{H}x{W} 16->{cout} ({rows} rows, {nt} tiles x {gy})", xd[:B], wd[:cout], conv[:B, :, :, :cout], sc[:cout].contiguous(),
                       sh[:cout].contiguous(), 3, 2, 1, 1, worst)
    finally:
        _print_worst("forward", worst)


@pytest.mark.parametrize("B,H,W,ci,co,k,s,pad,dil", T.HEAVY_CASES)
def test_forward_heavy_weights_take_64_row_tiles(dev, B, H, W, ci, co, k, s, pad, dil):
    """256 -> 256 channels at 8580 pixels: 9 * 256 * 256 weight elements move the launch from 32-row to 64-row tiles (8 channel tiles, two
    channel blocks, 72 K-steps) -- a stride-2 layer and a dilated one (DeepLabv3+'s ASPP pattern).  Measured maxima: module docstring."""
    OH, OW = T.out_size(H, k, s, pad, dil), T.out_size(W, k, s, pad, dil)
    assert B * OH * OW == 8580 and _plan(B * OH * OW, ci, co, k * k) == (64, 8, 2, 3)
    xd, wd, conv, sc, sh = _fwd_operands(B, H, W, ci, co, k, s, pad, dil)
    worst = {}
    try:
        _check_forward(dev, f"{B}x{H}x{W} {ci}->{co} k{k} s{s} d{dil}", xd, wd, conv, sc, sh, k, s, pad, dil, worst)
    finally:
        _print_worst("heavy", worst)


@functools.lru_cache(maxsize=None)
def _dgrad_operands(B, H, W, cin, cout):
    """dy, the weights and the fp64 CPU input gradient of a 3x3 / stride 2 / pad 1 convolution with ALL cin input channels -> device tensors
    (dy NHWC fp16, w (cout, cin, 3, 3) fp16, dx NHWC fp64); computed once, never written"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 100 + H + W + cin)
    OH, OW = T.out_size(H, 3, 2, 1, 1), T.out_size(W, 3, 2, 1, 1)
    dy16 = torch.randn(B, cout, OH, OW, generator=g).half()
    w16 = (torch.randn(cout, cin, 3, 3, generator=g) / (cout * 9 / 4) ** 0.5).half()   # 9 / 4 taps reach a pixel on average
    dx = torch.nn.grad.conv2d_input((B, cin, H, W), w16.double(), dy16.double(), stride=2, padding=1)   # autograd's formula, CPU, fp64
    assert dx.dtype == torch.float64 and dx.device.type == "cpu" and tuple(dx.shape) == (B, cin, H, W)
    return dy16.permute(0, 2, 3, 1).contiguous().to(dev), w16.to(dev), dx.permute(0, 2, 3, 1).contiguous().to(dev)


def _check_dgrad(dev, tag, dyd, w16, want, worst):
    B, H, W, cin = want.shape
    cout = dyd.shape[3]
    wtd = w16[:, :cin].permute(1, 2, 3, 0).contiguous()   # [cin][kh][kw][cout]
    dx, guard = _guarded((B, H, W, cin), torch.float16, dev)   # 7.0 everywhere: every pixel of every phase must be written
    L.check(L.load().cvx_conv2d_dgrad_nhwc(L.ptr(dyd), B, H, W, cin, L.ptr(wtd), cout, 3, 2, 1, 1, L.ptr(dx), L.stream_ptr(dev)), "dgrad")
    assert _guard_ok(guard), (tag, "guard cells overwritten")
    _localised(tag, dx, want, TOL16, worst, "fp16 dx", phases=2)


DG_CASES = [(rows, cin) for rows in T.DG_BATCHES for cin in T.DG_CINS]


@pytest.mark.parametrize("rows,cin", DG_CASES, ids=[f"{r}rows-dx{c}" for r, c in DG_CASES])
def test_merged_phase_data_gradient(dev, rows, cin):
    """The data gradient of 3x3 / stride 2 / pad 1, cin -> 16 channels on 513x515 as ONE launch over its four unequal phases (257x258, 257x257,
    256x258, 256x257; 1, 2, 2 and 4 taps): B = 2 runs 128-row tiles, B = 1 (image 0 of the same operands) 64-row tiles; dx channels 16, 48,
    80, 128, 144 = 1, 3, 5, 8 channel tiles and 5 in two blocks.  The odd map keeps it off the pixel-shuffle GEMM, the narrow dx off the
    GEMM-shaped kernel.  Measured maxima: module docstring."""
    H, W = T.DG_MAP
    B = T.DG_BATCHES[rows]
    nt, gy = T.TILES_BIG[cin]
    assert _plan(B * 257 * 258, T.DG_COUT_FWD, cin, T.DG_TAPS_PHASE0)[:3] == (rows, nt, gy)
    dyd, w16, dx = _dgrad_operands(2, H, W, T.DG_MAX_CIN, T.DG_COUT_FWD)
    worst = {}
    try:
        _check_dgrad(dev, f"{B}x{H}x{W} dx {cin} ({rows} rows, {nt} tiles x {gy})", dyd[:B], w16, dx[:B, :, :, :cin], worst)
    finally:
        _print_worst("merged data gradient", worst)


def test_merged_phase_data_gradient_on_a_small_map(dev):
    """the same geometry on 2x33x35, 144 dx channels: phases of 612, 578, 576 and 544 pixels in the 32-row family (3 channel pairs, two channel
    blocks) -- a 4-pixel and a 2-pixel tail, and two phases whose last workgroups of the grid return early"""
    B, H, W, cin = T.DG_SMALL
    assert _plan(B * 17 * 18, T.DG_COUT_FWD, cin, T.DG_TAPS_PHASE0)[:3] == (32, 3, 2)
    dyd, w16, dx = _dgrad_operands(B, H, W, cin, T.DG_COUT_FWD)
    worst = {}
    try:
        _check_dgrad(dev, f"{B}x{H}x{W} dx {cin} (32 rows)", dyd, w16, dx, worst)
    finally:
        _print_worst("merged data gradient, small map", worst)
