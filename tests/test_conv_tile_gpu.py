"""GPU (MI355X): every reachable instantiation and weight regime of the row-band convolution kernel (csrc/conv_tile.hip,
conv_tile_kernel.inc.h, conv_tile_k1 / k2.hip) against fp64 on the CPU.

The kernel the dispatcher asks first for 3x3 / stride 1 on maps of at most 40 x 40 has 24 reachable <MT, NTW> instantiations, each with a
compile-time lgkmcnt(MT + NTW) and inline-asm fragment reads, and three run-time weight regimes (one chunk, ring of 3, ring of 4) with counted
vmcnt waits, an XOR swizzle of four classes, magic-number divisions, a pack kernel and a staged epilogue whose lane map depends on the
channel block.  tests/conv_tile_cases.py lists a forced case for each of the 68 reachable (MT, NTW, regime) triples and four the force adds
(tests/test_conv_tile_plan_cpu.py holds the launcher to that list); here every one of them runs:

* forward through ``cvx_conv2d_nhwc(mode | 0x2000)`` under ``cvx_debug_conv_tile_force(TR, NTW)``, all four epilogues (plain fp16, folded
  BN + SiLU, bias -> fp32, raw fp32 + per-channel statistics), on 3x37x39 (W = 39 never fills a pixel group, short last bands, tile counts
  that are no multiple of 8) and 5x13x17 (cin 256 / 512); output channels leave the last 16-channel tile 8 wide and, with two channel
  blocks, the last block ragged;
* the data gradient through ``cvx_conv2d_dgrad_nhwc``'s natural dispatch (mirrored tap table: the pack kernel's wt_pack, the kernel's set_tap),
  free and with one forced case per MT;
* the extremes of the map: 4 pixels, a row of 512 pixels, 3 x 50, a last band of one row;
* the packed-weight buffer of stand-alone launches: one weight pointer under two NTW, weights changed in place;
* ``mode | 0x2000`` refuses shapes outside the kernel, and a forced pair without a plan, without launching.

Operands are fp16-valued; the reference is torch's convolution (its input gradient for the data gradient) in fp64 ON THE CPU, the widest one
computed once per (map, gathered channels) and sliced.  Comparison, bounds and subsets are those of tests/test_conv_dma_gpu.py, whose helpers
are used as they are (the forward and data-gradient drivers are those of tests/test_conv_resident_gpu.py): 5e-4 relative L2 for fp16 outputs,
1e-5 for fp32 outputs, statistics per channel (mean within 1e-5 of the channel's rms, mean square within 1e-5 relative), on the whole tensor
AND on every image, the one-pixel border frame, the last 256 pixels, the last 16-channel tile and that tile on the last pixels, each of at
least SUBSET_MIN_ELEMS elements; 64 guard elements of 7.0 behind every output must survive.  Cases too small for the subsets compare
element-wise as test_pw_fewer_tiles_than_waves does.

Measured on MI355X (pytest -s prints them), largest over all cases and subsets:
  forward, 72 forced cases: fp16 plain 2.166e-04 (3x37x39 128->200, MT 1 / NTW 9 x 2 / ring of 3, last channel tile, last pixels), fp16 BN + SiLU
                   2.204e-04 (3x37x39 128->56, MT 1 / NTW 4 / ring of 4, last channel tile, last pixels), fp32 bias 3.04e-07, fp32 raw 4.29e-07 (both
                   5x13x17, cin 512), mean / rms 3.8e-08, mean square 1.0e-07
  data gradient: 2.126e-04 (3x37x39 dy 64 -> dx 80, last channel tile, last pixels)
  1x2x512: fp16 plain 2.084e-04, fp16 BN + SiLU 2.116e-04, fp32 bias 6.6e-08, fp32 raw 9.2e-08, mean / rms 1.1e-08, mean square 8.8e-08
  element-wise cases: fp16 plain max abs 8.15e-04 (1x2x2, bound 2.13e-03) ... 9.75e-04 (2x5x23, bound 3.60e-03), BN + SiLU 7.12e-04 ... 1.65e-03 (bound
                   5.72e-03), fp32 bias <= 1.1e-07, fp32 raw <= 1.6e-07, mean / rms <= 1.3e-07, mean square <= 2.8e-07 (1x2x2: 4 pixels per channel)
  packed-weight buffer: 2.093e-04
No kernel fault was found: all 101 tests passed on the unchanged kernel.

That the tests can fail was shown once with three scratch builds (outside the tree), each with one purely numerical change to the kernel:
  A. the ring refill goes to the slot the load cursor is in, not to the retired one.  49 tests failed, rel-L2 1.1 ... 8.7 on the whole tensor
     against 5e-4: all 48 ring cases of test_tile_every_configuration (24 instantiations x ring of 3 / ring of 4) and
     test_tile_data_gradient[dy144-dx40-TR1], whose forced one-row plan streams its weights (NTW 3, chunks of 5).  The other 52 passed, rightly:
     the 24 one-chunk cases, the free data gradients (one chunk each), the extremes and the packed-weight test never refill a slot.
  B. the fragment address of pixel group 2 takes the column offset of the wrong tap (S0[2] = S1[2]).  33 tests failed, rel-L2 0.40 ... 0.46: the
     30 table cases with MT 3 or 4, the data gradients forced to TR 7 and TR 10, and the 512-pixel row (MT 4).  The other 68 passed, rightly: a
     wave with one or two pixel groups has no group 2.
  C. the staged epilogue reads row 4 in place of row 5 where BN / 8 does not divide 64.  38 tests failed, rel-L2 0.18 ... 0.40 (2x5x23: max
     abs error 5.23 against 3.6e-3), at the plain fp16 epilogue: the 36 forced cases with NTW 3, 5, 6 or 9 at every MT, the data gradient forced to
     TR 1 (NTW 3) and 2x5x23 (NTW 3).  The other 63 passed, rightly: NTW 1, 2 and 4 have 2, 4 and 8 lanes per row, which divide 64.
"""
import pytest
import torch

import conv_tile_cases as T
import test_conv_dma_gpu as D          # _subsets, _localised, _guarded, _guard_ok, _stat_replicas, _rel: the method, as it is
import test_conv_resident_gpu as RS    # _fwd_operands, _sliced, _check_forward, _dgrad_operands, _check_dgrad: stride-1 drivers on that method
from computervision.pytorch_amd import _lib as L

pytestmark = pytest.mark.gpu

TOL16, TOL32, SUBSET_MIN_ELEMS = D.TOL16, D.TOL32, D.SUBSET_MIN_ELEMS
TILE = 0x2000                   # cvx_conv2d_nhwc: run the row-band kernel directly
ALL_CASES = list(T.TABLE.items()) + list(T.FORCED_ONLY.items())
# widest cout of any case per (map, cin): one fp64 reference each
REF_COUT = {}
for (_cin, _B, _hw, _cout, _tr, _ntw) in list(T.TABLE) + list(T.FORCED_ONLY):
    REF_COUT[(_hw, _cin)] = max(REF_COUT.get((_hw, _cin), 0), _cout)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _print_worst(title, worst):
    for kind, (e, bound, tag, sub) in sorted(worst.items()):
        print(f"[conv tile] {title}: {kind}: largest {e:.3e} (bound {bound:.1e}) at {tag} {sub}")


def _operands(hw, cin, B, cout):
    H, W = hw
    return RS._sliced(RS._fwd_operands(T.REF_BATCH[hw], H, W, cin, REF_COUT[(hw, cin)], 3), B, cout)


@pytest.mark.parametrize("key,want", ALL_CASES, ids=[f"MT{w[0]}-NTW{w[1]}-R{w[5]}-cin{k[0]}-TR{k[4]}" for k, w in ALL_CASES])
def test_tile_every_configuration(dev, key, want):
    """3x3 / stride 1 / pad 1 under the forced (TR, NTW) of the case: the plan functions return the tuple the table states, then the four
    epilogues run through mode | 0x2000.  Measured maxima: module docstring."""
    cin, B, hw, cout, tr, ntw = key
    H, W = hw
    worst = {}
    try:
        with T.forced(tr, ntw):
            assert T.launch_key(B, H, W, cin, cout) == want and T.tile_plan(B, H, W, cin, cout)[0] == tr
            mt, _, nb, ksc, nch, R = want
            RS._check_forward(dev, f"{B}x{H}x{W} {cin}->{cout} (TR {tr}: MT {mt}, NTW {ntw} x {nb}, {nch} chunks of {ksc}, R {R})", TILE, 3,
                              *_operands(hw, cin, B, cout), worst)
    finally:
        _print_worst("forward", worst)


# ---- data gradient, natural dispatch ---------------------------------------------------------------------------------------------------
DG_CASES = [(dy, dxc, 0, 0) for dy in T.DG_GATHERED for dxc in T.DG_DX] + list(T.DG_FORCED)


@pytest.mark.parametrize("gathered,dxc,tr,ntw", DG_CASES, ids=[f"dy{g}-dx{d}" + (f"-TR{t}" if t else "") for g, d, t, _ in DG_CASES])
def test_tile_data_gradient(dev, gathered, dxc, tr, ntw):
    """The data gradient of a 3x3 / stride 1 / pad 1 convolution is a convolution of dy with the mirrored tap table and transposed weights:
    gathered channels = the forward's cout, produced channels = the forward's cin; dx is pre-filled with 7.0.  cvx_conv2d_dgrad_nhwc has no
    mode argument; the launch is the row-band kernel because of cvx_conv_igemm_launch's order: a stride-1 gradient has one phase and no
    pixel-shuffle store (the two early returns), the 7x7 / first-layer kernel wants 8 gathered channels (cvx_conv_stem7_supported: Cin == 8;
    these have 32 or more), and cvx_conv_tile_supported is asked next, before every other kernel.  It says yes: the map is at most 40 x 40
    (IW > max_w || IH > max_w -> false: 37 x 39), the gathered channels at most 144 (Cin > max_c -> false), and cvx_conv_tile_shape_ok holds --
    nine taps of a 3x3 neighbourhood on an output as large as the input, gathered % 8 == 0 and >= 32, produced % 8 == 0, and a plan exists
    (cvx_debug_conv_tile_plan asks the same function).  Under a force the same holds with the forced plan: one case per MT."""
    H, W = T.MAIN
    B = T.REF_BATCH[T.MAIN]
    assert max(H, W) <= 40 and 32 <= gathered <= 144 and gathered % 8 == 0 and gathered != 8 and dxc % 8 == 0
    dyd, w16, dx = RS._dgrad_operands(B, H, W, 3, gathered, max(T.DG_DX))
    worst = {}
    try:
        with T.forced(tr, ntw):
            plan = T.tile_plan(B, H, W, gathered, dxc)
            assert plan is not None and (tr == 0 or plan[0] == tr)
            RS._check_dgrad(dev, f"{B}x{H}x{W} dy {gathered} -> dx {dxc} (TR {plan[0]}, MT {plan[1]}, NTW {plan[2]} x {plan[3]}, KSC {plan[5]})", 3,
                            dyd, w16, dx[..., :dxc], worst)
    finally:
        _print_worst("data gradient", worst)


# ---- extremes of the map ---------------------------------------------------------------------------------------------------------------
def _fits_subsets(B, H, W, cout):
    return all(s.numel() >= SUBSET_MIN_ELEMS for _, s in D._subsets(torch.empty(B, H, W, cout, device="meta")))


def _check_elementwise(dev, tag, xd, wd, conv, sc, sh):
    """the four epilogues on a case too small for the subsets: max |got - want| <= 1e-3 * max(1, max |want|) for fp16 outputs, 1e-5 relative L2
    for fp32 outputs and the statistics bounds (test_pw_fewer_tiles_than_waves)"""
    lib = L.load()
    st = L.stream_ptr(dev)
    B, H, W, cin = xd.shape
    cout = conv.shape[3]
    args = (L.ptr(xd), B, H, W, cin, L.ptr(wd), cout, 3, 1, 1, 1)

    def close16(got, want, what):
        err, bound = float((got.double() - want).abs().max()), 1e-3 * max(1.0, float(want.abs().max()))
        print(f"[conv tile] {tag}: {what}: max abs error {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (tag, what, err, bound)

    out, guard = D._guarded((B, H, W, cout), torch.float16, dev)
    L.check(lib.cvx_conv2d_nhwc(*args, TILE | 0, None, None, L.ptr(out), st), "plain")
    assert D._guard_ok(guard), tag
    close16(out, conv, "fp16 plain")
    out.fill_(D.GUARD_VALUE)
    L.check(lib.cvx_conv2d_nhwc(*args, TILE | 1, L.ptr(sc), L.ptr(sh), L.ptr(out), st), "affine")
    assert D._guard_ok(guard), tag
    v = conv * sc.double() + sh.double()
    close16(out, v * torch.sigmoid(v), "fp16 BN + SiLU")
    out32, guard32 = D._guarded((B, H, W, cout), torch.float32, dev)
    L.check(lib.cvx_conv2d_nhwc(*args, TILE | 2, L.ptr(sh), None, L.ptr(out32), st), "bias")
    e_bias = D._rel(out32, conv + sh.double())
    assert D._guard_ok(guard32) and e_bias < TOL32, (tag, e_bias)
    out32.fill_(D.GUARD_VALUE)
    R = D._stat_replicas(cout)
    flat = torch.zeros(R * cout * 4 + D.GUARD, dtype=torch.int64, device=dev)
    flat[R * cout * 4:] = 7
    L.check(lib.cvx_conv2d_nhwc(*args, TILE | 3, None, L.ptr(flat), L.ptr(out32), st), "stats")
    e_raw = D._rel(out32, conv)
    assert D._guard_ok(guard32) and D._guard_ok(flat[R * cout * 4:]) and e_raw < TOL32, (tag, e_raw)
    tot = flat[:R * cout * 4].view(R, cout, 2, 2).sum(0).double()
    sums = (tot[..., 0] / 64.0 + tot[..., 1] / 2.0 ** 40) / (B * H * W)
    mean, msq = conv.mean((0, 1, 2)), (conv * conv).mean((0, 1, 2))
    e1, e2 = float(((sums[:, 0] - mean).abs() / msq.sqrt()).max()), float((sums[:, 1] / msq - 1).abs().max())
    print(f"[conv tile] {tag}: fp32 bias {e_bias:.3e}, fp32 raw {e_raw:.3e}, stat mean / rms {e1:.3e}, stat mean square {e2:.3e}")
    assert e1 < TOL32 and e2 < TOL32, (tag, e1, e2)


EXTREME_CASES = list(T.EXTREMES.items())


@pytest.mark.parametrize("key,want", EXTREME_CASES, ids=[f"{k[0]}x{k[1]}x{k[2]}-cin{k[3]}" for k, _ in EXTREME_CASES])
def test_tile_extremes_of_the_map(dev, key, want):
    """1x2x2: one pixel group of 4 pixels, seven waves that own none (they still issue their DMA pieces and owe the barriers).  1x2x512, cin 32,
    TR 1: the widest row the kernel plans, 32 pixel groups, the magic-number division by 512 and 514 at its largest operands.  1x3x50.
    2x5x23 under (4, 3): the second band of an image is ONE row, 23 pixels -- two pixel groups, six idle waves.  The 512-wide case is large
    enough for the subsets; the others compare element-wise."""
    B, H, W, cin, cout, tr, ntw = key
    ops = RS._fwd_operands(B, H, W, cin, cout, 3)
    tag = f"{B}x{H}x{W} {cin}->{cout}"
    with T.forced(tr, ntw):
        p = T.tile_plan(B, H, W, cin, cout)
        assert p is not None and (p[1], p[2]) == want
        if _fits_subsets(B, H, W, cout):
            worst = {}
            try:
                RS._check_forward(dev, f"{tag} (TR {p[0]}, MT {p[1]}, NTW {p[2]})", TILE, 3, *ops, worst)
            finally:
                _print_worst("extremes", worst)
        else:
            _check_elementwise(dev, tag, *ops)


# ---- the packed-weight buffer of stand-alone launches -------------------------------------------------------------------------------------
def test_tile_packed_weight_buffer_is_keyed_by_block_and_repacked(dev):
    """A stand-alone launch packs its weights into a cached buffer keyed by (weight pointer, tap order, BN = 16 NTW) and re-packs it at every
    launch.  One weight tensor runs under NTW = 2 (two channel blocks) and NTW = 4 (one) -- two buffers behind one pointer -- then its filters
    are reversed IN PLACE and both run again: the reference of the second pair is the first one's with its channels reversed."""
    lib = L.load()
    st = L.stream_ptr(dev)
    cin, cout = 64, 56
    B = T.REF_BATCH[T.MAIN]
    H, W = T.MAIN
    xd, wd, conv, _, _ = _operands(T.MAIN, cin, B, cout)
    w_work = wd.clone()
    out, guard = D._guarded((B, H, W, cout), torch.float16, dev)
    worst = {}
    try:
        for weights, want, when in ((wd, conv, "first weights"), (wd.flip(0).contiguous(), conv.flip(-1), "changed in place")):
            w_work.copy_(weights)
            for ntw, nb in ((2, 2), (4, 1)):
                with T.forced(4, ntw):
                    assert T.tile_plan(B, H, W, cin, cout)[2:4] == (ntw, nb)
                    out.fill_(D.GUARD_VALUE)
                    L.check(lib.cvx_conv2d_nhwc(L.ptr(xd), B, H, W, cin, L.ptr(w_work), cout, 3, 1, 1, 1, TILE | 0, None, None, L.ptr(out), st), "plain")
                assert D._guard_ok(guard)
                D._localised(f"{when}, NTW {ntw}", out, want, TOL16, worst, "fp16 plain")
    finally:
        _print_worst("packed-weight buffer", worst)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
REFUSED = [   # B, H, W, cin, cout, k, stride, pad, dilation, forced (TR, NTW), why
    (1, 12, 20, 32, 16, 3, 2, 1, 1, (0, 0), "stride 2"), (1, 12, 20, 32, 16, 3, 1, 2, 2, (0, 0), "dilation 2"), (1, 12, 20, 32, 16, 1, 1, 0, 1, (0, 0), "a 1x1"),
    (1, 12, 20, 24, 16, 3, 1, 1, 1, (0, 0), "cin 24"), (1, 12, 20, 32, 36, 3, 1, 1, 1, (0, 0), "cout 36"), (1, 12, 1, 32, 16, 3, 1, 1, 1, (0, 0), "a map 1 pixel wide"),
    (1, 2, 513, 32, 16, 3, 1, 1, 1, (0, 0), "a map 513 pixels wide"), (1, 37, 39, 32, 72, 3, 1, 1, 1, (10, 5), "a forced pair without a plan"),
]


@pytest.mark.parametrize("B,H,W,cin,cout,k,stride,pad,dil,force,why", REFUSED, ids=[r[10].replace(" ", "-") for r in REFUSED])
def test_tile_force_bit_refuses_foreign_shapes(dev, B, H, W, cin, cout, k, stride, pad, dil, force, why):
    """outside the kernel's conditions, and under a forced pair that has no plan (10 rows of 39 pixels are MT = 4, which the planner's register
    rule does not combine with 5 channel tiles: <4, 5> is compiled and never launched), mode | 0x2000 is an error and launches nothing: the
    7.0-filled output, its guard cells and the zeroed statistics slab stay as they are"""
    lib = L.load()
    oh, ow = RS._out_size(H, k, stride, pad, dil), RS._out_size(W, k, stride, pad, dil)
    xd = torch.ones(B, H, W, cin, dtype=torch.float16, device=dev)
    wd = torch.ones(cout, k, k, cin, dtype=torch.float16, device=dev)
    with T.forced(*force):
        if force != (0, 0):
            assert T.tile_plan(B, H, W, cin, cout) is None
        for mode in (0, 1, 2, 3):
            dtype = torch.float16 if mode < 2 else torch.float32
            out, guard = D._guarded((B, oh, ow, cout), dtype, dev)
            aux = torch.zeros(D._stat_replicas(cout) * cout * 4, dtype=torch.int64, device=dev)
            sc = torch.ones(cout, device=dev)
            rc = lib.cvx_conv2d_nhwc(L.ptr(xd), B, H, W, cin, L.ptr(wd), cout, k, stride, pad, dil, TILE | mode, L.ptr(sc), L.ptr(aux if mode == 3 else sc),
                                     L.ptr(out), L.stream_ptr(dev))
            torch.cuda.synchronize()
            assert rc != 0, (why, mode)
            assert bool((out == D.GUARD_VALUE).all()) and D._guard_ok(guard) and bool((aux == 0).all()), (why, mode, "the refused call wrote")
    if force != (0, 0):
        assert T.tile_plan(B, H, W, cin, cout) is not None      # free, the same shape has a plan
