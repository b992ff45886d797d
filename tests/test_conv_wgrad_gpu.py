"""GPU (MI355X): every reachable configuration of the five weight-gradient kernels (csrc/conv_wgrad_k3.hip, conv_wgrad_stream.hip,
conv_wgrad_halo.hip, conv_wgrad_gemm.hip and the generic kernel of conv_wgrad.hip) against fp64 on the CPU.

tests/conv_wgrad_cases.py lists one shape per (kernel, instantiation) -- 38 + 42 + 16 + 2 + 5 = 103 -- and tests/test_conv_wgrad_plan_cpu.py holds
the launchers to that list.  Here every one of them runs DIRECTLY (``cvx_debug_conv2d_wgrad_nhwc`` with the kernel forced: its conditions of
correctness stay, the dispatcher's preferences -- channel products, 800 k pixels -- are dropped), on the smallest map that still has every
tail, with five pixel-split counts:

* the engine's own count for that kernel (``nsplit = 0``), and the k3 planner's ``wide`` count where it differs;
* one split;
* more splits than work units: the surplus splits must store zero slabs;
* a count that is no multiple of 8 and does not divide the units: the grid is rounded up to 8 splits and the surplus workgroups must exit
  at once, the last split is ragged and the ranges end inside an image.

The slab workspace is exactly the bytes the plan entry reports, pre-filled with NaN (a slab element the reducer reads but no workgroup wrote
shows up in dw), with 64 guard floats of 7.0 behind it; dw has 64 guard floats of 7.0 behind it too.

Operands are fp16-valued; the reference is ``torch.nn.grad.conv2d_weight`` in fp64 ON THE CPU, computed once per (map, k, stride, dilation) at
the widest channel counts any case uses there and sliced (dW[co][tap][ci] does not depend on the other channels).  Only the norms of the
comparisons are evaluated on the device, in fp64.

Bound: the project's fp32 bound, 1e-5 relative L2 (TOL32), on the whole tensor, on every tap, on the last 16-channel co tile, the last
16-channel ci tile and their intersection.  A subset with fewer than 256 elements is widened by whole 16-channel tiles until it has them.
dw sums thousands of pixels, so every subset has a healthy norm; as a condition, the same subsets of torch's fp32 CPU gradient stay under
1e-6 against fp64 (tests/test_conv_wgrad_plan_cpu.py checks that, without a GPU).

Measured on MI355X (pytest -s prints them), largest over all cases, split counts and subsets:
  k3      4.326e-07 (2x2x993 64->32, CfgF / two ring slots / eight column blocks, one split, tap 3)
  stream  2.023e-07 (2x55x5 104->8 3x3, <1, 3> with seven ci blocks, one split, tap 3)
  halo    2.866e-07 (2x21x37 16->24, <2, 1>, one split, tap 8)
  gemm    2.097e-07 (2x19x27 72->136 3x3, 128 x 128 tile, one split, tap 3)
  generic 2.495e-07 (2x37x53 32->8 3x3 stride 2, 16 x 192 tile, one split, tap 4)
The largest errors are all at one split, the longest fp32 sums; torch's own fp32 gradient on the CPU is at most 6.2e-07 from fp64 on these inputs.

Further tests: two launches give bit-identical dw (the slabs are plain stores); operands that are channel slices of wider buffers (x_ld =
Cin + 24, dy_ld = Cout + 40, offset 8, the other channels 1000.0) give bit for bit the dense result; the gemm kernel on maps 8 wide and 4
high; a kernel forced on a shape outside its conditions returns non-zero and leaves dw and the workspace untouched.

That the tests can fail was shown once with three scratch builds (outside the tree), each with one purely numerical change:
  A. k3 kernel: the last K-step wave group (wk == WK - 1; every wave where WK = 1) skips the MFMAs of the last of its four K-steps of a chunk.
     40 tests failed at their first comparison, rel-L2 0.135 ... 0.501 on the whole tensor against 1e-5: 36 of the 38 k3 table cases and the 4
     strided k3 cases.  The two table cases that passed are CfgB with two ring slots on one-row maps (5x1x142, 3x1x283), and rightly: a chunk
     there is one row of 142 + 2 padded pixels, K-steps 0 .. 4 of the 8, and the last K-step of the second wave group is step 7 -- padding only.
     Every test of the other four kernels passed: they do not contain the change.
  B. stream launcher: ``units_per_split`` one too small (at least 1), so a split's last chunk is dropped.  50 tests failed, rel-L2 0.686 ...
     0.771: all 42 stream table cases (at the engine's count, their first launch) and the 8 strided stream cases; everything else passed.
  C. generic kernel: the pixel loop ends one iteration early (``mc + PK < m_end``).  9 tests failed, rel-L2 0.504 ... 0.525: the 5 generic
     table cases and the 4 strided generic cases; everything else passed.
"""
import functools

import pytest
import torch

import conv_wgrad_cases as T
from computervision.pytorch_amd import _lib as L
from test_conv_dma_gpu import TOL32, GUARD, _guarded, _guard_ok, _rel

pytestmark = pytest.mark.gpu

SUBSET_MIN = 256
CASES = T.all_cases()
FILL = 1000.0               # the channels of the wider buffers that do not belong to the layer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _widest():
    """(map, k, stride, dil) -> (widest cin, widest cout) over every case that runs there"""
    w = {}
    for c in CASES:
        key = (c.map, c.k, c.stride, c.dil)
        a, b = w.get(key, (0, 0))
        w[key] = (max(a, c.cin), max(b, c.cout))
    for kern, cin, cout, k, s, m in T.STRIDED_CASES:
        a, b = w.get((m, k, s, 1), (0, 0))
        w[(m, k, s, 1)] = (max(a, cin), max(b, cout))
    return w


def make_operands(m, k, stride, dil, cin, cout):
    """fp16-valued x (B, H, W, cin), dy (B, OH, OW, cout) and the fp64 CPU weight gradient (cout, k * k, cin); shared with the CPU condition"""
    B, H, W = m
    OH, OW = T.out_size(H, k, stride, dil), T.out_size(W, k, stride, dil)
    g = torch.Generator().manual_seed(1000 * H + 10 * W + k + stride + dil)
    x16 = torch.randn(B, H, W, cin, generator=g).half()
    dy16 = torch.randn(B, OH, OW, cout, generator=g).half()
    ref = torch.nn.grad.conv2d_weight(x16.permute(0, 3, 1, 2).double(), (cout, cin, k, k), dy16.permute(0, 3, 1, 2).double(), stride, dil * (k // 2), dil)
    assert ref.dtype == torch.float64 and ref.device.type == "cpu"
    return x16, dy16, ref.permute(0, 2, 3, 1).reshape(cout, k * k, cin).contiguous()


@functools.lru_cache(maxsize=None)
def _operands(m, k, stride, dil):
    """-> device tensors at the widest channel counts; computed once, never written"""
    cin, cout = _widest()[(m, k, stride, dil)]
    x16, dy16, ref = make_operands(m, k, stride, dil, cin, cout)
    d = torch.device("cuda:0")
    return x16.to(d), dy16.to(d), ref.to(d)


def _sliced(m, k, stride, dil, cin, cout):
    x, dy, ref = _operands(m, k, stride, dil)
    return x[..., :cin].contiguous(), dy[..., :cout].contiguous(), ref[:cout, :, :cin]


def subsets(t):
    """(name, elements) of a (cout, taps, cin) tensor: see the module docstring"""
    cout, taps, cin = t.shape
    yield "whole tensor", t
    if taps > 1:
        for tap in range(taps):
            yield f"tap {tap}", t[:, tap]
    c0, i0 = 16 * ((cout - 1) // 16), 16 * ((cin - 1) // 16)
    a = c0
    while (cout - a) * taps * cin < SUBSET_MIN and a > 0:
        a -= 16
    yield "last co tile", t[a:]
    b = i0
    while cout * taps * (cin - b) < SUBSET_MIN and b > 0:
        b -= 16
    yield "last ci tile", t[:, :, b:]
    a, b = c0, i0
    while (cout - a) * taps * (cin - b) < SUBSET_MIN and (a > 0 or b > 0):
        if a > 0 and (cout - a <= cin - b or b == 0):
            a -= 16
        else:
            b -= 16
    yield "last co tile x last ci tile", t[a:, :, b:]


def check_subsets(tag, got, want, tol, worst=None, kind=None):
    for (sub, g), (_, w) in zip(subsets(got), subsets(want)):
        assert w.numel() >= SUBSET_MIN, (tag, sub, w.numel())
        e = _rel(g, w)
        if worst is not None and e > worst.get(kind, (0.0,))[0]:
            worst[kind] = (e, tag, sub)
        assert e < tol, (tag, sub, e, tol)


def _workspace(nbytes, dev):
    """exactly nbytes of NaN with 64 guard floats of 7.0 behind -> (flat, slabs, guard)"""
    n = nbytes // 4
    flat = torch.full((n + GUARD,), 7.0, dtype=torch.float32, device=dev)
    flat[:n] = float("nan")
    return flat, flat[:n], flat[n:]


def _launch(dev, x, dy, m, cin, cout, k, stride, dil, kernel, nsplit, x_ld=None, dy_ld=None):
    """cvx_debug_conv2d_wgrad_nhwc into a guarded dw with a guarded NaN workspace of exactly the planned bytes -> dw (cout, k * k, cin)"""
    B, H, W = m
    p = T.plan(B, H, W, cin, cout, k, stride, kernel, nsplit, 0, dil, x_ld, dy_ld)
    assert p.nsplit == nsplit and p.slab_bytes == nsplit * cout * k * k * ((cin + 15) // 16 * 16) * 4
    flat, slabs, wguard = _workspace(p.slab_bytes, dev)
    dw, dguard = _guarded((cout, k * k, cin), torch.float32, dev)
    rc = L.load().cvx_debug_conv2d_wgrad_nhwc(L.ptr(x), L.ptr(dy), B, H, W, cin, cout, k, stride, dil * (k // 2), dil, x_ld or cin, dy_ld or cout,
                                              kernel, nsplit, L.ptr(dw), L.ptr(slabs), p.slab_bytes, L.stream_ptr(dev))
    L.check(rc, "cvx_debug_conv2d_wgrad_nhwc")
    torch.cuda.synchronize()
    assert _guard_ok(wguard), "the kernel wrote past the planned slabs"
    assert _guard_ok(dguard), "the reducer wrote past dw"
    return dw


def split_counts(c):
    """[(label, count)] of a table case: see the module docstring"""
    B, H, W = c.map
    OH, OW = T.out_size(H, c.k, c.stride, c.dil), T.out_size(W, c.k, c.stride, c.dil)
    p0 = T.case_plan(c)
    units = T.units_of(p0, B, OH, OW)
    out = [("engine", p0.nsplit)]
    if c.kernel == T.K3:
        pw = T.case_plan(c, wide=1)
        if pw.nsplit != p0.nsplit:
            out.append(("engine, wide", pw.nsplit))
    out.append(("one split", 1))
    out.append(("surplus splits", units + 3))
    odd = [r for r in (3, 5, 6, 7, 9, 11, 13) if r < units and units % r != 0 and all(r != n for _, n in out)]
    assert odd, (T.case_id(c), units)
    out.append(("ragged splits", odd[-1] if units > 16 else odd[0]))
    return out


_WORST = {}


@pytest.mark.parametrize("c", CASES, ids=[T.case_id(c) for c in CASES])
def test_every_instantiation_at_every_split_count(dev, c):
    x, dy, ref = _sliced(c.map, c.k, c.stride, c.dil, c.cin, c.cout)
    counts = split_counts(c)
    first = None
    for label, ns in counts:
        dw = _launch(dev, x, dy, c.map, c.cin, c.cout, c.k, c.stride, c.dil, c.kernel, ns)
        check_subsets(f"{T.case_id(c)} {label} ({ns})", dw, ref, TOL32, _WORST, T.KERNEL_NAMES[c.kernel])
        if first is None:
            first = dw
    # run to run: the slabs are plain stores, the reducer adds in a fixed order
    again = _launch(dev, x, dy, c.map, c.cin, c.cout, c.k, c.stride, c.dil, c.kernel, counts[0][1])
    assert torch.equal(first, again), (T.case_id(c), "two launches differ")


@pytest.fixture(scope="module", autouse=True)
def _print_the_measured_maxima():
    yield
    for kind, (e, tag, sub) in sorted(_WORST.items()):
        print(f"\n[conv wgrad] {kind}: largest {e:.3e} (bound {TOL32:.1e}) at {tag}, {sub}")


STRIDED_IDS = [f"{T.KERNEL_NAMES[s[0]]}-{s[1]}to{s[2]}-k{s[3]}s{s[4]}" for s in T.STRIDED_CASES]


@pytest.mark.parametrize("kernel,cin,cout,k,stride,m", T.STRIDED_CASES, ids=STRIDED_IDS)
def test_channel_slices_of_wider_buffers_give_the_dense_result(dev, kernel, cin, cout, k, stride, m):
    """x_ld = Cin + 24, dy_ld = Cout + 40 (gemm: dense dy), the layer's channels at offset 8, every other channel 1000.0: a DMA table or a
    guard that reads a neighbour's channels where the padded tile must read zeros changes the result"""
    x, dy, ref = _sliced(m, k, stride, 1, cin, cout)
    B, H, W = m
    ns = T.plan(B, H, W, cin, cout, k, stride, kernel).nsplit
    dense = _launch(dev, x, dy, m, cin, cout, k, stride, 1, kernel, ns)
    assert _rel(dense, ref) < TOL32
    x_ld, dy_ld = cin + 24, (cout if kernel == T.GEMM else cout + 40)
    xw = torch.full(x.shape[:3] + (x_ld,), FILL, dtype=torch.float16, device=dev)
    xw[..., 8:8 + cin] = x
    dyv = dy
    if dy_ld != cout:
        dyw = torch.full(dy.shape[:3] + (dy_ld,), FILL, dtype=torch.float16, device=dev)
        dyw[..., 8:8 + cout] = dy
        dyv = dyw[..., 8:8 + cout]
    got = _launch(dev, xw[..., 8:8 + cin], dyv, m, cin, cout, k, stride, 1, kernel, ns, x_ld, dy_ld)
    assert torch.equal(got, dense), (float((got - dense).abs().max()), "strided operands change the result")


GEMM_SMALLEST_MAPS = [(2, 8, 8, 256, 128), (3, 4, 8, 64, 136)]


@pytest.mark.parametrize("B,H,W,cin,cout", GEMM_SMALLEST_MAPS)
def test_the_gemm_kernel_on_the_smallest_maps_it_takes(dev, B, H, W, cin, cout):
    """output maps 8 wide (four row wraps inside one 32-pixel chunk) and 4 high (an image wrap per chunk).  The dispatcher gives the first
    shape -- an edge case of tests/test_gpu_parity.py -- to the k3 kernel, so the gemm kernel meets it here only."""
    x16, dy16, ref = make_operands((B, H, W), 3, 1, 1, cin, cout)
    x, dy, ref = x16.to(dev), dy16.to(dev), ref.to(dev)
    for ns in (T.plan(B, H, W, cin, cout, 3, 1, T.GEMM).nsplit, 1, 3, B * H * W // 32 + 3):
        dw = _launch(dev, x, dy, (B, H, W), cin, cout, 3, 1, 1, T.GEMM, ns)
        check_subsets(f"gemm {B}x{H}x{W} {cin}->{cout}, {ns} splits", dw, ref, TOL32, _WORST, "gemm")


# (kernel, cin, cout, k, stride, (B, H, W), dy_ld or None): shapes outside the kernel's conditions
REFUSALS = [
    ("k3 on a 1x1", T.K3, 32, 32, 1, 1, (2, 10, 13), None),
    ("k3 on OW = 3", T.K3, 32, 32, 3, 1, (2, 10, 3), None),
    ("k3 on stride 2 with 64 -> 64", T.K3, 64, 64, 3, 2, (2, 21, 25), None),
    ("stream on stride 2", T.STREAM, 32, 32, 3, 2, (2, 21, 25), None),
    ("halo on Cin = 8", T.HALO, 8, 32, 3, 1, (2, 21, 37), None),
    ("gemm on OW = 7", T.GEMM, 64, 128, 3, 1, (2, 10, 7), None),
    ("gemm on strided dy", T.GEMM, 64, 128, 3, 1, (2, 10, 13), 168),
]


@pytest.mark.parametrize("what,kernel,cin,cout,k,stride,m,dy_ld", REFUSALS, ids=[r[0].replace(" ", "-") for r in REFUSALS])
def test_a_forced_kernel_refuses_shapes_outside_its_conditions(dev, what, kernel, cin, cout, k, stride, m, dy_ld):
    B, H, W = m
    OH, OW = T.out_size(H, k, stride), T.out_size(W, k, stride)
    with pytest.raises(L.CvxError):
        T.plan(B, H, W, cin, cout, k, stride, kernel, 2, 0, 1, None, dy_ld)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, cin, generator=g).half().to(dev)
    dy = torch.randn(B, OH, OW, dy_ld or cout, generator=g).half().to(dev)
    nbytes = 2 * cout * k * k * ((cin + 15) // 16 * 16) * 4
    flat, slabs, wguard = _workspace(nbytes, dev)
    dw, dguard = _guarded((cout, k * k, cin), torch.float32, dev)
    rc = L.load().cvx_debug_conv2d_wgrad_nhwc(L.ptr(x), L.ptr(dy), B, H, W, cin, cout, k, stride, k // 2, 1, cin, dy_ld or cout, kernel, 2,
                                              L.ptr(dw), L.ptr(slabs), nbytes, L.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc != 0, what
    assert bool((dw == 7.0).all()) and _guard_ok(dguard), "a refused call wrote dw"
    assert bool(torch.isnan(slabs).all()) and _guard_ok(wguard), "a refused call wrote the workspace"
