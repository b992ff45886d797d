// Stand-alone check of csrc/conv_plan.h against the definition of a convolution, by brute force (host only; built and run by
// tests/test_conv_plan_cpu.py).  Forward: out[oy, ox] += in[oy*stride + r*dil - pad, ox*stride + s*dil - pad] * W[r, s], so the
// gradient of input pixel (y, x) gathers dy[oy, ox] * W[r, s] over every (oy, ox, r, s) with oy*stride + r*dil - pad == y and
// ox*stride + s*dil - pad == x.  The kernels read dy outside [0, OH) x [0, OW) as zero, so the sets are compared before clipping.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>

#include "conv_plan.h"

namespace {
long long g_cases = 0;

[[noreturn]] void fail(const char* what, int k, int stride, int pad, int dil, int ih, int iw) {
  std::printf("MISMATCH %s: k=%d stride=%d pad=%d dil=%d ih=%d iw=%d (after %lld cases)\n", what, k, stride, pad, dil, ih, iw, g_cases);
  std::exit(1);
}

int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

using Term = std::tuple<int, int, int>;  // (oy, ox, weight tap r * k + s)

void check_shape(int k, int stride, int pad, int dil, int ih, int iw) {
  const std::vector<ConvTap> fwd = cvx_conv_fwd_taps(k, pad, dil);
  if ((int)fwd.size() != k * k) fail("forward tap count", k, stride, pad, dil, ih, iw);
  for (int r = 0; r < k; ++r)
    for (int s = 0; s < k; ++s) {
      const ConvTap& t = fwd[r * k + s];
      if (t.dh != r * dil - pad || t.dw != s * dil - pad || t.wtap != r * k + s) fail("forward tap", k, stride, pad, dil, ih, iw);
    }
  const std::vector<DgradPhase> ph = cvx_conv_dgrad_phases(k, stride, pad, dil, ih, iw);
  if ((int)ph.size() != stride * stride) fail("phase class count", k, stride, pad, dil, ih, iw);
  for (int a = 0; a < stride; ++a)
    for (int b = 0; b < stride; ++b) {
      const DgradPhase& d = ph[a * stride + b];
      int rows = 0, cols = 0;  // pixels of the class inside the map
      for (int y = a; y < ih; y += stride) ++rows;
      for (int x = b; x < iw; x += stride) ++cols;
      if (d.oph != a || d.opw != b || d.OH2 != rows || d.OW2 != cols) fail("phase class order / extent", k, stride, pad, dil, ih, iw);
    }
  // the bound of oy that the definition can reach from inside the map: y in [0, ih) and r*dil - pad in [-pad, (k-1)*dil - pad]
  const int oy_lo = floor_div(-((k - 1) * dil - pad), stride) - 1, oy_hi = (ih - 1 + pad) / stride + 1;
  const int ox_lo = oy_lo, ox_hi = (iw - 1 + pad) / stride + 1;
  for (int y = 0; y < ih; ++y)
    for (int x = 0; x < iw; ++x) {
      std::vector<Term> want, got;
      for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int r = 0; r < k; ++r) {
          if (oy * stride + r * dil - pad != y) continue;
          for (int ox = ox_lo; ox <= ox_hi; ++ox)
            for (int s = 0; s < k; ++s)
              if (ox * stride + s * dil - pad == x) want.emplace_back(oy, ox, r * k + s);
        }
      const DgradPhase& d = ph[(y % stride) * stride + x % stride];
      for (const ConvTap& t : d.taps) got.emplace_back(y / stride + t.dh, x / stride + t.dw, t.wtap);
      std::sort(want.begin(), want.end());
      std::sort(got.begin(), got.end());
      if (std::adjacent_find(got.begin(), got.end()) != got.end()) fail("a phase class lists a term twice", k, stride, pad, dil, ih, iw);
      if (want != got) fail("data-gradient terms of an input pixel", k, stride, pad, dil, ih, iw);
      ++g_cases;
    }
  // pixel-shuffle description
  const PsDgrad ps = cvx_conv_ps_dgrad(k, stride, pad, dil, ih, iw, ph);
  const bool expect = k == 3 && stride == 2 && pad == 1 && dil == 1 && ih % 2 == 0 && iw % 2 == 0;
  if (ps.qualifies != expect) fail("pixel-shuffle: qualifies", k, stride, pad, dil, ih, iw);
  if (ps.qualifies) {
    if (cvx_conv_out_size(ih, k, stride, pad, dil) * 2 != ih || cvx_conv_out_size(iw, k, stride, pad, dil) * 2 != iw)
      fail("pixel-shuffle: output size", k, stride, pad, dil, ih, iw);
    for (int p = 0; p < 4; ++p) {  // the map yields exactly the class's taps, nothing more
      std::vector<Term> from_map, from_class;
      for (int tau = 0; tau < 4; ++tau)
        if (ps.wtap[p * 4 + tau] >= 0) from_map.emplace_back(tau >> 1, tau & 1, ps.wtap[p * 4 + tau]);
      for (const ConvTap& t : ph[p].taps) from_class.emplace_back(t.dh, t.dw, t.wtap);
      std::sort(from_class.begin(), from_class.end());
      if (from_map != from_class) fail("pixel-shuffle: wtap map vs phase classes", k, stride, pad, dil, ih, iw);
    }
    const std::vector<ConvTap> win = cvx_conv_ps_window_taps();
    for (int tau = 0; tau < 4; ++tau)
      if (win[tau].dh != (tau >> 1) || win[tau].dw != (tau & 1) || win[tau].wtap != tau) fail("pixel-shuffle: window taps", k, stride, pad, dil, ih, iw);
    ++g_cases;
  }
}

void expect_traits(const char* what, int k, int pad, int dil, const std::vector<ConvTap>& t, int pointwise, int std3x3, int std7x7, bool halo_ok) {
  const TapTraits tr = cvx_tap_traits(t);
  unsigned long long pos = 0, wt = 0;
  const bool packed = cvx_halo_pack_taps(t.data(), (int)t.size(), &pos, &wt);
  if (tr.pointwise != pointwise || tr.std3x3 != std3x3 || tr.std7x7 != std7x7 || tr.halo_ok != halo_ok || packed != halo_ok ||
      (halo_ok && (tr.halo_pos != pos || tr.halo_wt != wt)))
    fail(what, k, 1, pad, dil, 0, 0);
  if (halo_ok)
    for (int i = 0; i < 9; ++i)
      if ((int)((pos >> (4 * i)) & 15) != ((t[i].dh + 1) << 2 | (t[i].dw + 1)) || (int)((wt >> (4 * i)) & 15) != t[i].wtap) fail(what, k, 1, pad, dil, 0, 0);
  ++g_cases;
}

void check_traits() {
  expect_traits("traits 1x1", 1, 0, 1, cvx_conv_fwd_taps(1, 0, 1), 1, 0, 0, false);
  expect_traits("traits 1x1 pad 1", 1, 1, 1, cvx_conv_fwd_taps(1, 1, 1), 0, 0, 0, false);
  expect_traits("traits 3x3 pad 1", 3, 1, 1, cvx_conv_fwd_taps(3, 1, 1), 0, 1, 0, true);
  expect_traits("traits 3x3 pad 0", 3, 0, 1, cvx_conv_fwd_taps(3, 0, 1), 0, 0, 0, false);
  expect_traits("traits 3x3 pad 2", 3, 2, 1, cvx_conv_fwd_taps(3, 2, 1), 0, 0, 0, false);
  expect_traits("traits 3x3 pad 1 dil 2", 3, 1, 2, cvx_conv_fwd_taps(3, 1, 2), 0, 0, 0, false);
  expect_traits("traits 3x3 pad 2 dil 2", 3, 2, 2, cvx_conv_fwd_taps(3, 2, 2), 0, 0, 0, false);
  expect_traits("traits 7x7 pad 3", 7, 3, 1, cvx_conv_fwd_taps(7, 3, 1), 0, 0, 1, false);
  expect_traits("traits 7x7 pad 2", 7, 2, 1, cvx_conv_fwd_taps(7, 2, 1), 0, 0, 0, false);
  expect_traits("traits 7x7 pad 6 dil 2", 7, 6, 2, cvx_conv_fwd_taps(7, 6, 2), 0, 0, 0, false);
  expect_traits("traits 5x5 pad 2", 5, 2, 1, cvx_conv_fwd_taps(5, 2, 1), 0, 0, 0, false);
  expect_traits("traits empty", 0, 0, 1, {}, 0, 0, 0, false);
  // the stride-1 data gradient of the 3x3 / pad 1 convolution: inside the 3x3 neighbourhood, but mirrored -- halo yes, std3x3 no
  expect_traits("traits 3x3 dgrad", 3, 1, 1, cvx_conv_dgrad_phases(3, 1, 1, 1, 8, 8)[0].taps, 0, 0, 0, true);
  std::vector<ConvTap> swapped = cvx_conv_fwd_taps(3, 1, 1);  // right offsets, weight taps out of order
  std::swap(swapped[0].wtap, swapped[1].wtap);
  expect_traits("traits 3x3 permuted weights", 3, 1, 1, swapped, 0, 0, 0, true);
}
}  // namespace

int main() {
  // the formula against a count of the window positions that fit
  for (int k : {1, 2, 3, 5, 7})
    for (int stride = 1; stride <= 4; ++stride)
      for (int pad = 0; pad <= 3; ++pad)
        for (int dil = 1; dil <= 2; ++dil)
          for (int n = 1; n <= 9; ++n) {
            int fit = 0;
            for (int o = 0; o * stride + (k - 1) * dil - pad <= n - 1 + pad; ++o) ++fit;
            // (no window fits: outside the function's documented domain -- its callers reject maps smaller than the dilated kernel)
            if (fit > 0 && cvx_conv_out_size(n, k, stride, pad, dil) != fit) fail("output size", k, stride, pad, dil, n, n);
            ++g_cases;
          }
  for (int k : {1, 2, 3, 5, 7})
    for (int stride = 1; stride <= 4; ++stride)
      for (int pad = 0; pad <= 3; ++pad)
        for (int dil = 1; dil <= 2; ++dil)
          for (int ih = 1; ih <= 9; ++ih)
            for (int iw = 1; iw <= 9; ++iw) check_shape(k, stride, pad, dil, ih, iw);
  check_traits();
  std::printf("conv_plan_check: %lld cases ok\n", g_cases);
  return 0;
}
