// Convolution launch geometry, host-only: (k, stride, pad, dil, ih, iw) -> tap tables, their traits, the phase classes of the data
// gradient and the pixel-shuffle weight map.  Plain C++17 without HIP: the engine, the single-op entries and the CPU check
// (tests/conv_plan_check.cpp) all read the geometry from here, and nowhere else is it written out.
#pragma once
#include <vector>

// One tap of the gather: input pixel = (o2*IS + dh, o2w*IS + dw); weight block index wtap.
struct ConvTap {
  int dh, dw, wtap, pad_;
};

// Output extent along one axis.  Valid when the dilated kernel fits the padded map (in + 2 * pad >= dil * (k - 1) + 1): below that the
// truncating division does not yield "no output" (in = 1, k = 3, pad = 0, stride = 2 gives 1), so callers reject such maps themselves.
inline int cvx_conv_out_size(int in, int k, int stride, int pad, int dil) { return (in + 2 * pad - dil * (k - 1) - 1) / stride + 1; }

// Forward taps in weight order: tap r * k + s reads input pixel (oh * stride + r * dil - pad, ow * stride + s * dil - pad).
inline std::vector<ConvTap> cvx_conv_fwd_taps(int k, int pad, int dil) {
  std::vector<ConvTap> taps;
  for (int r = 0; r < k; ++r)
    for (int s = 0; s < k; ++s) taps.push_back(ConvTap{r * dil - pad, s * dil - pad, r * k + s, 0});
  return taps;
}

// Packs a 9-entry tap table whose offsets all lie in the 3x3 neighbourhood into two 64-bit words, 4 bits per tap:
// pos = (dh+1)*4 + (dw+1), wt = weight tap index.  Kernel arguments instead of a device table: the halo kernel reads
// no tap memory at all.  Returns false (and the generic kernels are used) for any other table.
inline bool cvx_halo_pack_taps(const ConvTap* t, int n, unsigned long long* pos, unsigned long long* wt) {
  *pos = *wt = 0;
  if (n != 9) return false;
  for (int i = 0; i < 9; ++i) {
    if (t[i].dh < -1 || t[i].dh > 1 || t[i].dw < -1 || t[i].dw > 1 || t[i].wtap < 0 || t[i].wtap > 15) return false;
    *pos |= (unsigned long long)(((t[i].dh + 1) << 2) | (t[i].dw + 1)) << (4 * i);
    *wt |= (unsigned long long)t[i].wtap << (4 * i);
  }
  return true;
}
// the single tap (0, 0, weight tap 0): a 1x1 convolution (conv_pw.hip)
inline int cvx_taps_pointwise(const ConvTap* t, int n) { return (n == 1 && t[0].dh == 0 && t[0].dw == 0 && t[0].wtap == 0) ? 1 : 0; }
// the k x k / pad k / 2 / dilation 1 neighbourhood in row-major weight order
inline int cvx_taps_std(const ConvTap* t, int n, int k) {
  if (n != k * k) return 0;
  for (int i = 0; i < n; ++i)
    if (t[i].dh != i / k - k / 2 || t[i].dw != i % k - k / 2 || t[i].wtap != i) return 0;
  return 1;
}
inline int cvx_taps_std3x3(const ConvTap* t, int n) { return cvx_taps_std(t, n, 3); }  // conv_tile / conv_wgrad_halo / conv_wgrad_k3
inline int cvx_taps_std7x7(const ConvTap* t, int n) { return cvx_taps_std(t, n, 7); }  // conv_stem7.hip

// What the dispatchers ask about a tap table.  std3x3 / std7x7 are computed whatever the dilation: a dilated table has offsets
// of 2 and more between neighbours and matches neither, so no `dil == 1` test is needed in front of them.
struct TapTraits {
  bool halo_ok = false;
  unsigned long long halo_pos = 0, halo_wt = 0;  // cvx_halo_pack_taps, valid when halo_ok
  int pointwise = 0, std3x3 = 0, std7x7 = 0;
};
inline TapTraits cvx_tap_traits(const ConvTap* t, int n) {
  TapTraits tr;
  tr.halo_ok = cvx_halo_pack_taps(t, n, &tr.halo_pos, &tr.halo_wt);
  tr.pointwise = cvx_taps_pointwise(t, n);
  tr.std3x3 = cvx_taps_std3x3(t, n);
  tr.std7x7 = cvx_taps_std7x7(t, n);
  return tr;
}
inline TapTraits cvx_tap_traits(const std::vector<ConvTap>& t) { return cvx_tap_traits(t.data(), (int)t.size()); }

// Data gradient dx = dy (*) W^T of a stride-S convolution: the input pixels (y, x) with (y % S, x % S) == (oph, opw) form one
// phase class.  Pixel (oh2 * S + oph, ow2 * S + opw), oh2 < OH2, ow2 < OW2, gathers dy[oh2 + dh, ow2 + dw] * W[wtap] over the
// class's taps; rows / columns of dy outside the map read as zero.  A class may have no taps (stride > kernel) or no pixels.
struct DgradPhase {
  int oph, opw, OH2, OW2;
  std::vector<ConvTap> taps;
};
// one entry per (ph, pw), ph outermost
inline std::vector<DgradPhase> cvx_conv_dgrad_phases(int k, int stride, int pad, int dil, int ih, int iw) {
  std::vector<DgradPhase> out;
  const int S = stride;
  for (int ph = 0; ph < S; ++ph)
    for (int pw = 0; pw < S; ++pw) {
      DgradPhase d{ph, pw, (ih - ph + S - 1) / S, (iw - pw + S - 1) / S, {}};
      for (int r = 0; r < k; ++r) {
        const int nh = ph + pad - r * dil;
        if (((nh % S) + S) % S != 0) continue;
        for (int s = 0; s < k; ++s) {
          const int nw = pw + pad - s * dil;
          if (((nw % S) + S) % S != 0) continue;
          d.taps.push_back(ConvTap{nh / S, nw / S, r * k + s, 0});  // exact division
        }
      }
      out.push_back(d);
    }
  return out;
}

// 3x3 / stride 2 / pad 1 on an even map: every phase's taps lie in the 2 x 2 window (dh, dw in {0, 1}) of dy, so the four phases are
// four channel blocks of ONE stride-1 GEMM over that window, stored with a pixel shuffle (ConvParams::ps_cin).
// wtap[(2 * ph + pw) * 4 + 2 * dh + dw] = weight tap that phase (ph, pw) applies at window position (dh, dw), -1 = none.
// Geometry only: which channel counts take the route is the dispatchers' business.
struct PsDgrad {
  bool qualifies = false;
  int wtap[16];
};
inline PsDgrad cvx_conv_ps_dgrad(int k, int stride, int pad, int dil, int ih, int iw, const std::vector<DgradPhase>& phases) {
  PsDgrad ps;
  for (int q = 0; q < 16; ++q) ps.wtap[q] = -1;
  if (!(stride == 2 && k == 3 && pad == 1 && dil == 1 && ih == 2 * cvx_conv_out_size(ih, k, stride, pad, dil) &&
        iw == 2 * cvx_conv_out_size(iw, k, stride, pad, dil)))
    return ps;
  for (const DgradPhase& d : phases)
    for (const ConvTap& t : d.taps) {
      if (t.dh < 0 || t.dh > 1 || t.dw < 0 || t.dw > 1) return ps;
      ps.wtap[(d.oph * 2 + d.opw) * 4 + t.dh * 2 + t.dw] = t.wtap;
    }
  ps.qualifies = true;
  return ps;
}
// the window's tap table: tap tau = 2 * dh + dw reads weight block tau of the pixel-shuffle weights
inline std::vector<ConvTap> cvx_conv_ps_window_taps() {
  std::vector<ConvTap> pt(4);
  for (int tau = 0; tau < 4; ++tau) pt[tau] = ConvTap{tau >> 1, tau & 1, tau, 0};
  return pt;
}
