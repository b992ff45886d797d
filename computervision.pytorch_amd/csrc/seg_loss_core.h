// The device code that the segmentation criterion's two files share: loss_seg.hip (FocalLoss / plain cross-entropy, cvx_seg_loss and
// cvx_seg_eval) and loss_seg_opts.hip (class weights, label smoothing, hard-pixel mining: cvx_seg_loss_opts and cvx_seg_eval_opts).
// The taps of a label pixel, the class loop, the fixed-order block sums, the adjoint of the bilinear resize and the finalize kernel moved
// here from loss_seg.hip unchanged; each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "cvx_common.h"
#include "seg_tail.h"

namespace {

constexpr int SEG_MAX_NC = 4096;  // sanity bound only: the kernels loop over the classes

// The four source rows of one label pixel and its weights; logit(c) is the value cvx_resize_bilinear_rows_to_nchw writes for class c
// there (bilinear_src / bilinear_mix, bilinear.h).
struct PixelTaps {
  const float *r00, *r01, *r10, *r11;
  float lx, ly;
  __device__ __forceinline__ PixelTaps(const float* rows, int ld, int b, int ih, int iw, int OH, int OW, int oy, int ox) {
    int y0, y1, x0, x1;
    bilinear_src(oy, (float)ih / (float)OH, ih, &y0, &y1, &ly);
    bilinear_src(ox, (float)iw / (float)OW, iw, &x0, &x1, &lx);
    const float* base = rows + (long long)b * ih * iw * ld;
    r00 = base + ((long long)y0 * iw + x0) * ld;
    r01 = base + ((long long)y0 * iw + x1) * ld;
    r10 = base + ((long long)y1 * iw + x0) * ld;
    r11 = base + ((long long)y1 * iw + x1) * ld;
  }
  __device__ __forceinline__ float logit(int c) const { return bilinear_mix(r00[c], r01[c], r10[c], r11[c], lx, ly); }
  // eight classes at a time with 16-byte loads issued together (rows with ld % 8 == 0 on a 16-byte boundary)
  __device__ __forceinline__ void logits8(int c0, float* z) const {
    float a[8], bq[8], cq[8], d[8];
    *reinterpret_cast<float4*>(a) = *reinterpret_cast<const float4*>(r00 + c0);
    *reinterpret_cast<float4*>(a + 4) = *reinterpret_cast<const float4*>(r00 + c0 + 4);
    *reinterpret_cast<float4*>(bq) = *reinterpret_cast<const float4*>(r01 + c0);
    *reinterpret_cast<float4*>(bq + 4) = *reinterpret_cast<const float4*>(r01 + c0 + 4);
    *reinterpret_cast<float4*>(cq) = *reinterpret_cast<const float4*>(r10 + c0);
    *reinterpret_cast<float4*>(cq + 4) = *reinterpret_cast<const float4*>(r10 + c0 + 4);
    *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(r11 + c0);
    *reinterpret_cast<float4*>(d + 4) = *reinterpret_cast<const float4*>(r11 + c0 + 4);
#pragma unroll
    for (int k = 0; k < 8; ++k) z[k] = bilinear_mix(a[k], bq[k], cq[k], d[k], lx, ly);
  }
};

// f(c, logit) for every class in order.  Rows with ld % 8 == 0 (the engine's: 16-byte aligned, padded to 8 columns) take logits8; a class
// loop of scalar loads waits for memory 4 * nc times per pass.
template <class F>
__device__ __forceinline__ void each_logit(const PixelTaps& tp, int nc, bool vec, F f) {
  if (vec) {
    for (int c0 = 0; c0 < nc; c0 += 8) {
      float z[8];
      tp.logits8(c0, z);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c0 + k < nc) f(c0 + k, z[k]);
    }
  } else {
    for (int c = 0; c < nc; ++c) f(c, tp.logit(c));
  }
}

// Block sums of (loss, valid pixels) in a fixed order; one pair per workgroup, summed in index order by seg_loss_finalize_kernel
// (deterministic, no same-address atomics).
__device__ __forceinline__ void block_pair_to_part(double my_loss, double my_cnt, double* s_sum, double* s_cnt, double* part) {
  for (int o = 32; o > 0; o >>= 1) {
    my_loss += __shfl_xor(my_loss, o);
    my_cnt += __shfl_xor(my_cnt, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = my_loss;
    s_cnt[threadIdx.x >> 6] = my_cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * (long long)blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    part[2 * (long long)blockIdx.x + 1] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
  }
}

constexpr int EV_PIX = 8, EV_LDS_CELLS = 8192;  // seg_eval_kernel: label pixels per thread, and the LDS histogram's cells (nc <= 90)

__device__ __forceinline__ void bilinear_dst_range(int s, float scale, int out_size, int* lo, int* hi) {
  const float a = ((float)s - 0.5f) / scale - 0.5f, b = ((float)s + 1.5f) / scale - 0.5f;
  int l = (int)floorf(a) - 1, h = (int)ceilf(b) + 1;
  *lo = l < 0 ? 0 : l;
  *hi = h > out_size - 1 ? out_size - 1 : h;
}

// dpred[b][y*iw + x][c] = scale * sum over label pixels of w(oy, y) * w(ox, x) * g[b][c][oy][ox]; columns nc..ld-1 are zeroed.
// norm_mode 0: scale = grad_scale / norm_const; 1: scale = grad_scale / acc[1] (valid pixels counted by the pixel kernel).
// A workgroup owns 32 consecutive pixels of the flattened (b, y, x) order and all ld columns: thread = (pixel lane, class lane of 8), so a
// wave reads two class planes along x (contiguous), and the 32 x ld results leave through LDS as whole rows (one contiguous run of
// 32 * ld halves) -- a thread per (class, pixel) would write single halves 2 * ld bytes apart from workgroups on different XCDs.
constexpr int RG_PIX = 32;
__global__ __launch_bounds__(256) void resize_grad_rows_kernel(const float* g, int B, int nc, int ih, int iw, int OH, int OW, float grad_scale,
                                                               int norm_mode, double norm_const, const double* acc, half_t* dpred, int ld) {
  extern __shared__ __attribute__((aligned(16))) half_t tile[];  // [RG_PIX][ld]
  const long long npix = (long long)B * ih * iw;
  const long long p0 = (long long)blockIdx.x * RG_PIX;
  const int pl = threadIdx.x & (RG_PIX - 1), cl = threadIdx.x >> 5;
  const long long pidx = p0 + pl;
  const bool live = pidx < npix;
  const int x = live ? (int)(pidx % iw) : 0;
  const long long t = live ? pidx / iw : 0;
  const int y = (int)(t % ih);
  const int b = (int)(t / ih);
  const float sh = (float)ih / (float)OH, sw = (float)iw / (float)OW;
  int oy0, oy1, ox0, ox1;
  bilinear_dst_range(y, sh, OH, &oy0, &oy1);
  bilinear_dst_range(x, sw, OW, &ox0, &ox1);
  const double denom = norm_mode == 0 ? norm_const : (acc[1] > 0.0 ? acc[1] : 1.0);
  const float scale = (float)((double)grad_scale / denom);
  constexpr int XC = 12;  // label columns per chunk (the whole range at DeepLab's 4x upsampling)
  for (int c = cl; c < ld; c += 8) {
    float accv = 0.f;
    if (live && c < nc) {
      const float* gp = g + ((long long)b * nc + c) * OH * OW;
      for (int oxc = ox0; oxc <= ox1; oxc += XC) {  // the column weights of a chunk once, then every label row against them
        float wx[XC];
        int xo[XC];
#pragma unroll
        for (int j = 0; j < XC; ++j) {
          int x0, x1;
          float lx;
          bilinear_src(oxc + j, sw, iw, &x0, &x1, &lx);
          wx[j] = oxc + j <= ox1 ? (x0 == x ? 1.f - lx : 0.f) + (x1 == x ? lx : 0.f) : 0.f;
          xo[j] = oxc + j <= ox1 ? oxc + j : ox1;  // clamped: the loads below are unconditional (issued together), the weight is 0 there
        }
        for (int oy = oy0; oy <= oy1; ++oy) {
          int y0, y1;
          float ly;
          bilinear_src(oy, sh, ih, &y0, &y1, &ly);
          const float wy = (y0 == y ? 1.f - ly : 0.f) + (y1 == y ? ly : 0.f);
          if (wy == 0.f) continue;
          const float* gr = gp + (long long)oy * OW;
          float gv[XC];
#pragma unroll
          for (int j = 0; j < XC; ++j) gv[j] = gr[xo[j]];
          float row = 0.f;
#pragma unroll
          for (int j = 0; j < XC; ++j) row = fmaf(wx[j], gv[j], row);
          accv = fmaf(wy, row, accv);
        }
      }
    }
    tile[pl * ld + c] = (half_t)(accv * scale);
  }
  __syncthreads();
  const long long nlive = npix - p0 < RG_PIX ? npix - p0 : RG_PIX;
  const int nhalf = (int)nlive * ld;
  half_t* dst = dpred + p0 * ld;
  if ((ld & 7) == 0 && (reinterpret_cast<uintptr_t>(dpred) & 15) == 0) {
    for (int i = threadIdx.x * 8; i < nhalf; i += 256 * 8) *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(tile + i);
  } else {
    for (int i = threadIdx.x; i < nhalf; i += 256) dst[i] = tile[i];
  }
}

__global__ __launch_bounds__(256) void seg_loss_finalize_kernel(const double* part, int nblocks, double* acc, int norm_mode, double norm_const,
                                                                float* loss) {
  __shared__ double s0[256], s1[256];
  double a = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) {
    a += part[2 * (long long)i];
    c += part[2 * (long long)i + 1];
  }
  s0[threadIdx.x] = a;
  s1[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      s0[threadIdx.x] += s0[threadIdx.x + o];
      s1[threadIdx.x] += s1[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    acc[0] = s0[0];
    acc[1] = s1[0];
    const double denom = norm_mode == 0 ? norm_const : s1[0];  // CE over zero valid pixels: 0 / 0 = nan, as torch
    loss[0] = (float)(s0[0] / denom);
  }
}

}  // namespace
