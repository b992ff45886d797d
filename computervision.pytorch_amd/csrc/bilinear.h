// Bilinear resampling, align_corners = False (F.interpolate(..., mode="bilinear"), deeplabv3plus.py:38,117-122,147), shared by every
// kernel that takes the taps: the NHWC / rows -> NCHW resizes (misc_ops.hip) and the segmentation loss and evaluation kernels
// (loss_seg.hip), which interpolate the logits per label pixel instead of reading a resized tensor and must see the same numbers.
#pragma once
#include "cvx_common.h"

// src = (dst + 0.5) * (in / out) - 0.5, clamped at 0; a 1x1 input degenerates to a broadcast.  Written as one fused multiply-add so that
// every caller rounds it the same way (left to the compiler, contraction is decided per inlining site).
__device__ __forceinline__ void bilinear_src(int d, float scale, int in_size, int* i0, int* i1, float* lam) {
  float s = __builtin_fmaf((float)d + 0.5f, scale, -0.5f);
  if (s < 0.f) s = 0.f;
  int a = (int)s;
  if (a > in_size - 1) a = in_size - 1;
  *i0 = a;
  *i1 = a + (a < in_size - 1 ? 1 : 0);
  *lam = s - (float)a;
}

// One value from its four taps: along x in both rows, then along y.  The roundings are spelled out -- a product, then one fused
// multiply-add, at both levels -- because callers compare results to the bit (cvx_seg_criterion_eval's arg max against the arg max of
// cvx_resize_bilinear_rows_to_nchw's output) and the compiler's own contraction of a * b + c * d differs from one inlining site to the
// next.  Pinning it is a choice, not a restatement of what each site compiled to before: a site where the compiler had contracted the
// other product may differ from the previous build by one ulp of the result, inside the tolerances its tests hold it to.
__device__ __forceinline__ float bilinear_mix(float v00, float v01, float v10, float v11, float lx, float ly) {
  const float top = __builtin_fmaf(lx, v01, (1.f - lx) * v00), bot = __builtin_fmaf(lx, v11, (1.f - lx) * v10);
  return __builtin_fmaf(1.f - ly, top, ly * bot);
}
