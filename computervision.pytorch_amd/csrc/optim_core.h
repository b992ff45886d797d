// The per-element arithmetic the optimiser kernels of misc_ops.hip (adam_ema_kernel, ema_update_kernel) and optim.hip (optim_kernel) share.
// Every function here fixes its own rounding: contraction is off inside it and the FMAs it wants are written out.
#pragma once
#include "cvx_common.h"

// The weight average (ModelEMA.update of the reference): e <- rn(rn(e * d) + rn(omd * p)), three correctly rounded fp32 operations in this
// order, which is what torch's `v *= d; v += (1 - d) * p` computes.  Contraction is switched off for exactly these three: this toolchain's
// __fmul_rn / __fadd_rn are plain `*` and `+` that the backend does fuse into an FMA (it did, in the 16-byte path).
__device__ __forceinline__ float ema_mix(float e, float p, float d, float omd) {
#pragma clang fp contract(off)
  const float a = e * d;
  const float b = omd * p;
  return a + b;
}

// adam_kernel's arithmetic with the contraction written out: adam_step4 / adam_step1 spell the FMAs adam_kernel (misc_ops.hip) compiles to for
// gfx950 in its 16-byte path and in its scalar tail (they differ: the tail keeps v and the denominator as multiply + add), with contraction off
// around them, so that a kernel which calls them leaves p, m and v bit for bit as adam_kernel does whatever else it fuses into the pass.
// tests/test_ema_gpu.py and tests/test_optim_gpu.py compare the paths on the device.
__device__ __forceinline__ void adam_step4(float& p, float& m, float& v, float g, float b1, float b2, float eps, float lr_over_bc1,
                                           float inv_sqrt_bc2) {
#pragma clang fp contract(off)
  const float g1 = (1.f - b1) * g, g2 = (1.f - b2) * g;
  m = __builtin_fmaf(b1, m, g1);
  v = __builtin_fmaf(b2, v, g2 * g);
  const float num = lr_over_bc1 * m;
  p = p - num / __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps);
}
__device__ __forceinline__ void adam_step1(float& p, float& m, float& v, float g, float b1, float b2, float eps, float lr_over_bc1,
                                           float inv_sqrt_bc2) {
#pragma clang fp contract(off)
  const float g1 = (1.f - b1) * g, g2 = (1.f - b2) * g;
  m = __builtin_fmaf(b1, m, g1);
  const float bv = b2 * v, gg = g2 * g;
  v = bv + gg;
  const float num = lr_over_bc1 * m, den = sqrtf(v) * inv_sqrt_bc2;
  p = p - num / (den + eps);
}
