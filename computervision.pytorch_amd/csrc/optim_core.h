// The per-element arithmetic of the optimiser kernels of optim.hip (optim_step_kernel, ema_update_kernel): the weight average and the Adam
// recurrence are spelled here and nowhere else.  Every function fixes its own rounding: contraction is off inside it and the FMAs it wants
// are written out, so what a kernel fuses around a call, or a compiler upgrade, does not move a bit.
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

// The Adam arithmetic of this library (torch.optim.Adam without weight decay or amsgrad; g arrives scaled, lr_over_bc1 = lr/(1-b1^t),
// inv_sqrt_bc2 = 1/sqrt(1-b2^t)): adam_step4 for the elements of a 16-byte chunk, adam_step1 for the scalar tail of n % 4 != 0.  Which
// products are FMAs is part of the definition.  The two differ -- the tail keeps v and the denominator as multiply + add -- and stay
// different because checkpoints and fixtures hold those bits: tests/golden/adam_trace.npz pins both (tests/test_optim_gpu.py), and
// tests/test_ema_gpu.py and tests/test_optim_gpu.py compare the instantiations of the step kernel with each other on the device.
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
