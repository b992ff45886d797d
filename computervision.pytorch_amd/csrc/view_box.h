// A row's box brought to the picture through its slot's affine map, the arithmetic the suite pins bit for bit, shared by the two fusions
// of several reports per frame: fuse_kernel (det_tta.hip) and wbf_kernel (box_fusion.hip).  (merge_kernel's map is an add and a clamp,
// to_frame of tiles.hip; the rows front end the two matrix kernels share is merge_rows.h.)  Plain operators with contraction switched off
// in each helper, every operation rounded on its own.  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "cvx_common.h"

namespace {

// what a slot reports -> the picture: a rounded product, a rounded add
__device__ __forceinline__ float through(float v, float a, float c) {
#pragma clang fp contract(off)
  const float m = v * a;
  return m + c;
}
__device__ __forceinline__ float clamp_to(float v, int size) { return fminf(fmaxf(v, 0.f), (float)size); }

// row [x1, y1, x2, y2, ...] through vm = [ax, cx, ay, cy]: the corners re-ordered (a flipped view swaps them), then clamped to the (fh, fw) frame
__device__ __forceinline__ float4 mapped_box(const float* __restrict__ row, const float* __restrict__ vm, int fh, int fw) {
  const float ax = vm[0], cx = vm[1], ay = vm[2], cy = vm[3];
  const float tx1 = through(row[0], ax, cx), ty1 = through(row[1], ay, cy), tx2 = through(row[2], ax, cx), ty2 = through(row[3], ay, cy);
  return make_float4(clamp_to(fminf(tx1, tx2), fw), clamp_to(fminf(ty1, ty2), fh), clamp_to(fmaxf(tx1, tx2), fw), clamp_to(fmaxf(ty1, ty2), fh));
}

}  // namespace
