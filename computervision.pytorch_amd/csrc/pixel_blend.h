// The 50/50 blend of the two overlay kernels (render.hip: cvx_seg_overlay, seg_tiles.hip: cvx_seg_stitch): cv2.addWeighted(a, .5, b, .5, 0)
// on uint8 in integers.
#pragma once
#include "cvx_common.h"

__device__ __forceinline__ unsigned blend_half(unsigned a, unsigned b) {  // (a + b) / 2, ties to even
  const unsigned s = a + b;
  return (s >> 1) + (s & (s >> 1) & 1u);
}
