// What nms_kernel (nms.hip) and soft_nms_kernel (soft_nms.hip) state once: the capacity of a block, the size its key array and workspace
// columns get, and the corner arithmetic of a candidate's box.  Their candidate front end (fill, sort, gather) stays in line in both
// kernels: behind one helper soft_nms_kernel measured up to 1.1 % slower and nms_kernel 1.1 % slower at capacity
// (profiles/suppress_refactor_ab.txt).  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "cvx_common.h"

namespace {

constexpr int NMS_CAP = 16384;  // candidates per block the LDS sort holds

// the key array and the workspace columns of a block are sized for the next power of two >= A, at least 64 and at most NMS_CAP
inline int nms_cap_for(int A) {
  int c = 64;
  while (c < A && c < NMS_CAP) c <<= 1;
  return c;
}

// The arithmetic the suite pins bit for bit: plain operators with contraction switched off (the pragma does not reach into the _rn
// intrinsics' own bodies, so they are not used here).  (cx, cy, w, h) -> corners, ultralytics_ops.py:360-375
__device__ __forceinline__ float4 box_corners(float cx, float cy, float w, float h) {
#pragma clang fp contract(off)
  const float hw = w * 0.5f, hh = h * 0.5f;
  return make_float4(cx - hw, cy - hh, cx + hw, cy + hh);
}

}  // namespace
