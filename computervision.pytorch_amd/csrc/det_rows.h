// The 6-float detection row [x1, y1, x2, y2, score, class] as the suppression family writes it, and the tail of a frame's rows past its
// count.  store_row: merge_kernel (tiles.hip) and wbf_kernel (box_fusion.hip).  zero_rows: those two, fuse_kernel (det_tta.hip, whose
// emit votes and stays its own) and soft_nms_kernel (soft_nms.hip, where it compiles to the instructions of the function it replaces).
// Not used: nms_kernel (nms.hip) leaves the rows past its count untouched, and its row store and soft_nms_kernel's stay in line -- with
// the helpers of this family called from them the two kernels measured up to 1.1 % slower (profiles/suppress_refactor_ab.txt), so both
// keep the parent's instructions.  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "cvx_common.h"

namespace {

__device__ __forceinline__ void store_row(float* o, const float4& bx, float score, float cls) {
  o[0] = bx.x;
  o[1] = bx.y;
  o[2] = bx.z;
  o[3] = bx.w;
  o[4] = score;
  o[5] = cls;
}

// Rows from .. max_det - 1 of a frame become zero rows, by the whole workgroup of THREADS threads; the frame's index columns get their
// fill values there (the anchor index 0 in soft-NMS; the source -1 and the members 0 in the merges).  col_b may be null.
template <int THREADS>
__device__ __forceinline__ void zero_rows(float* orow, int from, int max_det, int* col_a, int fill_a, int* col_b = nullptr, int fill_b = 0) {
  for (int r = from + (int)threadIdx.x; r < max_det; r += THREADS) {
    float* o = orow + (long long)r * 6;
    o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0.f;
    col_a[r] = fill_a;
    if (col_b) col_b[r] = fill_b;
  }
}

}  // namespace
