// The (score desc, index asc) key and the in-LDS bitonic sort of 64-bit keys, shared by every kernel that orders candidates: nms_kernel
// (nms.hip), soft_nms_kernel (soft_nms.hip), merge_kernel and fuse_kernel (tiles.hip, det_tta.hip, through merge_rows.h), wbf_kernel
// (box_fusion.hip), regions_emit_kernel (seg_regions.hip), topk_sorted / finish_kernel (centernet_decode.hip), coco_match_kernel
// (coco_eval.hip, the sort) and det_match_kernel (det_eval.hip, the key).  The suite pins the tie order and the padding key bit for bit, so they live in one
// place.  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "cvx_common.h"

namespace {

// Ascending keys = score descending, ties by index ascending.  `score_bits` are the bits of a non-negative fp32 (they order like the value).
__device__ __forceinline__ unsigned long long score_key_bits(unsigned score_bits, unsigned idx) {
  return ((unsigned long long)(0xFFFFFFFFu - score_bits) << 32) | idx;
}
__device__ __forceinline__ unsigned long long score_key(float score, unsigned idx) { return score_key_bits(__float_as_uint(score), idx); }

// Sorts keys[0 .. n) ascending, by the whole workgroup of THREADS threads: keys[n .. next power of two) are padded with ~0ull (they sort
// last; the array must hold that many), then the bitonic network runs with a barrier per stage.  The caller's writes of keys[0 .. n) need
// no barrier of their own before the call; the function returns after the last barrier.  n <= 16384.
template <int THREADS>
__device__ __forceinline__ void lds_sort_keys(unsigned long long* keys, int n) {
  const int tid = threadIdx.x;
  int cap2 = 1;
  while (cap2 < n) cap2 <<= 1;
  for (int i = n + tid; i < cap2; i += THREADS) keys[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= cap2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < cap2; i += THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long x = keys[i], z = keys[l];
          const bool up = (i & k) == 0;
          if ((x > z) == up) {
            keys[i] = z;
            keys[l] = x;
          }
        }
      }
      __syncthreads();
    }
}

}  // namespace
