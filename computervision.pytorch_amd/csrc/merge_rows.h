// What merge_kernel (tiles.hip) and fuse_kernel (det_tta.hip) share in front of their suppression matrix: the workspace, which
// cvx_det_merge_workspace_bytes sizes for both (include/cvx_engine.h), and the rows front end -- the count of a frame's rows with its
// overflow flagging, the key fill and the sort.  The kernels differ in how a slot of the frame is enumerated, which is the helper's one
// functor, and in the box map of their gather, which stays with them.  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "cvx_common.h"
#include "lds_sort.h"

namespace {

constexpr int MERGE_CAP = 8192;  // candidates per frame the LDS sort holds

struct MergeWs {
  float4* box;              // [frames][MERGE_CAP] sorted boxes in frame coordinates
  float* score;             // [frames][MERGE_CAP]
  float* cls;               // [frames][MERGE_CAP]
  int* ord;                 // [frames][MERGE_CAP]
  unsigned long long* mat;  // [frames][MERGE_CAP][MERGE_CAP / 64]
};

inline MergeWs merge_layout(cvx_carver& c, long long frames) {
  MergeWs ws;
  ws.box = c.take<float4>(frames * MERGE_CAP);
  ws.score = c.take<float>(frames * MERGE_CAP);
  ws.cls = c.take<float>(frames * MERGE_CAP);
  ws.ord = c.take<int>(frames * MERGE_CAP);
  ws.mat = c.take<unsigned long long>(frames * MERGE_CAP * (MERGE_CAP / 64));
  return ws;
}

// slot_of(k), k < nslots: the k-th slot that may belong to this frame, or -1 when it does not.  Called by the whole workgroup of THREADS
// threads; keys (LDS) holds MERGE_CAP entries.
//   1. how many candidates: the counts of the frame's slots; a count outside [0, max_det_in] contributes nothing and adds 1 to *overflow;
//   2. the keys (score desc, ordinal asc), the ordinal slot * max_det_in + r in the low word (the caller checked that it fits 31 bits);
//      then the sort.
// Returns the number of candidates, or -1, before any key is written, when there are more than MERGE_CAP: the caller flags the frame.
template <int THREADS, typename SlotOf>
__device__ __forceinline__ int merge_rows_front(const float* __restrict__ rows, const int* __restrict__ counts, int nslots, int max_det_in,
                                                unsigned long long* keys, int* overflow, SlotOf slot_of) {
  __shared__ int s_n, s_fill;
  const int tid = threadIdx.x;
  if (tid == 0) s_n = s_fill = 0;
  __syncthreads();
  for (int k = tid; k < nslots; k += THREADS) {
    const int s = slot_of(k);
    if (s < 0) continue;
    const int c = counts[s];
    if (c < 0 || c > max_det_in) atomicAdd(overflow, 1);
    else if (c > 0) atomicAdd(&s_n, c);
  }
  __syncthreads();
  const int n = s_n;
  if (n > MERGE_CAP) return -1;
  const unsigned cells = (unsigned)nslots * (unsigned)max_det_in;
  for (unsigned e = tid; e < cells; e += THREADS) {
    const int k = (int)(e / (unsigned)max_det_in), r = (int)(e - (unsigned)k * (unsigned)max_det_in);
    const int s = slot_of(k);
    if (s < 0) continue;
    const int c = counts[s];
    if (c < 0 || c > max_det_in || r >= c) continue;
    const long long o = (long long)s * max_det_in + r;
    const int at = atomicAdd(&s_fill, 1);
    keys[at] = score_key(rows[o * 6 + 4], (unsigned)o);
  }
  lds_sort_keys<THREADS>(keys, n);
  return n;
}

}  // namespace
