// The greedy walk over a suppression bit matrix, shared by nms_kernel (nms.hip), merge_kernel (tiles.hip) and fuse_kernel (det_tta.hip):
// they differ in where the keep list is parked, nothing else.  (soft_nms_kernel and wbf_kernel have no matrix: their picks depend on
// scores and boxes that change as they go.)  The suite pins the result bit for bit, so the fences live in one place.  Each kernel builds the
// matrix itself -- row i, word wj, bit j - 64 wj set when j > i and its pair test holds: behind a shared row builder that takes the test
// as a functor merge_kernel measured 3.6 % slower (profiles/eval_tail_refactor_ab.txt).  Each translation unit gets its own copy.
#pragma once
#include "cvx_common.h"

namespace {

// mat[i * nw + wj], nw = cdiv(n, 64), are the rows of n candidates sorted best first, written by this workgroup of THREADS threads.
// `removed` (LDS, nw words) is cleared, then wave 0 walks the rows in order: a candidate not yet removed is kept (its sorted position
// goes to keep[count], in global memory) and its row is OR-ed into `removed`; at most max_keep are kept.  Called by the whole
// workgroup; every thread gets the count, after a barrier behind which keep[0 .. count) is visible to all of them.
template <int THREADS>
__device__ __forceinline__ int greedy_walk(const unsigned long long* mat, unsigned long long* removed, int n, int max_keep, int* keep) {
  __shared__ int s_nkeep;
  const int tid = threadIdx.x, nw = (n + 63) / 64;
  for (int i = tid; i < nw; i += THREADS) removed[i] = 0;
  __threadfence_block();
  __syncthreads();  // the rows every wave wrote and the cleared words, visible to wave 0
  if (tid < 64) {
    int nkeep = 0;
    for (int i = 0; i < n && nkeep < max_keep; ++i) {
      const bool dead = (removed[i >> 6] >> (i & 63)) & 1ull;  // uniform
      if (dead) continue;
      if (tid == 0) keep[nkeep] = i;
      ++nkeep;
      for (int wj = tid; wj < nw; wj += 64) removed[wj] |= mat[(long long)i * nw + wj];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (tid == 0) s_nkeep = nkeep;
  }
  // Not needed for correctness: __syncthreads() is itself a workgroup-scope release fence, the barrier, and an acquire fence, which
  // already orders lane 0's stores to `keep` before the other waves' loads.  The stronger form is kept so that the hand-off of the
  // keep list does not lean on how the barrier is spelled in the runtime's headers.
  __threadfence_block();
  __syncthreads();
  return s_nkeep;
}

}  // namespace
