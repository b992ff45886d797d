// What the VOC (det_eval.hip), COCO (coco_eval.hip) and diagnostics (det_diag.hip) evaluation kernels share: the record cursor, the score
// text and threshold rules, the box map, the size limits and the workgroup scan.  Each translation unit gets its own copy of the kernels
// here (anonymous namespace).
#pragma once
#include "cvx_common.h"

namespace {

constexpr int DET_THREADS = 256;
enum { ST_CURSOR = 0, ST_OVERFLOW = 1, ST_LOW_SCORE = 2, ST_BAD_CLASS = 3 };

// str(np.float32(x))[:6] for x in [1e-4, 1]: the 4-decimal number k / 1e4 nearest to x is the text itself when it rounds back to x (the
// shortest round-trip text is then no longer than it), otherwise the text has more digits and the cut truncates.  x * 1e4 is exact in fp64.
__device__ __forceinline__ float det_quantize(float x) {
  const double p = (double)x * 1e4;
  const double k = rint(p);
  if ((float)(k / 1e4) == x) return x;
  return (float)(floor(p) / 1e4);
}

__device__ __forceinline__ int det_count(int c, int max_det) { return (c < 0 || c > max_det) ? 0 : c; }

// what the per-image VOC kernels (det_eval.hip, det_diag.hip) hold in LDS at most, and the flag of a record
constexpr int DET_MAX_ROWS = 16384;       // what cvx_nms can return per image
constexpr int DET_MAX_GT = 1024;
constexpr int DET_MAX_LDS = 160 * 1024;
enum { FLAG_FP = 0, FLAG_TP = 1, FLAG_NEITHER = 2 };

__host__ __device__ inline int det_gt_slots(int G) { return (G + 1) & ~1; }

__device__ __forceinline__ bool det_score_reaches(float s, double threshold, int quantize) {
  return (quantize ? rint((double)s * 1e4) / 1e4 : (double)s) >= threshold;  // float("0.xxxx") >= score_threshold
}

__global__ __launch_bounds__(DET_THREADS) void det_cursor_kernel(const int* __restrict__ counts, int B, int max_det, long long capacity,
                                                                 unsigned long long* state) {
  __shared__ long long red[DET_THREADS / 64];
  long long total = 0;
  for (int i = threadIdx.x; i < B; i += DET_THREADS) total += det_count(counts[i], max_det);
  for (int o = 32; o > 0; o >>= 1) total += __shfl_down(total, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long next = (long long)state[ST_CURSOR] + red[0] + red[1] + red[2] + red[3];
    state[ST_CURSOR] = (unsigned long long)(next < capacity ? next : capacity);
  }
}

// box-map mode 1: core/utils/boxes.py:undo_letterbox in fp32, one rounding per operation
__device__ __forceinline__ void det_undo_letterbox(float& x1, float& y1, float& x2, float& y2, float px, float py, float gx, float gy) {
  x1 = __fmul_rn(__fsub_rn(x1, px), gx);
  y1 = __fmul_rn(__fsub_rn(y1, py), gy);
  x2 = __fmul_rn(__fsub_rn(x2, px), gx);
  y2 = __fmul_rn(__fsub_rn(y2, py), gy);
}

// inclusive scan over the workgroup's 256 values (Hillis-Steele through LDS; the segments are short and this runs once per evaluation)
template <typename T, typename Op>
__device__ __forceinline__ T det_block_scan(T v, T* buf, int lane, bool backward, Op op) {
  const int i = backward ? DET_THREADS - 1 - lane : lane;
  buf[i] = v;
  __syncthreads();
  for (int o = 1; o < DET_THREADS; o <<= 1) {
    T other = v;
    const bool has = i >= o;
    if (has) other = buf[i - o];
    __syncthreads();
    if (has) v = op(other, v);
    buf[i] = v;
    __syncthreads();
  }
  return v;
}

}  // namespace
