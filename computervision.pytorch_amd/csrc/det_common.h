// What the VOC (det_eval.hip), COCO (coco_eval.hip) and diagnostics (det_diag.hip) evaluation kernels share, stated once: the size limits,
// the score text and threshold rules, how an image is admitted (det_image_refused), where its records go (det_record_base, the record
// cursor), how a box is read (det_box_map -- render.hip's too -- det_row_box, det_int_overlap), the VOC ground truth in LDS (det_stage_gt),
// the LDS layouts of det_match_kernel and det_confusion_kernel, the packed fields of the counting scans, the workgroup scan, and the host's
// checks and launch of the per-batch entries.  Each translation unit gets its own copy of the kernels here (anonymous namespace).
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

// what the per-image kernels (det_eval.hip, coco_eval.hip, det_diag.hip) hold in LDS at most, and the flag of a record
constexpr int DET_MAX_ROWS = 16384;       // what cvx_nms can return per image
constexpr int DET_MAX_GT = 1024;
constexpr int DET_MAX_LDS = 160 * 1024;
enum { FLAG_FP = 0, FLAG_TP = 1, FLAG_NEITHER = 2 };

__host__ __device__ inline int det_gt_slots(int G) { return (G + 1) & ~1; }
__host__ __device__ inline int det_row_slots(int max_det) { return (max_det + 3) & ~3; }

__device__ __forceinline__ bool det_score_reaches(float s, double threshold, int quantize) {
  return (quantize ? rint((double)s * 1e4) / 1e4 : (double)s) >= threshold;  // float("0.xxxx") >= score_threshold
}

// sum of det_count over counts[0, n), in every thread of the workgroup: a wave shuffle, four partials in `red`, one barrier -- which also
// publishes whatever the caller stored to LDS ahead of the call
__device__ __forceinline__ long long det_count_sum(const int* __restrict__ counts, int n, int max_det, long long* red) {
  long long total = 0;
  for (int i = threadIdx.x; i < n; i += DET_THREADS) total += det_count(counts[i], max_det);
  for (int o = 32; o > 0; o >>= 1) total += __shfl_down(total, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = total;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// first record of image b: the cursor the previous batch left, plus the records of the images before b in this one
__device__ __forceinline__ long long det_record_base(const int* __restrict__ counts, int b, int max_det, const unsigned long long* state,
                                                     long long* red) {
  return (long long)state[ST_CURSOR] + det_count_sum(counts, b, max_det, red);
}

// cursor += sum(counts), a launch of its own: the match kernels read the cursor of the previous batch
__global__ __launch_bounds__(DET_THREADS) void det_cursor_kernel(const int* __restrict__ counts, int B, int max_det, long long capacity,
                                                                 unsigned long long* state) {
  __shared__ long long red[DET_THREADS / 64];
  const long long added = det_count_sum(counts, B, max_det, red);
  if (threadIdx.x == 0) {
    const long long next = (long long)state[ST_CURSOR] + added;
    state[ST_CURSOR] = (unsigned long long)(next < capacity ? next : capacity);
  }
}

// true for an image that contributes nothing: NMS overflow (-1), a count past its block, a ground-truth count past G or -- for the record
// writers, which pass their base and capacity -- no room left; `counter` takes one add per such image.  The answer is the same in every
// thread, and the whole workgroup returns on it before any later barrier.
__device__ __forceinline__ bool det_image_refused(int n, int max_det, int ng, int G, unsigned long long* counter, long long base = 0,
                                                  long long capacity = 0x7fffffffffffffffLL) {
  const bool bad = n < 0 || n > max_det || ng < 0 || ng > G || base + det_count(n, max_det) > capacity;
  if (bad && threadIdx.x == 0) atomicAdd(counter, 1ull);
  return bad;
}

// box-map mode 1: core/utils/boxes.py:undo_letterbox in fp32, one rounding per operation
struct det_box_map {
  float px, py, gx, gy;
};
__device__ __forceinline__ det_box_map det_load_box_map(int box_mode, const float* __restrict__ box_map, int b) {
  if (box_mode != 1) return {0.f, 0.f, 1.f, 1.f};
  const float* m = &box_map[b * 4];
  return {m[0], m[1], m[2], m[3]};
}
__device__ __forceinline__ void det_undo_letterbox(float& x1, float& y1, float& x2, float& y2, const det_box_map& m) {
  x1 = __fmul_rn(__fsub_rn(x1, m.px), m.gx);
  y1 = __fmul_rn(__fsub_rn(y1, m.py), m.gy);
  x2 = __fmul_rn(__fsub_rn(x2, m.px), m.gx);
  y2 = __fmul_rn(__fsub_rn(y2, m.py), m.gy);
}

struct det_ibox {
  long long l, t, r, b;
};
// the box of a row as the VOC writers print it: mode 1 (x - px) * gx uncontracted, then int() towards zero
__device__ __forceinline__ det_ibox det_row_box(const float* row, int box_mode, const det_box_map& m) {
  float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
  if (box_mode == 1) det_undo_letterbox(x1, y1, x2, y2, m);
  return {(long long)__float2int_rz(x1), (long long)__float2int_rz(y1), (long long)__float2int_rz(x2), (long long)__float2int_rz(y2)};
}

// get_map's overlap of a row box and a staged ground truth (det_stage_gt): +1 pixel convention, integers below 2^53 and one fp64 division,
// the one rounding Python's iw * ih / ua has.  `met(overlap)` runs for boxes that meet and nothing runs for boxes that do not: that is
// no overlap of 0 -- get_map skips such a pair, and a threshold may be <= 0 (cvx_det_match does not bound min_overlap from below).  A
// callback and no returned value: the caller's comparison then stays inside the branch of the pairs that meet, where both kernels had it.
template <typename Met>
__device__ __forceinline__ void det_int_overlap(const det_ibox& d, const int* g, Met met) {
  const long long gl = g[1], gt = g[2], gr = g[3], gb = g[4];
  const long long iw = min(d.r, gr) - max(d.l, gl) + 1, ih = min(d.b, gb) - max(d.t, gt) + 1;
  if (iw > 0 && ih > 0) {
    const long long inter = iw * ih;
    const long long ua = (d.r - d.l + 1) * (d.b - d.t + 1) + (gr - gl + 1) * (gb - gt + 1) - inter;
    met((double)inter / (double)ua);
  }
}

// VOC ground truth src = [cls, l, t, r, b, difficult] into its six LDS ints, the class -1 when it is outside [0, nc) (it then matches no
// detection, and bad_class counts it); returns the staged class
__device__ __forceinline__ int det_stage_gt(const int* __restrict__ src, int nc, int* dst, unsigned long long& bad_class) {
  int cls = src[0];
  if (cls < 0 || cls >= nc) {
    ++bad_class;
    cls = -1;
  }
  dst[0] = cls;
  dst[1] = src[1];
  dst[2] = src[2];
  dst[3] = src[3];
  dst[4] = src[4];
  dst[5] = src[5] != 0;
  return cls;
}

// LDS layouts: byte offsets into the dynamic LDS, read by the host for the size and by the kernel for its pointers
struct det_match_layout {
  size_t best, gbox, match, qscore, total;
};
__host__ __device__ inline det_match_layout det_match_layout_of(int max_det, int G) {
  det_match_layout l;
  l.best = 32;                                              // behind the 4 wave partials: rank key of the TP per ground truth
  l.gbox = l.best + (size_t)8 * det_gt_slots(G);            // [cls, l, t, r, b, difficult] per ground truth
  l.match = l.gbox + (size_t)24 * det_gt_slots(G);          // per detection: ground truth, -1 FP, -2 neither
  l.qscore = l.match + (size_t)4 * det_row_slots(max_det);  // per detection: the score as it is recorded
  l.total = l.qscore + (size_t)4 * det_row_slots(max_det);
  return l;
}

struct det_confusion_layout {
  size_t top, gbox, winner, choice, total;
};
__host__ __device__ inline det_confusion_layout det_confusion_layout_of(int max_det, int G) {
  det_confusion_layout l;
  l.top = 0;                                              // per ground truth: the bits of the largest overlap that chose it
  l.gbox = l.top + (size_t)8 * det_gt_slots(G);           // [cls (-1: outside [0, nc)), l, t, r, b, difficult]
  l.winner = l.gbox + (size_t)24 * det_gt_slots(G);       // the lowest row among the detections that reach `top`
  l.choice = l.winner + (size_t)4 * det_gt_slots(G);      // per detection: its ground truth or a CH_ value
  l.total = l.choice + (size_t)4 * max_det;
  return l;
}

// the counting scans of the per-class kernels: three counts packed 20 bits apart -- inside a chunk of 256 each field adds at most 256, so
// one 64-bit scan carries all three -- and carried unpacked from chunk to chunk
__device__ __forceinline__ unsigned long long det_pack3(unsigned long long a, unsigned long long b, unsigned long long c) {
  return a | (b << 20) | (c << 40);
}
__device__ __forceinline__ long long det_field(unsigned long long v, int i) { return (long long)((v >> (20 * i)) & ((1ull << 20) - 1)); }
__device__ __forceinline__ void det_add3(unsigned long long v, long long& a, long long& b, long long& c) {
  a += det_field(v, 0);
  b += det_field(v, 1);
  c += det_field(v, 2);
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

// the argument checks cvx_det_match, cvx_coco_match and cvx_det_confusion share; `own`: the entry's further pointers are all there
inline int det_check_batch(const void* rows, const void* counts, const void* gt_counts, bool own, int batch, int max_det, int box_mode,
                           const void* box_map, const void* gt, int max_gt, int nc) {
  CVX_CHECK(rows && counts && gt_counts && own, "null arguments");
  CVX_CHECK(batch > 0 && max_det > 0 && max_det <= DET_MAX_ROWS && max_gt >= 0 && max_gt <= DET_MAX_GT && nc > 0, "bad sizes");
  CVX_CHECK(max_gt == 0 || gt, "null ground truth");
  CVX_CHECK(box_mode == 0 || (box_mode == 1 && box_map), "box_mode: 0 final boxes, 1 (x - px) * gx with box_map (batch, 4)");
  return 0;
}

// one workgroup per image with `lds` bytes of dynamic LDS: opt in when the layout is past 64 KB, then launch
template <typename Kernel, typename... Args>
inline int det_launch_lds(Kernel kernel, unsigned long long* optin, size_t lds, int batch, hipStream_t st, Args... args) {
  CVX_CHECK(lds <= (size_t)DET_MAX_LDS, "max_det and max_gt do not fit the LDS");
  if (lds > 65536) CVX_TRY(cvx_lds_optin((const void*)kernel, DET_MAX_LDS, optin));
  hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(DET_THREADS), lds, st, args...);
  return 0;
}

}  // namespace
