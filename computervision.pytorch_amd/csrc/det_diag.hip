// Diagnostics of the four detectors on gfx950, beside the VOC mAP of det_eval.hip: the confusion matrix at one (confidence, IoU) pair, per
// batch (cvx_det_confusion), and precision / recall / F1 against the confidence threshold with the log-average miss rate's nine miss
// rates, once per evaluation (cvx_det_conf_curves).  Nothing is read by the host between the batches.
//
// The confusion rule is the project's own statement of Ultralytics' ConfusionMatrix.process_batch with the ties decided; it is restated
// sequentially in tests/det_diag_restatement.py and every number here is held to that restatement bit for bit.  Reference semantics of the
// miss rates (file:line under the reference tree):
//   log_average_miss_rate        core/metrics/mAP.py:34-70       fppi = fp_cumsum / n_images, mr = 1 - recall, both with a sentinel in
//                                                                front (-1, 1); per point of logspace(-2, 0, 9) the miss rate of the last
//                                                                record whose fppi <= the point; exp(mean(log(max(1e-10, .)))) -- the host's
//   counter_images_per_class     core/metrics/mAP.py:396-401     images that hold a non-difficult ground truth of the class
//
//   K1 det_confusion  one workgroup per image, its ground truths in LDS.  Pass 1: every detection that reaches `conf` maps and truncates its
//                     box as det_match does, picks the ground truth of ANY class it overlaps most (strictly above `iou`, lowest index on a
//                     tie) and atomic-maxes the overlap's bits into that ground truth's cell (positive doubles order as their bits).  Pass 2:
//                     the detections whose overlap (recomputed: the same integers, the same division) equals the cell atomic-min their row.
//                     Pass 3: the winner adds to [its class, the ground truth's class], every other participating detection to the background
//                     column, a ground truth without a winner to the background row.  A detection that chose a difficult ground truth counts
//                     nowhere.  Integer atomics on the int64 tables: the order of the additions changes nothing.
//   K2 det_curves     one workgroup per class over the records in cvx_det_ap's order: per grid point a binary search for the records that
//                     reach it (scores descend) and the precision / recall cvx_det_ap left at the last of them; a chunked scan of the FP
//                     flags counts, per reference point, the records whose fppi stays at or below it (fppi never falls, so they are a prefix)
//   K3 det_best       nc + 1 workgroups: the mean F1 over the classes with a ground truth (ascending class), the moving average with edge
//                     replication of it and of every class's F1, and the first maximum of each smoothed curve
#include "det_common.h"
#include "../../include/cvx_engine.h"

namespace {

constexpr int DIAG_MAX_POINTS = 4096;
constexpr int DIAG_MAX_WINDOW = 65535;    // bounds the smoothing loop: points x window additions per curve
constexpr int DIAG_REF_POINTS = 9;
enum { DG_SEEN = 0, DG_SKIPPED = 1, DG_BAD_CLASS = 2 };
enum { CH_NONE = -1, CH_DIFFICULT = -2, CH_OUT = -3 };  // a detection's choice: no candidate, a difficult ground truth, takes no part

__global__ __launch_bounds__(DET_THREADS) void det_confusion_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int max_det,
                                                                    int box_mode, const float* __restrict__ box_map, const int* __restrict__ gt,
                                                                    const int* __restrict__ gt_counts, int G, int nc, double conf, double iou,
                                                                    int quantize, unsigned long long* confusion, unsigned long long* images_per_class,
                                                                    unsigned long long* state) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const det_confusion_layout L = det_confusion_layout_of(max_det, G);
  unsigned long long* top = reinterpret_cast<unsigned long long*>(smem + L.top);
  int* gbox = reinterpret_cast<int*>(smem + L.gbox);
  int* winner = reinterpret_cast<int*>(smem + L.winner);
  int* choice = reinterpret_cast<int*>(smem + L.choice);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = counts[b], ng = gt_counts[b];
  if (det_image_refused(n, max_det, ng, G, &state[DG_SKIPPED])) return;
  if (tid == 0) atomicAdd(&state[DG_SEEN], 1ull);
  const long long stride = (long long)nc + 1;
  unsigned long long bad_class = 0;

  for (int g = tid; g < ng; g += DET_THREADS) {
    det_stage_gt(gt + ((long long)b * G + g) * 6, nc, gbox + g * 6, bad_class);
    top[g] = 0ull;
    winner[g] = 0x7fffffff;
  }
  __syncthreads();

  const det_box_map map = det_load_box_map(box_mode, box_map, b);
  // pass 1: the choice
  for (int r = tid; r < n; r += DET_THREADS) {
    const float* row = rows + ((long long)b * max_det + r) * 6;
    const float score = row[4];
    const int cls = __float2int_rz(row[5]);
    int m = CH_OUT;
    if (cls < 0 || cls >= nc) {
      ++bad_class;
    } else if (det_score_reaches(quantize ? det_quantize(score) : score, conf, quantize)) {
      const det_ibox box = det_row_box(row, box_mode, map);
      double ovmax = iou;
      m = CH_NONE;
      for (int g = 0; g < ng; ++g) {
        if (gbox[g * 6] < 0) continue;
        det_int_overlap(box, gbox + g * 6, [&](double ov) {
          if (ov > ovmax) {  // strict: above the threshold, and the lowest index keeps a tie
            ovmax = ov;
            m = g;
          }
        });
      }
      if (m >= 0) {
        if (gbox[m * 6 + 5])
          m = CH_DIFFICULT;
        else
          atomicMax(&top[m], (unsigned long long)__double_as_longlong(ovmax));
      }
    }
    choice[r] = m;
  }
  __syncthreads();
  // pass 2: of the detections that reach a ground truth's largest overlap, the lowest row
  for (int r = tid; r < n; r += DET_THREADS) {
    const int m = choice[r];
    if (m < 0) continue;
    const det_ibox box = det_row_box(rows + ((long long)b * max_det + r) * 6, box_mode, map);
    det_int_overlap(box, gbox + m * 6, [&](double ov) {
      if ((unsigned long long)__double_as_longlong(ov) == top[m]) atomicMin(&winner[m], r);
    });
  }
  __syncthreads();
  // pass 3: the counts
  for (int r = tid; r < n; r += DET_THREADS) {
    const int m = choice[r];
    if (m == CH_OUT || m == CH_DIFFICULT) continue;
    const long long cls = __float2int_rz(rows[((long long)b * max_det + r) * 6 + 5]);
    const long long truth = (m >= 0 && winner[m] == r) ? gbox[m * 6] : nc;
    atomicAdd(&confusion[cls * stride + truth], 1ull);
  }
  for (int g = tid; g < ng; g += DET_THREADS) {
    const int cls = gbox[g * 6];
    if (cls < 0 || gbox[g * 6 + 5]) continue;
    if (winner[g] == 0x7fffffff) atomicAdd(&confusion[(long long)nc * stride + cls], 1ull);
    bool first = true;  // the image counts once per class: at the first non-difficult ground truth of it
    for (int e = 0; e < g && first; ++e) first = gbox[e * 6] != cls || gbox[e * 6 + 5];
    if (first) atomicAdd(&images_per_class[cls], 1ull);
  }
  if (bad_class) atomicAdd(&state[DG_BAD_CLASS], bad_class);
}

// layout of cvx_det_conf_curves' output, in 8-byte words
struct diag_layout {
  long long prec, rec, f1, mean, smooth, mr9, best, words;
};
__host__ __device__ inline diag_layout det_diag_layout(int nc, int P) {
  diag_layout o;
  const long long plane = (long long)nc * P;
  o.prec = 0;
  o.rec = plane;
  o.f1 = 2 * plane;
  o.mean = 3 * plane;
  o.smooth = o.mean + P;
  o.mr9 = o.smooth + P;
  o.best = o.mr9 + (long long)nc * DIAG_REF_POINTS;
  o.words = o.best + nc + 1;
  return o;
}

__global__ __launch_bounds__(DET_THREADS) void det_curves_kernel(const float* __restrict__ score, const double* __restrict__ prec,
                                                                 const double* __restrict__ rec, const int* __restrict__ flag,
                                                                 const long long* __restrict__ seg_off, const unsigned long long* __restrict__ images_per_class,
                                                                 int nc, int quantize, int P, const double* __restrict__ ref_points, double* out) {
#pragma clang fp contract(off)
  __shared__ unsigned long long sbuf[DET_THREADS];
  __shared__ unsigned long long below[DIAG_REF_POINTS];
  const int c = blockIdx.x, tid = threadIdx.x;
  const long long lo = seg_off[c], hi = seg_off[c + 1], n = hi - lo;
  const diag_layout at = det_diag_layout(nc, P);

  for (int k = tid; k < P; k += DET_THREADS) {
    const double x = (double)k / (double)(P - 1);
    long long a = 0, z = n;  // the first record that does not reach x: the scores descend
    while (a < z) {
      const long long mid = (a + z) >> 1;
      if (det_score_reaches(score[lo + mid], x, quantize))
        a = mid + 1;
      else
        z = mid;
    }
    double p = 1.0, r = 0.0, f1 = 0.0;
    if (a > 0) {
      p = prec[lo + a - 1];
      r = rec[lo + a - 1];
      const double s = p + r;
      f1 = r * p * 2 / (s == 0.0 ? 1.0 : s);
    }
    out[at.prec + (long long)c * P + k] = p;
    out[at.rec + (long long)c * P + k] = r;
    out[at.f1 + (long long)c * P + k] = f1;
  }

  // miss rates: fp_cum / n_img never falls along the records, so the records at or below a reference point are a prefix; count them
  if (tid < DIAG_REF_POINTS) below[tid] = 0ull;
  double ref[DIAG_REF_POINTS];
  for (int i = 0; i < DIAG_REF_POINTS; ++i) ref[i] = ref_points[i];
  const long long n_img = (long long)images_per_class[c];
  unsigned long long mine[DIAG_REF_POINTS] = {};
  long long fp_before = 0;
  for (long long start = lo; start < hi; start += DET_THREADS) {
    const long long i = start + tid;
    unsigned long long v = (i < hi && flag[i] == FLAG_FP) ? 1ull : 0ull;
    v = det_block_scan(v, sbuf, tid, false, [](unsigned long long a, unsigned long long x) { return a + x; });
    if (i < hi && n_img > 0) {
      const double fppi = (double)(fp_before + (long long)v) / (double)n_img;
      for (int q = 0; q < DIAG_REF_POINTS; ++q) mine[q] += fppi <= ref[q] ? 1ull : 0ull;
    }
    fp_before += (long long)sbuf[DET_THREADS - 1];
    __syncthreads();  // sbuf is rewritten by the next chunk
  }
  __syncthreads();    // `below` is cleared (a segment may be empty: no barrier in the loop then)
  for (int q = 0; q < DIAG_REF_POINTS; ++q)
    if (mine[q]) atomicAdd(&below[q], mine[q]);
  __syncthreads();
  if (tid < DIAG_REF_POINTS) {
    const long long m = (long long)below[tid];
    out[at.mr9 + (long long)c * DIAG_REF_POINTS + tid] = m > 0 ? 1.0 - rec[lo + m - 1] : 1.0;
  }
}

__global__ __launch_bounds__(DET_THREADS) void det_best_kernel(const unsigned long long* __restrict__ gt_per_class, int nc, int P, int window, double* out) {
#pragma clang fp contract(off)
  __shared__ double vbuf[DET_THREADS];
  __shared__ int ibuf[DET_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const diag_layout at = det_diag_layout(nc, P);
  const double* y = out + at.f1 + (long long)b * P;
  if (b == nc) {  // the mean over the classes with a ground truth, in ascending class
    for (int k = tid; k < P; k += DET_THREADS) {
      double sum = 0.0;
      long long classes = 0;
      for (int c = 0; c < nc; ++c)
        if (gt_per_class[c] > 0) {
          sum += out[at.f1 + (long long)c * P + k];
          ++classes;
        }
      out[at.mean + k] = classes ? sum / (double)classes : 0.0;
    }
    __threadfence_block();
    __syncthreads();  // the smoothing reads what other threads of this workgroup wrote
    y = out + at.mean;
  }
  const int half = window / 2;
  double best = -1.0;  // every value is >= 0
  int best_i = 0x7fffffff;
  for (int i = tid; i < P; i += DET_THREADS) {
    double sum = 0.0;
    for (int j = 0; j < window; ++j) {
      const int src = i - half + j;
      sum += y[src < 0 ? 0 : (src > P - 1 ? P - 1 : src)];
    }
    const double v = sum / (double)window;
    if (b == nc) out[at.smooth + i] = v;
    if (v > best) {  // ascending i: the first maximum stays
      best = v;
      best_i = i;
    }
  }
  vbuf[tid] = best;
  ibuf[tid] = best_i;
  __syncthreads();
  for (int o = DET_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const double v = vbuf[tid + o];
      const int i = ibuf[tid + o];
      if (v > vbuf[tid] || (v == vbuf[tid] && i < ibuf[tid])) {
        vbuf[tid] = v;
        ibuf[tid] = i;
      }
    }
    __syncthreads();
  }
  if (tid == 0) reinterpret_cast<long long*>(out + at.best)[b] = ibuf[0];
}

unsigned long long g_confusion_optin = 0;

}  // namespace

extern "C" int cvx_det_confusion(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, int32_t box_mode, const float* box_map,
                                 const int32_t* gt, const int32_t* gt_counts, int32_t max_gt, int32_t nc, double conf, double iou,
                                 int32_t quantize, int64_t* confusion, int64_t* images_per_class, int64_t* state, void* hip_stream) {
  CVX_TRY(det_check_batch(rows, counts, gt_counts, confusion && images_per_class && state, batch, max_det, box_mode, box_map, gt, max_gt, nc));
  CVX_CHECK(conf >= 0.0 && conf <= 1.0 && iou >= 0.0 && iou < 1.0, "conf in [0, 1], iou in [0, 1)");
  CVX_TRY(det_launch_lds(det_confusion_kernel, &g_confusion_optin, det_confusion_layout_of(max_det, max_gt).total, batch, (hipStream_t)hip_stream,
                         rows, counts, max_det, box_mode, box_map, gt, gt_counts, max_gt, nc, conf, iou, quantize, (unsigned long long*)confusion,
                         (unsigned long long*)images_per_class, (unsigned long long*)state));
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_det_conf_curves(const float* score, const double* prec, const double* rec, const int32_t* flag, const int64_t* seg_off,
                                   const int64_t* gt_per_class, const int64_t* images_per_class, int32_t nc, int32_t quantize, int32_t points,
                                   int32_t window, const double* ref_points, double* out, int64_t out_words, void* hip_stream) {
  CVX_CHECK(score && prec && rec && flag && seg_off && gt_per_class && images_per_class && ref_points && out, "null arguments");
  CVX_CHECK(nc > 0 && points >= 2 && points <= DIAG_MAX_POINTS, "nc > 0 and 2 <= points <= 4096");
  CVX_CHECK(window >= 1 && (window & 1) && window <= DIAG_MAX_WINDOW, "window: odd, 1 .. 65535");
  CVX_CHECK(out_words >= det_diag_layout(nc, points).words, "out holds fewer than 3 * nc * points + 2 * points + 10 * nc + 1 words");
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(det_curves_kernel, dim3((unsigned)nc), dim3(DET_THREADS), 0, st, score, prec, rec, flag, (const long long*)seg_off,
                     (const unsigned long long*)images_per_class, nc, quantize, points, ref_points, out);
  hipLaunchKernelGGL(det_best_kernel, dim3((unsigned)nc + 1), dim3(DET_THREADS), 0, st, (const unsigned long long*)gt_per_class, nc, points, window, out);
  CVX_HIP(hipGetLastError());
  return 0;
}
