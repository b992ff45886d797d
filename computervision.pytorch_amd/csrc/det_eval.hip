// VOC mAP evaluation of the four detectors on gfx950: detection-to-ground-truth matching per batch (cvx_det_match) and the per-class
// precision / recall / AP reduction once per evaluation (cvx_det_ap).  Nothing is read by the host between the batches.
//
// Reference semantics (file:line under the reference tree):
//   get_map                      core/metrics/mAP.py:302-834     detections of a class sorted by float(score text) descending (stable, file order
//                                                                then line order); per detection the ground truth of its class and image with
//                                                                the largest IoU (+1 pixel convention, strict >, first in file order wins a tie,
//                                                                difficult boxes included, the `used` flags ignored); IoU >= 0.5: difficult ->
//                                                                neither TP nor FP, unused -> TP (and used), used -> FP; otherwise FP
//   voc_ap                       core/metrics/mAP.py:107-148     sentinels, suffix maximum of the precision, sum over the recall change points
//   the detection writers        core/algorithms/*.py::evaluate_on_voc   "class str(score)[:6] int(l) int(t) int(r) int(b)"
//
//   K1 det_match    one workgroup per image.  Its ground truth and one (match, score) pair per detection live in LDS.  Pass 1: every
//                   detection maps its box to the original image (mode 1: (x - px) * gx, uncontracted), truncates it, quantises its score
//                   to the 4 decimals the reference's text keeps and picks its ground truth.  Because that choice ignores `used`, the
//                   sequential rule is the same as: of the detections of one image that chose ground truth g with IoU >= threshold, the TP
//                   is the first by (score descending, row ascending) -- an LDS atomic-min on that key (lds_sort.h).  Pass 2 writes the flags.  Records go
//                   to [cursor + prefix(counts)[image], ...): image order, then row order, whatever order the workgroups run in.
//   K2 det_cursor   cursor += sum(counts) (a launch of its own: K1 reads the cursor of the previous batch)
//   K3 det_ap       one workgroup per class over the records in the reference's order: chunked inclusive scans of TP and FP -> precision
//                   and recall in fp64; a second, backward sweep carries the suffix maximum and sums the change-point terms
//   K4 det_map      mean of the APs of the classes that have a non-difficult ground truth
#include "det_common.h"
#include "lds_sort.h"
#include "../../include/cvx_engine.h"

namespace {

__global__ __launch_bounds__(DET_THREADS) void det_match_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int B, int max_det,
                                                                int box_mode, const float* __restrict__ box_map, const int* __restrict__ gt,
                                                                const int* __restrict__ gt_counts, int G, int nc, double min_overlap, int quantize,
                                                                float* __restrict__ rec_score, int* __restrict__ rec_class, int* __restrict__ rec_flag,
                                                                long long capacity, unsigned long long* state, unsigned long long* gt_per_class) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const det_match_layout L = det_match_layout_of(max_det, G);
  long long* red = reinterpret_cast<long long*>(smem);  // 4 wave partials
  unsigned long long* best = reinterpret_cast<unsigned long long*>(smem + L.best);
  int* gbox = reinterpret_cast<int*>(smem + L.gbox);
  int* match = reinterpret_cast<int*>(smem + L.match);
  float* qscore = reinterpret_cast<float*>(smem + L.qscore);
  const int b = blockIdx.x, tid = threadIdx.x;

  const long long base = det_record_base(counts, b, max_det, state, red);
  const int n = counts[b], ng = gt_counts[b];
  if (det_image_refused(n, max_det, ng, G, &state[ST_OVERFLOW], base, capacity)) return;
  unsigned long long bad_class = 0, low_score = 0;

  for (int g = tid; g < ng; g += DET_THREADS) {
    const int cls = det_stage_gt(gt + ((long long)b * G + g) * 6, nc, gbox + g * 6, bad_class);
    if (cls >= 0 && !gbox[g * 6 + 5]) atomicAdd(&gt_per_class[cls], 1ull);
    best[g] = ~0ull;
  }
  __syncthreads();

  const det_box_map map = det_load_box_map(box_mode, box_map, b);
  for (int r = tid; r < n; r += DET_THREADS) {
    const float* row = rows + ((long long)b * max_det + r) * 6;
    const float score = row[4];
    int cls = __float2int_rz(row[5]);
    const det_ibox box = det_row_box(row, box_mode, map);
    if (!(score >= 1e-4f)) ++low_score;  // the reference prints these in scientific notation: rejected at the end, not emulated
    const float q = quantize ? det_quantize(score) : score;
    if (cls < 0 || cls >= nc) {
      ++bad_class;
      cls = 0;
    }
    double ovmax = -1.0;
    int m = -1;
    for (int g = 0; g < ng; ++g) {
      if (gbox[g * 6] != cls) continue;
      det_int_overlap(box, gbox + g * 6, [&](double ov) {  // boxes that do not meet are no candidate, whatever min_overlap is
        if (ov > ovmax) {
          ovmax = ov;
          m = g;
        }
      });
    }
    const unsigned long long key = score_key(q, (unsigned)r);
    if (m >= 0 && ovmax >= min_overlap) {
      if (gbox[m * 6 + 5])
        m = -2;
      else
        atomicMin(&best[m], key);
    } else {
      m = -1;
    }
    match[r] = m;
    qscore[r] = q;
    rec_score[base + r] = q;
    rec_class[base + r] = cls;
  }
  __syncthreads();
  for (int r = tid; r < n; r += DET_THREADS) {
    const int m = match[r];
    int flag = FLAG_FP;
    if (m == -2) {
      flag = FLAG_NEITHER;
    } else if (m >= 0) {
      const unsigned long long key = score_key(qscore[r], (unsigned)r);
      flag = best[m] == key ? FLAG_TP : FLAG_FP;
    }
    rec_flag[base + r] = flag;
  }
  if (bad_class) atomicAdd(&state[ST_BAD_CLASS], bad_class);
  if (low_score) atomicAdd(&state[ST_LOW_SCORE], low_score);
}

__global__ __launch_bounds__(DET_THREADS) void det_ap_kernel(const float* __restrict__ score, const int* __restrict__ flag,
                                                             const long long* __restrict__ seg_off, const unsigned long long* __restrict__ gt_per_class,
                                                             double score_threshold, int quantize, double* prec, double* rec, double* stats) {
  __shared__ unsigned long long sbuf[DET_THREADS];
  __shared__ double dbuf[DET_THREADS];
  const int c = blockIdx.x, tid = threadIdx.x;
  const long long lo = seg_off[c], hi = seg_off[c + 1], n = hi - lo;
  const long long n_gt = (long long)gt_per_class[c];
  const double gt_div = (double)(n_gt > 1 ? n_gt : 1);  // np.maximum(gt_counter_per_class, 1)

  // forward sweep: TP, FP and "score >= threshold" counts, the packed fields of det_common.h
  long long tp_before = 0, fp_before = 0, reach = 0;
  for (long long start = lo; start < hi; start += DET_THREADS) {
    const long long i = start + tid;
    unsigned long long v = 0;
    if (i < hi) {
      const int f = flag[i];
      v = det_pack3(f == FLAG_TP, f == FLAG_FP, det_score_reaches(score[i], score_threshold, quantize));
    }
    v = det_block_scan(v, sbuf, tid, false, [](unsigned long long a, unsigned long long x) { return a + x; });
    if (i < hi) {
      const long long tp = tp_before + det_field(v, 0), fp = fp_before + det_field(v, 1);
      rec[i] = (double)tp / gt_div;
      prec[i] = (double)tp / (double)(tp + fp > 1 ? tp + fp : 1);
    }
    det_add3(sbuf[DET_THREADS - 1], tp_before, fp_before, reach);
    __syncthreads();  // sbuf is rewritten by the next chunk
  }
  __threadfence_block();
  __syncthreads();  // the backward sweep reads prec / rec other threads of this workgroup wrote

  // backward sweep: mpre[i] = max(prec[i:], 0) and the sum of (mrec[i] - mrec[i-1]) * mpre[i] where the recall changes.  The closing
  // sentinel pair (recall 1, precision 0) adds (1 - rec[n-1]) * 0 and is left out.
  double later_max = 0.0, ap = 0.0;
  const long long chunks = (n + DET_THREADS - 1) / DET_THREADS;
  for (long long k = chunks - 1; k >= 0; --k) {
    const long long i = lo + k * DET_THREADS + tid;
    const bool valid = i < hi;
    double m = valid ? prec[i] : 0.0;
    m = det_block_scan(m, dbuf, tid, true, [](double a, double x) { return a > x ? a : x; });
    const double chunk_max = dbuf[DET_THREADS - 1];  // the backward scan's last slot is thread 0's: the maximum of the chunk
    __syncthreads();
    m = m > later_max ? m : later_max;
    double term = 0.0;
    if (valid) {
      const double r = rec[i], r_prev = i > lo ? rec[i - 1] : 0.0;
      if (r != r_prev) term = (r - r_prev) * m;
    }
    dbuf[tid] = term;
    __syncthreads();
    for (int o = DET_THREADS / 2; o > 0; o >>= 1) {  // fixed tree: the same bits every run
      if (tid < o) dbuf[tid] += dbuf[tid + o];
      __syncthreads();
    }
    ap += dbuf[0];
    later_max = later_max > chunk_max ? later_max : chunk_max;
    __syncthreads();
  }

  if (tid == 0) {
    // values "at the threshold": the last index whose score reaches it (scores descend), index 0 when none does
    double p = 0.0, r = 0.0, f1 = 0.0;
    if (n > 0) {
      const long long idx = lo + (reach > 0 ? reach - 1 : 0);
      p = prec[idx];
      r = rec[idx];
      const double s = p + r;
      f1 = r * p * 2 / (s == 0.0 ? 1.0 : s);
    }
    double* out = stats + (long long)c * 8;
    out[0] = ap;
    out[1] = p;
    out[2] = r;
    out[3] = f1;
    out[4] = (double)tp_before;
    out[5] = (double)n;
    out[6] = (double)n_gt;
    out[7] = 0.0;
  }
}

__global__ void det_map_kernel(const unsigned long long* __restrict__ gt_per_class, int nc, double* stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sum = 0.0;
  long long classes = 0;
  for (int c = 0; c < nc; ++c)
    if (gt_per_class[c] > 0) {
      sum += stats[(long long)c * 8];
      ++classes;
    }
  stats[(long long)nc * 8 + 0] = classes ? sum / (double)classes : 0.0;
  stats[(long long)nc * 8 + 1] = (double)classes;
}

unsigned long long g_match_optin = 0;

}  // namespace

extern "C" int cvx_det_match(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, int32_t box_mode, const float* box_map,
                             const int32_t* gt, const int32_t* gt_counts, int32_t max_gt, int32_t nc, double min_overlap, int32_t quantize,
                             float* rec_score, int32_t* rec_class, int32_t* rec_flag, int64_t capacity, int64_t* state, int64_t* gt_per_class,
                             void* hip_stream) {
  CVX_TRY(det_check_batch(rows, counts, gt_counts, rec_score && rec_class && rec_flag && state && gt_per_class, batch, max_det, box_mode, box_map, gt,
                          max_gt, nc));
  CVX_CHECK(capacity > 0, "bad sizes");
  hipStream_t st = (hipStream_t)hip_stream;
  CVX_TRY(det_launch_lds(det_match_kernel, &g_match_optin, det_match_layout_of(max_det, max_gt).total, batch, st, rows, counts, batch, max_det,
                         box_mode, box_map, gt, gt_counts, max_gt, nc, min_overlap, quantize, rec_score, rec_class, rec_flag, (long long)capacity,
                         (unsigned long long*)state, (unsigned long long*)gt_per_class));
  hipLaunchKernelGGL(det_cursor_kernel, dim3(1), dim3(DET_THREADS), 0, st, counts, batch, max_det, (long long)capacity, (unsigned long long*)state);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_det_ap(const float* score, const int32_t* flag, const int64_t* seg_off, const int64_t* gt_per_class, int32_t nc,
                          double score_threshold, int32_t quantize, double* prec, double* rec, double* stats, void* hip_stream) {
  CVX_CHECK(score && flag && seg_off && gt_per_class && prec && rec && stats, "null arguments");
  CVX_CHECK(nc > 0, "bad sizes");
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(det_ap_kernel, dim3((unsigned)nc), dim3(DET_THREADS), 0, st, score, flag, (const long long*)seg_off,
                     (const unsigned long long*)gt_per_class, score_threshold, quantize, prec, rec, stats);
  hipLaunchKernelGGL(det_map_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)gt_per_class, nc, stats);
  CVX_HIP(hipGetLastError());
  return 0;
}
