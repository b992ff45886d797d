// COCO detection metric (AP@[.5:.95], AR) of the four detectors on gfx950: pycocotools' COCOeval(gt, dt, 'bbox') -- evaluate(), accumulate(),
// summarize() -- as tests/coco_eval_restatement.py states it.  Matching once per batch (cvx_coco_match), the precision / recall tables once
// per evaluation (cvx_coco_accumulate) and the twelve means (cvx_coco_summarize).  Nothing is read by the host between the batches.
//
//   K1 coco_match   one workgroup per image.  Its ground truth lives in LDS; its rows are ordered there by (class, score descending, row) --
//                   one 64-bit key per row, the bitonic sort of lds_sort.h -- which puts every class's detections in COCOeval's order; the first 100 of a
//                   class are evaluated.  Then a wave takes one class at a time: its lanes stage the class's boxes (box map, int(), widths
//                   in fp32, then fp64), and lane a * 10 + t runs evaluateImg's greedy walk for area range a and IoU threshold t over them,
//                   IoUs computed as it goes (fp64, no contraction).  Nothing crosses lanes: the "ground truth already matched" bits and
//                   the per-detection flags are lane-private LDS.  The greedy walk never looks ahead, so maxDet = 1 / 10 are prefixes of
//                   this maxDet = 100 result: the record keeps the rank and cvx_coco_accumulate cuts.  Records go to
//                   [cursor + prefix(counts)[image], ...): image order, then row order, whatever order the workgroups run in.
//   K2 det_cursor   cursor += sum(counts) (det_common.h)
//   K3 coco_accumulate   one workgroup per (class, area range, maxDet) over the records in (class, score descending, image, row) order.
//                   Per threshold a counting sweep, then a backward sweep in chunks of 256: suffix counts give tp and fp at every record,
//                   a suffix maximum gives the precision envelope, and the record at which the recall first reaches a recall threshold
//                   writes that threshold's precision (searchsorted side='left').
//   K4 coco_summarize    the twelve means over the entries > -1, partial sums in a fixed tree order
#include "det_common.h"
#include "lds_sort.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)  // COCOeval's doubles are rounded after every operation

namespace {

constexpr int COCO_TOP = 100;             // maxDets[-1]
constexpr int COCO_T = 10, COCO_A = 4, COCO_M = 3, COCO_R = 101;
constexpr int COCO_WALKS = COCO_T * COCO_A;
constexpr int COCO_WAVES = DET_THREADS / 64;
constexpr int KEY_ROW_BITS = 14, KEY_CLS_SHIFT = 46;
constexpr int COCO_MAX_NC = (1 << (64 - KEY_CLS_SHIFT)) - 2;

__host__ __device__ inline double coco_area_lo(int a) { return a == 2 ? 1024.0 : a == 3 ? 9216.0 : 0.0; }
__host__ __device__ inline double coco_area_hi(int a) { return a == 1 ? 1024.0 : a == 2 ? 9216.0 : 1e10; }

struct CocoLds {
  int P, S, W;  // sort slots (a power of two), segment slots, mask words per walk
  size_t keys, gbox, gcls, gcrowd, seg, dbox, dflag, gmask, total;
};
inline int coco_pow2(int v) {
  int p = 2;
  while (p < v) p <<= 1;
  return p;
}
__host__ __device__ inline CocoLds coco_lds(int P, int G, int nc) {
  CocoLds l;
  l.P = P;
  l.S = ((P < nc ? P : nc) + 1) & ~1;
  l.W = (G + 31) / 32 + ((G + 31) / 32 == 0);
  const int Gs = det_gt_slots(G);
  l.keys = 48;  // 4 wave partials, the segment counter
  l.gbox = l.keys + (size_t)8 * P;
  l.gcls = l.gbox + (size_t)40 * Gs;
  l.gcrowd = l.gcls + (size_t)4 * Gs;
  l.seg = l.gcrowd + (size_t)4 * Gs;
  l.dbox = l.seg + (size_t)4 * l.S;
  l.dflag = l.dbox + (size_t)COCO_WAVES * COCO_TOP * 40;
  l.gmask = l.dflag + (size_t)COCO_WAVES * COCO_TOP * COCO_WALKS;
  l.total = l.gmask + (size_t)COCO_WAVES * COCO_WALKS * l.W * 4;
  return l;
}

// first position in keys[0, n) whose key is >= bound
__device__ __forceinline__ int coco_lower_bound(const unsigned long long* keys, int n, unsigned long long bound) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < bound)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// maskApi's bbIou for one pair: d and g are [x, y, w, h, area]
__device__ __forceinline__ double coco_iou(const double* d, const double* g, bool crowd) {
  const double w = fmin(d[0] + d[2], g[0] + g[2]) - fmax(d[0], g[0]);
  if (w <= 0) return 0.0;
  const double h = fmin(d[1] + d[3], g[1] + g[3]) - fmax(d[1], g[1]);
  if (h <= 0) return 0.0;
  const double i = w * h;
  const double u = crowd ? d[2] * d[3] : d[2] * d[3] + g[2] * g[3] - i;
  return i / u;
}

__global__ __launch_bounds__(DET_THREADS) void coco_match_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int B, int max_det,
                                                                 int P, int box_mode, const float* __restrict__ box_map, int truncate, int quantize,
                                                                 const double* __restrict__ gt, const int* __restrict__ gt_counts, int G, int nc,
                                                                 const double* __restrict__ iou_thrs, float* __restrict__ rec_score,
                                                                 int* __restrict__ rec_class, int* __restrict__ rec_rank,
                                                                 unsigned long long* __restrict__ rec_matched,
                                                                 unsigned long long* __restrict__ rec_ignored, long long capacity,
                                                                 unsigned long long* state, unsigned long long* npig) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const CocoLds L = coco_lds(P, G, nc);
  long long* red = reinterpret_cast<long long*>(smem);
  int* nseg = reinterpret_cast<int*>(smem + 32);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + L.keys);
  double* gbox = reinterpret_cast<double*>(smem + L.gbox);     // [x, y, w, h, area] per ground truth
  int* gcls = reinterpret_cast<int*>(smem + L.gcls);
  int* gcrowd = reinterpret_cast<int*>(smem + L.gcrowd);
  int* seg = reinterpret_cast<int*>(smem + L.seg);              // first sorted position of every class present
  double* dbox = reinterpret_cast<double*>(smem + L.dbox);     // per wave: [x, y, w, h, area] of the class's first 100 detections
  unsigned char* dflag = reinterpret_cast<unsigned char*>(smem + L.dflag);  // per wave, detection and walk: matched | ignored << 1
  unsigned* gmask = reinterpret_cast<unsigned*>(smem + L.gmask);            // per wave and walk: ground truths matched so far
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  if (tid == 0) *nseg = 0;  // ahead of det_record_base: its barrier publishes this store
  const long long base = det_record_base(counts, b, max_det, state, red);
  const int n = counts[b], ng = gt_counts[b];
  if (det_image_refused(n, max_det, ng, G, &state[ST_OVERFLOW], base, capacity)) return;
  unsigned long long bad_class = 0, low_score = 0;

  for (int g = tid; g < ng; g += DET_THREADS) {
    const double* src = gt + ((long long)b * G + g) * 7;
    int cls = (int)src[0];
    const int crowd = src[6] != 0.0;
    const double area = src[5];
    if (!(src[0] >= 0.0 && src[0] < (double)nc)) {
      ++bad_class;
      cls = -1;  // matches no detection
    } else {
      for (int a = 0; a < COCO_A; ++a)
        if (!(crowd || area < coco_area_lo(a) || area > coco_area_hi(a))) atomicAdd(&npig[(long long)cls * COCO_A + a], 1ull);
    }
    gcls[g] = cls;
    gcrowd[g] = crowd;
    gbox[g * 5 + 0] = src[1];
    gbox[g * 5 + 1] = src[2];
    gbox[g * 5 + 2] = src[3];
    gbox[g * 5 + 3] = src[4];
    gbox[g * 5 + 4] = area;
  }

  // one key per row: class, inverted score bits, row -- ascending = COCOeval's order inside every class
  for (int r = tid; r < P; r += DET_THREADS) {
    unsigned long long key = ~0ull;
    if (r < n) {
      const float* row = rows + ((long long)b * max_det + r) * 6;
      const float score = row[4];
      int cls = __float2int_rz(row[5]);
      if (quantize ? !(score >= 1e-4f) : !(score >= 0.f)) ++low_score;  // quantised: as cvx_det_match; otherwise a score the key cannot order
      const float q = quantize ? det_quantize(score) : score;
      if (cls < 0 || cls >= nc) {
        ++bad_class;
        cls = 0;
      }
      key = ((unsigned long long)cls << KEY_CLS_SHIFT) | ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(q)) << KEY_ROW_BITS) | (unsigned)r;
    }
    keys[r] = key;
  }
  lds_sort_keys<DET_THREADS>(keys, P);  // P is a power of two: nothing is padded

  // score, class and rank of every record; the records past a class's first 100 take part in nothing
  for (int i = tid; i < n; i += DET_THREADS) {
    const unsigned long long key = keys[i];
    const int cls = (int)(key >> KEY_CLS_SHIFT), row = (int)(key & ((1u << KEY_ROW_BITS) - 1));
    const int rank = i - coco_lower_bound(keys, n, (unsigned long long)cls << KEY_CLS_SHIFT);
    rec_score[base + row] = __uint_as_float(0xFFFFFFFFu - (unsigned)((key >> KEY_ROW_BITS) & 0xFFFFFFFFu));
    rec_class[base + row] = cls;
    rec_rank[base + row] = rank;
    if (rank >= COCO_TOP) {
      rec_matched[base + row] = 0ull;
      rec_ignored[base + row] = 0ull;
    }
    if (rank == 0) seg[atomicAdd(nseg, 1)] = i;
  }
  __syncthreads();

  const det_box_map map = det_load_box_map(box_mode, box_map, b);
  const int segments = *nseg;
  double* my_dbox = dbox + (size_t)wave * COCO_TOP * 5;
  unsigned char* my_dflag = dflag + (size_t)wave * COCO_TOP * COCO_WALKS;
  for (int s_base = 0; s_base < segments; s_base += COCO_WAVES) {  // the same trip count in every wave: the barriers below are workgroup-wide
    const bool active = s_base + wave < segments;
    int s0 = 0, cls = 0, D = 0;
    if (active) {
      s0 = seg[s_base + wave];
      cls = (int)(keys[s0] >> KEY_CLS_SHIFT);
      D = coco_lower_bound(keys, n, (unsigned long long)(cls + 1) << KEY_CLS_SHIFT) - s0;
      D = D < COCO_TOP ? D : COCO_TOP;
    }
    for (int dl = lane; dl < D; dl += 64) {
      const int r = (int)(keys[s0 + dl] & ((1u << KEY_ROW_BITS) - 1));
      const float* row = rows + ((long long)b * max_det + r) * 6;
      float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
      if (box_mode == 1) det_undo_letterbox(x1, y1, x2, y2, map);
      if (truncate) {  // the VOC writers' int(): towards zero
        x1 = truncf(x1);
        y1 = truncf(y1);
        x2 = truncf(x2);
        y2 = truncf(y2);
      }
      const double w = (double)__fsub_rn(x2, x1), h = (double)__fsub_rn(y2, y1);  // float(right - left) on numpy float32
      my_dbox[dl * 5 + 0] = (double)x1;
      my_dbox[dl * 5 + 1] = (double)y1;
      my_dbox[dl * 5 + 2] = w;
      my_dbox[dl * 5 + 3] = h;
      my_dbox[dl * 5 + 4] = w * h;
    }
    __syncthreads();
    if (active && lane < COCO_WALKS) {
      const int a = lane / COCO_T, t = lane % COCO_T;
      const double lo = coco_area_lo(a), hi = coco_area_hi(a);
      const double thr = fmin(iou_thrs[t], 1 - 1e-10);
      unsigned* matched = gmask + (size_t)(wave * COCO_WALKS + lane) * L.W;
      for (int w = 0; w < L.W; ++w) matched[w] = 0u;
      for (int dl = 0; dl < D; ++dl) {
        const double* d = my_dbox + dl * 5;
        double iou = thr;
        int m = -1;
        // the ground truths sorted by _ignore: the kept ones in order, then the ignored ones -- which evaluateImg leaves ("break") once a
        // kept one is matched
        for (int ignored_pass = 0; ignored_pass < 2 && m < 0; ++ignored_pass)
          for (int g = 0; g < ng; ++g) {
            if (gcls[g] != cls) continue;
            const bool crowd = gcrowd[g] != 0;
            const double ga = gbox[g * 5 + 4];
            if ((int)(crowd || ga < lo || ga > hi) != ignored_pass) continue;
            if (((matched[g >> 5] >> (g & 31)) & 1u) && !crowd) continue;
            const double v = coco_iou(d, gbox + g * 5, crowd);
            if (v < iou) continue;
            iou = v;
            m = g;
          }
        unsigned flag;
        if (m < 0) {
          flag = (d[4] < lo || d[4] > hi) ? 2u : 0u;
        } else {
          const double ga = gbox[m * 5 + 4];
          flag = 1u | ((gcrowd[m] != 0 || ga < lo || ga > hi) ? 2u : 0u);
          matched[m >> 5] |= 1u << (m & 31);
        }
        my_dflag[dl * COCO_WALKS + lane] = (unsigned char)flag;
      }
    }
    __syncthreads();
    for (int dl = lane; dl < D; dl += 64) {
      unsigned long long mm = 0, ig = 0;
      for (int w = 0; w < COCO_WALKS; ++w) {
        const unsigned f = my_dflag[dl * COCO_WALKS + w];
        mm |= (unsigned long long)(f & 1u) << w;
        ig |= (unsigned long long)((f >> 1) & 1u) << w;
      }
      const int r = (int)(keys[s0 + dl] & ((1u << KEY_ROW_BITS) - 1));
      rec_matched[base + r] = mm;
      rec_ignored[base + r] = ig;
    }
  }
  if (bad_class) atomicAdd(&state[ST_BAD_CLASS], bad_class);
  if (low_score) atomicAdd(&state[ST_LOW_SCORE], low_score);
}

// ---- cvx_coco_accumulate -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DET_THREADS) void coco_accumulate_kernel(const int* __restrict__ rank, const unsigned long long* __restrict__ matched,
                                                                      const unsigned long long* __restrict__ ignored,
                                                                      const long long* __restrict__ seg_off,
                                                                      const unsigned long long* __restrict__ npig_all, int nc,
                                                                      const double* __restrict__ rec_thrs, double* precision, double* recall) {
  __shared__ unsigned long long sbuf[DET_THREADS];
  __shared__ double dbuf[DET_THREADS];
  __shared__ double rthr[COCO_R];
  const int k = blockIdx.x / (COCO_A * COCO_M), a = (blockIdx.x / COCO_M) % COCO_A, m = blockIdx.x % COCO_M, tid = threadIdx.x;
  const int max_det = m == 0 ? 1 : m == 1 ? 10 : COCO_TOP;
  const long long lo = seg_off[k], hi = seg_off[k + 1], n = hi - lo;
  const long long npig = (long long)npig_all[(long long)k * COCO_A + a];
  const auto p_at = [&](int t, int r) { return ((((long long)t * COCO_R + r) * nc + k) * COCO_A + a) * COCO_M + m; };
  const auto r_at = [&](int t) { return (((long long)t * nc + k) * COCO_A + a) * COCO_M + m; };

  const double fill = npig == 0 ? -1.0 : 0.0;
  for (int i = tid; i < COCO_T * COCO_R; i += DET_THREADS) precision[p_at(i / COCO_R, i % COCO_R)] = fill;
  if (npig == 0) {
    if (tid < COCO_T) recall[r_at(tid)] = -1.0;
    return;
  }
  for (int i = tid; i < COCO_R; i += DET_THREADS) rthr[i] = rec_thrs[i];
  __syncthreads();  // the zeros above are in place before another thread writes a precision over one of them

  const auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
  const long long chunks = (n + DET_THREADS - 1) / DET_THREADS;
  for (int t = 0; t < COCO_T; ++t) {
    const int bit = a * COCO_T + t;
    // what record i adds: tp, fp and kept, the packed fields of det_common.h
    const auto term = [&](long long i) -> unsigned long long {
      if (i >= hi || rank[i] >= max_det) return 0ull;
      const unsigned long long mt = (matched[i] >> bit) & 1ull, ig = (ignored[i] >> bit) & 1ull;
      return det_pack3(mt & ~ig & 1ull, ~mt & ~ig & 1ull, 1ull);
    };
    long long tp_all = 0, fp_all = 0, kept_all = 0;
    for (long long start = lo; start < hi; start += DET_THREADS) {
      det_block_scan(term(start + tid), sbuf, tid, false, add);
      det_add3(sbuf[DET_THREADS - 1], tp_all, fp_all, kept_all);
      __syncthreads();  // sbuf is rewritten by the next chunk
    }
    if (tid == 0) recall[r_at(t)] = kept_all ? (double)tp_all / (double)npig : 0.0;

    long long tp_after = 0, fp_after = 0, kept_after = 0;
    double later_max = 0.0;
    for (long long c = chunks - 1; c >= 0; --c) {
      const long long i = lo + c * DET_THREADS + tid;
      const unsigned long long v = term(i);
      const bool valid = det_field(v, 2) != 0;
      const long long tpb = det_field(v, 0);
      const unsigned long long sfx = det_block_scan(v, sbuf, tid, true, add);  // this record and the later ones of the chunk
      const unsigned long long chunk = sbuf[DET_THREADS - 1];                  // the backward scan's last slot is thread 0's
      __syncthreads();
      const long long tp = tp_all - tp_after - (det_field(sfx, 0) - tpb);
      const long long fp = fp_all - fp_after - (det_field(sfx, 1) - det_field(v, 1));
      const long long kept = kept_all - kept_after - (det_field(sfx, 2) - 1);
      const double pr = valid ? (double)tp / (((double)fp + (double)tp) + 0x1p-52) : 0.0;  // np.spacing(1)
      double env = det_block_scan(pr, dbuf, tid, true, [](double x, double y) { return x > y ? x : y; });
      const double chunk_max = dbuf[DET_THREADS - 1];
      __syncthreads();
      env = env > later_max ? env : later_max;
      const bool first = kept == 1;
      if (valid && (tpb || first)) {  // the recall rises here: this record is searchsorted's answer for the thresholds it newly reaches
        const double rc = (double)tp / (double)npig, rc_prev = (double)(tp - tpb) / (double)npig;
        int ri = first ? 0 : (int)(rc_prev * 100.0) - 1;
        for (ri = ri < 0 ? 0 : ri; ri < COCO_R && rthr[ri] <= rc; ++ri)
          if (first || rthr[ri] > rc_prev) precision[p_at(t, ri)] = env;
      }
      det_add3(chunk, tp_after, fp_after, kept_after);
      later_max = later_max > chunk_max ? later_max : chunk_max;
    }
  }
}

// ---- cvx_coco_summarize ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DET_THREADS) void coco_summarize_kernel(const double* __restrict__ precision, const double* __restrict__ recall, int nc,
                                                                     double* stats) {
  __shared__ double sum[DET_THREADS];
  __shared__ long long cnt[DET_THREADS];
  const int tid = threadIdx.x;
  for (int s = 0; s < 12; ++s) {
    // pycocotools' order: AP, AP50, AP75, APs, APm, APl (maxDets 100); AR1, AR10, AR100, ARs, ARm, ARl
    const bool ap = s < 6;
    const int t0 = s == 1 ? 0 : s == 2 ? 5 : 0, t1 = s == 1 ? 1 : s == 2 ? 6 : COCO_T;
    const int a = ap ? (s >= 3 ? s - 2 : 0) : (s >= 9 ? s - 8 : 0);
    const int m = ap ? 2 : (s == 6 ? 0 : s == 7 ? 1 : 2);
    const long long inner = ap ? (long long)COCO_R * nc : nc, total = (t1 - t0) * inner;
    double part = 0.0;
    long long valid = 0;
    for (long long i = tid; i < total; i += DET_THREADS) {
      const long long t = t0 + i / inner, rest = i % inner;  // rest = r * nc + k for the precision, k for the recall
      const double v = ap ? precision[((t * COCO_R * nc + rest) * COCO_A + a) * COCO_M + m] : recall[((t * nc + rest) * COCO_A + a) * COCO_M + m];
      if (v > -1.0) {
        part += v;
        ++valid;
      }
    }
    sum[tid] = part;
    cnt[tid] = valid;
    __syncthreads();
    for (int o = DET_THREADS / 2; o > 0; o >>= 1) {  // fixed tree: the same bits every run
      if (tid < o) {
        sum[tid] += sum[tid + o];
        cnt[tid] += cnt[tid + o];
      }
      __syncthreads();
    }
    if (tid == 0) stats[s] = cnt[0] ? sum[0] / (double)cnt[0] : -1.0;
    __syncthreads();
  }
}

unsigned long long g_coco_optin = 0;

}  // namespace

extern "C" int cvx_coco_match(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, int32_t box_mode, const float* box_map,
                              int32_t truncate, int32_t quantize, const double* gt, const int32_t* gt_counts, int32_t max_gt, int32_t nc,
                              const double* iou_thrs, float* rec_score, int32_t* rec_class, int32_t* rec_rank, int64_t* rec_matched,
                              int64_t* rec_ignored, int64_t capacity, int64_t* state, int64_t* npig, void* hip_stream) {
  CVX_TRY(det_check_batch(rows, counts, gt_counts, iou_thrs && rec_score && rec_class && rec_rank && rec_matched && rec_ignored && state && npig,
                          batch, max_det, box_mode, box_map, gt, max_gt, nc));
  CVX_CHECK(nc <= COCO_MAX_NC && capacity > 0, "bad sizes");
  const int P = coco_pow2(max_det);
  hipStream_t st = (hipStream_t)hip_stream;
  CVX_TRY(det_launch_lds(coco_match_kernel, &g_coco_optin, coco_lds(P, max_gt, nc).total, batch, st, rows, counts, batch, max_det, P, box_mode,
                         box_map, truncate, quantize, gt, gt_counts, max_gt, nc, iou_thrs, rec_score, rec_class, rec_rank,
                         (unsigned long long*)rec_matched, (unsigned long long*)rec_ignored, (long long)capacity, (unsigned long long*)state,
                         (unsigned long long*)npig));
  hipLaunchKernelGGL(det_cursor_kernel, dim3(1), dim3(DET_THREADS), 0, st, counts, batch, max_det, (long long)capacity, (unsigned long long*)state);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_coco_accumulate(const int32_t* rank, const int64_t* matched, const int64_t* ignored, const int64_t* seg_off, const int64_t* npig,
                                   int32_t nc, const double* rec_thrs, double* precision, double* recall, void* hip_stream) {
  CVX_CHECK(rank && matched && ignored && seg_off && npig && rec_thrs && precision && recall, "null arguments");
  CVX_CHECK(nc > 0 && nc <= COCO_MAX_NC, "bad sizes");
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)nc * COCO_A * COCO_M), dim3(DET_THREADS), 0, st, rank, (const unsigned long long*)matched,
                     (const unsigned long long*)ignored, (const long long*)seg_off, (const unsigned long long*)npig, nc, rec_thrs, precision, recall);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_coco_summarize(const double* precision, const double* recall, int32_t nc, double* stats, void* hip_stream) {
  CVX_CHECK(precision && recall && stats, "null arguments");
  CVX_CHECK(nc > 0 && nc <= COCO_MAX_NC, "bad sizes");
  hipLaunchKernelGGL(coco_summarize_kernel, dim3(1), dim3(DET_THREADS), 0, (hipStream_t)hip_stream, precision, recall, nc, stats);
  CVX_HIP(hipGetLastError());
  return 0;
}
