// Multi-object tracking on gfx950: cvx_track_update gives every detection row of a batch of video frames a track
// id, with the tracker's state in device memory and nothing read by the host.  The rules are stated in include/cvx_engine.h and restated
// in numpy in tests/track_restatement.py; this file is held to the restatement bit for bit.
//
//   One workgroup of 1024 threads per stream walks the stream's frames in batch order.  Thread t holds track slot t in registers for the
//   whole batch (id, hits, miss, cls, p, v); what the other threads read of it -- the predicted box, class, id and its match -- is in LDS.
//   The rows of a frame are staged in LDS (box, class) when there are at most DET_LDS of them and read from global memory otherwise; the
//   per-row state (unmatched high / unmatched low / ignored / matched slot) lives beside them, or in the frame's out_ids row, which is
//   rewritten with the ids at the end of the frame.  The two cases are two instantiations of the frame's body (Dets<STAGED>), so the
//   staged one reads LDS with LDS instructions.
//   Association: the greedy walk over the pairs sorted by (IoU desc, track id asc, row asc) is run as rounds without a sort.  The key is
//   a strict total order, so a pair that is both its track's best and its row's best among the unmatched is exactly a pair the sorted walk
//   takes; a round matches every such pair, and the rounds end when one matches nothing (__syncthreads_or).  Phase A: a thread per track
//   scans the rows; phase B: a thread per row scans the tracks and takes the pair when it is mutual.  IoUs are recomputed on the fly
//   (box_overlap.h:iou_value, always (track, row) in that order).  A scan is a chain of dependent instructions in a few waves, so it is
//   cut into parts over the idle threads and folded in key order (associate).
//   Deletions compact the table in slot order through LDS (ballot scan), births are appended in row order (ballot scan over the rows).
// Latency-bound: a frame is a few dozen barriers; no bandwidth to speak of.  Every fp32 step is one rounded operation: contraction is off.
//
//   cvx_track_update_model: the motion model and the association are compile-time choices of the frame's body
//   (track_frame<STAGED, MOTION, ASSIGN>), so track_kernel -- alpha-beta, greedy -- is the instance it was.  Under the Kalman model thread t
//   also keeps the slot's covariance (Pxx, Pxv, Pvv), loaded from and stored to the stream's extension block, and the compaction carries it
//   along.  The optimal association (assign_optimal) counts the allowed rows of every candidate track and the allowed tracks of every
//   candidate row with the split scans of the greedy rounds, takes the pairs that are alone on both sides, compacts what is left through
//   ballot scans into two index maps in LDS and runs assign_solver.h:solve on it, the cost of a cell recomputed from the boxes through the
//   maps: one column per lane up to 1024 columns, four up to 4096.
#include "assign_solver.h"
#include "box_overlap.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int CAP = CVX_TRACK_CAP;
constexpr int THREADS = 1024;   // one thread per track slot
constexpr int WAVES = THREADS / 64;
constexpr int DET_LDS = 1024;   // rows of a frame staged in LDS; their boxes' bytes then carry the velocities through the compaction
constexpr int MAX_OPT = CVX_TRACK_OPTIMAL_MAX_DET;        // rows of a frame under the optimal association: four columns per lane
enum { DET_HIGH = -1, DET_LOW = -2, DET_IGNORED = -3 };   // per-row state; >= 0: the slot of the matched track
enum { TRK_OPEN = -1, TRK_OUT = -2 };                     // per-track match; >= 0: the matched row
enum { AB = CVX_TRACK_MOTION_ALPHA_BETA, KALMAN = CVX_TRACK_MOTION_KALMAN, GREEDY = CVX_TRACK_ASSIGN_GREEDY, OPTIMAL = CVX_TRACK_ASSIGN_OPTIMAL };

static_assert(THREADS == CAP, "thread t owns slot t");
static_assert(THREADS == SOLVE_THREADS && MAX_OPT == 4 * THREADS, "the solver's workgroup; a lane owns up to four columns");
static_assert(DET_LDS >= CAP, "the staging area holds one float4 per slot");
constexpr int LDS_BYTES = (CAP + DET_LDS) * 16 + (2 * CAP + 2 * DET_LDS + 2 * THREADS + 3 * CAP) * 4 + WAVES * 4;
// the model kernels add the solver (u 8 KB, p and way 16 KB each, the reduction cells) and the two index maps (4 KB and 16 KB); the row
// map's bytes carry the covariances through the compaction
constexpr int MODEL_LDS_BYTES = LDS_BYTES + CAP * 8 + 2 * MAX_OPT * 4 + 2 * WAVES * 16 + CAP * 4 + MAX_OPT * 4;
static_assert(LDS_BYTES % 16 == 0 && MAX_OPT * 4 >= CAP * 16, "the solver's potentials are 8-byte aligned; one float4 per slot in the row map");
static_assert(MODEL_LDS_BYTES <= 160 * 1024, "one workgroup's LDS on gfx950");

struct Shared {
  float4* tp;     // predicted box
  float* tcls;
  int* tid;       // track id
  int* tm;        // match (TRK_*)
  int* tbest;     // phase A's choice of the round
  int* tnew;      // phase B's matches of the round; the rows of the births
  float* piou;    // a scan's parts: the best IoU and its row (phase A) or slot (phase B), by thread
  int* pidx;
};

__device__ __forceinline__ float4 det_box(const float* rows, int d) {
  const float* r = rows + 6 * (long long)d;
  return make_float4(r[0], r[1], r[2], r[3]);
}

// the rows of one frame as the association sees them: in LDS, or in global memory with the state in the frame's ids row
template <bool STAGED>
struct Dets {
  const float4* lbox;   // LDS
  const float* lcls;
  int* lstate;
  const float* rows;    // global: the frame's (max_det, 6) block and its out_ids row
  int* ids;
  __device__ __forceinline__ float4 box(int d) const { return STAGED ? lbox[d] : det_box(rows, d); }
  __device__ __forceinline__ float cls(int d) const { return STAGED ? lcls[d] : rows[6 * (long long)d + 5]; }
  __device__ __forceinline__ int state(int d) const { return STAGED ? lstate[d] : ids[d]; }
  __device__ __forceinline__ void set_state(int d, int v) const {
    if (STAGED) lstate[d] = v;
    else ids[d] = v;
  }
};

// inclusive-exclusive rank of `flag` over the workgroup in thread order, and the total; two barriers
__device__ __forceinline__ int block_rank(bool flag, int* wave_tot, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) wave_tot[wave] = __popcll(m);
  __syncthreads();
  int pos = __popcll(m & ((1ull << lane) - 1ull)), sum = 0;
  for (int k = 0; k < WAVES; ++k) {
    const int c = wave_tot[k];
    if (k < wave) pos += c;
    sum += c;
  }
  *total = sum;
  __syncthreads();
  return pos;
}

// one association stage: rows in state `code` against the tracks whose match is TRK_OPEN, IoU above thr.  A scan by one thread per track
// (or row) leaves most of the workgroup idle and is bound by the latency of its own dependent instructions, so a scan is cut into parts:
// with TS = nT rounded up to whole waves, thread (g, t) = (tid / TS, tid % TS) scans part g of the rows for track t, and the thread of
// part 0 folds the parts in ascending order, which keeps the order of the key.  Phase B does the same over the tracks when the rows are
// staged (n <= 1024).
template <bool STAGED>
__device__ __forceinline__ void associate(const Shared& s, const Dets<STAGED>& det, int code, float thr, bool agnostic, int nT, int n) {
  const int tid = threadIdx.x;
  const int TS = (nT + 63) & ~63, DS = (n + 63) & ~63;
  const int PA = TS ? THREADS / TS : 1, PB = (STAGED && DS) ? THREADS / DS : 1;
  const int ga = TS ? tid / TS : 0, ta = tid - ga * TS;
  const int gb = (STAGED && DS) ? tid / DS : 0, db = tid - gb * DS;
  const int chunk_a = (n + PA - 1) / PA, chunk_b = (nT + PB - 1) / PB;
  for (;;) {
    // A: the best open row of each open track -- IoU descending, row ascending (strict > while walking up)
    {
      int bd = -1;
      float best = thr;
      if (ga < PA && ta < nT && s.tm[ta] == TRK_OPEN) {
        const float4 p = s.tp[ta];
        const float ap = box_area(p), cls = s.tcls[ta];
        const int d1 = min(n, (ga + 1) * chunk_a);
#pragma unroll 4
        for (int d = ga * chunk_a; d < d1; ++d) {
          const int st = det.state(d);
          const float dc = det.cls(d);
          const float4 z = det.box(d);
          const float o = iou_value(p, ap, z, box_area(z));
          if (st == code && (agnostic || dc == cls) && o > best) {
            best = o;
            bd = d;
          }
        }
      }
      s.piou[tid] = best;
      s.pidx[tid] = bd;
      __syncthreads();
      if (tid < nT) {
        bd = -1, best = thr;
        for (int g = 0; g < PA; ++g) {
          const int e = s.pidx[g * TS + tid];
          const float o = s.piou[g * TS + tid];
          if (e >= 0 && o > best) {
            best = o;
            bd = e;
          }
        }
      }
      s.tbest[tid] = tid < nT ? bd : -1;
      __syncthreads();
    }
    // B: the best open track of each open row -- IoU descending, track id ascending; taken when the track chose this row too
    int any = 0;
    if (STAGED) {
      int bt = -1, bid = 0;
      float best = thr;
      if (gb < PB && db < n && det.state(db) == code) {
        const float4 z = det.box(db);
        const float az = box_area(z), dc = det.cls(db);
        const int t1 = min(nT, (gb + 1) * chunk_b);
#pragma unroll 4
        for (int t = gb * chunk_b; t < t1; ++t) {
          const int m = s.tm[t], ti = s.tid[t];
          const float tc = s.tcls[t];
          const float4 q = s.tp[t];
          const float o = iou_value(q, box_area(q), z, az);
          if (m == TRK_OPEN && (agnostic || tc == dc) && (o > best || (bt >= 0 && o == best && ti < bid))) {
            best = o;
            bt = t;
            bid = ti;
          }
        }
      }
      s.piou[tid] = best;
      s.pidx[tid] = bt;
      __syncthreads();
      if (tid < n && det.state(tid) == code) {
        bt = -1, best = thr, bid = 0;
        for (int g = 0; g < PB; ++g) {
          const int e = s.pidx[g * DS + tid];
          const float o = s.piou[g * DS + tid];
          if (e >= 0 && (o > best || (bt >= 0 && o == best && s.tid[e] < bid))) {
            best = o;
            bt = e;
            bid = s.tid[e];
          }
        }
        if (bt >= 0 && s.tbest[bt] == tid) {
          det.set_state(tid, bt);
          s.tnew[bt] = tid;
          any = 1;
        }
      }
    } else {
      for (int d = tid; d < n; d += THREADS) {
        if (det.state(d) != code) continue;
        const float4 z = det.box(d);
        const float az = box_area(z), dc = det.cls(d);
        int bt = -1, bid = 0;
        float best = thr;
#pragma unroll 4
        for (int t = 0; t < nT; ++t) {
          const int m = s.tm[t], ti = s.tid[t];
          const float tc = s.tcls[t];
          const float4 q = s.tp[t];
          const float o = iou_value(q, box_area(q), z, az);
          if (m == TRK_OPEN && (agnostic || tc == dc) && (o > best || (bt >= 0 && o == best && ti < bid))) {
            best = o;
            bt = t;
            bid = ti;
          }
        }
        if (bt >= 0 && s.tbest[bt] == d) {
          det.set_state(d, bt);
          s.tnew[bt] = d;
          any = 1;
        }
      }
    }
    any = __syncthreads_or(any);
    const int m = s.tnew[tid];   // tm changes only here, between the rounds' scans
    if (m >= 0) {
      s.tm[tid] = m;
      s.tnew[tid] = -1;
    }
    if (!any) break;
    __syncthreads();             // the next round's scans read tm of other slots
  }
}

struct Track {   // slot threadIdx.x, in registers
  int id, hits, miss;
  float cls;
  float4 p, v;
  float pxx, pxv, pvv;   // the Kalman model's covariance of (position, velocity), one for the four coordinates
};

struct Stream {   // uniform over the workgroup
  int frame, next_id, n_tracks;
};

struct Lds {
  Shared s;
  float4* dbox;   // the staged rows; the velocities during the compaction
  float* dcls;
  int* dstate;
  int* wave;
  // the model kernels only
  Solver sv;
  int* tmap;      // the slots of the tracks the solver assigns, in slot order
  int* rmap;      // the rows it assigns, in row order; the covariances during the compaction
};

// the cost of a cell of the solver's matrix, recomputed from the boxes: section 7ac's integer for an allowed pair, BIG otherwise
template <bool STAGED>
struct PairCost {
  const Shared& s;
  const Dets<STAGED>& det;
  const int *tmap, *rmap;
  float thr;
  bool agnostic, tracks_drive;
  __device__ __forceinline__ long long operator()(int i, int j) const {
    const int t = tmap[tracks_drive ? i : j], d = rmap[tracks_drive ? j : i];
    const float4 p = s.tp[t], z = det.box(d);
    const float o = iou_value(p, box_area(p), z, box_area(z));
    if (!(o > thr) || !(agnostic || s.tcls[t] == det.cls(d))) return BIG;
    return (long long)(int)rintf((1.f - o) * 65536.f);
  }
};

// one association stage as a minimum-cost assignment: the candidates of `associate`, a pair allowed when its IoU is above thr and the
// classes agree.  (a) an allowed pair that is the only one of its track and of its row is taken at once; (b) candidates without an allowed
// pair are set aside; (c) the rest, tracks in slot order (ascending id) and rows in row order, go to the solver: the smaller side drives,
// the tracks when the sides are equal.  A thread owns the rows tid, tid + THREADS, ... of the frame.
template <bool STAGED>
__device__ __forceinline__ void assign_optimal(const Lds& L, const Dets<STAGED>& det, int code, float thr, bool agnostic, int nT, int n) {
  constexpr int RPT = STAGED ? 1 : MAX_OPT / THREADS;
  const Shared& s = L.s;
  const int tid = threadIdx.x;
  int* pcnt = reinterpret_cast<int*>(s.piou);   // a scan's parts: the number of allowed partners and the last of them
  // the allowed rows of each candidate track, the scan cut into parts as in associate
  int tc = 0;
  {
    const int TS = (nT + 63) & ~63;
    const int PA = TS ? THREADS / TS : 1;
    const int ga = TS ? tid / TS : 0, ta = tid - ga * TS;
    const int chunk_a = (n + PA - 1) / PA;
    int cnt = 0;
    if (ga < PA && ta < nT && s.tm[ta] == TRK_OPEN) {
      const float4 p = s.tp[ta];
      const float ap = box_area(p), cls = s.tcls[ta];
      const int d1 = min(n, (ga + 1) * chunk_a);
#pragma unroll 4
      for (int d = ga * chunk_a; d < d1; ++d) {
        const int st = det.state(d);
        const float dc = det.cls(d);
        const float4 z = det.box(d);
        const float o = iou_value(p, ap, z, box_area(z));
        if (st == code && (agnostic || dc == cls) && o > thr) cnt += 1;
      }
    }
    pcnt[tid] = cnt;
    __syncthreads();
    if (tid < nT)
      for (int g = 0; g < PA; ++g) tc += pcnt[g * TS + tid];
    s.tbest[tid] = tc;   // 0 past nT and for a track that is no candidate
    __syncthreads();
  }
  // the allowed tracks of each candidate row, and the one when there is just one
  int rc[RPT], ro[RPT];
#pragma unroll
  for (int k = 0; k < RPT; ++k) rc[k] = 0, ro[k] = -1;
  if (STAGED) {
    const int DS = (n + 63) & ~63;
    const int PB = DS ? THREADS / DS : 1;
    const int gb = DS ? tid / DS : 0, db = tid - gb * DS;
    const int chunk_b = (nT + PB - 1) / PB;
    int cnt = 0, one = -1;
    if (gb < PB && db < n && det.state(db) == code) {
      const float4 z = det.box(db);
      const float az = box_area(z), dc = det.cls(db);
      const int t1 = min(nT, (gb + 1) * chunk_b);
#pragma unroll 4
      for (int t = gb * chunk_b; t < t1; ++t) {
        const int m = s.tm[t];
        const float tcl = s.tcls[t];
        const float4 q = s.tp[t];
        const float o = iou_value(q, box_area(q), z, az);
        if (m == TRK_OPEN && (agnostic || tcl == dc) && o > thr) {
          cnt += 1;
          one = t;
        }
      }
    }
    pcnt[tid] = cnt;
    s.pidx[tid] = one;
    __syncthreads();
    if (tid < n)
      for (int g = 0; g < PB; ++g) {
        const int c = pcnt[g * DS + tid];
        if (c > 0) rc[0] += c, ro[0] = s.pidx[g * DS + tid];
      }
  } else {
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int d = tid + k * THREADS;
      if (d >= n || det.state(d) != code) continue;
      const float4 z = det.box(d);
      const float az = box_area(z), dc = det.cls(d);
#pragma unroll 4
      for (int t = 0; t < nT; ++t) {
        const int m = s.tm[t];
        const float tcl = s.tcls[t];
        const float4 q = s.tp[t];
        const float o = iou_value(q, box_area(q), z, az);
        if (m == TRK_OPEN && (agnostic || tcl == dc) && o > thr) {
          rc[k] += 1;
          ro[k] = t;
        }
      }
    }
  }
  // (a) a row with one allowed track whose one allowed row it then is: the pair is alone on both sides
#pragma unroll
  for (int k = 0; k < RPT; ++k)
    if (rc[k] == 1 && s.tbest[ro[k]] == 1) {
      det.set_state(tid + k * THREADS, ro[k]);
      s.tnew[ro[k]] = tid + k * THREADS;
      rc[k] = 0;
    }
  __syncthreads();
  {
    const int m = s.tnew[tid];
    if (m >= 0) {
      s.tm[tid] = m;
      s.tnew[tid] = -1;
      tc = 0;
    }
  }
  // (b), (c) what has an allowed pair left, each side compacted in order
  int nrt, nrr = 0;
  {
    const int pos = block_rank(tc > 0, L.wave, &nrt);
    if (tc > 0) L.tmap[pos] = tid;
  }
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    int chunk;
    const int pos = nrr + block_rank(rc[k] > 0, L.wave, &chunk);
    if (rc[k] > 0) L.rmap[pos] = tid + k * THREADS;
    nrr += chunk;
  }
  __syncthreads();
  if (nrt == 0 || nrr == 0) return;   // uniform
  const bool tracks_drive = nrt <= nrr;
  const int rows_n = tracks_drive ? nrt : nrr, cols_m = tracks_drive ? nrr : nrt;
  const PairCost<STAGED> cost = {s, det, L.tmap, L.rmap, thr, agnostic, tracks_drive};
  if (STAGED || cols_m <= THREADS)
    solve<1>(L.sv, cost, rows_n, cols_m);
  else
    solve<MAX_OPT / THREADS>(L.sv, cost, rows_n, cols_m);
  for (int j = tid; j < cols_m; j += THREADS) {
    const int i = L.sv.p[j];
    if (i >= 0 && cost(i, j) < BIG) {   // a pair on a forbidden cell is dropped
      const int t = L.tmap[tracks_drive ? i : j], d = L.rmap[tracks_drive ? j : i];
      det.set_state(d, t);
      s.tm[t] = d;
    }
  }
  __syncthreads();
}

// the Kalman model's noise scale of a box: its height, min_scale at the least (also for a NaN)
__device__ __forceinline__ float noise_scale(float y1, float y2, const cvx_track_model& mdl) { return fmaxf(y2 - y1, mdl.min_scale); }

// one frame of the stream: n rows at grow, their ids to `ids`
template <bool STAGED, int MOTION, int ASSIGN>
__device__ __forceinline__ void track_frame(const Lds& L, const cvx_track_params& prm, const cvx_track_model mdl, const float* __restrict__ grow, int n,
                                            int max_det, int* ids, int* overflow, Track& k, Stream& st) {
  const Shared& s = L.s;
  const int tid = threadIdx.x, nT = st.n_tracks;
  const bool agnostic = prm.class_agnostic != 0;
  const Dets<STAGED> det = {L.dbox, L.dcls, L.dstate, grow, ids};
  // ---- 1. count and clear; 2. predict; 3. split ----
  st.frame += 1;
  const bool live = tid < nT;
  if (live) {
    if (MOTION == KALMAN) {   // the scale of the box before the move
      const float sc = noise_scale(k.p.y, k.p.w, mdl);
      float a = k.pxv + k.pxv, b = mdl.q_pos * sc, c = mdl.q_vel * sc;
      a = a + k.pvv;
      b = b * b;
      a = a + b;
      k.pxx = k.pxx + a;
      k.pxv = k.pxv + k.pvv;
      c = c * c;
      k.pvv = k.pvv + c;
    }
    k.p.x = k.p.x + k.v.x;
    k.p.y = k.p.y + k.v.y;
    k.p.z = k.p.z + k.v.z;
    k.p.w = k.p.w + k.v.w;
  }
  s.tp[tid] = k.p;
  s.tcls[tid] = k.cls;
  s.tid[tid] = k.id;
  s.tm[tid] = live ? TRK_OPEN : TRK_OUT;
  s.tnew[tid] = -1;
  for (int d = tid; d < max_det; d += THREADS) {
    int code = -1;
    if (d < n) {
      const float* r = grow + 6 * (long long)d;
      const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], sc = r[4], c = r[5];
      code = !(x1 == x1 && y1 == y1 && x2 == x2 && y2 == y2) ? DET_IGNORED : (sc >= prm.high ? DET_HIGH : DET_LOW);
      if (STAGED) {
        L.dbox[d] = make_float4(x1, y1, x2, y2);
        L.dcls[d] = c;
        L.dstate[d] = code;
        code = -1;
      }
    }
    ids[d] = code;   // -1, or the row's state when the ids row holds it for this frame
  }
  __syncthreads();
  // ---- 4. stage 1; 5. stage 2 ----
  if (ASSIGN == OPTIMAL)
    assign_optimal(L, det, DET_HIGH, prm.iou_high, agnostic, nT, n);
  else
    associate(s, det, DET_HIGH, prm.iou_high, agnostic, nT, n);
  if (live && s.tm[tid] < 0) s.tm[tid] = (k.hits >= prm.min_hits && k.miss == 0) ? TRK_OPEN : TRK_OUT;
  __syncthreads();
  if (ASSIGN == OPTIMAL)
    assign_optimal(L, det, DET_LOW, prm.iou_low, agnostic, nT, n);
  else
    associate(s, det, DET_LOW, prm.iou_low, agnostic, nT, n);
  // ---- 6. update the matched; 7. age or delete the unmatched ----
  int label_row = -1, label = -1;
  bool keep = false;
  if (live) {
    const int m = s.tm[tid];
    if (m >= 0) {
      const float4 z = det.box(m);
      float kx = prm.alpha, kv = prm.beta;
      if (MOTION == KALMAN) {   // the gains from the covariance, at the scale of the predicted box
        float e = mdl.r_pos * noise_scale(k.p.y, k.p.w, mdl);
        e = e * e;
        e = k.pxx + e;
        kx = k.pxx / e;
        kv = k.pxv / e;
      }
      float r;
      r = z.x - k.p.x, k.p.x = k.p.x + kx * r, k.v.x = k.v.x + kv * r;
      r = z.y - k.p.y, k.p.y = k.p.y + kx * r, k.v.y = k.v.y + kv * r;
      r = z.z - k.p.z, k.p.z = k.p.z + kx * r, k.v.z = k.v.z + kv * r;
      r = z.w - k.p.w, k.p.w = k.p.w + kx * r, k.v.w = k.v.w + kv * r;
      if (MOTION == KALMAN) {
        k.pvv = k.pvv - kv * k.pxv;
        k.pxv = k.pxv - kx * k.pxv;
        k.pxx = k.pxx - kx * k.pxx;
      }
      k.hits += 1;
      k.miss = 0;
      k.cls = det.cls(m);
      label_row = m;
      label = (k.hits >= prm.min_hits || st.frame <= prm.min_hits) ? k.id : -1;
      keep = true;
    } else if (k.hits >= prm.min_hits) {
      k.miss += 1;
      keep = k.miss <= prm.max_age;
    }
  }
  // the survivors move down to slots [0, kept) in slot order, through LDS (the staged boxes' bytes carry the velocities: the births
  // below read the rows from global memory)
  int kept;
  const int pos = block_rank(keep, L.wave, &kept);   // its barriers also end every read of the arrays written next
  if (keep) {
    s.tp[pos] = k.p;
    L.dbox[pos] = k.v;
    s.tid[pos] = k.id;
    s.tm[pos] = k.hits;
    s.tbest[pos] = k.miss;
    s.tcls[pos] = k.cls;
    if (MOTION == KALMAN) reinterpret_cast<float4*>(L.rmap)[pos] = make_float4(k.pxx, k.pxv, k.pvv, 0.f);
  }
  __syncthreads();
  if (tid < kept) {
    k.p = s.tp[tid];
    k.v = L.dbox[tid];
    k.id = s.tid[tid];
    k.hits = s.tm[tid];
    k.miss = s.tbest[tid];
    k.cls = s.tcls[tid];
    if (MOTION == KALMAN) {
      const float4 c = reinterpret_cast<const float4*>(L.rmap)[tid];
      k.pxx = c.x, k.pxv = c.y, k.pvv = c.z;
    }
  }
  // ---- 8. births, in row order ----
  const int room = CAP - kept;
  int wanted = 0;
  for (int d0 = 0; d0 < n; d0 += THREADS) {
    const int d = d0 + tid;
    const int dst = d < n ? det.state(d) : 0;
    const bool born = d < n && dst == DET_HIGH && grow[6 * (long long)d + 4] >= prm.new_score;
    int chunk;
    const int r = wanted + block_rank(born, L.wave, &chunk);
    if (d < n && dst < 0) {   // a matched row gets its label from its track, below
      int idv = -1;
      if (born && r < room) {
        s.tnew[kept + r] = d;
        if (1 >= prm.min_hits || st.frame <= prm.min_hits) idv = st.next_id + r;
      }
      ids[d] = idv;
    }
    wanted += chunk;
  }
  const int born_total = min(wanted, room);
  if (tid == 0 && wanted > born_total) atomicAdd(overflow, wanted - born_total);
  __syncthreads();
  if (tid >= kept && tid < kept + born_total) {
    const int d = s.tnew[tid];
    k.id = st.next_id + (tid - kept);
    k.p = det_box(grow, d);
    k.v = make_float4(0.f, 0.f, 0.f, 0.f);
    k.hits = 1;
    k.miss = 0;
    k.cls = grow[6 * (long long)d + 5];
    if (MOTION == KALMAN) {
      const float sc = noise_scale(k.p.y, k.p.w, mdl);
      float a = mdl.init_pos * mdl.r_pos, b = mdl.init_vel * mdl.q_vel;
      a = a * sc;
      b = b * sc;
      k.pxx = a * a;
      k.pxv = 0.f;
      k.pvv = b * b;
    }
  }
  st.next_id += born_total;
  st.n_tracks = kept + born_total;
  if (label_row >= 0) ids[label_row] = label;   // after the births have read the rows' states
  __syncthreads();
}

// a stream's workgroup: the state into registers, the stream's frames in batch order, the state back.  ext: the stream's covariances
// (Kalman only).  The launch gives LDS_BYTES of LDS, MODEL_LDS_BYTES when MODEL_LDS.
template <int MOTION, int ASSIGN, bool MODEL_LDS>
__device__ __forceinline__ void track_stream(const float* __restrict__ rows, const int* __restrict__ counts, int batch, int max_det,
                                             const int* __restrict__ frame_stream, int streams, const cvx_track_params& prm,
                                             const cvx_track_model mdl, cvx_track_stream* __restrict__ state, float4* __restrict__ ext, int* out_ids,
                                             int* overflow) {
  extern __shared__ float4 lds[];   // more than the 64 KB a kernel has without asking
  float4* s_tp = lds;
  float4* s_dbox = s_tp + CAP;
  float* s_tcls = reinterpret_cast<float*>(s_dbox + DET_LDS);
  float* s_dcls = s_tcls + CAP;
  float* s_piou = s_dcls + DET_LDS;
  int* s_tid = reinterpret_cast<int*>(s_piou + THREADS);
  int* s_tm = s_tid + CAP;
  int* s_tbest = s_tm + CAP;
  int* s_tnew = s_tbest + CAP;
  int* s_pidx = s_tnew + CAP;
  int* s_dstate = s_pidx + THREADS;
  int* s_wave = s_dstate + DET_LDS;
  // the model kernels' part lies behind LDS_BYTES, a multiple of 16: the row map (float4 during the compaction) first
  int* s_rmap = s_wave + WAVES;
  long long* s_u = reinterpret_cast<long long*>(s_rmap + MAX_OPT);
  Red* s_red = reinterpret_cast<Red*>(s_u + CAP);
  int* s_p = reinterpret_cast<int*>(s_red + 2 * WAVES);
  int* s_way = s_p + MAX_OPT;
  int* s_tmap = s_way + MAX_OPT;
  const Lds L = {{s_tp, s_tcls, s_tid, s_tm, s_tbest, s_tnew, s_piou, s_pidx}, s_dbox, s_dcls, s_dstate, s_wave, {s_u, s_p, s_way, s_red}, s_tmap, s_rmap};
  static_assert(MODEL_LDS || (MOTION == AB && ASSIGN == GREEDY), "only track_kernel does without the model kernels' LDS: it reads none of it");
  const int sid = blockIdx.x, tid = threadIdx.x;
  cvx_track_stream* gs = state + sid;
  float4* gc = MOTION == KALMAN ? ext + (long long)sid * CAP : nullptr;

  Stream st = {gs->frame, gs->next_id, min(max(gs->n_tracks, 0), CAP)};
  Track k = {0, 0, 0, 0.f, make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f, 0.f};
  if (tid < st.n_tracks) {
    k.id = gs->id[tid], k.hits = gs->hits[tid], k.miss = gs->miss[tid], k.cls = gs->cls[tid];
    k.p = make_float4(gs->p[tid][0], gs->p[tid][1], gs->p[tid][2], gs->p[tid][3]);
    k.v = make_float4(gs->v[tid][0], gs->v[tid][1], gs->v[tid][2], gs->v[tid][3]);
    if (MOTION == KALMAN) {
      const float4 c = gc[tid];
      k.pxx = c.x, k.pxv = c.y, k.pvv = c.z;
    }
  }

  for (int b = 0; b < batch; ++b) {
    const int fs = frame_stream ? frame_stream[b] : 0;
    int* ids = out_ids + (long long)b * max_det;
    if (fs < 0 || fs >= streams) {   // nobody's frame: workgroup 0 clears its ids and flags it
      if (sid == 0) {
        for (int d = tid; d < max_det; d += THREADS) ids[d] = -1;
        if (tid == 0) atomicAdd(overflow, 1);
      }
      continue;
    }
    if (fs != sid) continue;
    const int raw = counts[b];
    const bool bad = raw < 0 || raw > max_det;
    const int n = bad ? 0 : raw;   // a bad count: flagged, and the frame is processed as empty
    if (bad && tid == 0) atomicAdd(overflow, 1);
    const float* grow = rows + (long long)b * max_det * 6;
    if (n <= DET_LDS)
      track_frame<true, MOTION, ASSIGN>(L, prm, mdl, grow, n, max_det, ids, overflow, k, st);
    else
      track_frame<false, MOTION, ASSIGN>(L, prm, mdl, grow, n, max_det, ids, overflow, k, st);
  }

  if (tid < st.n_tracks) {
    gs->id[tid] = k.id, gs->hits[tid] = k.hits, gs->miss[tid] = k.miss, gs->cls[tid] = k.cls;
    gs->p[tid][0] = k.p.x, gs->p[tid][1] = k.p.y, gs->p[tid][2] = k.p.z, gs->p[tid][3] = k.p.w;
    gs->v[tid][0] = k.v.x, gs->v[tid][1] = k.v.y, gs->v[tid][2] = k.v.z, gs->v[tid][3] = k.v.w;
    if (MOTION == KALMAN) gc[tid] = make_float4(k.pxx, k.pxv, k.pvv, 0.f);
  }
  if (tid == 0) gs->frame = st.frame, gs->next_id = st.next_id, gs->n_tracks = st.n_tracks;
}

__global__ __launch_bounds__(THREADS) void track_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int batch, int max_det,
                                                        const int* __restrict__ frame_stream, int streams, cvx_track_params prm,
                                                        cvx_track_stream* __restrict__ state, int* out_ids, int* overflow) {
  const cvx_track_model none = {AB, GREEDY, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  track_stream<AB, GREEDY, false>(rows, counts, batch, max_det, frame_stream, streams, prm, none, state, nullptr, out_ids, overflow);
}

template <int MOTION, int ASSIGN>
__global__ __launch_bounds__(THREADS) void track_model_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int batch, int max_det,
                                                              const int* __restrict__ frame_stream, int streams, cvx_track_params prm,
                                                              cvx_track_model mdl, cvx_track_stream* __restrict__ state, float4* __restrict__ ext,
                                                              int* out_ids, int* overflow) {
  track_stream<MOTION, ASSIGN, true>(rows, counts, batch, max_det, frame_stream, streams, prm, mdl, state, ext, out_ids, overflow);
}

int check_params(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, int32_t streams, const cvx_track_params* params, void* state,
                 int32_t* out_ids, int32_t* overflow) {
  static_assert(sizeof(cvx_track_stream) == 16 + 48 * CVX_TRACK_CAP && sizeof(cvx_track_params) == 40, "the layouts track.py reads");
  CVX_CHECK(rows && counts && params && state && out_ids && overflow, "null arguments");
  CVX_CHECK(batch > 0 && max_det > 0 && streams > 0 && streams <= 65535, "bad sizes");
  const cvx_track_params& q = *params;
  CVX_CHECK(q.high >= 0.f && q.high <= 1.f && q.new_score >= 0.f && q.new_score <= 1.f && q.iou_high >= 0.f && q.iou_high <= 1.f &&
                q.iou_low >= 0.f && q.iou_low <= 1.f,
            "the thresholds must lie in [0,1]");
  CVX_CHECK(q.alpha == q.alpha && q.beta == q.beta, "alpha and beta are numbers");
  CVX_CHECK(q.min_hits >= 1 && q.max_age >= 0, "min_hits >= 1 and max_age >= 0");
  return 0;
}

template <int MOTION, int ASSIGN>
int launch_model(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, const int32_t* frame_stream, int32_t streams,
                 const cvx_track_params& q, const cvx_track_model& m, void* state, void* ext, int32_t* out_ids, int32_t* overflow, void* hip_stream) {
  static unsigned long long optin = 0;   // one per instance
  CVX_TRY(cvx_lds_optin((const void*)track_model_kernel<MOTION, ASSIGN>, MODEL_LDS_BYTES, &optin));
  hipLaunchKernelGGL((track_model_kernel<MOTION, ASSIGN>), dim3((unsigned)streams), dim3(THREADS), (size_t)MODEL_LDS_BYTES, (hipStream_t)hip_stream, rows, counts,
                     batch, max_det, frame_stream, streams, q, m, (cvx_track_stream*)state, (float4*)ext, out_ids, overflow);
  CVX_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int64_t cvx_track_state_bytes(int32_t streams) { return streams > 0 ? (int64_t)streams * (int64_t)sizeof(cvx_track_stream) : 0; }

extern "C" int cvx_track_update(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, const int32_t* frame_stream, int32_t streams,
                                const cvx_track_params* params, void* state, int32_t* out_ids, int32_t* overflow, void* hip_stream) {
  CVX_TRY(check_params(rows, counts, batch, max_det, streams, params, state, out_ids, overflow));
  static unsigned long long optin = 0;
  CVX_TRY(cvx_lds_optin((const void*)track_kernel, LDS_BYTES, &optin));
  hipLaunchKernelGGL(track_kernel, dim3((unsigned)streams), dim3(THREADS), (size_t)LDS_BYTES, (hipStream_t)hip_stream, rows, counts, batch, max_det, frame_stream,
                     streams, *params, (cvx_track_stream*)state, out_ids, overflow);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t cvx_track_ext_bytes(int32_t streams) { return streams > 0 ? (int64_t)streams * CVX_TRACK_CAP * 16 : 0; }

extern "C" int cvx_track_update_model(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, const int32_t* frame_stream,
                                      int32_t streams, const cvx_track_params* params, const cvx_track_model* model, void* state, void* ext,
                                      int32_t* out_ids, int32_t* overflow, void* hip_stream) {
  static_assert(sizeof(cvx_track_model) == 32, "the layout track.py reads");
  CVX_TRY(check_params(rows, counts, batch, max_det, streams, params, state, out_ids, overflow));
  CVX_CHECK(model && ext, "null arguments");
  CVX_CHECK(((uintptr_t)ext & 15) == 0, "ext is 16-byte aligned");
  const cvx_track_model& m = *model;
  const bool kalman = m.motion == KALMAN, optimal = m.assign == OPTIMAL;
  CVX_CHECK((m.motion == AB || kalman) && (m.assign == GREEDY || optimal), "unknown motion or assign");
  CVX_CHECK(m.q_pos >= 0.f && m.q_pos < INFINITY && m.q_vel >= 0.f && m.q_vel < INFINITY && m.r_pos >= 0.f && m.r_pos < INFINITY &&
                m.init_pos >= 0.f && m.init_pos < INFINITY && m.init_vel >= 0.f && m.init_vel < INFINITY,
            "the noise weights are finite and not negative");
  CVX_CHECK(m.min_scale > 0.f && m.min_scale < INFINITY, "min_scale > 0");
  CVX_CHECK(!optimal || max_det <= CVX_TRACK_OPTIMAL_MAX_DET, "the optimal association takes at most 4096 rows per frame");
#define CVX_TRACK_LAUNCH(M, A) launch_model<M, A>(rows, counts, batch, max_det, frame_stream, streams, *params, m, state, ext, out_ids, overflow, hip_stream)
  return kalman ? (optimal ? CVX_TRACK_LAUNCH(KALMAN, OPTIMAL) : CVX_TRACK_LAUNCH(KALMAN, GREEDY))
                : (optimal ? CVX_TRACK_LAUNCH(AB, OPTIMAL) : CVX_TRACK_LAUNCH(AB, GREEDY));
#undef CVX_TRACK_LAUNCH
}
