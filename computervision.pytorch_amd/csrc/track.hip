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
#include "box_overlap.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int CAP = CVX_TRACK_CAP;
constexpr int THREADS = 1024;   // one thread per track slot
constexpr int WAVES = THREADS / 64;
constexpr int DET_LDS = 1024;   // rows of a frame staged in LDS; their boxes' bytes then carry the velocities through the compaction
enum { DET_HIGH = -1, DET_LOW = -2, DET_IGNORED = -3 };   // per-row state; >= 0: the slot of the matched track
enum { TRK_OPEN = -1, TRK_OUT = -2 };                     // per-track match; >= 0: the matched row

static_assert(THREADS == CAP, "thread t owns slot t");
static_assert(DET_LDS >= CAP, "the staging area holds one float4 per slot");
constexpr int LDS_BYTES = (CAP + DET_LDS) * 16 + (2 * CAP + 2 * DET_LDS + 2 * THREADS + 3 * CAP) * 4 + WAVES * 4;

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
};

// one frame of the stream: n rows at grow, their ids to `ids`
template <bool STAGED>
__device__ __forceinline__ void track_frame(const Lds& L, const cvx_track_params& prm, const float* __restrict__ grow, int n, int max_det, int* ids,
                                            int* overflow, Track& k, Stream& st) {
  const Shared& s = L.s;
  const int tid = threadIdx.x, nT = st.n_tracks;
  const bool agnostic = prm.class_agnostic != 0;
  const Dets<STAGED> det = {L.dbox, L.dcls, L.dstate, grow, ids};
  // ---- 1. count and clear; 2. predict; 3. split ----
  st.frame += 1;
  const bool live = tid < nT;
  if (live) {
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
  associate(s, det, DET_HIGH, prm.iou_high, agnostic, nT, n);
  if (live && s.tm[tid] < 0) s.tm[tid] = (k.hits >= prm.min_hits && k.miss == 0) ? TRK_OPEN : TRK_OUT;
  __syncthreads();
  associate(s, det, DET_LOW, prm.iou_low, agnostic, nT, n);
  // ---- 6. update the matched; 7. age or delete the unmatched ----
  int label_row = -1, label = -1;
  bool keep = false;
  if (live) {
    const int m = s.tm[tid];
    if (m >= 0) {
      const float4 z = det.box(m);
      float r;
      r = z.x - k.p.x, k.p.x = k.p.x + prm.alpha * r, k.v.x = k.v.x + prm.beta * r;
      r = z.y - k.p.y, k.p.y = k.p.y + prm.alpha * r, k.v.y = k.v.y + prm.beta * r;
      r = z.z - k.p.z, k.p.z = k.p.z + prm.alpha * r, k.v.z = k.v.z + prm.beta * r;
      r = z.w - k.p.w, k.p.w = k.p.w + prm.alpha * r, k.v.w = k.v.w + prm.beta * r;
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
  }
  __syncthreads();
  if (tid < kept) {
    k.p = s.tp[tid];
    k.v = L.dbox[tid];
    k.id = s.tid[tid];
    k.hits = s.tm[tid];
    k.miss = s.tbest[tid];
    k.cls = s.tcls[tid];
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
  }
  st.next_id += born_total;
  st.n_tracks = kept + born_total;
  if (label_row >= 0) ids[label_row] = label;   // after the births have read the rows' states
  __syncthreads();
}

__global__ __launch_bounds__(THREADS) void track_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int batch, int max_det,
                                                        const int* __restrict__ frame_stream, int streams, cvx_track_params prm,
                                                        cvx_track_stream* __restrict__ state, int* out_ids, int* overflow) {
  extern __shared__ float4 lds[];   // LDS_BYTES: more than the 64 KB a kernel has without asking
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
  const Lds L = {{s_tp, s_tcls, s_tid, s_tm, s_tbest, s_tnew, s_piou, s_pidx}, s_dbox, s_dcls, s_dstate, s_wave};
  const int sid = blockIdx.x, tid = threadIdx.x;
  cvx_track_stream* gs = state + sid;

  Stream st = {gs->frame, gs->next_id, min(max(gs->n_tracks, 0), CAP)};
  Track k = {0, 0, 0, 0.f, make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  if (tid < st.n_tracks) {
    k.id = gs->id[tid], k.hits = gs->hits[tid], k.miss = gs->miss[tid], k.cls = gs->cls[tid];
    k.p = make_float4(gs->p[tid][0], gs->p[tid][1], gs->p[tid][2], gs->p[tid][3]);
    k.v = make_float4(gs->v[tid][0], gs->v[tid][1], gs->v[tid][2], gs->v[tid][3]);
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
      track_frame<true>(L, prm, grow, n, max_det, ids, overflow, k, st);
    else
      track_frame<false>(L, prm, grow, n, max_det, ids, overflow, k, st);
  }

  if (tid < st.n_tracks) {
    gs->id[tid] = k.id, gs->hits[tid] = k.hits, gs->miss[tid] = k.miss, gs->cls[tid] = k.cls;
    gs->p[tid][0] = k.p.x, gs->p[tid][1] = k.p.y, gs->p[tid][2] = k.p.z, gs->p[tid][3] = k.p.w;
    gs->v[tid][0] = k.v.x, gs->v[tid][1] = k.v.y, gs->v[tid][2] = k.v.z, gs->v[tid][3] = k.v.w;
  }
  if (tid == 0) gs->frame = st.frame, gs->next_id = st.next_id, gs->n_tracks = st.n_tracks;
}

}  // namespace

extern "C" int64_t cvx_track_state_bytes(int32_t streams) { return streams > 0 ? (int64_t)streams * (int64_t)sizeof(cvx_track_stream) : 0; }

extern "C" int cvx_track_update(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, const int32_t* frame_stream, int32_t streams,
                                const cvx_track_params* params, void* state, int32_t* out_ids, int32_t* overflow, void* hip_stream) {
  static_assert(sizeof(cvx_track_stream) == 16 + 48 * CVX_TRACK_CAP && sizeof(cvx_track_params) == 40, "the layouts track.py reads");
  CVX_CHECK(rows && counts && params && state && out_ids && overflow, "null arguments");
  CVX_CHECK(batch > 0 && max_det > 0 && streams > 0 && streams <= 65535, "bad sizes");
  const cvx_track_params& q = *params;
  CVX_CHECK(q.high >= 0.f && q.high <= 1.f && q.new_score >= 0.f && q.new_score <= 1.f && q.iou_high >= 0.f && q.iou_high <= 1.f &&
                q.iou_low >= 0.f && q.iou_low <= 1.f,
            "the thresholds must lie in [0,1]");
  CVX_CHECK(q.alpha == q.alpha && q.beta == q.beta, "alpha and beta are numbers");
  CVX_CHECK(q.min_hits >= 1 && q.max_age >= 0, "min_hits >= 1 and max_age >= 0");
  static unsigned long long optin = 0;
  CVX_TRY(cvx_lds_optin((const void*)track_kernel, LDS_BYTES, &optin));
  hipLaunchKernelGGL(track_kernel, dim3((unsigned)streams), dim3(THREADS), (size_t)LDS_BYTES, (hipStream_t)hip_stream, rows, counts, batch, max_det, frame_stream,
                     streams, q, (cvx_track_stream*)state, out_ids, overflow);
  CVX_HIP(hipGetLastError());
  return 0;
}
