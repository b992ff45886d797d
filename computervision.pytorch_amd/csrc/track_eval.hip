// Tracking evaluation on gfx950: CLEAR-MOT and the identity measures of a tracker's ids against ground-truth
// identities, with the evaluator's state in device memory and nothing read by the host before cvx_mot_summary's table.  The rules are
// stated in include/cvx_engine.h and restated in numpy in tests/track_eval_restatement.py; this file is held to the restatement bit for
// bit -- past the quantisation of the IoU to a 16-bit cost everything is an integer.
//
//   cvx_mot_frames: one workgroup of 1024 threads per stream walks the stream's frames in batch order (as cvx_track_update does).  A
//   frame's hypotheses (rows with id >= 0) and ground truths are compacted into LDS in row order, the flagged ones dropped; thread t
//   then owns identity t of the frame (continuity, the counters) or column t of the assignment.  All pairs are gated once: the pass that
//   counts c[o, h] also fills the cost matrix of the identities and hypotheses that continuity left over, in LDS when it has at most
//   MAT_LDS cells and in the caller's workspace otherwise -- two instantiations of the frame's body, so the first reads it with LDS
//   instructions.
//   The assignment (assign_solver.h:solve) is the shortest-augmenting-path method with potentials, rows inserted in order: one lane per column keeps
//   the column's slack, potential and visited bit in registers, a workgroup reduction takes the arg min (lowest column on a tie), and
//   there is one barrier per step of a path.  Forbidden cells cost BIG = 2^27 > 1024 * 65536, so a minimum-cost assignment of the smaller
//   side has the maximal number of allowed pairs and, among those, the minimal sum; the potentials reach 1024 * BIG and are 64-bit.
//   cvx_mot_summary: one workgroup per stream classifies the identities, compacts the non-empty rows and columns of c and solves the
//   maximum-weight assignment with the same solver (cost -c, up to four columns per lane); a second one-workgroup launch sums the table.
// Only a stream's workgroup touches its state: no floating-point atomics, nothing read across workgroups within a launch.
#include "assign_solver.h"
#include "box_overlap.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int CAP = CVX_MOT_FRAME_CAP;        // identities, and hypotheses, of one frame
constexpr int MAX_GT = CVX_MOT_MAX_GT_IDS;    // bounds of max_gt_ids / max_track_ids: the summary's maps are LDS arrays
constexpr int MAX_TR = CVX_MOT_MAX_TRACK_IDS;
constexpr int MAT_LDS = 16384;                // cells of a cost matrix kept in LDS (128 x 128)
static_assert(THREADS == SOLVE_THREADS, "the solver's workgroup (assign_solver.h: Red, red_min, Solver, solve, BIG, INF)");
static_assert(THREADS == CAP, "thread t owns identity t / column t of a frame");
static_assert(MAX_TR == 4 * THREADS, "the summary gives a lane four columns");

// header words of a stream's state (cvx_mot_stream_header.v) and columns of the result table
enum { H_FRAMES, H_OBJECTS, H_HYPS, H_MATCHES, H_MISSES, H_FP, H_SWITCHES, H_FRAGS, H_COST, H_FLAG_NAN, H_FLAG_DUP_ROW, H_FLAG_DUP_GT,
       H_FLAG_IDENTITY, H_FLAG_TRACK, H_FLAG_FRAME, H_FLAG_EXCESS, H_WORDS };
static_assert(H_WORDS == CVX_MOT_HEADER_WORDS, "the header track_eval.py reads");

struct State {   // one stream's block
  long long* head;
  int *mem, *last, *present, *matched, *gap, *c;
};
__device__ __host__ inline long long state_bytes(int gi, int ti) { return (8ll * H_WORDS + 20ll * gi + 4ll * gi * (long long)ti + 7) & ~7ll; }
__device__ __forceinline__ State state_of(void* base, int sid, int gi, int ti) {
  char* b = (char*)base + sid * state_bytes(gi, ti);
  State s;
  s.head = (long long*)b;
  s.mem = (int*)(b + 8 * H_WORDS);
  s.last = s.mem + gi, s.present = s.last + gi, s.matched = s.present + gi, s.gap = s.matched + gi, s.c = s.gap + gi;
  return s;
}

// rank of `flag` over the workgroup in thread order, and the total; two barriers
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

// sum over the workgroup, to every thread; two barriers
__device__ __forceinline__ long long block_sum(long long v, long long* wave_sum) {
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
  for (int k = 0; k < WAVES; ++k) s += wave_sum[k];
  __syncthreads();
  return s;
}

struct Side {   // the hypotheses or the ground truths of a frame, compacted in row order
  float4* box;
  float* cls;
  int* id;      // track id / identity
  int* match;   // the index on the other side, -1 unmatched
  int* rank;    // the row or column of the assignment, -1 when continuity took it; dead once the matrix is filled (Solver::p, way)
  int* list;    // the inverse of rank
};

struct Lds {
  Side g, h;
  int* gcost;   // the cost of an identity's match
  int* gnew;    // 1: the match came from the assignment
  int* mat;     // MAT_LDS cells
  Solver s;
  int* wave;
  long long* wsum;
};
constexpr int LDS_BYTES = 2 * CAP * (16 + 5 * 4) + 2 * CAP * 4 + MAT_LDS * 4 + CAP * 8 + 2 * WAVES * 16 + WAVES * 4 + WAVES * 8;
static_assert(LDS_BYTES <= 160 * 1024, "one workgroup's LDS on gfx950");

template <bool IN_LDS>
struct FrameCost {
  const int* lmat;   // LDS
  const int* gmat;   // the workspace
  int m;
  __device__ __forceinline__ long long operator()(int i, int j) const {
    const int c = IN_LDS ? lmat[i * m + j] : gmat[(long long)i * m + j];
    return c < 0 ? BIG : (long long)c;
  }
};

struct Prm {
  float iou;
  int agnostic, gi, ti;
};

__device__ __forceinline__ bool box_is_nan(const float4& b) { return !(b.x == b.x && b.y == b.y && b.z == b.z && b.w == b.w); }

// the gate and the cost of a pair: -1 forbidden
__device__ __forceinline__ int pair_cost(const Side& g, int t, const Side& h, int s, const Prm& prm) {
  const float4 a = g.box[t], b = h.box[s];
  const float o = iou_value(a, box_area(a), b, box_area(b));
  if (!(o >= prm.iou) || !(prm.agnostic || g.cls[t] == h.cls[s])) return -1;
  return (int)rintf((1.f - o) * 65536.f);
}

// drops the flagged entries [0, nc) of a side (ok == 0) and closes the gaps in order; returns the count
__device__ __forceinline__ int compact_side(const Side& z, int nc, bool ok, int* wave) {
  const int tid = threadIdx.x;
  const float4 b = z.box[tid];
  const float c = z.cls[tid];
  const int id = z.id[tid];
  int kept;
  const int pos = block_rank(tid < nc && ok, wave, &kept);
  if (tid < nc && ok) z.box[pos] = b, z.cls[pos] = c, z.id[pos] = id;
  __syncthreads();
  return kept;
}

// the part of a frame behind the compaction: continuity, the matrix, the assignment, the counters
template <bool IN_LDS>
__device__ __forceinline__ void mot_assign(const Lds& L, const Prm& prm, const State& st, int nG, int nH, int nrg, int nrh, int* gmat) {
  const int tid = threadIdx.x;
  const bool rows_are_gt = nrg <= nrh;
  const int n = rows_are_gt ? nrg : nrh, m = rows_are_gt ? nrh : nrg;
  int* mat = IN_LDS ? L.mat : gmat;
  // every pair once: c, and the left-over pairs' cells
  const int pairs = nG * nH;
  for (int e = tid; e < pairs; e += THREADS) {
    const int t = e / nH, s = e - t * nH;
    const int c = pair_cost(L.g, t, L.h, s, prm);
    if (c >= 0) st.c[(long long)L.g.id[t] * prm.ti + L.h.id[s]] += 1;   // one pair, one thread: the frame's ids are distinct
    const int rt = L.g.rank[t], rs = L.h.rank[s];
    if (rt >= 0 && rs >= 0) {
      const long long cell = rows_are_gt ? (long long)rt * m + rs : (long long)rs * m + rt;
      if (IN_LDS) L.mat[cell] = c;
      else gmat[cell] = c;
    }
  }
  __syncthreads();
  if (n > 0) {
    const FrameCost<IN_LDS> cost = {L.mat, gmat, m};
    solve<1>(L.s, cost, n, m);
    if (tid < m) {
      const int i = L.s.p[tid];
      if (i >= 0) {
        const int c = IN_LDS ? L.mat[i * m + tid] : mat[(long long)i * m + tid];
        if (c >= 0) {
          const int t = rows_are_gt ? L.g.list[i] : L.g.list[tid], s = rows_are_gt ? L.h.list[tid] : L.h.list[i];
          L.g.match[t] = s;
          L.gcost[t] = c;
          L.gnew[t] = 1;
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(THREADS) void mot_frames_kernel(const float* __restrict__ rows, const int* __restrict__ counts, const int* __restrict__ ids,
                                                             int batch, int max_det, const float* __restrict__ gt, const int* __restrict__ gt_counts,
                                                             int max_gt, const int* __restrict__ frame_stream, int streams, Prm prm, void* state,
                                                             int* workspace) {
  extern __shared__ float4 lds[];   // LDS_BYTES
  Lds L;
  L.g.box = lds;
  L.h.box = L.g.box + CAP;
  L.s.u = reinterpret_cast<long long*>(L.h.box + CAP);
  L.s.red = reinterpret_cast<Red*>(L.s.u + CAP);
  L.wsum = reinterpret_cast<long long*>(L.s.red + 2 * WAVES);
  L.g.cls = reinterpret_cast<float*>(L.wsum + WAVES);
  L.h.cls = L.g.cls + CAP;
  L.g.id = reinterpret_cast<int*>(L.h.cls + CAP);
  L.h.id = L.g.id + CAP;
  L.g.match = L.h.id + CAP, L.h.match = L.g.match + CAP;
  L.g.rank = L.h.match + CAP, L.h.rank = L.g.rank + CAP;
  L.g.list = L.h.rank + CAP, L.h.list = L.g.list + CAP;
  L.gcost = L.h.list + CAP, L.gnew = L.gcost + CAP;
  L.s.p = L.g.rank, L.s.way = L.h.rank;   // the ranks are read for the last time when the matrix is filled
  L.wave = L.gnew + CAP;
  L.mat = L.wave + WAVES;
  const int sid = blockIdx.x, tid = threadIdx.x;
  const State st = state_of(state, sid, prm.gi, prm.ti);
  int* gmat = workspace + (long long)sid * CAP * CAP;
  long long tot[H_WORDS];   // uniform over the workgroup
#pragma unroll
  for (int k = 0; k < H_WORDS; ++k) tot[k] = st.head[k];

  for (int b = 0; b < batch; ++b) {
    const int fs = frame_stream ? frame_stream[b] : 0;
    if (fs < 0 || fs >= streams) {   // nobody's frame: stream 0 flags it
      if (sid == 0) tot[H_FLAG_FRAME] += 1;
      continue;
    }
    if (fs != sid) continue;
    const int nrow = counts[b], ngt = gt_counts[b];
    if (nrow < 0 || nrow > max_det || ngt < 0 || ngt > max_gt) {   // a bad count: flagged, the frame is skipped whole
      tot[H_FLAG_FRAME] += 1;
      continue;
    }
    const int frame = (int)(tot[H_FRAMES] += 1);
    const float* grow = rows + (long long)b * max_det * 6;
    const int* gids = ids + (long long)b * max_det;
    const float* ggt = gt + (long long)b * max_gt * 6;
    // ---- the hypotheses: rows with id >= 0, in row order, CAP at the most ----
    int nc = 0;
    for (int d0 = 0; d0 < nrow; d0 += THREADS) {
      const int d = d0 + tid;
      const int id = d < nrow ? gids[d] : -1;
      int chunk;
      const int pos = nc + block_rank(id >= 0, L.wave, &chunk);
      if (id >= 0 && pos < CAP) {
        const float* r = grow + 6 * (long long)d;
        L.h.box[pos] = make_float4(r[0], r[1], r[2], r[3]);
        L.h.cls[pos] = r[5];
        L.h.id[pos] = id;
      }
      nc += chunk;
    }
    if (nc > CAP) tot[H_FLAG_EXCESS] += nc - CAP, nc = CAP;
    __syncthreads();
    int nH;
    {
      const bool mine = tid < nc;
      const bool nan = mine && box_is_nan(L.h.box[tid]);
      const int id = mine ? L.h.id[tid] : 0;
      const bool far = mine && !nan && id >= prm.ti;
      const bool ok1 = mine && !nan && !far;
      L.h.match[tid] = ok1;
      __syncthreads();
      bool dup = false;
      if (ok1)
        for (int j = 0; j < tid; ++j) dup |= L.h.match[j] && L.h.id[j] == id;
      tot[H_FLAG_NAN] += __syncthreads_count(nan);
      tot[H_FLAG_TRACK] += __syncthreads_count(far);
      tot[H_FLAG_DUP_ROW] += __syncthreads_count(dup);
      nH = compact_side(L.h, nc, ok1 && !dup, L.wave);
    }
    // ---- the ground truths ----
    int nG;
    {
      const bool mine = tid < ngt;
      float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
      float cl = 0.f, fi = 0.f;
      if (mine) {
        const float* r = ggt + 6 * (long long)tid;
        bx = make_float4(r[0], r[1], r[2], r[3]), cl = r[4], fi = r[5];
      }
      const bool nan = mine && box_is_nan(bx);
      const bool far = mine && !nan && !(fi >= 0.f && fi < (float)prm.gi && fi == truncf(fi));
      const bool ok1 = mine && !nan && !far;
      const int id = ok1 ? (int)fi : 0;
      L.g.box[tid] = bx, L.g.cls[tid] = cl, L.g.id[tid] = id;
      L.g.match[tid] = ok1;
      __syncthreads();
      bool dup = false;
      if (ok1)
        for (int j = 0; j < tid; ++j) dup |= L.g.match[j] && L.g.id[j] == id;
      tot[H_FLAG_NAN] += __syncthreads_count(nan);
      tot[H_FLAG_IDENTITY] += __syncthreads_count(far);
      tot[H_FLAG_DUP_GT] += __syncthreads_count(dup);
      nG = compact_side(L.g, ngt, ok1 && !dup, L.wave);
    }
    // ---- 1. continuity: an identity matched in the stream's previous frame keeps its track when the pair still passes the gate ----
    L.h.match[tid] = -1;
    L.g.match[tid] = -1;
    L.gnew[tid] = 0;
    L.gcost[tid] = 0;
    __syncthreads();
    int ident = 0, remembered = 0;
    if (tid < nG) {
      ident = L.g.id[tid];
      remembered = st.mem[ident];
      st.present[ident] += 1;
      if (remembered > 0 && st.last[ident] == frame - 1) {
        int s = -1;
        for (int j = 0; j < nH; ++j)
          if (L.h.id[j] == remembered - 1) s = j;   // one at the most
        if (s >= 0) {
          const int c = pair_cost(L.g, tid, L.h, s, prm);
          if (c >= 0) L.g.match[tid] = s, L.h.match[s] = tid, L.gcost[tid] = c;   // one identity per track: last frame's matching was one to one
        }
      }
    }
    __syncthreads();
    // ---- 2. the left-over identities and hypotheses, each in order ----
    int nrg, nrh;
    {
      const bool fg = tid < nG && L.g.match[tid] < 0, fh = tid < nH && L.h.match[tid] < 0;
      const int rg = block_rank(fg, L.wave, &nrg);
      const int rh = block_rank(fh, L.wave, &nrh);
      L.g.rank[tid] = fg ? rg : -1;
      L.h.rank[tid] = fh ? rh : -1;
      if (fg) L.g.list[rg] = tid;
      if (fh) L.h.list[rh] = tid;
      __syncthreads();
    }
    if ((long long)nrg * nrh <= MAT_LDS)
      mot_assign<true>(L, prm, st, nG, nH, nrg, nrh, gmat);
    else
      mot_assign<false>(L, prm, st, nG, nH, nrg, nrh, gmat);
    // ---- 3, 4. the counters ----
    bool hit = false, sw = false, frag = false;
    int cst = 0;
    if (tid < nG) {
      const int s = L.g.match[tid];
      hit = s >= 0;
      if (hit) {
        cst = L.gcost[tid];
        const int h1 = L.h.id[s] + 1;
        sw = L.gnew[tid] && remembered > 0 && remembered != h1;
        st.mem[ident] = h1;
        st.last[ident] = frame;
        const int before = st.matched[ident];
        frag = before > 0 && st.gap[ident] != 0;
        st.matched[ident] = before + 1;
        st.gap[ident] = 0;
      } else {
        st.gap[ident] = 1;
      }
    }
    const int hits = __syncthreads_count(hit);
    tot[H_SWITCHES] += __syncthreads_count(sw);
    tot[H_FRAGS] += __syncthreads_count(frag);
    tot[H_COST] += block_sum(cst, L.wsum);
    tot[H_OBJECTS] += nG, tot[H_HYPS] += nH, tot[H_MATCHES] += hits, tot[H_MISSES] += nG - hits, tot[H_FP] += nH - hits;
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < H_WORDS; ++k) st.head[k] = tot[k];
  }
}

// ---- the summary ------------------------------------------------------------------------------------------------------------------------------
struct SumCost {
  const int* c;
  const int *rowmap, *colmap;   // LDS: the identities / tracks of the compacted rows and columns of c
  int ti;
  bool rows_are_gt;
  __device__ __forceinline__ long long operator()(int i, int j) const {
    const int o = rows_are_gt ? rowmap[i] : rowmap[j], h = rows_are_gt ? colmap[j] : colmap[i];
    return -(long long)c[(long long)o * ti + h];
  }
};

constexpr int SUM_LDS_BYTES = MAX_GT * 8 + 2 * WAVES * 16 + WAVES * 8 + 2 * MAX_TR * 4 + MAX_GT * 4 + MAX_TR * 4 + WAVES * 4;

__global__ __launch_bounds__(THREADS) void mot_summary_kernel(void* state, int gi, int ti, long long* table) {
  extern __shared__ float4 lds[];   // SUM_LDS_BYTES
  Solver S;
  S.u = reinterpret_cast<long long*>(lds);
  S.red = reinterpret_cast<Red*>(S.u + MAX_GT);
  long long* wsum = reinterpret_cast<long long*>(S.red + 2 * WAVES);
  S.p = reinterpret_cast<int*>(wsum + WAVES);
  S.way = S.p + MAX_TR;
  int* rowmap = S.way + MAX_TR;   // first the flags, then the maps
  int* colmap = rowmap + MAX_GT;
  int* wave = colmap + MAX_TR;
  const int sid = blockIdx.x, tid = threadIdx.x;
  const State st = state_of(state, sid, gi, ti);
  // mostly tracked / partly tracked / mostly lost
  int mt = 0, pt = 0, ml = 0, seen = 0;
  for (int o = tid; o < gi; o += THREADS) {
    const int n = st.present[o], k = st.matched[o];
    if (n > 0) {
      seen += 1;
      if (5ll * k >= 4ll * n) mt += 1;
      else if (5ll * k < (long long)n) ml += 1;
      else pt += 1;
    }
    rowmap[o] = 0;
  }
  for (int h = tid; h < ti; h += THREADS) colmap[h] = 0;
  __syncthreads();
  for (int o = 0; o < gi; ++o) {
    if (st.present[o] == 0) continue;   // uniform: an identity never seen has an empty row
    const int* row = st.c + (long long)o * ti;
    for (int h = tid; h < ti; h += THREADS)
      if (row[h] > 0) rowmap[o] = 1, colmap[h] = 1;   // every writer writes 1
  }
  __syncthreads();
  int nr = 0, ncol = 0;
  for (int o0 = 0; o0 < gi; o0 += THREADS) {
    const int o = o0 + tid;
    const bool f = o < gi && rowmap[o] != 0;
    int chunk;
    const int pos = nr + block_rank(f, wave, &chunk);   // its barriers end the reads of this chunk; pos <= o
    if (f) rowmap[pos] = o;
    nr += chunk;
    __syncthreads();
  }
  for (int h0 = 0; h0 < ti; h0 += THREADS) {
    const int h = h0 + tid;
    const bool f = h < ti && colmap[h] != 0;
    int chunk;
    const int pos = ncol + block_rank(f, wave, &chunk);
    if (f) colmap[pos] = h;
    ncol += chunk;
    __syncthreads();
  }
  long long idtp = 0;
  const bool rows_are_gt = nr <= ncol;
  const int n = rows_are_gt ? nr : ncol, m = rows_are_gt ? ncol : nr;
  if (n > 0) {
    const SumCost cost = {st.c, rowmap, colmap, ti, rows_are_gt};
    solve<4>(S, cost, n, m);
    long long part = 0;
    for (int j = tid; j < m; j += THREADS) {
      const int i = S.p[j];
      if (i >= 0) part -= cost(i, j);
    }
    idtp = block_sum(part, wsum);
  }
  const long long smt = block_sum(mt, wsum), spt = block_sum(pt, wsum), sml = block_sum(ml, wsum), sseen = block_sum(seen, wsum);
  if (tid == 0) {
    long long* r = table + (long long)sid * CVX_MOT_TABLE_WORDS;
    for (int k = 0; k <= H_COST; ++k) r[k] = st.head[k];
    r[9] = smt, r[10] = spt, r[11] = sml, r[12] = idtp;
    for (int k = H_FLAG_NAN; k < H_WORDS; ++k) r[13 + k - H_FLAG_NAN] = st.head[k];
    r[20] = sseen, r[21] = ncol, r[22] = 0, r[23] = 0;
  }
}

__global__ void mot_total_kernel(long long* table, int streams) {
  const int k = threadIdx.x;
  if (k >= CVX_MOT_TABLE_WORDS) return;
  long long s = 0;
  for (int i = 0; i < streams; ++i) s += table[(long long)i * CVX_MOT_TABLE_WORDS + k];
  table[(long long)streams * CVX_MOT_TABLE_WORDS + k] = s;
}

bool sizes_ok(int streams, int gi, int ti) { return streams > 0 && streams <= 65535 && gi > 0 && gi <= MAX_GT && ti > 0 && ti <= MAX_TR; }

}  // namespace

extern "C" int64_t cvx_mot_state_bytes(int32_t streams, int32_t max_gt_ids, int32_t max_track_ids) {
  return sizes_ok(streams, max_gt_ids, max_track_ids) ? (int64_t)streams * state_bytes(max_gt_ids, max_track_ids) : 0;
}

extern "C" int64_t cvx_mot_workspace_bytes(int32_t streams) {
  return streams > 0 && streams <= 65535 ? (int64_t)streams * CAP * CAP * 4 : 0;
}

extern "C" int cvx_mot_frames(const float* rows, const int32_t* counts, const int32_t* ids, int32_t batch, int32_t max_det, const float* gt,
                              const int32_t* gt_counts, int32_t max_gt, const int32_t* frame_stream, int32_t streams, const cvx_mot_params* params,
                              void* state, void* workspace, int64_t workspace_bytes, void* hip_stream) {
  static_assert(sizeof(cvx_mot_params) == 24 && sizeof(cvx_mot_stream_header) == 8 * H_WORDS && sizeof(Red) == 16, "the layouts track_eval.py reads");
  CVX_CHECK(rows && counts && ids && gt && gt_counts && params && state && workspace, "null arguments");
  CVX_CHECK(batch > 0 && max_det > 0 && max_gt > 0 && max_gt <= CAP, "bad sizes: a frame has at most 1024 ground truths");
  const cvx_mot_params& q = *params;
  CVX_CHECK(sizes_ok(streams, q.max_gt_ids, q.max_track_ids), "streams in [1, 65535], max_gt_ids in [1, 1024], max_track_ids in [1, 4096]");
  CVX_CHECK(q.iou >= 0.f && q.iou <= 1.f, "the gate must lie in [0,1]");
  CVX_CHECK(((uintptr_t)state & 7) == 0 && ((uintptr_t)workspace & 3) == 0, "state is 8-byte aligned");
  CVX_CHECK(workspace_bytes >= cvx_mot_workspace_bytes(streams), "workspace too small: cvx_mot_workspace_bytes");
  static unsigned long long optin = 0;
  CVX_TRY(cvx_lds_optin((const void*)mot_frames_kernel, LDS_BYTES, &optin));
  const Prm prm = {q.iou, q.class_agnostic != 0, q.max_gt_ids, q.max_track_ids};
  hipLaunchKernelGGL(mot_frames_kernel, dim3((unsigned)streams), dim3(THREADS), (size_t)LDS_BYTES, (hipStream_t)hip_stream, rows, counts, ids, batch, max_det,
                     gt, gt_counts, max_gt, frame_stream, streams, prm, state, (int*)workspace);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_mot_summary(void* state, int32_t streams, int32_t max_gt_ids, int32_t max_track_ids, int64_t* table, void* hip_stream) {
  CVX_CHECK(state && table, "null arguments");
  CVX_CHECK(sizes_ok(streams, max_gt_ids, max_track_ids), "streams in [1, 65535], max_gt_ids in [1, 1024], max_track_ids in [1, 4096]");
  CVX_CHECK(((uintptr_t)state & 7) == 0, "state is 8-byte aligned");
  static unsigned long long optin = 0;
  CVX_TRY(cvx_lds_optin((const void*)mot_summary_kernel, SUM_LDS_BYTES, &optin));
  hipLaunchKernelGGL(mot_summary_kernel, dim3((unsigned)streams), dim3(THREADS), (size_t)SUM_LDS_BYTES, (hipStream_t)hip_stream, state, max_gt_ids,
                     max_track_ids, (long long*)table);
  hipLaunchKernelGGL(mot_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, (long long*)table, streams);
  CVX_HIP(hipGetLastError());
  return 0;
}
