// The assignment solver of one workgroup of 1024 threads, shared by the kernels that match one to one: mot_frames_kernel and
// mot_summary_kernel (track_eval.hip) and the optimal association of track_model_kernel (track.hip, section 7ad).
// Shortest augmenting paths with potentials, rows inserted in order: one lane per column keeps the column's slack, potential and visited
// bit in registers, a workgroup reduction takes the arg min (lowest column on a tie), and there is one barrier per step of a path.  A
// forbidden cell costs BIG = 2^27 > 1024 * 65536, so a minimum-cost assignment of the smaller side has the maximal number of allowed pairs
// and, among those, the minimal sum; the potentials reach 1024 * BIG and are 64-bit.  The suites pin every tie bit for bit
// (tests/track_eval_restatement.py:solve), so the solver lives in one place.  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "cvx_common.h"

#include <limits.h>

namespace {

constexpr int SOLVE_THREADS = 1024;           // the workgroup
constexpr int SOLVE_WAVES = SOLVE_THREADS / 64;
constexpr long long BIG = 1ll << 27;          // a forbidden cell
constexpr long long INF = LLONG_MAX / 4;

struct Red {
  long long v;
  int j, pad;
};

__device__ __forceinline__ void red_min(long long& v, int& j, long long ov, int oj) {
  if (ov < v || (ov == v && oj < j)) v = ov, j = oj;
}

struct Solver {   // LDS of the assignment
  long long* u;   // row potentials [n]
  int* p;         // the row of each column, -1 free [m]
  int* way;       // the previous column on the path [m]
  Red* red;       // 2 * SOLVE_WAVES: the partial arg mins of the waves, two steps deep
};

// Minimum-cost assignment of the n rows to n of the m >= n columns (n <= SOLVE_THREADS, m <= CPT * SOLVE_THREADS); cost(i, j) is a 64-bit
// integer.  Rows are inserted in order; in every arg min the lowest column wins a tie.  Lane t owns the columns t, t + SOLVE_THREADS, ...:
// slack, column potential and visited bit in registers.  Leaves s.p; every thread must call it.
template <int CPT, class Cost>
__device__ __forceinline__ void solve(const Solver& s, const Cost& cost, int n, int m) {
  constexpr int THREADS = SOLVE_THREADS, WAVES = SOLVE_WAVES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long v[CPT], minv[CPT];
  bool used[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    v[k] = 0;
    const int j = tid + k * THREADS;
    if (j < m) s.p[j] = -1;
  }
  for (int i = tid; i < n; i += THREADS) s.u[i] = 0;
  __syncthreads();
  int par = 0;
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int k = 0; k < CPT; ++k) minv[k] = INF, used[k] = false;
    int j0 = -1, i0 = i;
    for (;;) {
      const long long ui = s.u[i0];
      long long bv = INF;
      int bj = INT_MAX;
#pragma unroll
      for (int k = 0; k < CPT; ++k) {
        const int j = tid + k * THREADS;
        if (j < m && !used[k]) {
          const long long cur = cost(i0, j) - ui - v[k];
          if (cur < minv[k]) {
            minv[k] = cur;
            s.way[j] = j0;
          }
          red_min(bv, bj, minv[k], j);
        }
      }
      for (int o = 1; o < 64; o <<= 1) {
        const long long ov = __shfl_xor(bv, o);
        const int oj = __shfl_xor(bj, o);
        red_min(bv, bj, ov, oj);
      }
      if (lane == 0) s.red[par * WAVES + wave] = {bv, bj, 0};
      __syncthreads();
      bv = INF, bj = INT_MAX;
      for (int k = 0; k < WAVES; ++k) {
        const Red r = s.red[par * WAVES + k];
        red_min(bv, bj, r.v, r.j);
      }
      par ^= 1;
      const long long delta = bv;
      const int j1 = bj;   // m >= n: a free column always remains, so j1 is a column
#pragma unroll
      for (int k = 0; k < CPT; ++k) {
        const int j = tid + k * THREADS;
        if (j < m) {
          if (used[k]) {
            s.u[s.p[j]] += delta;   // the rows of the visited columns are distinct, and none is row i
            v[k] -= delta;
          } else {
            minv[k] -= delta;
          }
          if (j == j1) used[k] = true;
        }
      }
      if (tid == 0) s.u[i] += delta;
      j0 = j1;
      const int r = s.p[j0];   // p changes only between the barriers below
      if (r < 0) break;
      i0 = r;                  // its potential was not touched in this step: column j1 was not visited
    }
    __syncthreads();
    if (tid == 0) {
      while (j0 >= 0) {
        const int jp = s.way[j0];
        s.p[j0] = jp < 0 ? i : s.p[jp];
        j0 = jp;
      }
    }
    __syncthreads();
  }
}

}  // namespace
