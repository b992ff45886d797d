// Device helpers shared by the BatchNorm streaming passes (bn_act.hip) and the fp32 stem kernels (stem.hip).
#pragma once
#include "bn_act.h"

namespace cvx_bn {

__device__ __forceinline__ long long view_off(const ViewDesc& v, long long m, int hw) {
  if (v.bstride == (long long)hw * v.ld) return m * v.ld;  // images are back to back (block-uniform test): no division
  const unsigned mu = (unsigned)m;  // M < 2^32 (checked on the host): one 32-bit division per row
  const unsigned b = mu / (unsigned)hw;
  const unsigned pix = mu - b * (unsigned)hw;
  return (long long)b * v.bstride + (long long)pix * v.ld;
}

// LDS bytes the callers of fold_replicas set aside for C channels (their own arrays follow at this offset): the result, [2 values][C]
// doubles, takes the first half
__host__ __device__ constexpr int fold_ws_bytes(int C) { return C * 2 * CVX_FIX_WORDS * 8; }

// Sums the cvx_stat_replicas(C) fixed-point slabs [R][C][2][CVX_FIX_WORDS] and leaves the two per-channel totals as doubles
// in ws: value q of channel c at ((double*)ws)[q * C + c].  A thread owns (channel, value) pairs cv = thread, thread + 256, ...
// and adds their R replica entries in REGISTERS: integer adds, exact and order-independent, so every block of every launch
// gets the same bits whatever the order.  All loads of a round are requested before the first is used (one memory latency;
// consecutive threads read consecutive 16-byte entries of a slab), and the only LDS traffic is the result and ONE barrier.
// (Until this form the entries went through 64-bit LDS atomics -- zeroed accumulators, four barriers -- from a loop of one
// load and its adds per trip, which compiled to a wait per trip: R * C / 128 = 4 dependent latencies on every layer up to
// 256 channels.)  Every thread of the 256-thread block must call it; it ends with a barrier.
template <int R>
__device__ __forceinline__ void fold_replicas_of(const long long* part, int C, double* out) {
  constexpr int RB = R < 8 ? R : 8;   // replica entries of one pair in flight
  constexpr int KU = 8 / RB;          // pairs per thread and round: 8 loads of 16 bytes in flight
  const int ncv = C * 2;
  for (int cv0 = threadIdx.x; cv0 < ncv; cv0 += 256 * KU) {
    unsigned long long hi[KU], lo[KU];
#pragma unroll
    for (int k = 0; k < KU; ++k) hi[k] = lo[k] = 0;
#pragma unroll
    for (int r0 = 0; r0 < R; r0 += RB) {
      longlong2 q[KU][RB];
      // pairs past the end re-read the last one and are dropped below: a branch-free load (a select between a load and a
      // constant makes the compiler branch, and wait, per element)
#pragma unroll
      for (int k = 0; k < KU; ++k)
#pragma unroll
        for (int r = 0; r < RB; ++r)
          q[k][r] = *reinterpret_cast<const longlong2*>(part + ((long long)(r0 + r) * ncv + min(cv0 + 256 * k, ncv - 1)) * CVX_FIX_WORDS);
#pragma unroll
      for (int k = 0; k < KU; ++k)
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          hi[k] += (unsigned long long)q[k][r].x;
          lo[k] += (unsigned long long)q[k][r].y;
        }
    }
#pragma unroll
    for (int k = 0; k < KU; ++k) {
      const int cv = cv0 + 256 * k;  // channel * 2 + value
      if (cv < ncv) out[(cv & 1) * C + (cv >> 1)] = cvx_fix_to_double((long long)hi[k], (long long)lo[k]);
    }
  }
}
__device__ __forceinline__ void fold_replicas(const long long* part, int C, long long* ws) {
  double* out = reinterpret_cast<double*>(ws);
  switch (cvx_stat_replicas(C)) {  // block-uniform
    case 16: fold_replicas_of<16>(part, C, out); break;
    case 8: fold_replicas_of<8>(part, C, out); break;
    case 4: fold_replicas_of<4>(part, C, out); break;
    case 2: fold_replicas_of<2>(part, C, out); break;
    default: fold_replicas_of<1>(part, C, out); break;
  }
  __syncthreads();
}

// block-level accumulation of per-thread channel sums, bit-reproducible.  Lanes of a wave that share a channel group
// (lane % CG, when CG divides 64) are folded with a fixed xor-butterfly; each wave parks its CG*8*NV sums in its own
// LDS slot; NV*C threads add the four wave slots in fixed order and issue ONE fixed-point atomic add per value.
// Channel-group counts that do not divide 64 (C = 80, 144: Detect head) take the parked-partials column walk instead.
// part: replica slabs [R][C][2] fixed-point values; NV = 1 fills value 0 only.
// rep_block: the block's ordinal among the blocks that feed `part` (picks the replica slab)
template <int NV>
__device__ __forceinline__ void block_channel_sums(float (&v)[NV][8], int C, int CG, int cg, bool active, float* sred, long long* part,
                                                   int rep_block) {
  const bool pow2 = (64 % CG) == 0;
  if (pow2) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float x = v[q][i];  // every thread is active when CG divides 64 (RP * CG == 256)
        for (int o = CG; o < 64; o <<= 1) x += __shfl_xor(x, o);
        if (lane < CG) sred[(wave * C + cg * 8 + i) * NV + q] = x;
      }
    __syncthreads();
    for (int j = threadIdx.x; j < NV * C; j += 256) {
      const int c = j / NV, q = j - c * NV;
      const float acc = (sred[(0 * C + c) * NV + q] + sred[(1 * C + c) * NV + q]) + (sred[(2 * C + c) * NV + q] + sred[(3 * C + c) * NV + q]);
      cvx_fix_atomic_add(part, ((long long)(rep_block % cvx_stat_replicas(C)) * C + c) * 2 + q, acc);
    }
    return;
  }
  const int RP = 256 / CG;
  if (active) {
    float* dst = sred + (size_t)threadIdx.x * (NV * 8);
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int i = 0; i < 8; ++i) dst[q * 8 + i] = v[q][i];
  }
  __syncthreads();
  for (int j = threadIdx.x; j < NV * C; j += 256) {
    const int c = j / NV, q = j - c * NV;
    const int g = c >> 3, i = c & 7;
    float acc = 0.f;
    for (int r = 0; r < RP; ++r) acc += sred[(size_t)(r * CG + g) * (NV * 8) + q * 8 + i];
    cvx_fix_atomic_add(part, ((long long)(rep_block % cvx_stat_replicas(C)) * C + c) * 2 + q, acc);
  }
}

// batch statistics of C channels from the folded sums (ws as left by fold_replicas) -> mean / invstd (fp32, LDS or
// registers of the caller); thread 0's block also publishes them and updates the running statistics.
struct BnMoments {
  float mean, invstd;
};
__device__ __forceinline__ BnMoments moments_of(const long long* ws, int C, int c, long long M, float eps, double* var_out) {
  const double* s = reinterpret_cast<const double*>(ws);
  const double cnt = (double)M;
  const double mu = s[c] / cnt;
  double var = s[C + c] / cnt - mu * mu;
  if (var < 0.0) var = 0.0;
  if (var_out) *var_out = var;
  return BnMoments{(float)mu, (float)(1.0 / sqrt(var + (double)eps))};
}

}  // namespace cvx_bn
