// A segmented, stable LSD radix sort of (uint32 key, payload) pairs by DESCENDING key, for the Lovasz term of the segmentation criterion
// (loss_seg.hip).  The library's other orderings are a radix SELECT (OHEM, SSD mining) and in-LDS sorts of a few thousand items
// (lds_sort.h); this is the device-wide one.
//
// Segments: nseg runs of capacity q.ng elements each, segment s at element offset s * q.ng of every buffer.  Segment s = (group, class)
// holds nvalid[group] elements -- a count the DEVICE knows, not the host -- so the grid covers the capacity and a tile past the count
// leaves at once, as does every tile of a class without a target pixel under skip_absent (gc[s] == 0).
//
// One pass per 8-bit digit, from the lowest, with bin = 255 - digit so that ascending bins are descending keys:
//   lv_hist     a tile = LV_TILE consecutive elements of one segment; its 256 bin counts -> tilehist[tile][bin]
//   lv_scan     one workgroup per segment, thread = bin: the exclusive running count of its bin over the tiles in order (in place), then
//               the exclusive scan of the 256 bin totals -> binbase[segment][bin]
//   lv_scatter  the tile again: element -> binbase + tilehist + its rank among the tile's elements of the same bin; the tile is put in
//               bin order in LDS first, so that a bin's elements leave as one run of consecutive addresses
// The rank is a count, never an arrival order: a wave owns 256 consecutive elements, taken 64 at a time; the lanes holding one bin are
// found with eight ballots, a lane's rank is the count of such lanes below it plus what the wave has seen of the bin before, and the
// waves' totals are joined in wave order.  So equal keys keep their order in every pass (stable), two calls give the same bits, and
// after the last pass equal keys lie in the order they had on input.
//
// Kernel boundaries are the only synchronisation between workgroups.  Any bit pattern is a key: a digit is 0 .. 255 whatever the
// float behind it was, and the destination, a sum of counts of the same keys, stays inside the segment (the store checks it all the
// same).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

constexpr int LV_TILE = 1024;  // elements per tile: 256 threads x 4

struct LvGeom {
  long long ng;  // capacity of a segment (the pixels of a group), < 2^31
  int tps;       // tiles per segment = cdiv(ng, LV_TILE)
  int nc;        // segments per group
  int skip_absent;
};

struct LvTile {
  long long base;  // element offset of the segment
  int seg, tile, n;
  bool live;
};
// The tile of workgroup blockIdx.x = segment * tps + tile; the answer is the same for every thread of the workgroup.
__device__ __forceinline__ LvTile lv_tile(const LvGeom& q, const int* nvalid, const int* gc) {
  LvTile t;
  t.seg = (int)(blockIdx.x / (unsigned)q.tps);
  t.tile = (int)(blockIdx.x % (unsigned)q.tps);
  t.n = nvalid[t.seg / q.nc];
  t.live = (long long)t.tile * LV_TILE < (long long)t.n && !(q.skip_absent && gc[t.seg] == 0);
  t.base = (long long)t.seg * q.ng;
  return t;
}
__device__ __forceinline__ bool lv_segment_live(const LvGeom& q, const int* nvalid, const int* gc, int seg, int* ntiles) {
  const int n = nvalid[seg / q.nc];
  *ntiles = n > 0 ? (n - 1) / LV_TILE + 1 : 0;
  return n > 0 && !(q.skip_absent && gc[seg] == 0);
}

__device__ __forceinline__ int lv_bin(unsigned key, int shift) { return 255 - (int)((key >> shift) & 255u); }

// Exclusive scan of one value per thread over the 256 threads; *total: the sum.  sh: 256 cells, free again on return.
__device__ __forceinline__ unsigned lv_excl_scan_256(unsigned v, unsigned* sh, unsigned* total) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned a = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0u;
    __syncthreads();
    sh[threadIdx.x] += a;
    __syncthreads();
  }
  const unsigned incl = sh[threadIdx.x];
  *total = sh[255];
  __syncthreads();
  return incl - v;
}

// f[j]: a flag of element j * 256 + threadIdx.x of a tile; rank[j]: how many flagged elements precede it in index order; *total: all of
// them.  Ballots and counts only.  sh: 16 cells, free again on return.  Every thread of the workgroup calls it.
__device__ __forceinline__ void lv_rank4(const bool (&f)[4], unsigned* sh, unsigned (&rank)[4], unsigned* total) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned long long bal = __ballot(f[j] ? 1 : 0);
    rank[j] = (unsigned)__popcll(bal & below);
    if (lane == 0) sh[j * 4 + w] = (unsigned)__popcll(bal);
  }
  __syncthreads();
  unsigned run = 0;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    if ((s & 3) == w) rank[s >> 2] += run;
    run += sh[s];
  }
  *total = run;
  __syncthreads();
}

__global__ __launch_bounds__(256) void lv_hist_kernel(const unsigned* keys, LvGeom q, const int* nvalid, const int* gc, int shift, unsigned* tilehist) {
  __shared__ unsigned h[256];
  const LvTile t = lv_tile(q, nvalid, gc);
  if (!t.live) return;
  h[threadIdx.x] = 0u;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long i = (long long)t.tile * LV_TILE + j * 256 + threadIdx.x;
    if (i < t.n) atomicAdd(&h[lv_bin(keys[t.base + i], shift)], 1u);  // a count: the order of the adds does not show
  }
  __syncthreads();
  tilehist[(long long)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(256) void lv_scan_kernel(LvGeom q, const int* nvalid, const int* gc, unsigned* tilehist, unsigned* binbase) {
  __shared__ unsigned sh[256];
  const int seg = blockIdx.x;
  int nt;
  if (!lv_segment_live(q, nvalid, gc, seg, &nt)) return;
  unsigned* th = tilehist + (long long)seg * q.tps * 256 + threadIdx.x;
  unsigned run = 0u;
  int t = 0;
  for (; t + 8 <= nt; t += 8) {  // eight loads in flight, then the eight stores
    unsigned v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = th[(long long)(t + k) * 256];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      th[(long long)(t + k) * 256] = run;
      run += v[k];
    }
  }
  for (; t < nt; ++t) {
    const unsigned v = th[(long long)t * 256];
    th[(long long)t * 256] = run;
    run += v;
  }
  unsigned total;
  binbase[(long long)seg * 256 + threadIdx.x] = lv_excl_scan_256(run, sh, &total);
}

template <class PL>
__global__ __launch_bounds__(256) void lv_scatter_kernel(const unsigned* kin, const PL* pin, unsigned* kout, PL* pout, LvGeom q, const int* nvalid,
                                                         const int* gc, int shift, const unsigned* tilehist, const unsigned* binbase) {
  __shared__ unsigned seen[4][256];  // per wave: the elements of a bin the wave has ranked so far; in the end the wave's count of the bin
  __shared__ unsigned scan[256], binstart[256], gbase[256], skey[LV_TILE];
  __shared__ PL spay[LV_TILE];
  const LvTile t = lv_tile(q, nvalid, gc);
  if (!t.live) return;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) seen[k][threadIdx.x] = 0u;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned key[4], rank[4];
  PL pay[4];
  int bin[4];
  bool ok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long i = (long long)t.tile * LV_TILE + w * 256 + j * 64 + lane;
    ok[j] = i < t.n;
    key[j] = ok[j] ? kin[t.base + i] : 0u;
    pay[j] = ok[j] ? pin[t.base + i] : PL(0);
    bin[j] = lv_bin(key[j], shift);
    unsigned long long same = __ballot(ok[j] ? 1 : 0);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int bit = (bin[j] >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    rank[j] = ok[j] ? seen[w][bin[j]] + (unsigned)__popcll(same & below) : 0u;
    __syncthreads();  // every lane has read the count before the bin's last lane moves it on
    if (ok[j] && lane == 63 - __clzll((long long)same)) seen[w][bin[j]] += (unsigned)__popcll(same);
    __syncthreads();
  }
  // The tile's elements in bin order in LDS first (a bin's elements in wave order, then rank: their order on input), so that the stores
  // of one bin are one run of consecutive addresses instead of single dwords spread over the 256 bins.
  unsigned total;
  const unsigned start = lv_excl_scan_256(seen[0][threadIdx.x] + seen[1][threadIdx.x] + seen[2][threadIdx.x] + seen[3][threadIdx.x], scan, &total);
  binstart[threadIdx.x] = start;
  // place `slot` of the bin-ordered tile goes to gbase[bin] + slot (modulo 2^32: the bin's start inside the tile is taken off again)
  gbase[threadIdx.x] = binbase[(long long)t.seg * 256 + threadIdx.x] + tilehist[(long long)blockIdx.x * 256 + threadIdx.x] - start;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!ok[j]) continue;
    unsigned at = binstart[bin[j]] + rank[j];
    for (int k = 0; k < w; ++k) at += seen[k][bin[j]];
    if (at < (unsigned)LV_TILE) {  // always true: a sum of counts of the tile's own keys
      skey[at] = key[j];
      spay[at] = pay[j];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned slot = r * 256 + threadIdx.x;
    if (slot >= total) continue;
    const unsigned k = skey[slot];
    const unsigned at = gbase[lv_bin(k, shift)] + slot;
    if (at < (unsigned)t.n) {  // always true: a sum of counts of the segment's own keys
      kout[t.base + at] = k;
      pout[t.base + at] = spay[slot];
    }
  }
}

// One sort: four passes, ping (in, and the result: an even number of passes) and pong.
template <class PL>
inline void lv_sort(unsigned* ka, PL* pa, unsigned* kb, PL* pb, const LvGeom& q, int nseg, const int* nvalid, const int* gc, unsigned* tilehist,
                    unsigned* binbase, hipStream_t st) {
  const unsigned tiles = (unsigned)nseg * (unsigned)q.tps;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(lv_hist_kernel, dim3(tiles), dim3(256), 0, st, (const unsigned*)ka, q, nvalid, gc, shift, tilehist);
    hipLaunchKernelGGL(lv_scan_kernel, dim3((unsigned)nseg), dim3(256), 0, st, q, nvalid, gc, tilehist, binbase);
    hipLaunchKernelGGL(lv_scatter_kernel<PL>, dim3(tiles), dim3(256), 0, st, (const unsigned*)ka, (const PL*)pa, kb, pb, q, nvalid, gc, shift,
                       (const unsigned*)tilehist, (const unsigned*)binbase);
    std::swap(ka, kb);
    std::swap(pa, pb);
  }
}
