// Connected-component regions of uint8 label maps on gfx950: boxes, areas and scores of the connected regions of
// each class, in the detectors' row format, for every frame of a batch.  The rules are in include/cvx_engine.h (cvx_seg_regions) and, as
// the specification, in tests/seg_regions_restatement.py; every quantity is an integer or one rounded division of integers, so the
// kernels are held to the restatement bit for bit.
//
// A union-find over the pixels, every link pointing to a strictly lower linear index y * w + x, so a region's root is its seed.  Five
// launches per call, six with a region map or a clean map, whatever the maps hold:
//   K1 tile     a workgroup per 64 x 32 tile, grid (cdiv(max_w, 64), cdiv(max_h, 32), frames) -- the shape of seg_stitch_kernel.  The tile
//               is labelled entirely in LDS (the lock-free union below on LDS words), and the statistics of every component of the tile
//               are reduced in LDS, a tile row at a time (a row that is one component costs one set of LDS atomics, Guideline 12).  Out:
//               parent[p] = the GLOBAL linear index of p's tile root (-1: not selected); the tile roots carry their component's area, q
//               sum and box, every other selected pixel area 0.
//   K2 border   a thread per pixel of a tile's top row, left column and right column: the unions across tile borders, on the parent
//               plane in global memory.
//   K3 flatten  every selected pixel finds its root and writes it back; a tile root that is not the region's root adds its component's
//               statistics to the root's with integer atomics -- one set per (tile, region) pair, not per pixel, so a region that fills
//               the frame is a few dozen atomics on its root, not h * w.
//   K4 collect  the roots with area >= min_area append themselves to the frame's candidate list through an atomic counter (the order of
//               arrival cannot show: the sort's key is a strict total order).
//   K5 emit     a workgroup per frame sorts the candidates by (area descending, seed ascending) with lds_sort_keys, writes rows, counts,
//               total, areas and seeds and stamps parent[seed] = -2 - row for the emitted ones.
//   K6 map      per pixel: the stamp of its root into the region map, the label or `fill` into the clean map.
//
// Visibility between workgroups (MI355X: the XCDs' L2s are not coherent, a plain load may be stale).  Inside K2 and K3, every value that
// decides something -- "is this word a root", "did my link land", the next step of a walk -- is the return value of an agent-scope atomic
// or a relaxed agent-scope atomic load, never a plain load.  No workgroup waits for another: there is no flag, no spin and no ticket; the
// union retries only when its own atomicMin reports that another link landed first, and every retry continues from a strictly lower
// index, so every walk ends whatever the dispatch order.  Everything else crosses a kernel boundary: K1's plain stores are read by K2,
// K3's atomics by K4, K5's stamps by K6.  A word K3 reads with a plain load (a non-root tile root's statistics) is written by K1 alone.
//
// Workspace: 28 bytes per pixel of a (max_h x max_w) plane per frame -- parent 4, area 4, q sum 8, min_x 4, max_x 4, max_y 4 (min_y is
// the seed's row) -- plus 32 KB of candidates and a counter per frame.
#include "lds_sort.h"
#include "../../include/cvx_engine.h"

namespace {

constexpr int TW = 64, TH = 32, TPX = TW * TH;   // one wave instruction of the tile loops is one tile row
constexpr int TILE_THREADS = 256, PX_PER_THREAD = TPX / TILE_THREADS;
constexpr int BORDER_THREADS = TW + 2 * TH;      // top row, left column, right column
constexpr int REGION_CAP = 8192;                 // candidates per frame the LDS sort holds (MERGE_CAP of tiles.hip)
constexpr int EMIT_THREADS = 1024;
constexpr int FRAME_HEAD = 64;                   // int32 words per frame in front of its candidates; word 0 is the counter

struct ClassMask {
  uint32_t w[8];
};

struct Planes {   // [frames][plane_px] each
  int* parent;
  unsigned* area;
  unsigned long long* qsum;
  int *min_x, *max_x, *max_y;
  int* head;      // [frames][FRAME_HEAD + REGION_CAP]
  long long plane_px;
};

__device__ __forceinline__ bool frame_ok(int h, int w, int max_h, int max_w) {
  return h > 0 && w > 0 && h <= max_h && w <= max_w && (long long)h * w < (1ll << 31);
}
__device__ __forceinline__ bool selected(const ClassMask& m, int c) { return (m.w[c >> 5] >> (c & 31)) & 1u; }

// ---- the lock-free union-find, on LDS words (workgroup scope) or on the parent plane (agent scope) ----
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* P, int a) {
  for (;;) {
    const int p = __hip_atomic_load(P + a, __ATOMIC_RELAXED, SCOPE);
    if (p == a) return a;
    a = p;   // p < a: the walk ends
  }
}
template <int SCOPE>
__device__ __forceinline__ void uf_union(int* P, int a, int b) {
  for (;;) {
    a = uf_find<SCOPE>(P, a);
    b = uf_find<SCOPE>(P, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;   // a was a root and now points to b
    a = old;                // another link landed on a first (old < a): whatever the word holds now, old and b are still to be joined
  }
}

__device__ __forceinline__ unsigned conf_q(float c) {
  // fmaxf / fminf return the other operand for a NaN: NaN -> 0
  return (unsigned)rintf(fminf(fmaxf(c, 0.0f), 1.0f) * 65535.0f);
}

// ---- K1 ----
__global__ __launch_bounds__(TILE_THREADS) void regions_tile_kernel(const cvx_seg_map* __restrict__ label_maps, const int* __restrict__ frame_hw,
                                                                    int max_h, int max_w, ClassMask mask, int conn8,
                                                                    const cvx_seg_plane* __restrict__ conf, Planes ws) {
  __shared__ int s_lab[TPX];
  __shared__ short s_cls[TPX];
  __shared__ unsigned s_area[TPX];
  __shared__ unsigned long long s_q[TPX];
  __shared__ int s_minx[TPX], s_maxx[TPX], s_maxy[TPX];
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
  const int f = blockIdx.z, tid = threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) ws.head[(long long)f * (FRAME_HEAD + REGION_CAP)] = 0;
  const int h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
  if (!frame_ok(h, w, max_h, max_w)) return;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  if (x0 >= w || y0 >= h) return;   // the grid is sized for the largest frame (uniform over the workgroup)
  const cvx_seg_map lm = label_maps[f];
  const float* cdata = conf != nullptr ? conf[f].data : nullptr;
  const long long cpitch = conf != nullptr ? conf[f].pitch : 0;

#pragma unroll
  for (int k = 0; k < PX_PER_THREAD; ++k) {
    const int i = tid + k * TILE_THREADS, gx = x0 + (i & (TW - 1)), gy = y0 + (i >> 6);
    int c = -1;
    if (gx < w && gy < h) {
      c = lm.data[(long long)gy * lm.pitch + gx];
      if (!selected(mask, c)) c = -1;
    }
    s_cls[i] = (short)c;
    s_lab[i] = c >= 0 ? i : -1;
    s_area[i] = 0u;
    s_q[i] = 0ull;
    s_minx[i] = 0x7FFFFFFF;
    s_maxx[i] = -1;
    s_maxy[i] = -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PX_PER_THREAD; ++k) {
    const int i = tid + k * TILE_THREADS, lx = i & (TW - 1), ly = i >> 6;
    const int c = s_cls[i];
    if (c < 0) continue;
    if (lx > 0 && s_cls[i - 1] == c) uf_union<WG>(s_lab, i, i - 1);
    if (ly > 0) {
      if (s_cls[i - TW] == c) uf_union<WG>(s_lab, i, i - TW);
      if (conn8) {
        if (lx > 0 && s_cls[i - TW - 1] == c) uf_union<WG>(s_lab, i, i - TW - 1);
        if (lx < TW - 1 && s_cls[i - TW + 1] == c) uf_union<WG>(s_lab, i, i - TW + 1);
      }
    }
  }
  __syncthreads();   // the forest is final: every find below ends at the component's lowest index
  int root[PX_PER_THREAD];
#pragma unroll
  for (int k = 0; k < PX_PER_THREAD; ++k) {
    const int i = tid + k * TILE_THREADS, lx = i & (TW - 1), gy = y0 + (i >> 6);   // the wave's 64 lanes are one tile row
    const bool sel = s_cls[i] >= 0;
    const int r = sel ? uf_find<WG>(s_lab, i) : -1;
    root[k] = r;
    unsigned q = 0u;
    if (sel && cdata != nullptr) q = conf_q(cdata[(long long)gy * cpitch + x0 + lx]);
    const unsigned long long live = __ballot(sel);
    if (live == 0ull) continue;
    const int first = __ffsll((long long)live) - 1, last = 63 - __clzll((long long)live);
    const int r0 = __shfl(r, first);
    if (__ballot(sel && r != r0) == 0ull) {   // the row's selected pixels are one component: one set of LDS atomics
      unsigned qs = q;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) qs += __shfl_xor(qs, o);   // <= 64 * 65535
      if ((tid & 63) == first) {
        atomicAdd(&s_area[r0], (unsigned)__popcll(live));
        if (cdata != nullptr) atomicAdd(&s_q[r0], (unsigned long long)qs);
        atomicMin(&s_minx[r0], x0 + first);
        atomicMax(&s_maxx[r0], x0 + last);
        atomicMax(&s_maxy[r0], gy);
      }
    } else if (sel) {
      atomicAdd(&s_area[r], 1u);
      if (cdata != nullptr) atomicAdd(&s_q[r], (unsigned long long)q);
      atomicMin(&s_minx[r], x0 + lx);
      atomicMax(&s_maxx[r], x0 + lx);
      atomicMax(&s_maxy[r], gy);
    }
  }
  __syncthreads();
  const long long base = (long long)f * ws.plane_px;
#pragma unroll
  for (int k = 0; k < PX_PER_THREAD; ++k) {
    const int i = tid + k * TILE_THREADS, gx = x0 + (i & (TW - 1)), gy = y0 + (i >> 6);
    if (gx >= w || gy >= h) continue;
    const long long p = base + (long long)gy * w + gx;
    const int r = root[k];
    if (r < 0) {
      ws.parent[p] = -1;
      continue;
    }
    ws.parent[p] = (y0 + (r >> 6)) * w + x0 + (r & (TW - 1));
    if (r == i) {
      ws.area[p] = s_area[i];
      ws.qsum[p] = s_q[i];
      ws.min_x[p] = s_minx[i];
      ws.max_x[p] = s_maxx[i];
      ws.max_y[p] = s_maxy[i];
    } else {
      ws.area[p] = 0u;
    }
  }
}

// ---- K2 ----
__global__ __launch_bounds__(BORDER_THREADS) void regions_border_kernel(const cvx_seg_map* __restrict__ label_maps, const int* __restrict__ frame_hw,
                                                                        int max_h, int max_w, ClassMask mask, int conn8, Planes ws) {
  constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
  const int f = blockIdx.z, tid = threadIdx.x;
  const int h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
  if (!frame_ok(h, w, max_h, max_w)) return;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  if (x0 >= w || y0 >= h) return;
  int lx, ly;
  if (tid < TW) {
    lx = tid, ly = 0;
  } else if (tid < TW + TH) {
    lx = 0, ly = tid - TW;
  } else {
    lx = TW - 1, ly = tid - TW - TH;
  }
  if (ly == 0 && tid >= TW) return;   // the two corners belong to the top row's threads
  const int x = x0 + lx, y = y0 + ly;
  if (x >= w || y >= h) return;
  const cvx_seg_map lm = label_maps[f];
  const uint8_t* row = lm.data + (long long)y * lm.pitch;
  const int c = row[x];
  if (!selected(mask, c)) return;
  int* P = ws.parent + (long long)f * ws.plane_px;
  const int p = y * w + x;
  if (lx == 0 && x > 0 && row[x - 1] == c) uf_union<AG>(P, p, p - 1);
  if (y > 0) {
    const uint8_t* up = row - lm.pitch;
    if (ly == 0 && up[x] == c) uf_union<AG>(P, p, p - w);
    if (conn8) {
      if (x > 0 && (ly == 0 || lx == 0) && up[x - 1] == c) uf_union<AG>(P, p, p - w - 1);
      if (x + 1 < w && (ly == 0 || lx == TW - 1) && up[x + 1] == c) uf_union<AG>(P, p, p - w + 1);
    }
  }
}

// ---- K3 ----
__global__ __launch_bounds__(TILE_THREADS) void regions_flatten_kernel(const int* __restrict__ frame_hw, int max_h, int max_w, int with_q, Planes ws) {
  constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
  const int f = blockIdx.z, tid = threadIdx.x;
  const int h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
  if (!frame_ok(h, w, max_h, max_w)) return;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  if (x0 >= w || y0 >= h) return;
  const long long base = (long long)f * ws.plane_px;
  int* P = ws.parent + base;
#pragma unroll
  for (int k = 0; k < PX_PER_THREAD; ++k) {
    const int i = tid + k * TILE_THREADS, x = x0 + (i & (TW - 1)), y = y0 + (i >> 6);
    if (x >= w || y >= h) continue;
    const int p = y * w + x;
    const int up = __hip_atomic_load(P + p, __ATOMIC_RELAXED, AG);
    if (up < 0 || up == p) continue;   // not selected, or a root (a root's word never changes again)
    const int r = uf_find<AG>(P, up);
    if (r != up) __hip_atomic_store(P + p, r, __ATOMIC_RELAXED, AG);
    const unsigned a = ws.area[base + p];   // K1's, and nothing adds to a word that is not a root's
    if (a == 0u) continue;
    // p was its tile's root for a component of the region: the component's statistics go to the region's root
    __hip_atomic_fetch_add(ws.area + base + r, a, __ATOMIC_RELAXED, AG);
    if (with_q) __hip_atomic_fetch_add(ws.qsum + base + r, ws.qsum[base + p], __ATOMIC_RELAXED, AG);
    __hip_atomic_fetch_min(ws.min_x + base + r, ws.min_x[base + p], __ATOMIC_RELAXED, AG);
    __hip_atomic_fetch_max(ws.max_x + base + r, ws.max_x[base + p], __ATOMIC_RELAXED, AG);
    __hip_atomic_fetch_max(ws.max_y + base + r, ws.max_y[base + p], __ATOMIC_RELAXED, AG);
  }
}

// ---- K4 ----
__global__ __launch_bounds__(TILE_THREADS) void regions_collect_kernel(const int* __restrict__ frame_hw, int max_h, int max_w, int min_area, Planes ws) {
  const int f = blockIdx.z, tid = threadIdx.x;
  const int h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
  if (!frame_ok(h, w, max_h, max_w)) return;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  if (x0 >= w || y0 >= h) return;
  const long long base = (long long)f * ws.plane_px;
  int* head = ws.head + (long long)f * (FRAME_HEAD + REGION_CAP);
#pragma unroll
  for (int k = 0; k < PX_PER_THREAD; ++k) {
    const int i = tid + k * TILE_THREADS, x = x0 + (i & (TW - 1)), y = y0 + (i >> 6);
    if (x >= w || y >= h) continue;
    const int p = y * w + x;
    if (ws.parent[base + p] != p || ws.area[base + p] < (unsigned)min_area) continue;
    const int slot = atomicAdd(head, 1);
    if (slot < REGION_CAP) head[FRAME_HEAD + slot] = p;
  }
}

// ---- K5 ----
__global__ __launch_bounds__(EMIT_THREADS) void regions_emit_kernel(const cvx_seg_map* __restrict__ label_maps, const int* __restrict__ frame_hw,
                                                                    int max_h, int max_w, int max_det, int with_q, float* __restrict__ rows,
                                                                    int* __restrict__ counts, int* __restrict__ total, int* __restrict__ areas,
                                                                    int* __restrict__ seeds, int* __restrict__ overflow, Planes ws) {
  extern __shared__ unsigned long long keys[];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
  const bool ok = frame_ok(h, w, max_h, max_w);
  const int* head = ws.head + (long long)f * (FRAME_HEAD + REGION_CAP);
  const int n = ok ? head[0] : 0;
  const bool over = n > REGION_CAP;   // more than the in-LDS sort holds: flagged, never truncated
  const int kept = over ? 0 : min(n, max_det);
  float* out = rows + (long long)f * max_det * 6;
  if (tid == 0) {
    total[f] = n;
    counts[f] = over ? -1 : kept;
    if (over || !ok) atomicAdd(overflow, 1);
  }
  for (int i = kept + tid; i < max_det; i += EMIT_THREADS) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[i * 6 + k] = 0.0f;
    areas[(long long)f * max_det + i] = -1;
    seeds[(long long)f * max_det + i] = -1;
  }
  if (kept == 0) return;
  const long long base = (long long)f * ws.plane_px;
  for (int i = tid; i < n; i += EMIT_THREADS) {
    const int seed = head[FRAME_HEAD + i];
    keys[i] = ((unsigned long long)(0xFFFFFFFFu - ws.area[base + seed]) << 32) | (unsigned)seed;
  }
  lds_sort_keys<EMIT_THREADS>(keys, n);
  const cvx_seg_map lm = label_maps[f];
  for (int i = tid; i < kept; i += EMIT_THREADS) {
    const unsigned long long key = keys[i];
    const int seed = (int)(unsigned)key;
    const unsigned area = 0xFFFFFFFFu - (unsigned)(key >> 32);
    const int sy = seed / w, sx = seed - sy * w;
    float score = 1.0f;
    if (with_q) score = (float)((double)ws.qsum[base + seed] / ((double)area * 65535.0));
    float* r = out + i * 6;
    r[0] = (float)ws.min_x[base + seed];
    r[1] = (float)sy;   // the seed is the region's first pixel in raster order: its row is min_y
    r[2] = (float)(ws.max_x[base + seed] + 1);
    r[3] = (float)(ws.max_y[base + seed] + 1);
    r[4] = score;
    r[5] = (float)lm.data[(long long)sy * lm.pitch + sx];
    areas[(long long)f * max_det + i] = (int)area;
    seeds[(long long)f * max_det + i] = seed;
    ws.parent[base + seed] = -2 - i;   // the stamp K6 reads; a root that was filtered or cut keeps parent == itself
  }
}

// ---- K6 ----
__global__ __launch_bounds__(TILE_THREADS) void regions_map_kernel(const cvx_seg_map* __restrict__ label_maps, const int* __restrict__ frame_hw,
                                                                   int max_h, int max_w, int min_area, int fill, const int* __restrict__ counts,
                                                                   const cvx_seg_imap* __restrict__ region_maps,
                                                                   const cvx_seg_map* __restrict__ clean_maps, Planes ws) {
  const int f = blockIdx.z, tid = threadIdx.x;
  const int h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
  if (!frame_ok(h, w, max_h, max_w)) return;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  if (x0 >= w || y0 >= h) return;
  int32_t* rmap = region_maps != nullptr ? region_maps[f].data : nullptr;
  const long long rpitch = region_maps != nullptr ? region_maps[f].pitch : 0;
  uint8_t* cmap = clean_maps != nullptr ? clean_maps[f].data : nullptr;
  const long long cpitch = clean_maps != nullptr ? clean_maps[f].pitch : 0;
  if (rmap == nullptr && cmap == nullptr) return;
  const cvx_seg_map lm = label_maps[f];
  const bool flagged = counts[f] < 0;
  const long long base = (long long)f * ws.plane_px;
#pragma unroll
  for (int k = 0; k < PX_PER_THREAD; ++k) {
    const int i = tid + k * TILE_THREADS, x = x0 + (i & (TW - 1)), y = y0 + (i >> 6);
    if (x >= w || y >= h) continue;
    const int p = y * w + x;
    int v = ws.parent[base + p], root = p, stamp = -1;
    bool small = false;
    if (v != -1) {
      if (v >= 0 && v != p) {
        root = v;
        v = ws.parent[base + root];
      }
      if (v <= -2) stamp = -2 - v;
      small = ws.area[base + root] < (unsigned)min_area;
    }
    if (rmap != nullptr) rmap[(long long)y * rpitch + x] = flagged ? -1 : stamp;
    if (cmap != nullptr) cmap[(long long)y * cpitch + x] = small ? (uint8_t)fill : lm.data[(long long)y * lm.pitch + x];
  }
}

Planes regions_layout(cvx_carver& c, long long frames, long long plane_px) {
  const long long px = frames * plane_px;
  Planes ws;
  ws.qsum = c.take<unsigned long long>(px);
  ws.parent = c.take<int>(px);
  ws.area = c.take<unsigned>(px);
  ws.min_x = c.take<int>(px);
  ws.max_x = c.take<int>(px);
  ws.max_y = c.take<int>(px);
  ws.head = c.take<int>(frames * (FRAME_HEAD + REGION_CAP));
  ws.plane_px = plane_px;
  return ws;
}

}  // namespace

extern "C" int64_t cvx_seg_regions_workspace_bytes(int32_t frames, int32_t max_h, int32_t max_w) {
  if (frames <= 0 || max_h <= 0 || max_w <= 0 || (long long)max_h * max_w >= (1ll << 31)) return 0;
  cvx_carver c(nullptr);
  regions_layout(c, frames, (long long)max_h * max_w);
  return c.total();
}

extern "C" int cvx_seg_regions(const cvx_seg_map* label_maps, const int32_t* frame_hw, int32_t frames, int32_t max_h, int32_t max_w,
                               const uint32_t* class_mask_host, int32_t connectivity, int32_t min_area, int32_t max_det, int32_t fill,
                               const cvx_seg_plane* conf, const cvx_seg_imap* region_maps, const cvx_seg_map* clean_maps, float* rows,
                               int32_t* counts, int32_t* total, int32_t* areas, int32_t* seeds, int32_t* overflow, void* workspace,
                               int64_t workspace_bytes, void* hip_stream) {
  CVX_CHECK(label_maps && frame_hw && class_mask_host && rows && counts && total && areas && seeds && overflow && workspace, "null arguments");
  CVX_CHECK(frames > 0 && frames <= 65535 && max_h > 0 && max_w > 0 && (long long)max_h * max_w < (1ll << 31), "bad sizes");
  CVX_CHECK(cvx_cdiv(max_h, TH) <= 65535, "max_h: at most 65535 tile rows");
  CVX_CHECK(connectivity == 4 || connectivity == 8, "connectivity: 4 or 8");
  CVX_CHECK(min_area >= 1, "min_area >= 1");
  CVX_CHECK(max_det >= 1 && max_det <= REGION_CAP, "max_det must lie in [1,8192]");
  CVX_CHECK(clean_maps == nullptr || (fill >= 0 && fill <= 255), "fill: a label byte");
  CVX_CHECK(workspace_bytes >= cvx_seg_regions_workspace_bytes(frames, max_h, max_w), "workspace too small");
  CVX_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace: 8-byte aligned");
  ClassMask mask;
  for (int i = 0; i < 8; ++i) mask.w[i] = class_mask_host[i];
  cvx_carver carver(workspace);
  const Planes ws = regions_layout(carver, frames, (long long)max_h * max_w);
  const hipStream_t s = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)cvx_cdiv(max_w, TW), (unsigned)cvx_cdiv(max_h, TH), (unsigned)frames);
  const int conn8 = connectivity == 8, with_q = conf != nullptr;
  hipLaunchKernelGGL(regions_tile_kernel, grid, dim3(TILE_THREADS), 0, s, label_maps, frame_hw, max_h, max_w, mask, conn8, conf, ws);
  hipLaunchKernelGGL(regions_border_kernel, grid, dim3(BORDER_THREADS), 0, s, label_maps, frame_hw, max_h, max_w, mask, conn8, ws);
  hipLaunchKernelGGL(regions_flatten_kernel, grid, dim3(TILE_THREADS), 0, s, frame_hw, max_h, max_w, with_q, ws);
  hipLaunchKernelGGL(regions_collect_kernel, grid, dim3(TILE_THREADS), 0, s, frame_hw, max_h, max_w, min_area, ws);
  static unsigned long long optin = 0;   // 64 KB of keys: beyond the default dynamic LDS limit
  CVX_TRY(cvx_lds_optin((const void*)regions_emit_kernel, REGION_CAP * 8, &optin));
  hipLaunchKernelGGL(regions_emit_kernel, dim3(frames), dim3(EMIT_THREADS), (size_t)REGION_CAP * 8, s, label_maps, frame_hw, max_h, max_w, max_det,
                     with_q, rows, counts, total, areas, seeds, overflow, ws);
  if (region_maps != nullptr || clean_maps != nullptr)
    hipLaunchKernelGGL(regions_map_kernel, grid, dim3(TILE_THREADS), 0, s, label_maps, frame_hw, max_h, max_w, min_area, fill, counts, region_maps,
                       clean_maps, ws);
  CVX_HIP(hipGetLastError());
  return 0;
}
