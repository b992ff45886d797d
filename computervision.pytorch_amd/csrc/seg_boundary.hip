// Boundary metrics of uint8 label maps on gfx950: the counts behind trimap mIoU, Boundary IoU and the boundary
// F-score (BF) of a prediction against a target, for every frame of a batch.  The rules are in include/cvx_engine.h (cvx_seg_boundary)
// and, as the specification, in tests/seg_boundary_restatement.py; every quantity is an integer, so the kernels are held to the
// restatement bit for bit and two calls give the same bytes.
//
// All three measures need the Chebyshev distance of a pixel to the nearest label change, capped at the frame's widest band dmax <= 64.
// The square search is separable.  Three launches per call, whatever the maps hold, each a workgroup per 64 x 32 tile, grid
// (cdiv(max_w, 64), cdiv(max_h, 32), frames) -- the shape of seg_stitch_kernel:
//   K1 rows   stages the tile's rows with dmax columns on either side in LDS, voids both maps (G' = G if G < nc; P' = P if G < nc and
//             P < nc; else 255) and writes, per pixel and map, the voided label and the run radius R: the largest r <= dmax with every
//             pixel of [x - r, x + r] that lies in the row equal to the pixel's label.  The edge variant is min(R, x, w - 1 - x) and is
//             not stored.
//   K2 cols   stages the tile's columns with dmax rows above and below (label and R of both maps, 4 bytes per pixel) and takes
//             D(y, x) = min over |j| <= dmax of |j| where row y + j lies outside the picture (edge only) or M[y + j, x] != c, and of
//             max(|j|, R(y + j, x) + 1) elsewhere -- walking |j| upwards and stopping once |j| reaches the best so far.  It counts the
//             trimap and Boundary IoU tables and writes the contour planes: the pixel's class where D^noedge == 1, else 255.
//   K3 near   a tile without a contour pixel ends at once.  The others stage both contour planes of the tile with dmax pixels on every
//             side (255 outside the picture).  Each contour pixel's thread looks for a contour pixel of its class in the other map
//             within two pixels; what is not found there is listed in LDS and searched ring by ring, a wave per listed pixel.  Counts
//             the BF table.
// Nothing crosses workgroups inside a launch: K1's planes are read by K2, K2's by K3, each across a kernel boundary.  No workgroup
// reads what another wrote in the same launch and none waits for another -- no flag, no spin, no ticket -- so nothing can hang.  Every
// loop is bounded by dmax <= 64 or by the tile.
//
// Counts go through per-workgroup uint32 cells in LDS (the scheme of hist_add / hist_flush in seg_tail.h; a tile has 2048 pixels, so a
// cell cannot wrap) and are flushed with one 64-bit atomic per non-zero cell.  The trimap needs K * nc * nc cells: above 4096 of them
// (nc > 22 at K = 8) its counts go to the global table directly.  Boundary IoU (K * nc * 3) and BF (K * nc * 4) always fit.
//
// Workspace: 6 bytes per pixel of a (max_h x max_w) plane per frame -- G', P', R_G, R_P (K1 -> K2) and the two contour planes (K2 -> K3).
#include "cvx_common.h"
#include "../../include/cvx_engine.h"

namespace {

constexpr int TW = 64, TH = 32, TPX = TW * TH;   // one wave instruction of the tile loops is one tile row
constexpr int THREADS = 256, PX_PER_THREAD = TPX / THREADS;
constexpr int HALO = CVX_SEG_BOUNDARY_MAX_WIDTH;  // the LDS windows are laid out for the widest band; a frame stages its own dmax only
constexpr int KMAX = CVX_SEG_BOUNDARY_MAX_WIDTHS;
constexpr int VOIDL = 255;                        // nc <= 255: the byte no class uses
constexpr int ROW_PITCH = TW + 2 * HALO;          // 192: a tile row with its halo
constexpr int COL_ROWS = TH + 2 * HALO;           // 160: a tile column with its halo
constexpr int TRI_CELLS = 4096;                   // uint32 cells of LDS the trimap may take
constexpr int COLS_STAGE = 4 * COL_ROWS * TW;     // K2: label and R of both maps, 40960 bytes
constexpr int NEAR_STAGE = 2 * COL_ROWS * ROW_PITCH;   // K3: both contour planes, 61440 bytes
constexpr int NEAR_LIST = 2 * TPX * 2;            // K3: a uint16 per pixel and direction, 8192 bytes
constexpr int LDS_OPTIN = 112 * 1024;             // K3 at nc = 255, K = 8: 61440 + 8192 + 32640 = 102272

struct Planes {   // [frames][plane_px] each, a frame's rows packed at its own width
  uint8_t *gv, *pv, *rg, *rp, *cg, *cp;
  long long plane_px;
};

// The frame's size and widest band; false for a frame the call skips: a NULL map, a size outside the grid, a width outside 1 .. 64.
// Uniform over the workgroup.
__device__ __forceinline__ bool frame_setup(const cvx_seg_map& pm, const cvx_seg_map& tm, const int* __restrict__ frame_hw,
                                            const int* __restrict__ widths, int K, int f, int max_h, int max_w, int& h, int& w, int& dmax) {
  h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
  dmax = 0;
  if (pm.data == nullptr || tm.data == nullptr || h <= 0 || w <= 0 || h > max_h || w > max_w) return false;
  bool ok = true;
  for (int k = 0; k < K; ++k) {
    const int d = widths[f * K + k];
    ok = ok && d >= 1 && d <= HALO;
    dmax = max(dmax, d);
  }
  return ok;
}

// ---- K1 ----
__global__ __launch_bounds__(THREADS) void boundary_rows_kernel(const cvx_seg_map* __restrict__ pred_maps, const cvx_seg_map* __restrict__ target_maps,
                                                                const int* __restrict__ frame_hw, int max_h, int max_w, int nc,
                                                                const int* __restrict__ widths, int K, Planes ws) {
  __shared__ uint8_t s_g[TH * ROW_PITCH], s_p[TH * ROW_PITCH];
  const int f = blockIdx.z, tid = threadIdx.x;
  const cvx_seg_map pm = pred_maps[f], tm = target_maps[f];
  int h, w, dmax;
  if (!frame_setup(pm, tm, frame_hw, widths, K, f, max_h, max_w, h, w, dmax)) return;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  if (x0 >= w || y0 >= h) return;   // the grid is sized for the largest frame (uniform over the workgroup)
  const int xa = max(x0 - dmax, 0), xb = min(x0 + TW + dmax, w), span = xb - xa;   // the staged columns, all inside the row
  const int rows = min(TH, h - y0);
  for (int i = tid; i < rows * span; i += THREADS) {
    const int ly = i / span, gx = xa + (i - ly * span), gy = y0 + ly;
    const int g = tm.data[(long long)gy * tm.pitch + gx], p = pm.data[(long long)gy * pm.pitch + gx];
    const int at = ly * ROW_PITCH + HALO + gx - x0;   // in [HALO - dmax, HALO + TW + dmax)
    s_g[at] = (uint8_t)(g < nc ? g : VOIDL);
    s_p[at] = (uint8_t)(g < nc && p < nc ? p : VOIDL);
  }
  __syncthreads();
  const long long base = (long long)f * ws.plane_px;
#pragma unroll
  for (int k = 0; k < PX_PER_THREAD; ++k) {
    const int i = tid + k * THREADS, lx = i & (TW - 1), ly = i >> 6, gx = x0 + lx, gy = y0 + ly;
    if (gx >= w || gy >= h) continue;
    const long long q = base + (long long)gy * w + gx;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const uint8_t* row = (m == 0 ? s_g : s_p) + ly * ROW_PITCH + HALO + lx;
      const int c = row[0];
      int r = 0;
      if (c != VOIDL) {
        while (r < dmax) {
          const int n = r + 1;   // gx - n >= xa whenever gx - n >= 0, and gx + n < xb whenever gx + n < w
          if ((gx - n >= 0 && row[-n] != c) || (gx + n < w && row[n] != c)) break;
          r = n;
        }
      }
      (m == 0 ? ws.gv : ws.pv)[q] = (uint8_t)c;
      (m == 0 ? ws.rg : ws.rp)[q] = (uint8_t)r;
    }
  }
}

// D^edge and D^noedge of the pixel at staged row sr, column lx, from the staged labels and run radii of its column
__device__ __forceinline__ void column_distance(const uint8_t* lab, const uint8_t* rad, int sr, int lx, int gx, int gy, int h, int w, int dmax,
                                                int& d_edge, int& d_noedge) {
  const int c = lab[sr * TW + lx];
  if (c == VOIDL) {
    d_edge = d_noedge = 0;
    return;
  }
  const int ex = min(gx, w - 1 - gx);
  int bn = dmax + 1, be = min(dmax + 1, min(gy + 1, h - gy));   // the first row outside the picture, above and below
  for (int a = 0; a <= dmax; ++a) {
    if (a >= bn && a >= be) break;   // every term at |j| = a is at least a
#pragma unroll
    for (int s = -1; s <= 1; s += 2) {
      if (a == 0 && s == 1) continue;
      const int yy = gy + s * a;
      if (yy < 0 || yy >= h) continue;
      const int at = (sr + s * a) * TW + lx;
      if (lab[at] != c) {
        bn = min(bn, a);
        be = min(be, a);
      } else {
        const int r = rad[at];
        bn = min(bn, max(a, r + 1));
        be = min(be, max(a, min(r, ex) + 1));
      }
    }
  }
  d_edge = be;
  d_noedge = bn;
}

// ---- K2 ----
__global__ __launch_bounds__(THREADS) void boundary_cols_kernel(const cvx_seg_map* __restrict__ pred_maps, const cvx_seg_map* __restrict__ target_maps,
                                                                const int* __restrict__ frame_hw, int max_h, int max_w, int nc,
                                                                const int* __restrict__ widths, int K, int tri_in_lds,
                                                                unsigned long long* __restrict__ trimap, unsigned long long* __restrict__ biou,
                                                                uint8_t* __restrict__ planes, Planes ws) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint8_t *s_gv = smem, *s_pv = smem + COL_ROWS * TW, *s_rg = smem + 2 * COL_ROWS * TW, *s_rp = smem + 3 * COL_ROWS * TW;
  unsigned* s_bio = reinterpret_cast<unsigned*>(smem + COLS_STAGE);   // [K][nc][3]
  unsigned* s_tri = s_bio + K * nc * 3;                               // [K][nc][nc] when tri_in_lds
  const int f = blockIdx.z, tid = threadIdx.x;
  const cvx_seg_map pm = pred_maps[f], tm = target_maps[f];
  int h, w, dmax;
  if (!frame_setup(pm, tm, frame_hw, widths, K, f, max_h, max_w, h, w, dmax)) return;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  if (x0 >= w || y0 >= h) return;
  const int bio_cells = K * nc * 3, tri_cells = tri_in_lds ? K * nc * nc : 0;
  for (int i = tid; i < bio_cells + tri_cells; i += THREADS) s_bio[i] = 0u;   // s_tri follows s_bio
  const long long base = (long long)f * ws.plane_px;
  const int ya = max(y0 - dmax, 0), yb = min(y0 + TH + dmax, h), cols = min(TW, w - x0);
  for (int i = tid; i < (yb - ya) * TW; i += THREADS) {
    const int lx = i & (TW - 1), gy = ya + (i >> 6);
    if (lx >= cols) continue;
    const long long q = base + (long long)gy * w + x0 + lx;
    const int at = (gy - y0 + HALO) * TW + lx;   // row in [HALO - dmax, HALO + TH + dmax)
    s_gv[at] = ws.gv[q];
    s_pv[at] = ws.pv[q];
    s_rg[at] = ws.rg[q];
    s_rp[at] = ws.rp[q];
  }
  int wd[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) wd[k] = k < K ? widths[f * K + k] : 0;
  __syncthreads();
#pragma unroll 1
  for (int p = 0; p < PX_PER_THREAD; ++p) {
    const int i = tid + p * THREADS, lx = i & (TW - 1), ly = i >> 6, gx = x0 + lx, gy = y0 + ly;
    if (gx >= w || gy >= h) continue;
    const int sr = ly + HALO;
    int ge, gn, pe, pn;
    column_distance(s_gv, s_rg, sr, lx, gx, gy, h, w, dmax, ge, gn);
    column_distance(s_pv, s_rp, sr, lx, gx, gy, h, w, dmax, pe, pn);
    const int g = s_gv[sr * TW + lx], pv = s_pv[sr * TW + lx];
    const long long q = base + (long long)gy * w + gx;
    ws.cg[q] = (uint8_t)(g != VOIDL && gn == 1 ? g : VOIDL);
    ws.cp[q] = (uint8_t)(pv != VOIDL && pn == 1 ? pv : VOIDL);
    if (planes != nullptr) {
      const long long plane = (long long)max_h * max_w;
      uint8_t* out = planes + (long long)f * 6 * plane + (long long)gy * max_w + gx;
      out[0] = (uint8_t)ge;
      out[plane] = (uint8_t)gn;
      out[2 * plane] = (uint8_t)pe;
      out[3 * plane] = (uint8_t)pn;
    }
    if (g == VOIDL) continue;   // P' is void wherever G' is: the pixel takes part in no count
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k >= K) break;
      const int d = wd[k];
      const bool gb = ge <= d, pb = pv != VOIDL && pe <= d;
      if (gb) atomicAdd(&s_bio[(k * nc + g) * 3 + 1], 1u);
      if (pb) atomicAdd(&s_bio[(k * nc + pv) * 3 + 2], 1u);
      if (gb && pb && g == pv) atomicAdd(&s_bio[(k * nc + g) * 3 + 0], 1u);
      if (pv != VOIDL && gn <= d) {
        const int cell = (k * nc + g) * nc + pv;
        if (tri_in_lds)
          atomicAdd(&s_tri[cell], 1u);
        else
          atomicAdd(trimap + cell, 1ull);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < bio_cells; i += THREADS) {
    const unsigned v = s_bio[i];
    if (v) atomicAdd(biou + i, (unsigned long long)v);
  }
  for (int i = tid; i < tri_cells; i += THREADS) {
    const unsigned v = s_tri[i];
    if (v) atomicAdd(trimap + i, (unsigned long long)v);
  }
}

// The Chebyshev distance from the window's centre pixel to the nearest pixel that holds c, dmax + 1 when none lies within dmax.  The
// whole wave searches for one pixel: ring d has 8 d cells -- the top row, the bottom row, then the left and the right column without
// their corners -- which the lanes share; a ballot ends the search at the first ring with a hit.  A thread of its own per pixel would
// hold its wave for the longest search among 64 pixels, and a pixel whose class the other map lacks nearby looks at (2 dmax + 1)^2 cells.
// Starts at ring `first`: the rings below it were the pixel's own thread's (nearest_own).
__device__ __forceinline__ int nearest_in_window(const uint8_t* centre, int c, int first, int dmax, int lane) {
  for (int d = first; d <= dmax; ++d) {
    const int side = 2 * d + 1, cells = 8 * d;
    bool hit = false;
    for (int t = lane; t < cells; t += CVX_WAVE) {
      int dy, dx;
      if (t < side) {
        dy = -d, dx = t - d;
      } else if (t < 2 * side) {
        dy = d, dx = t - side - d;
      } else if (t < 3 * side - 2) {
        dx = -d, dy = t - 2 * side - d + 1;
      } else {
        dx = d, dy = t - (3 * side - 2) - d + 1;
      }
      hit |= centre[dy * ROW_PITCH + dx] == c;
    }
    if (__ballot(hit) != 0ull) return d;
  }
  return dmax + 1;
}

// The same within NEAR_OWN rings, by one thread: where a prediction is near its target most searches end here.  -1: not found.
constexpr int NEAR_OWN = 2;
__device__ __forceinline__ int nearest_own(const uint8_t* centre, int c, int dmax) {
  if (centre[0] == c) return 0;
  const int last = min(dmax, NEAR_OWN);
  for (int d = 1; d <= last; ++d) {
    bool hit = false;
    for (int t = -d; t <= d; ++t)
      hit |= centre[-d * ROW_PITCH + t] == c || centre[d * ROW_PITCH + t] == c || centre[t * ROW_PITCH - d] == c || centre[t * ROW_PITCH + d] == c;
    if (hit) return d;
  }
  return -1;
}

// One finished search of a contour pixel of class c: its plane byte, and (mp, cp) or, swapped, (mg, cg) of every width
__device__ __forceinline__ void near_record(unsigned* s_bf, uint8_t* out, int c, int n, int swapped, int nc, int K, const int* wd) {
  if (out != nullptr) *out = (uint8_t)(n + 1);
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k >= K) break;
    unsigned* cell = &s_bf[(k * nc + c) * 4 + 2 * swapped];
    atomicAdd(cell + 1, 1u);
    if (n <= wd[k]) atomicAdd(cell, 1u);
  }
}

// ---- K3 ----
__global__ __launch_bounds__(THREADS) void boundary_near_kernel(const cvx_seg_map* __restrict__ pred_maps, const cvx_seg_map* __restrict__ target_maps,
                                                                const int* __restrict__ frame_hw, int max_h, int max_w, int nc,
                                                                const int* __restrict__ widths, int K, unsigned long long* __restrict__ bf,
                                                                uint8_t* __restrict__ planes, Planes ws) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint8_t *s_cg = smem, *s_cp = smem + COL_ROWS * ROW_PITCH;
  unsigned short* s_list = reinterpret_cast<unsigned short*>(smem + NEAR_STAGE);   // [2 * TPX]: the tile's searches
  unsigned* s_bf = reinterpret_cast<unsigned*>(smem + NEAR_STAGE + NEAR_LIST);       // [K][nc][4]
  __shared__ int s_count;
  const int f = blockIdx.z, tid = threadIdx.x;
  const cvx_seg_map pm = pred_maps[f], tm = target_maps[f];
  int h, w, dmax;
  if (!frame_setup(pm, tm, frame_hw, widths, K, f, max_h, max_w, h, w, dmax)) return;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  if (x0 >= w || y0 >= h) return;
  const long long base = (long long)f * ws.plane_px;
  // Most tiles of a real map hold no contour pixel: they count nothing and need no window (30 times the tile's own bytes at dmax = 64).
  int any = 0;
#pragma unroll
  for (int p = 0; p < PX_PER_THREAD; ++p) {
    const int i = tid + p * THREADS, gx = x0 + (i & (TW - 1)), gy = y0 + (i >> 6);
    if (gx >= w || gy >= h) continue;
    const long long q = base + (long long)gy * w + gx;
    any |= ws.cg[q] != VOIDL || ws.cp[q] != VOIDL;
  }
  if (!__syncthreads_or(any)) {   // uniform over the workgroup
    if (planes != nullptr) {
      const long long plane = (long long)max_h * max_w;
#pragma unroll
      for (int p = 0; p < PX_PER_THREAD; ++p) {
        const int i = tid + p * THREADS, gx = x0 + (i & (TW - 1)), gy = y0 + (i >> 6);
        if (gx >= w || gy >= h) continue;
        uint8_t* out = planes + ((long long)f * 6 + 4) * plane + (long long)gy * max_w + gx;
        out[0] = 0;
        out[plane] = 0;
      }
    }
    return;
  }
  const int bf_cells = K * nc * 4;
  for (int i = tid; i < bf_cells; i += THREADS) s_bf[i] = 0u;
  const int win_w = TW + 2 * dmax, win_h = TH + 2 * dmax;   // the whole window is written: 255 outside the picture
  for (int i = tid; i < win_h * win_w; i += THREADS) {
    const int wy = i / win_w, wx = i - wy * win_w, gy = y0 - dmax + wy, gx = x0 - dmax + wx;
    int cg = VOIDL, cp = VOIDL;
    if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
      const long long q = base + (long long)gy * w + gx;
      cg = ws.cg[q];
      cp = ws.cp[q];
    }
    const int at = (wy + HALO - dmax) * ROW_PITCH + wx + HALO - dmax;
    s_cg[at] = (uint8_t)cg;
    s_cp[at] = (uint8_t)cp;
  }
  int wd[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) wd[k] = k < K ? widths[f * K + k] : 0;
  if (tid == 0) s_count = 0;
  __syncthreads();
  // Every contour pixel looks at its first rings itself; what it does not find there is listed for the waves: pixel * 2 + (0:
  // prediction -> target, 1: target -> prediction)
  const long long plane = (long long)max_h * max_w;
  uint8_t* const near_planes = planes != nullptr ? planes + ((long long)f * 6 + 4) * plane : nullptr;
#pragma unroll 1
  for (int p = 0; p < PX_PER_THREAD; ++p) {
    const int i = tid + p * THREADS, lx = i & (TW - 1), ly = i >> 6, gx = x0 + lx, gy = y0 + ly;
    if (gx >= w || gy >= h) continue;
    const int at = (ly + HALO) * ROW_PITCH + lx + HALO;
#pragma unroll
    for (int swapped = 0; swapped < 2; ++swapped) {
      const int c = (swapped ? s_cg : s_cp)[at];
      uint8_t* out = near_planes != nullptr ? near_planes + swapped * plane + (long long)gy * max_w + gx : nullptr;
      if (c == VOIDL) {   // off the contour
        if (out != nullptr) *out = 0;
        continue;
      }
      int n = nearest_own((swapped ? s_cp : s_cg) + at, c, dmax);
      if (n < 0 && dmax <= NEAR_OWN) n = dmax + 1;
      if (n >= 0)
        near_record(s_bf, out, c, n, swapped, nc, K, wd);
      else
        s_list[atomicAdd(&s_count, 1)] = (unsigned short)(i * 2 + swapped);
    }
  }
  __syncthreads();
  const int searches = s_count, lane = tid & (CVX_WAVE - 1);
  for (int e = tid / CVX_WAVE; e < searches; e += THREADS / CVX_WAVE) {   // uniform over the wave
    const int code = s_list[e], i = code >> 1, swapped = code & 1;
    const int lx = i & (TW - 1), ly = i >> 6, at = (ly + HALO) * ROW_PITCH + lx + HALO;
    const int c = (swapped ? s_cg : s_cp)[at];
    const int n = nearest_in_window((swapped ? s_cp : s_cg) + at, c, NEAR_OWN + 1, dmax, lane);
    if (lane == 0)
      near_record(s_bf, near_planes != nullptr ? near_planes + swapped * plane + (long long)(y0 + ly) * max_w + x0 + lx : nullptr, c, n, swapped, nc,
                  K, wd);
  }
  __syncthreads();
  for (int i = tid; i < bf_cells; i += THREADS) {
    const unsigned v = s_bf[i];
    if (v) atomicAdd(bf + i, (unsigned long long)v);
  }
}

Planes boundary_layout(cvx_carver& c, long long frames, long long plane_px) {
  const long long px = frames * plane_px;
  Planes ws;
  ws.gv = c.take<uint8_t>(px);
  ws.pv = c.take<uint8_t>(px);
  ws.rg = c.take<uint8_t>(px);
  ws.rp = c.take<uint8_t>(px);
  ws.cg = c.take<uint8_t>(px);
  ws.cp = c.take<uint8_t>(px);
  ws.plane_px = plane_px;
  return ws;
}

}  // namespace

extern "C" int64_t cvx_seg_boundary_workspace_bytes(int32_t frames, int32_t max_h, int32_t max_w) {
  if (frames <= 0 || max_h <= 0 || max_w <= 0 || (long long)max_h * max_w >= (1ll << 31)) return 0;
  cvx_carver c(nullptr);
  boundary_layout(c, frames, (long long)max_h * max_w);
  return c.total();
}

extern "C" int cvx_seg_boundary(const cvx_seg_map* pred_maps, const cvx_seg_map* target_maps, const int32_t* frame_hw, int32_t frames, int32_t max_h,
                                int32_t max_w, int32_t nc, const int32_t* widths, int32_t K, int64_t* trimap, int64_t* biou, int64_t* bf,
                                uint8_t* planes, void* workspace, int64_t workspace_bytes, void* hip_stream) {
  CVX_CHECK(pred_maps && target_maps && frame_hw && widths && trimap && biou && bf && workspace, "null arguments");
  CVX_CHECK(frames > 0 && frames <= 65535 && max_h > 0 && max_w > 0, "bad sizes");
  CVX_CHECK((long long)max_h * max_w < (1ll << 31), "max_h * max_w stays below 2^31");
  CVX_CHECK(cvx_cdiv(max_h, TH) <= 65535, "max_h: at most 65535 tile rows");
  CVX_CHECK(nc >= 1 && nc <= 255, "nc lies in [1,255]: 255 is the void byte");
  CVX_CHECK(K >= 1 && K <= KMAX, "K lies in [1,8]");
  CVX_CHECK(workspace_bytes >= cvx_seg_boundary_workspace_bytes(frames, max_h, max_w), "workspace too small");
  cvx_carver carver(workspace);
  const Planes ws = boundary_layout(carver, frames, (long long)max_h * max_w);
  const hipStream_t s = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)cvx_cdiv(max_w, TW), (unsigned)cvx_cdiv(max_h, TH), (unsigned)frames);
  const int tri_in_lds = (long long)K * nc * nc <= TRI_CELLS;
  const size_t cols_lds = COLS_STAGE + 4 * ((size_t)K * nc * 3 + (tri_in_lds ? (size_t)K * nc * nc : 0));
  const size_t near_lds = NEAR_STAGE + NEAR_LIST + 4 * (size_t)K * nc * 4;
  static unsigned long long optin_cols = 0, optin_near = 0;   // beyond the default dynamic LDS limit at large nc
  CVX_TRY(cvx_lds_optin((const void*)boundary_cols_kernel, LDS_OPTIN, &optin_cols));
  CVX_TRY(cvx_lds_optin((const void*)boundary_near_kernel, LDS_OPTIN, &optin_near));
  hipLaunchKernelGGL(boundary_rows_kernel, grid, dim3(THREADS), 0, s, pred_maps, target_maps, frame_hw, max_h, max_w, nc, widths, K, ws);
  hipLaunchKernelGGL(boundary_cols_kernel, grid, dim3(THREADS), cols_lds, s, pred_maps, target_maps, frame_hw, max_h, max_w, nc, widths, K,
                     tri_in_lds, reinterpret_cast<unsigned long long*>(trimap), reinterpret_cast<unsigned long long*>(biou), planes, ws);
  hipLaunchKernelGGL(boundary_near_kernel, grid, dim3(THREADS), near_lds, s, pred_maps, target_maps, frame_hw, max_h, max_w, nc, widths, K,
                     reinterpret_cast<unsigned long long*>(bf), planes, ws);
  CVX_HIP(hipGetLastError());
  return 0;
}
