// Sliding-window segmentation on gfx950: a large frame is cut into overlapping tiles at network size
// (render.tile_grid, cvx_tiles_u8_to_nchw), every tile runs through the network, and this file stitches the tiles' logits back into the
// frame.  Nothing is read by the host and no full-resolution logits exist in memory.
//
//   K1 seg_stitch   a thread per 4 neighbouring pixels of a frame row, grid (cdiv(max_w, 1024), max_h, frames) -- the shape of
//                   seg_overlay_kernel (render.hip).  The tile grid of a frame is the product of its y tiles and its x tiles, so a pixel
//                   scans ny + nx table entries.  Per covering tile, row-major: the tile-local pixel, the taps of bilinear.h at the scale
//                   of a full network input (the number cvx_resize_bilinear_rows_to_nchw has for that slot), the weight (1, or the
//                   integer distance-to-border product), acc = fma(w, z, acc).  No division by the weight sum: the arg max (strict >, the
//                   lowest class wins a tie) does not need it.  Then the label byte, the 50/50 palette blend into the frame in place, and
//                   confusion[target][label] += 1 through a per-workgroup LDS histogram that is flushed with one 64-bit atomic per
//                   non-zero entry.  The arg max, the pixel quad and the histogram are seg_tail.h's.
//                   The y side (covering ty range, taps, row weight) is the same for the whole workgroup: it is worked out once into LDS,
//                   not per class chunk.  Classes go four at a time with the tile loop inside, so no nc-sized register array exists; 16
//                   accumulators per thread.  HBM sees 1 label byte + 3 read + 3 written frame bytes per pixel; the taps come from L2
//                   (a slot's logits are ~1.6 MB at 513 x 513 and every value is read by about 16 pixels) and are what the launch
//                   costs: 0.55 ms for two 1024 x 2048 frames, with or without the overlay and the counts.
// Every fp32 step is one rounded operation, so the file is compiled with contraction off (bilinear.h spells its fused steps out) and
// tests/seg_tiled_restatement.py holds the kernel to the bit.
#include "seg_tail.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int STITCH_THREADS = 256;
constexpr int Y_STASH = 16;          // covering y tiles whose taps are kept in LDS; further ones (overlap > 0.93) are worked out on the fly
constexpr int COUNT_MAX_NC = 128;    // nc * nc int32 histogram entries = 64 KB

struct YTap {
  int slot0;   // slot of tile (ty, 0)
  int i0, i1;  // feature rows
  int wy;      // min(dy + 1, th - dy), 0: the tile does not cover the row
  float lam;
};

__device__ __forceinline__ YTap y_tap(const int* __restrict__ ay, int ty, int y, int first_slot, int nx, float scale, int lh) {
  YTap t;
  const int y0 = ay[2 * ty], th = ay[2 * ty + 1], dy = y - y0;
  bilinear_src(dy, scale, lh, &t.i0, &t.i1, &t.lam);   // clamped into [0, lh - 1] whatever dy is
  t.wy = dy >= 0 && dy < th ? min(dy + 1, th - dy) : 0;
  t.slot0 = first_slot + ty * nx;
  return t;
}

__global__ __launch_bounds__(STITCH_THREADS) void seg_stitch_kernel(const float* __restrict__ logits, int slots, int ld, int nc, int lh, int lw, int NH,
                                                                    int NW, const cvx_seg_tile_frame* __restrict__ table,
                                                                    const int* __restrict__ axes, int n_axes,
                                                                    const cvx_frame_job* __restrict__ jobs,
                                                                    const cvx_seg_map* __restrict__ label_maps,
                                                                    const cvx_seg_map* __restrict__ target_maps,
                                                                    unsigned long long* __restrict__ confusion, const uint8_t* __restrict__ lut,
                                                                    int linear, int draw, int bgr_out) {
  extern __shared__ unsigned char smem[];
  YTap* stash = reinterpret_cast<YTap*>(smem);
  unsigned* hist = reinterpret_cast<unsigned*>(smem + Y_STASH * sizeof(YTap));
  const cvx_frame_job jb = jobs[blockIdx.z];
  const cvx_seg_tile_frame tf = table[blockIdx.z];
  const int h = jb.h, w = jb.w, y = blockIdx.y;
  if (y >= h || (int)blockIdx.x * 1024 >= w) return;   // the grid is sized for the largest frame (uniform over the workgroup)
  const int ny = tf.ny, nx = tf.nx;
  if (ny <= 0 || nx <= 0 || tf.y_off < 0 || tf.x_off < 0 || (long long)tf.y_off + 2ll * ny > n_axes || (long long)tf.x_off + 2ll * nx > n_axes)
    return;                                            // a table that points outside the axis array stitches nothing
  const int* ay = axes + tf.y_off;
  const int* ax = axes + tf.x_off;
  const int tid = threadIdx.x, x0 = (blockIdx.x * STITCH_THREADS + tid) * 4;
  const bool count = confusion != nullptr && target_maps != nullptr && target_maps[blockIdx.z].data != nullptr;
  const float sy = (float)lh / (float)NH, sx = (float)lw / (float)NW;

  // ---- the y side, once per workgroup: the covering ty range and its taps ----
  int ty_lo = ny, ty_hi = -1;
  for (int ty = 0; ty < ny; ++ty) {
    const int d = y - ay[2 * ty];
    if (d >= 0 && d < ay[2 * ty + 1]) {
      ty_lo = min(ty_lo, ty);
      ty_hi = ty;
    }
  }
  if (tid <= ty_hi - ty_lo && tid < Y_STASH) stash[tid] = y_tap(ay, ty_lo + tid, y, tf.first_slot, nx, sy, lh);
  if (count) hist_zero<STITCH_THREADS>(hist, nc);
  __syncthreads();

  const int npx = min(4, w - x0);   // <= 0: this thread has no pixel, it only helps with the histogram
  // ---- the x side: the tiles that cover any of this thread's pixels ----
  int tx_lo = nx, tx_hi = -1;
  if (npx > 0)
    for (int tx = 0; tx < nx; ++tx) {
      const int s = ax[2 * tx];
      if (s <= x0 + npx - 1 && s + ax[2 * tx + 1] > x0) {
        tx_lo = min(tx_lo, tx);
        tx_hi = tx;
      }
    }

  uint8_t* p = jb.data + (long long)y * jb.stride + (long long)x0 * 3;
  const bool wide = draw && quad_is_wide(jb.data, jb.stride, npx);
  pixel_quad px;
  if (draw) quad_load(p, npx, wide, px);

  const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  const long long slot_stride = (long long)lh * lw * ld;
  float best[4] = {0.f, 0.f, 0.f, 0.f};
  int arg[4] = {0, 0, 0, 0};
  for (int c0 = 0; c0 < nc; c0 += 4) {
    float acc[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[k][i] = 0.f;
    for (int ty = ty_lo; ty <= ty_hi; ++ty) {      // row-major over the covering tiles: ty outer, tx inner
      const YTap t = ty - ty_lo < Y_STASH ? stash[ty - ty_lo] : y_tap(ay, ty, y, tf.first_slot, nx, sy, lh);
      if (t.wy == 0) continue;
      for (int tx = tx_lo; tx <= tx_hi; ++tx) {
        const int tx0 = ax[2 * tx], tw = ax[2 * tx + 1], slot = t.slot0 + tx;
        if (slot < 0 || slot >= slots) continue;   // a table that names a slot the logits do not have
        const float* ra = logits + slot * slot_stride + (long long)t.i0 * lw * ld + c0;
        const float* rb = logits + slot * slot_stride + (long long)t.i1 * lw * ld + c0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int dx = x0 + k - tx0;
          if (k >= npx || dx < 0 || dx >= tw) continue;
          int xa, xb;
          float lx;
          bilinear_src(dx, sx, lw, &xa, &xb, &lx);
          const float wk = linear ? (float)(t.wy * min(dx + 1, tw - dx)) : 1.0f;   // an integer below 2^24: exact
          // the chunk of seg_tail.h's logits4, kept in line: through the helper this loop compiled to a different schedule that measured
          // 3.5 % slower (0.57 against 0.55 ms for two 1024 x 2048 frames, profiles/eval_tail_refactor_ab.txt)
          const float *r00 = ra + (long long)xa * ld, *r01 = ra + (long long)xb * ld;
          const float *r10 = rb + (long long)xa * ld, *r11 = rb + (long long)xb * ld;
          float z[4];
          if (vec && c0 + 4 <= ld) {
            const f4 a = *reinterpret_cast<const f4*>(r00), b = *reinterpret_cast<const f4*>(r01);
            const f4 c = *reinterpret_cast<const f4*>(r10), d = *reinterpret_cast<const f4*>(r11);
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = bilinear_mix(a[i], b[i], c[i], d[i], lx, t.lam);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = c0 + i < nc ? bilinear_mix(r00[i], r01[i], r10[i], r11[i], lx, t.lam) : 0.f;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[k][i] = __builtin_fmaf(wk, z[i], acc[k][i]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) argmax4(acc[k], c0, nc, best[k], arg[k]);
  }

  if (npx > 0) {
    // ---- the label bytes ----
    if (label_maps != nullptr && label_maps[blockIdx.z].data != nullptr) {
      const cvx_seg_map lm = label_maps[blockIdx.z];
      uint8_t* q = lm.data + (long long)y * lm.pitch + x0;
      if (npx == 4 && ((reinterpret_cast<uintptr_t>(lm.data) | (uintptr_t)lm.pitch) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(q) = (uint32_t)arg[0] | (uint32_t)arg[1] << 8 | (uint32_t)arg[2] << 16 | (uint32_t)arg[3] << 24;
      } else {
        for (int k = 0; k < npx; ++k) q[k] = (uint8_t)arg[k];
      }
    }
    // ---- the overlay, in place ----
    if (draw) {
      for (int k = 0; k < npx; ++k) quad_blend(px, k, lut + 3 * arg[k], bgr_out);
      quad_store(p, npx, wide, px);
    }
    // ---- the confusion counts of this row segment ----
    if (count) {
      const cvx_seg_map tm = target_maps[blockIdx.z];
      const uint8_t* q = tm.data + (long long)y * tm.pitch + x0;
      for (int k = 0; k < npx; ++k) {
        const int tg = q[k];
        if (tg < nc) hist_add(hist, nc, tg, arg[k]);
      }
    }
  }
  if (count) hist_flush<STITCH_THREADS>(hist, nc, confusion);
}

}  // namespace

extern "C" int cvx_seg_stitch(const float* logits_rows, int32_t slots, int32_t ld, int32_t nc, int32_t lh, int32_t lw, int32_t net_h, int32_t net_w,
                              const cvx_seg_tile_frame* tile_frames, const int32_t* tile_axes, int32_t n_axes, const cvx_frame_job* jobs,
                              int32_t frames, int32_t max_h, int32_t max_w, const cvx_seg_map* label_maps, const cvx_seg_map* target_maps,
                              int64_t* confusion, const uint8_t* lut, int32_t weight_mode, int32_t draw, int32_t bgr_out, void* hip_stream) {
  CVX_CHECK(logits_rows && tile_frames && tile_axes && jobs, "null arguments");
  CVX_CHECK(!draw || lut, "the overlay needs the palette");
  CVX_CHECK((target_maps == nullptr) == (confusion == nullptr), "targets and counts come together");
  CVX_CHECK(slots > 0 && n_axes > 0 && frames > 0 && frames <= 65535 && max_h > 0 && max_h <= 65535 && max_w > 0, "bad sizes");
  CVX_CHECK(nc > 0 && nc <= 256 && ld >= nc && lh > 0 && lw > 0 && net_h > 0 && net_w > 0, "bad logits shape (labels are bytes: nc <= 256)");
  CVX_CHECK(((long long)net_h + 1) * ((long long)net_w + 1) / 4 < (1ll << 24), "network input too large for an exact fp32 weight");
  CVX_CHECK(weight_mode == 0 || weight_mode == 1, "weight_mode: 0 mean, 1 linear");
  CVX_CHECK(confusion == nullptr || nc <= COUNT_MAX_NC, "counting keeps an nc x nc int32 histogram in LDS: nc <= 128");
  const int lds = (int)(Y_STASH * sizeof(YTap)) + (confusion ? nc * nc * 4 : 0);
  static unsigned long long optin_done = 0;
  if (lds > 48 * 1024)
    CVX_TRY(cvx_lds_optin((const void*)seg_stitch_kernel, (int)(Y_STASH * sizeof(YTap)) + COUNT_MAX_NC * COUNT_MAX_NC * 4, &optin_done));
  hipLaunchKernelGGL(seg_stitch_kernel, dim3((unsigned)cvx_cdiv(max_w, 1024), (unsigned)max_h, (unsigned)frames), dim3(STITCH_THREADS), (size_t)lds,
                     (hipStream_t)hip_stream, logits_rows, slots, ld, nc, lh, lw, net_h, net_w, tile_frames, tile_axes, n_axes, jobs, label_maps,
                     target_maps, reinterpret_cast<unsigned long long*>(confusion), lut, weight_mode, draw, bgr_out);
  CVX_HIP(hipGetLastError());
  return 0;
}
