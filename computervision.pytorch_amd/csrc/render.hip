// Output side of batched prediction on gfx950: NMS rows -> original-image coordinates (cvx_det_to_image), the detections painted into the
// uint8 frames (cvx_draw_detections; cvx_draw_tracks for rows with track ids) and the segmentation result coloured and blended into them (cvx_seg_overlay).  Nothing is read by the
// host; every frame of a batch has its own size and row stride (cvx_frame_job).
//
//   K1 det_to_image   one thread per row: mode 1 is det_undo_letterbox (det_common.h), the function cvx_det_match maps its boxes with, so
//                     the coordinates are core/utils/boxes.py:undo_letterbox's to the bit.  Rows past the count are zero.  A count of -1
//                     (NMS overflow) or past max_det -> count 0 and overflow += 1.
//   K2 draw           a workgroup owns a 64 x 16 pixel tile, a thread 4 pixels of one row.  Painter's order is box 0 first and, inside a
//                     box, outline, tag, text; the kernel walks the boxes from the LAST to the first and a pixel takes the first layer
//                     that covers it, so it is written once and nothing is read.  The boxes are taken 256 at a time: each thread tests
//                     one box against the tile, the hits are compacted in order into an LDS list (ballot scan) with their label already
//                     spelled out, then every thread walks the list for its pixels that are still open.  A tile no box meets writes
//                     nothing.
//   K3 seg_overlay    a thread per 4 pixels of a frame row: nearest source pixel at network size (OpenCV's resizeNN index rule, as the
//                     letterbox kernel has it), the nc logits there from the four feature rows (bilinear.h: the numbers cvx_seg_criterion_eval and
//                     cvx_resize_bilinear_rows_to_nchw see), arg max (strict >: the lowest class wins a tie), palette, 50/50 blend in
//                     integers with round-half-even (cv2.addWeighted(a, .5, b, .5, 0) on uint8).  The logit chunk, the arg max and the
//                     pixel quad are seg_tail.h's, shared with seg_tiles.hip and seg_tta.hip.
// Byte kernels, HBM-bound: 12 bytes per thread go out (and, in K3, come in) as three dwords when the frame's base and stride allow it.
// Every fp32 step is one rounded operation, so the file is compiled with contraction off (bilinear.h spells its fused steps out).
#include "det_common.h"
#include "seg_tail.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int TW = 64, TH = 16;       // tile of one workgroup; 16 threads x 4 pixels per row
constexpr int LIST = 256;             // boxes per chunk = capacity of the LDS list
constexpr int MAX_CHARS = 12;         // "9999:999.9%"
enum { GLYPH_COLON = 10, GLYPH_DOT = 11, GLYPH_PERCENT = 12 };

// The project's 5 x 7 font for 0-9 : . % -- one byte per glyph row, bit 4 is the left column (render.py FONT is the same table)
__constant__ uint8_t FONT[13][7] = {
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E},  // 0
    {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E},  // 1
    {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},  // 2
    {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E},  // 3
    {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02},  // 4
    {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},  // 5
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E},  // 6
    {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},  // 7
    {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},  // 8
    {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C},  // 9
    {0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00},  // :
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C},  // .
    {0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03},  // %
};

__global__ __launch_bounds__(DET_THREADS) void det_to_image_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int max_det,
                                                                   int box_mode, const float* __restrict__ box_map, float* __restrict__ out_rows,
                                                                   int* __restrict__ out_counts, int* __restrict__ overflow) {
  const int b = blockIdx.y, r = blockIdx.x * DET_THREADS + threadIdx.x;
  const int raw = counts[b], n = det_count(raw, max_det);
  if (r == 0) {
    out_counts[b] = n;
    if (raw < 0 || raw > max_det) atomicAdd(overflow, 1);
  }
  if (r >= max_det) return;
  const float* row = rows + ((long long)b * max_det + r) * 6;
  float* o = out_rows + ((long long)b * max_det + r) * 6;
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, score = 0.f, cls = 0.f;
  if (r < n) {
    x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3], score = row[4], cls = row[5];
    if (box_mode == 1) det_undo_letterbox(x1, y1, x2, y2, det_load_box_map(box_mode, box_map, b));
  }
  o[0] = x1;
  o[1] = y1;
  o[2] = x2;
  o[3] = y2;
  o[4] = score;
  o[5] = cls;
}

// ---- drawing ------------------------------------------------------------------------------------------------------------------------
struct DrawBox {
  int x0, y0, x1, y1;    // truncated corners
  int tx, ty, tw;        // tag origin and width (its height is 9 * font_scale)
  int nch;
  unsigned colour, tag, text;   // r | g << 8 | b << 16 in the LUT's channel order
  unsigned char ch[MAX_CHARS];
};

__device__ __forceinline__ int draw_coord(float v) {  // int(): towards zero; far-away values stay far away without overflowing the sums below
  return (int)fminf(fmaxf(v, -1048576.f), 1048576.f);
}

// "{cls}:{p}%" with p = '{:.1f}'.format(score * 100) -- fp32 product, then round-half-even on the exact value
__device__ __forceinline__ int draw_label(int cls, float score, unsigned char* ch) {
  double t = rint((double)(score * 100.0f) * 10.0);
  if (!(t >= 0.0)) t = 0.0;
  if (t > 9999.0) t = 9999.0;
  const int tenths = (int)t;
  int n = 0;
  unsigned char tmp[4];
  int k = 0, v = cls;
  do {
    tmp[k++] = (unsigned char)(v % 10);
    v /= 10;
  } while (v > 0);
  while (k > 0) ch[n++] = tmp[--k];
  ch[n++] = GLYPH_COLON;
  v = tenths / 10;
  do {
    tmp[k++] = (unsigned char)(v % 10);
    v /= 10;
  } while (v > 0);
  while (k > 0) ch[n++] = tmp[--k];
  ch[n++] = GLYPH_DOT;
  ch[n++] = (unsigned char)(tenths % 10);
  ch[n++] = GLYPH_PERCENT;
  return n;
}

// "{id % 1000000}:{cls}": digits and the colon only
__device__ __forceinline__ int draw_track_label(int id, int cls, unsigned char* ch) {
  int n = 0;
  unsigned char tmp[6];
  int k = 0, v = id % 1000000;
  do {
    tmp[k++] = (unsigned char)(v % 10);
    v /= 10;
  } while (v > 0);
  while (k > 0) ch[n++] = tmp[--k];
  ch[n++] = GLYPH_COLON;
  v = cls;
  do {
    tmp[k++] = (unsigned char)(v % 10);
    v /= 10;
  } while (v > 0);
  while (k > 0) ch[n++] = tmp[--k];
  return n;
}

__device__ __forceinline__ bool rects_meet(int ax0, int ay0, int ax1, int ay1, int bx0, int by0, int bx1, int by1) {  // inclusive corners
  return ax0 <= bx1 && bx0 <= ax1 && ay0 <= by1 && by0 <= ay1;
}

// TRACKS: the rows carry track ids (cvx_draw_tracks) -- a negative id paints nothing, the label spells the id and the class, the colour
// follows the id; everything else is one body
template <bool TRACKS>
__global__ __launch_bounds__(256) void draw_kernel(const cvx_frame_job* __restrict__ jobs, const float* __restrict__ rows,
                                                   const int* __restrict__ counts, int max_det, const int* __restrict__ ids,
                                                   const uint8_t* __restrict__ lut, int n_lut, int thick, int fs) {
  __shared__ DrawBox list[LIST];
  __shared__ int wave_tot[4];
  const cvx_frame_job jb = jobs[blockIdx.y];
  const int h = jb.h, w = jb.w;
  const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;   // the grid is sized for the largest frame of the batch
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int X0 = tile_x * TW, Y0 = tile_y * TH;
  const int X1 = min(X0 + TW, w) - 1, Y1 = min(Y0 + TH, h) - 1;   // the tile inside the frame, inclusive
  const int py = Y0 + (tid >> 4), px = X0 + (tid & 15) * 4;
  const int n = det_count(counts[blockIdx.y], max_det);
  const int grow = thick / 2, shrink = (thick + 1) / 2, tag_h = 9 * fs, cell = 6 * fs;

  unsigned colour[4];
  unsigned open = 0;   // bit k: pixel px + k is inside the frame and not painted yet
  unsigned painted = 0;
  if (py < h)
    for (int k = 0; k < 4; ++k)
      if (px + k < w) open |= 1u << k;

  for (int start = 0; start < n; start += LIST) {
    if (__syncthreads_or(open != 0) == 0) break;   // every pixel of the tile has its final layer (also the barrier that frees the list)
    const int j = n - 1 - (start + tid);           // this thread's box of the chunk, last box first
    bool hit = false;
    DrawBox d;
    int track = 0;
    if constexpr (TRACKS) track = j >= 0 ? ids[(long long)blockIdx.y * max_det + j] : -1;
    if (j >= 0 && track >= 0) {
      const float* row = rows + ((long long)blockIdx.y * max_det + j) * 6;
      const float fx0 = row[0], fy0 = row[1], fx1 = row[2], fy1 = row[3];
      if (fx0 == fx0 && fy0 == fy0 && fx1 == fx1 && fy1 == fy1) {   // a NaN coordinate paints nothing
        d.x0 = draw_coord(fx0), d.y0 = draw_coord(fy0), d.x1 = draw_coord(fx1), d.y1 = draw_coord(fy1);
        if (d.x1 >= d.x0 && d.y1 >= d.y0) {                         // an inverted box paints nothing
          int cls = draw_coord(row[5]);
          cls = cls < 0 ? 0 : (cls > 9999 ? 9999 : cls);
          d.nch = TRACKS ? draw_track_label(track, cls, d.ch) : draw_label(cls, row[4], d.ch);
          d.tw = (6 * d.nch + 1) * fs;
          d.tx = d.x0;
          d.ty = d.y0 - tag_h >= 0 ? d.y0 - tag_h : d.y0;           // above the box where it fits, else inside it
          hit = rects_meet(d.x0 - grow, d.y0 - grow, d.x1 + grow, d.y1 + grow, X0, Y0, X1, Y1) ||
                rects_meet(d.tx, d.ty, d.tx + d.tw - 1, d.ty + tag_h - 1, X0, Y0, X1, Y1);
          if (hit) {
            const uint8_t* c = lut + 3 * (TRACKS ? (int)(((long long)track + 1) % n_lut) : (cls + 1) % n_lut);
            const unsigned r = c[0], g = c[1], b = c[2];
            d.colour = r | g << 8 | b << 16;
            d.tag = (r * 7 / 10) | (g * 7 / 10) << 8 | (b * 7 / 10) << 16;
            d.text = r + g + b > 382 ? 0u : 0xFFFFFFu;
          }
        }
      }
    }
    // rank among the hits of the chunk, in thread order = reverse box order (ballot + popcount, the wave totals through LDS)
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int pos = __popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) pos += wave_tot[k];
    const int total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    if (hit) list[pos] = d;
    __syncthreads();

    for (int e = 0; e < total && open; ++e) {
      const DrawBox& q = list[e];
      const int dy = py - q.ty;
      const bool tag_row = dy >= 0 && dy < tag_h;
      const bool out_row = py >= q.y0 - grow && py <= q.y1 + grow;
      if (!tag_row && !out_row) continue;
      const bool in_row = py >= q.y0 + shrink && py <= q.y1 - shrink;
      const int v = dy - fs;
      const bool text_row = tag_row && v >= 0 && v < 7 * fs;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!(open >> k & 1)) continue;
        const int x = px + k, dx = x - q.tx;
        unsigned c;
        if (tag_row && dx >= 0 && dx < q.tw) {
          c = q.tag;
          const int u = dx - fs;
          if (text_row && u >= 0) {
            const int ci = u / cell, gx = (u - ci * cell) / fs;
            if (ci < q.nch && gx < 5 && (FONT[q.ch[ci]][v / fs] >> (4 - gx) & 1)) c = q.text;
          }
        } else if (out_row && x >= q.x0 - grow && x <= q.x1 + grow && !(in_row && x >= q.x0 + shrink && x <= q.x1 - shrink)) {
          c = q.colour;
        } else {
          continue;
        }
        colour[k] = c;
        open &= ~(1u << k);
        painted |= 1u << k;
      }
    }
  }

  if (!painted) return;
  uint8_t* p = jb.data + (long long)py * jb.stride + (long long)px * 3;
  if (painted == 15u && ((reinterpret_cast<uintptr_t>(jb.data) | (uintptr_t)jb.stride) & 3) == 0) {   // px * 3 is a multiple of 12
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = (colour[0] & 0xFFFFFFu) | (colour[1] & 0xFFu) << 24;
    q[1] = (colour[1] >> 8 & 0xFFFFu) | (colour[2] & 0xFFFFu) << 16;
    q[2] = (colour[2] >> 16 & 0xFFu) | (colour[3] & 0xFFFFFFu) << 8;
    return;
  }
  for (int k = 0; k < 4; ++k)
    if (painted >> k & 1) {
      p[3 * k + 0] = (uint8_t)(colour[k] & 0xFF);
      p[3 * k + 1] = (uint8_t)(colour[k] >> 8 & 0xFF);
      p[3 * k + 2] = (uint8_t)(colour[k] >> 16 & 0xFF);
    }
}

// ---- segmentation overlay -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_overlay_kernel(const cvx_frame_job* __restrict__ jobs, const float* __restrict__ logits, int ld, int nc,
                                                          int lh, int lw, int NH, int NW, const uint8_t* __restrict__ lut, int bgr_out) {
  const cvx_frame_job jb = jobs[blockIdx.z];
  const int h = jb.h, w = jb.w;
  const int y = blockIdx.y, x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (y >= h || x0 >= w) return;
  // cv::resize(colours at network size, (w, h), INTER_NEAREST): src = min(floor(dst * (1 / (dsize / ssize))), ssize - 1), in doubles
  const double ify = 1.0 / ((double)h / (double)NH), ifx = 1.0 / ((double)w / (double)NW);
  int sy = (int)floor((double)y * ify);
  sy = sy < NH - 1 ? sy : NH - 1;
  int y0, y1;
  float ly;
  bilinear_src(sy, (float)lh / (float)NH, lh, &y0, &y1, &ly);
  const float* base = logits + (long long)blockIdx.z * lh * lw * ld;
  const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  const int npx = min(4, w - x0);
  uint8_t* p = jb.data + (long long)y * jb.stride + (long long)x0 * 3;
  const bool wide = quad_is_wide(jb.data, jb.stride, npx);
  pixel_quad px;
  quad_load(p, npx, wide, px);
  const float* ra = base + (long long)y0 * lw * ld;
  const float* rb = base + (long long)y1 * lw * ld;
  for (int k = 0; k < npx; ++k) {
    int sx = (int)floor((double)(x0 + k) * ifx);
    sx = sx < NW - 1 ? sx : NW - 1;
    int xa, xb;
    float lx;
    bilinear_src(sx, (float)lw / (float)NW, lw, &xa, &xb, &lx);
    float best = 0.f, z[4];
    int arg = 0;
    for (int c0 = 0; c0 < nc; c0 += 4) {
      logits4(ra + c0, rb + c0, xa, xb, lx, ly, ld, c0, nc, vec, z);
      argmax4(z, c0, nc, best, arg);
    }
    quad_blend(px, k, lut + 3 * arg, bgr_out);
  }
  quad_store(p, npx, wide, px);
}

}  // namespace

extern "C" int cvx_det_to_image(const float* rows, const int32_t* counts, int32_t batch, int32_t max_det, int32_t box_mode, const float* box_map,
                                float* out_rows, int32_t* out_counts, int32_t* overflow, void* hip_stream) {
  CVX_CHECK(rows && counts && out_rows && out_counts && overflow, "null arguments");
  CVX_CHECK(batch > 0 && batch <= 65535 && max_det > 0, "bad sizes");
  CVX_CHECK(box_mode == 0 || (box_mode == 1 && box_map), "box_mode: 0 final boxes, 1 (x - px) * gx with box_map (batch, 4)");
  hipLaunchKernelGGL(det_to_image_kernel, dim3((unsigned)cvx_cdiv(max_det, DET_THREADS), (unsigned)batch), dim3(DET_THREADS), 0, (hipStream_t)hip_stream,
                     rows, counts, max_det, box_mode, box_map, out_rows, out_counts, overflow);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_draw_detections(const cvx_frame_job* jobs, int32_t batch, int32_t max_h, int32_t max_w, const float* rows, const int32_t* counts,
                                   int32_t max_det, const uint8_t* lut, int32_t lut_entries, int32_t thickness, int32_t font_scale, void* hip_stream) {
  CVX_CHECK(jobs && rows && counts && lut, "null arguments");
  CVX_CHECK(batch > 0 && batch <= 65535 && max_h > 0 && max_w > 0 && max_det > 0 && lut_entries > 0, "bad sizes");
  CVX_CHECK(thickness >= 1 && thickness <= 64 && font_scale >= 1 && font_scale <= 16, "thickness 1 .. 64, font_scale 1 .. 16");
  const long long tiles = (long long)cvx_cdiv(max_w, TW) * cvx_cdiv(max_h, TH);
  CVX_CHECK(tiles <= 0x7FFFFFFF, "frame too large");
  hipLaunchKernelGGL(draw_kernel<false>, dim3((unsigned)tiles, (unsigned)batch), dim3(256), 0, (hipStream_t)hip_stream, jobs, rows, counts, max_det,
                     (const int*)nullptr, lut, lut_entries, thickness, font_scale);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_draw_tracks(const cvx_frame_job* jobs, int32_t batch, int32_t max_h, int32_t max_w, const float* rows, const int32_t* counts,
                               int32_t max_det, const int32_t* ids, const uint8_t* lut, int32_t lut_entries, int32_t thickness, int32_t font_scale,
                               void* hip_stream) {
  CVX_CHECK(jobs && rows && counts && ids && lut, "null arguments");
  CVX_CHECK(batch > 0 && batch <= 65535 && max_h > 0 && max_w > 0 && max_det > 0 && lut_entries > 0, "bad sizes");
  CVX_CHECK(thickness >= 1 && thickness <= 64 && font_scale >= 1 && font_scale <= 16, "thickness 1 .. 64, font_scale 1 .. 16");
  const long long tiles = (long long)cvx_cdiv(max_w, TW) * cvx_cdiv(max_h, TH);
  CVX_CHECK(tiles <= 0x7FFFFFFF, "frame too large");
  hipLaunchKernelGGL(draw_kernel<true>, dim3((unsigned)tiles, (unsigned)batch), dim3(256), 0, (hipStream_t)hip_stream, jobs, rows, counts, max_det, ids,
                     lut, lut_entries, thickness, font_scale);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_seg_overlay(const cvx_frame_job* jobs, int32_t batch, int32_t max_h, int32_t max_w, const float* logits_rows, int32_t ld, int32_t nc,
                               int32_t lh, int32_t lw, int32_t net_h, int32_t net_w, const uint8_t* lut, int32_t bgr_out, void* hip_stream) {
  CVX_CHECK(jobs && logits_rows && lut, "null arguments");
  CVX_CHECK(batch > 0 && batch <= 65535 && max_h > 0 && max_h <= 65535 && max_w > 0, "bad sizes");
  CVX_CHECK(nc > 0 && ld >= nc && lh > 0 && lw > 0 && net_h > 0 && net_w > 0, "bad logits shape");
  hipLaunchKernelGGL(seg_overlay_kernel, dim3((unsigned)cvx_cdiv(max_w, 1024), (unsigned)max_h, (unsigned)batch), dim3(256), 0, (hipStream_t)hip_stream, jobs,
                     logits_rows, ld, nc, lh, lw, net_h, net_w, lut, bgr_out);
  CVX_HIP(hipGetLastError());
  return 0;
}
