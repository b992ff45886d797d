// Scale and flip test-time augmentation for the four detectors on gfx950: the network runs on the batch at a few
// zooms and on its mirror image, every view at the network's own input size, and the boxes of all views of a frame are brought back to
// the picture and fused.  Both ends live here, one launch each; nothing is read by the host.
//
//   K1 det_tta_inputs   one launch for every view of every picture: slot k * B + b of the output receives picture b resized to (h_k, w_k)
//                       -- the taps and the mix of bilinear.h, align_corners = False, no antialiasing -- inside the rectangle at
//                       (top_k, left_k), `pad` outside it, and, for a flipped view, all of that mirrored along x.  The view table (at most
//                       8 views) is a kernel argument.  The store side has the shape of tiles_kernel (tiles.hip): a thread owns 4
//                       neighbouring pixels of a row in all three planes and writes one 16-byte store per plane where W and the base
//                       allow it, one pixel otherwise; a capped grid strides over the work.  On the 16-byte path the values are
//                       computed with neighbouring lanes on neighbouring pixels and change hands through LDS.
//   K2 det_fuse_views   one workgroup per frame, the shape of merge_kernel (tiles.hip): the rows of the frame's V slots go through their
//                       view's affine map (a rounded product, then a rounded add, per corner; the corners re-ordered, since a flipped
//                       view swaps them; the clamp to the frame), are ordered by (score desc, ordinal asc) with the key and the bitonic
//                       network of lds_sort.h, the IoU suppression matrix is built as 64-bit row masks by all 16 waves and wave 0 walks it
//                       (greedy_walk of mask_nms.h).  Then a wave per kept row gathers the row's members -- its own matrix row for the
//                       candidates behind it, a ballot over the column for those before it -- and walks them in sorted order: the member
//                       and view counts and, in mode 1, the box vote (weights IoU * score, every operation rounded on its own).
// Every fp32 step is one rounded operation: the file is compiled with contraction off (bilinear.h spells its fused steps out) and
// tests/det_tta_restatement.py holds both kernels to the bit.
#include "bilinear.h"
#include "box_overlap.h"
#include "det_rows.h"
#include "mask_nms.h"
#include "merge_rows.h"
#include "view_box.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_VIEWS = 8;
constexpr int IN_THREADS = 256;
constexpr int IN_MAX_BLOCKS = 2048;

// a view as the kernels read it: cvx_det_view and the two tap scales, (float)H / (float)h and (float)W / (float)w -- true fp32 divisions
// made once on the host, the same bits the division gives on the device
struct DevView {
  int h, w, top, left, flip;
  float sy, sx;
  int reserved;
};
struct ViewTable {
  DevView v[MAX_VIEWS];
};
static_assert(sizeof(cvx_det_view) == 24 && sizeof(ViewTable) == 256, "cvx_det_view is 24 bytes; the kernel's table is 8 entries of 32");

// the three planes of pixel (y, x) of a slot that shows picture `src` through view `vw`: the resize first, the mirror second
__device__ __forceinline__ void view_pixel(const float* __restrict__ src, const DevView& vw, int y, int x, int H, int W, long long plane, float pad,
                                           float& v0, float& v1, float& v2) {
  v0 = v1 = v2 = pad;
  const int cy = y - vw.top, cx = (vw.flip ? W - 1 - x : x) - vw.left;
  if (cy < 0 || cy >= vw.h || cx < 0 || cx >= vw.w) return;
  int ya, yb, xa, xb;
  float ly, lx;
  bilinear_src(cy, vw.sy, H, &ya, &yb, &ly);
  bilinear_src(cx, vw.sx, W, &xa, &xb, &lx);
  const float *ra = src + (long long)ya * W, *rb = src + (long long)yb * W;
  v0 = bilinear_mix(ra[xa], ra[xb], rb[xa], rb[xb], lx, ly);
  v1 = bilinear_mix(ra[plane + xa], ra[plane + xb], rb[plane + xa], rb[plane + xb], lx, ly);
  v2 = bilinear_mix(ra[2 * plane + xa], ra[2 * plane + xb], rb[2 * plane + xa], rb[2 * plane + xb], lx, ly);
}

// W % 4 == 0 and a 16-byte aligned base.  A workgroup finishes IN_CHUNK consecutive pixels of the (slot, y, x) order per pass.  They are
// computed with neighbouring lanes on neighbouring pixels, so a wave's tap loads fall on two or three cache lines, parked in LDS, and
// written out with each thread owning 4 neighbouring pixels: one 16-byte store per plane, lane = consecutive address.  The 64-bit
// division that finds the pass's place is made once per pass; a pixel costs one 32-bit division.
constexpr int IN_CHUNK = IN_THREADS * 4;

__global__ __launch_bounds__(IN_THREADS) void det_tta_inputs_wide_kernel(const float* __restrict__ in, const ViewTable tab, int batch, long long chunks,
                                                                         long long total, float pad, float* __restrict__ out, int H, int W) {
  __shared__ __attribute__((aligned(16))) float stage[3][IN_CHUNK];
  const long long plane = (long long)H * W;
  const int tid = threadIdx.x;
  for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
    const long long p0 = c * IN_CHUNK;
    const int slot0 = (int)(p0 / plane), q0 = (int)(p0 - (long long)slot0 * plane);
    const int y0 = q0 / W, x0 = q0 - y0 * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int at = tid + j * IN_THREADS;
      float v0 = 0.f, v1 = 0.f, v2 = 0.f;
      if (p0 + at < total) {
        const unsigned xx = (unsigned)x0 + (unsigned)at, dy = xx / (unsigned)W;
        int y = y0 + (int)dy, slot = slot0;
        while (y >= H) y -= H, ++slot;   // more than once only where a plane is smaller than a pass
        const int k = slot / batch;
        view_pixel(in + (long long)(slot - k * batch) * 3 * plane, tab.v[k], y, (int)(xx - dy * (unsigned)W), H, W, plane, pad, v0, v1, v2);
      }
      stage[0][at] = v0;
      stage[1][at] = v1;
      stage[2][at] = v2;
    }
    __syncthreads();
    if (p0 + 4 * tid < total) {   // total is a multiple of 4, and so is every row's start: the 4 pixels lie in one row
      long long q = (long long)q0 + 4 * tid, slot = slot0;
      while (q >= plane) q -= plane, ++slot;
      float* dst = out + slot * 3 * plane + q;
      *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(&stage[0][4 * tid]);
      *reinterpret_cast<float4*>(dst + plane) = *reinterpret_cast<const float4*>(&stage[1][4 * tid]);
      *reinterpret_cast<float4*>(dst + 2 * plane) = *reinterpret_cast<const float4*>(&stage[2][4 * tid]);
    }
    __syncthreads();
  }
}

// any W, any base: a thread per pixel, 4-byte stores
__global__ __launch_bounds__(IN_THREADS) void det_tta_inputs_kernel(const float* __restrict__ in, const ViewTable tab, int batch, long long total, float pad,
                                                                    float* __restrict__ out, int H, int W) {
  const long long plane = (long long)H * W;
  for (long long p = (long long)blockIdx.x * IN_THREADS + threadIdx.x; p < total; p += (long long)gridDim.x * IN_THREADS) {
    const int slot = (int)(p / plane), q = (int)(p - (long long)slot * plane);
    const int y = q / W, k = slot / batch;
    float v0, v1, v2;
    view_pixel(in + (long long)(slot - k * batch) * 3 * plane, tab.v[k], y, q - y * W, H, W, plane, pad, v0, v1, v2);
    float* dst = out + (long long)slot * 3 * plane + q;
    dst[0] = v0;
    dst[plane] = v1;
    dst[2 * plane] = v2;
  }
}

// ---- fusion ---------------------------------------------------------------------------------------------------------------------------
constexpr int FUSE_CAP = MERGE_CAP;  // candidates per frame: cvx_det_merge_tiles's, whose workspace (MergeWs of merge_rows.h) this kernel shares
constexpr int FUSE_THREADS = 1024;

__global__ __launch_bounds__(FUSE_THREADS) void fuse_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int max_det_in,
                                                            const float* __restrict__ view_map, const int* __restrict__ frame_hw, int frames, int views,
                                                            float threshold, int class_agnostic, int mode, int score_mode, int max_det, MergeWs ws,
                                                            float* __restrict__ out_rows, int* __restrict__ out_counts, int* out_source,
                                                            int* __restrict__ out_members, int* overflow) {
  extern __shared__ unsigned long long keys[];  // cap2 entries (power of two >= candidates)
  __shared__ unsigned long long s_removed[FUSE_CAP / 64];
  const int f = blockIdx.x, tid = threadIdx.x;
  float* orow = out_rows + (long long)f * max_det * 6;
  int* osrc = out_source + (long long)f * max_det;
  int* omem = out_members + (long long)f * max_det;
  // ---- 1-2. the rows of this frame's slots k * frames + f, counted, keyed by (score desc, ordinal asc) and sorted (merge_rows.h) ----
  const int n = merge_rows_front<FUSE_THREADS>(rows, counts, views, max_det_in, keys, overflow, [&](int k) { return k * frames + f; });
  if (n < 0) {  // more than the in-LDS sort holds: flagged, never truncated
    zero_rows<FUSE_THREADS>(orow, 0, max_det, osrc, -1, omem, 0);
    if (tid == 0) {
      out_counts[f] = -1;
      atomicAdd(overflow, 1);
    }
    return;
  }
  // ---- 3. gather the sorted candidates in picture coordinates ----
  float4* box = ws.box + (long long)f * FUSE_CAP;
  float* score = ws.score + (long long)f * FUSE_CAP;
  float* cls = ws.cls + (long long)f * FUSE_CAP;
  int* ord = ws.ord + (long long)f * FUSE_CAP;
  const int fh = frame_hw[2 * f], fw = frame_hw[2 * f + 1];
  for (int i = tid; i < n; i += FUSE_THREADS) {
    const int e = (int)(keys[i] & 0xFFFFFFFFu);
    const int s = e / max_det_in;
    const float* row = rows + (long long)e * 6;
    box[i] = mapped_box(row, view_map + 4 * s, fh, fw);   // view_box.h
    score[i] = row[4];
    cls[i] = row[5];
    ord[i] = e;
  }
  __syncthreads();
  // ---- 4. suppression matrix: bit j of row i set when j > i, same class (unless agnostic), IoU > threshold ----
  const int nw = (n + 63) / 64;
  unsigned long long* mat = ws.mat + (long long)f * FUSE_CAP * (FUSE_CAP / 64);
  for (long long t = tid; t < (long long)n * nw; t += FUSE_THREADS) {
    const int i = (int)(t / nw), wj = (int)(t - (long long)i * nw);
    unsigned long long bits = 0;
    if (wj * 64 + 63 > i) {
      const float4 bi = box[i];
      const float ai = box_area(bi);
      const float ci = cls[i];
      const int j0 = max(wj * 64, i + 1), j1 = min(n, wj * 64 + 64);
      for (int j = j0; j < j1; ++j) {
        if (!class_agnostic && !(cls[j] == ci)) continue;
        const float4 bj = box[j];
        if (iou_gt(bi, ai, bj, box_area(bj), threshold)) bits |= 1ull << (j - wj * 64);
      }
    }
    mat[(long long)i * nw + wj] = bits;
  }
  // ---- 5. greedy walk by wave 0 (mask_nms.h): the keep list lives in the source column until step 6 ----
  const int nk = greedy_walk<FUSE_THREADS>(mat, s_removed, n, max_det, osrc);
  // ---- 6. a wave per kept row: its members in sorted order, the vote, the emit ----
  const int lane = tid & 63, wave = tid >> 6;
  const int per_view = frames * max_det_in;   // ordinal / per_view is the view
  for (int r = wave; r < nk; r += FUSE_THREADS / 64) {
    const int i = osrc[r];   // (this wave alone reads and rewrites slot r)
    const float4 bi = box[i];
    const float ai = box_area(bi), si = score[i];
    const int wi = i >> 6;
    float wt = 0.f, x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    int members = 0;
    unsigned seen = 0;   // bit k: view k has a member
    for (int wj = 0; wj < nw; ++wj) {
      // the members among candidates wj * 64 .. + 63: before i the column of the matrix (bit i of row j), behind i the row of i
      const int jl = wj * 64 + lane;
      const bool before = jl < i && ((mat[(long long)jl * nw + wi] >> (i & 63)) & 1ull);
      unsigned long long m = __ballot(before) | mat[(long long)i * nw + wj];
      if (wj == wi) m |= 1ull << (i & 63);
      while (m) {   // uniform: every lane walks the same members, in sorted order
        const int j = wj * 64 + __builtin_ctzll(m);
        m &= m - 1;
        float w;
        float4 bj;
        if (j == i) {
          w = si;
          bj = bi;
        } else {
          bj = box[j];
          w = iou_value(bi, ai, bj, box_area(bj)) * score[j];
        }
        ++members;
        seen |= 1u << (ord[j] / per_view);
        wt = wt + w;
        x1 = x1 + w * bj.x;
        y1 = y1 + w * bj.y;
        x2 = x2 + w * bj.z;
        y2 = y2 + w * bj.w;
      }
    }
    if (lane == 0) {
      float* o = orow + (long long)r * 6;
      const bool vote = mode == 1 && members > 1 && wt > 0.f;   // a lone row, or no weight: its own box, bit for bit
      o[0] = vote ? x1 / wt : bi.x;
      o[1] = vote ? y1 / wt : bi.y;
      o[2] = vote ? x2 / wt : bi.z;
      o[3] = vote ? y2 / wt : bi.w;
      o[4] = score_mode == 1 ? (si * (float)__popc(seen)) / (float)views : si;
      o[5] = cls[i];
      osrc[r] = ord[i];
      omem[r] = members;
    }
  }
  zero_rows<FUSE_THREADS>(orow, nk, max_det, osrc, -1, omem, 0);
  if (tid == 0) out_counts[f] = nk;
}

}  // namespace

extern "C" int cvx_det_tta_inputs(const float* images_nchw, int32_t batch, int32_t H, int32_t W, const cvx_det_view* views_host, int32_t n_views,
                                  float pad, float* out_nchw, void* hip_stream) {
  CVX_CHECK(images_nchw && views_host && out_nchw, "null arguments");
  CVX_CHECK(batch > 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31), "bad sizes");
  CVX_CHECK(n_views >= 1 && n_views <= MAX_VIEWS, "1 <= n_views <= 8: the table is a kernel argument");
  CVX_CHECK((long long)n_views * batch < (1LL << 31), "too many slots");
  ViewTable tab = {};
  for (int k = 0; k < n_views; ++k) {
    const cvx_det_view v = views_host[k];
    CVX_CHECK(v.h >= 1 && v.w >= 1 && v.top >= 0 && v.left >= 0 && (long long)v.top + v.h <= H && (long long)v.left + v.w <= W,
              "a view: a content rectangle inside the network input");
    CVX_CHECK(v.flip == 0 || v.flip == 1, "a view: flip 0 or 1");
    tab.v[k] = DevView{v.h, v.w, v.top, v.left, v.flip, (float)H / (float)v.h, (float)W / (float)v.w, 0};
  }
  const bool wide = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out_nchw) & 15) == 0;
  const long long total = (long long)n_views * batch * H * W;   // pixels per plane
  const long long want = (total + (wide ? IN_CHUNK : IN_THREADS) - 1) / (wide ? IN_CHUNK : IN_THREADS);
  const dim3 grid((unsigned)(want < IN_MAX_BLOCKS ? want : IN_MAX_BLOCKS));
  if (wide)
    hipLaunchKernelGGL(det_tta_inputs_wide_kernel, grid, dim3(IN_THREADS), 0, (hipStream_t)hip_stream, images_nchw, tab, batch, want, total, pad, out_nchw,
                       H, W);
  else
    hipLaunchKernelGGL(det_tta_inputs_kernel, grid, dim3(IN_THREADS), 0, (hipStream_t)hip_stream, images_nchw, tab, batch, total, pad, out_nchw, H, W);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_det_fuse_views(const float* rows, const int32_t* counts, int32_t max_det_in, const float* view_map, const int32_t* frame_hw,
                                  int32_t frames, int32_t views, float threshold, int32_t class_agnostic, int32_t mode, int32_t score_mode,
                                  int32_t max_det_out, float* out_rows, int32_t* out_counts, int32_t* out_source, int32_t* out_members,
                                  int32_t* overflow, void* workspace, int64_t workspace_bytes, void* hip_stream) {
  CVX_CHECK(rows && counts && view_map && frame_hw && out_rows && out_counts && out_source && out_members && overflow && workspace, "null arguments");
  CVX_CHECK(views >= 1 && views <= MAX_VIEWS, "1 <= views <= 8");
  CVX_CHECK(max_det_in > 0 && frames > 0 && (long long)views * frames * max_det_in < (1LL << 31), "bad sizes: the ordinal is 32 bits");
  CVX_CHECK(threshold >= 0.f && threshold <= 1.f, "the threshold must lie in [0,1]");
  CVX_CHECK(mode == 0 || mode == 1, "mode: 0 nms, 1 vote");
  CVX_CHECK(score_mode == 0 || score_mode == 1, "score_mode: 0 max, 1 views");
  CVX_CHECK(max_det_out >= 1 && max_det_out <= FUSE_CAP, "max_det_out must lie in [1,8192]");
  CVX_CHECK(workspace_bytes >= cvx_det_merge_workspace_bytes(frames), "workspace too small");
  cvx_carver carver(workspace);
  const MergeWs ws = merge_layout(carver, frames);
  static unsigned long long optin = 0;  // 64 KB of keys + the static words: beyond the default dynamic LDS limit
  CVX_TRY(cvx_lds_optin((const void*)fuse_kernel, FUSE_CAP * 8, &optin));
  hipLaunchKernelGGL(fuse_kernel, dim3(frames), dim3(FUSE_THREADS), (size_t)FUSE_CAP * 8, (hipStream_t)hip_stream, rows, counts, max_det_in, view_map,
                     frame_hw, frames, views, threshold, class_agnostic, mode, score_mode, max_det_out, ws, out_rows, out_counts, out_source,
                     out_members, overflow);
  CVX_HIP(hipGetLastError());
  return 0;
}
