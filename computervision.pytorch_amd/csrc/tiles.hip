// Tiled prediction on gfx950: a large frame is cut into overlapping tiles at network size, the tiles run as one batch,
// and the detections of all tiles of a frame are merged across the tile borders.  Both ends live here; nothing is read by the host.
//
//   K1 tiles_u8_to_nchw   one launch for every tile of every frame: slot `out` of the network batch receives the crop [y0, y0 + th) x
//                         [x0, x0 + tw) of a uint8 HWC frame, anchored top-left, byte / 255 (a true fp32 division, as preprocess.hip);
//                         the rest of the slot, and whatever a bad job would read outside its frame, is 128 / 255.  No resampling: exact by
//                         construction.  The frame is read in place through its row pitch.  HBM-bound, 12 bytes out for 3 in: a thread owns
//                         4 neighbouring pixels of a row and writes one 16-byte store per plane (lane = consecutive address) where W and the
//                         base allow it, one pixel otherwise; a capped grid strides over the work.
//   K2 det_merge_tiles    one workgroup per frame, the shape of nms_kernel (nms.hip): the rows of the frame's slots are moved to frame
//                         coordinates (one fp32 add, then the clamp to the frame), ordered by (score desc, ordinal asc) with the 64-bit key and
//                         the in-LDS bitonic network of lds_sort.h (<= 8192 candidates = 64 KB), the suppression matrix is built as 64-bit
//                         row masks in the workspace by all 16 waves, and one wave walks it (greedy_walk of mask_nms.h).  The overlap test is
//                         iou_gt or ios_gt of box_overlap.h.
#include "box_overlap.h"
#include "det_rows.h"
#include "mask_nms.h"
#include "merge_rows.h"
#include "../../include/cvx_engine.h"

namespace {

constexpr int TILE_THREADS = 256;
constexpr int TILE_MAX_BLOCKS = 2048;

template <int V>
__global__ __launch_bounds__(TILE_THREADS) void tiles_kernel(const cvx_tile_job* __restrict__ jobs, long long total, int swap_rb, float pad,
                                                             float* __restrict__ out, int H, int W) {
  const int WV = W / V;
  const long long per_job = (long long)H * WV, plane = (long long)H * W;
  for (long long i = (long long)blockIdx.x * TILE_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * TILE_THREADS) {
    const int j = (int)(i / per_job);
    const int p = (int)(i - (long long)j * per_job);
    const int y = p / WV, x = (p - y * WV) * V;
    const cvx_tile_job jb = jobs[j];
    const int sy = jb.y0 + y;
    const bool row_in = y < jb.th && sy >= 0 && sy < jb.h;
    const uint8_t* src = jb.src + (long long)sy * jb.stride;
    float v0[V], v1[V], v2[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int sx = jb.x0 + x + k;
      v0[k] = v1[k] = v2[k] = pad;
      if (row_in && x + k < jb.tw && sx >= 0 && sx < jb.w) {
        const uint8_t* q = src + (long long)sx * 3;
        v0[k] = (float)q[swap_rb ? 2 : 0] / 255.0f;
        v1[k] = (float)q[1] / 255.0f;
        v2[k] = (float)q[swap_rb ? 0 : 2] / 255.0f;
      }
    }
    float* dst = out + (long long)jb.out * 3 * plane + (long long)y * W + x;
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(dst) = make_float4(v0[0], v0[1], v0[2], v0[3]);
      *reinterpret_cast<float4*>(dst + plane) = make_float4(v1[0], v1[1], v1[2], v1[3]);
      *reinterpret_cast<float4*>(dst + 2 * plane) = make_float4(v2[0], v2[1], v2[2], v2[3]);
    } else {
      dst[0] = v0[0];
      dst[plane] = v1[0];
      dst[2 * plane] = v2[0];
    }
  }
}

// ---- merge ----------------------------------------------------------------------------------------------------------------------------
constexpr int MERGE_THREADS = 1024;  // MERGE_CAP, MergeWs and its layout: merge_rows.h

// slot pixels -> frame pixels: one fp32 add, then the clamp to the frame
__device__ __forceinline__ float to_frame(float v, int off, int size) {
#pragma clang fp contract(off)
  const float s = v + (float)off;
  return fminf(fmaxf(s, 0.f), (float)size);
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int slots, int max_det_in,
                                                              const int* __restrict__ slot_map, const int* __restrict__ frame_hw, int metric,
                                                              float threshold, int class_agnostic, int max_det, MergeWs ws,
                                                              float* __restrict__ out_rows, int* __restrict__ out_counts, int* out_source,
                                                              int* overflow) {
  extern __shared__ unsigned long long keys[];  // cap2 entries (power of two >= candidates)
  __shared__ unsigned long long s_removed[MERGE_CAP / 64];
  const int f = blockIdx.x, tid = threadIdx.x;
  float* orow = out_rows + (long long)f * max_det * 6;
  int* osrc = out_source + (long long)f * max_det;
  // ---- 1-2. the rows of this frame's slots, counted, keyed by (score desc, ordinal asc) and sorted (merge_rows.h) ----
  const int n = merge_rows_front<MERGE_THREADS>(rows, counts, slots, max_det_in, keys, overflow, [&](int s) { return slot_map[4 * s] == f ? s : -1; });
  if (n < 0) {  // more than the in-LDS sort holds: flagged, never truncated
    zero_rows<MERGE_THREADS>(orow, 0, max_det, osrc, -1);
    if (tid == 0) {
      out_counts[f] = -1;
      atomicAdd(overflow, 1);
    }
    return;
  }
  // ---- 3. gather the sorted candidates in frame coordinates ----
  float4* box = ws.box + (long long)f * MERGE_CAP;
  float* score = ws.score + (long long)f * MERGE_CAP;
  float* cls = ws.cls + (long long)f * MERGE_CAP;
  int* ord = ws.ord + (long long)f * MERGE_CAP;
  const int fh = frame_hw[2 * f], fw = frame_hw[2 * f + 1];
  for (int i = tid; i < n; i += MERGE_THREADS) {
    const int e = (int)(keys[i] & 0xFFFFFFFFu);
    const int s = e / max_det_in;
    const int x0 = slot_map[4 * s + 1], y0 = slot_map[4 * s + 2];
    const float* row = rows + (long long)e * 6;
    box[i] = make_float4(to_frame(row[0], x0, fw), to_frame(row[1], y0, fh), to_frame(row[2], x0, fw), to_frame(row[3], y0, fh));
    score[i] = row[4];
    cls[i] = row[5];
    ord[i] = e;
  }
  __syncthreads();
  // ---- 4. suppression matrix: bit j of row i set when j > i, same class (unless agnostic), metric > threshold ----
  const int nw = (n + 63) / 64;
  unsigned long long* mat = ws.mat + (long long)f * MERGE_CAP * (MERGE_CAP / 64);
  for (long long t = tid; t < (long long)n * nw; t += MERGE_THREADS) {
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
        const float aj = box_area(bj);
        const bool hit = metric == 0 ? iou_gt(bi, ai, bj, aj, threshold) : ios_gt(bi, ai, bj, aj, threshold);
        if (hit) bits |= 1ull << (j - wj * 64);
      }
    }
    mat[(long long)i * nw + wj] = bits;
  }
  // ---- 5. greedy walk by wave 0 (mask_nms.h): the keep list lives in the source column until step 6 ----
  const int nk = greedy_walk<MERGE_THREADS>(mat, s_removed, n, max_det, osrc);
  // ---- 6. emit: the kept rows in order, zero rows and source -1 past the count ----
  for (int r = tid; r < nk; r += MERGE_THREADS) {
    const int i = osrc[r];  // (each thread reads and rewrites only its own slots)
    store_row(orow + (long long)r * 6, box[i], score[i], cls[i]);
    osrc[r] = ord[i];
  }
  zero_rows<MERGE_THREADS>(orow, nk, max_det, osrc, -1);
  if (tid == 0) out_counts[f] = nk;
}

}  // namespace

extern "C" int cvx_tiles_u8_to_nchw(const cvx_tile_job* jobs, int32_t n_jobs, int32_t swap_rb, float* out_nchw, int32_t H, int32_t W,
                                    void* hip_stream) {
  static_assert(sizeof(cvx_tile_job) == 40, "cvx_tile_job is 40 bytes");
  CVX_CHECK(jobs && out_nchw && n_jobs > 0 && H > 0 && W > 0, "bad arguments");
  CVX_CHECK((long long)H * W < (1LL << 31), "the network input is too large");
  const bool wide = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out_nchw) & 15) == 0;
  const long long total = (long long)n_jobs * H * (wide ? W / 4 : W);
  const long long want = (total + TILE_THREADS - 1) / TILE_THREADS;
  const dim3 grid((unsigned)(want < TILE_MAX_BLOCKS ? want : TILE_MAX_BLOCKS));
  if (wide)
    hipLaunchKernelGGL(tiles_kernel<4>, grid, dim3(TILE_THREADS), 0, (hipStream_t)hip_stream, jobs, total, swap_rb, 128.0f / 255.0f, out_nchw, H, W);
  else
    hipLaunchKernelGGL(tiles_kernel<1>, grid, dim3(TILE_THREADS), 0, (hipStream_t)hip_stream, jobs, total, swap_rb, 128.0f / 255.0f, out_nchw, H, W);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t cvx_det_merge_workspace_bytes(int32_t frames) {
  cvx_carver c(nullptr);
  merge_layout(c, frames > 0 ? frames : 0);
  return c.total();
}

extern "C" int cvx_det_merge_tiles(const float* rows, const int32_t* counts, int32_t slots, int32_t max_det_in, const int32_t* slot_map,
                                   const int32_t* frame_hw, int32_t frames, int32_t metric, float threshold, int32_t class_agnostic,
                                   int32_t max_det_out, float* out_rows, int32_t* out_counts, int32_t* out_source, int32_t* overflow,
                                   void* workspace, int64_t workspace_bytes, void* hip_stream) {
  CVX_CHECK(rows && counts && slot_map && frame_hw && out_rows && out_counts && out_source && overflow && workspace, "null arguments");
  CVX_CHECK(slots > 0 && max_det_in > 0 && frames > 0 && (long long)slots * max_det_in < (1LL << 31), "bad sizes: the ordinal is 32 bits");
  CVX_CHECK(metric == 0 || metric == 1, "metric: 0 IoU, 1 IoS");
  CVX_CHECK(threshold >= 0.f && threshold <= 1.f, "the threshold must lie in [0,1]");
  CVX_CHECK(max_det_out >= 1 && max_det_out <= MERGE_CAP, "max_det_out must lie in [1,8192]");
  CVX_CHECK(workspace_bytes >= cvx_det_merge_workspace_bytes(frames), "workspace too small");
  cvx_carver carver(workspace);
  const MergeWs ws = merge_layout(carver, frames);
  static unsigned long long optin = 0;  // 64 KB of keys + the static words: beyond the default dynamic LDS limit
  CVX_TRY(cvx_lds_optin((const void*)merge_kernel, MERGE_CAP * 8, &optin));
  hipLaunchKernelGGL(merge_kernel, dim3(frames), dim3(MERGE_THREADS), (size_t)MERGE_CAP * 8, (hipStream_t)hip_stream, rows, counts, slots, max_det_in,
                     slot_map, frame_hw, metric, threshold, class_agnostic, max_det_out, ws, out_rows, out_counts, out_source, overflow);
  CVX_HIP(hipGetLastError());
  return 0;
}
