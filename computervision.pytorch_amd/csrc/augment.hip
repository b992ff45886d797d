// Training-side input path of the two YOLO trainers on gfx950: the reference's per-image CPU augmentation
// (core/data/detection_dataset.py:132-220 get_random_data, :222-345 mosaic_body / mosaic_for_voc, :405-449 merge_bboxes, :100-130 label
// normalisation, core/data/collate.py:5-29) as two launches per batch.  The random draws stay on the host (augment.draw_params); what
// arrives here is a table of jobs, one per source picture:
//
//   plain output  : 1 job,  canvas of 128, resized picture pasted at (dx, dy) with cv2_paste's clipping (image_process.py:132-158),
//                   flip mirrors the CANVAS (:188-191), rect = the whole output;
//   mosaic output : 4 jobs, each its own 128-canvas with a paste; flip mirrors the SOURCE before the resize (:227-231); the job's rect is
//                   its quadrant of the output (:321-328; quad 0 top-left, 1 bottom-left, 2 bottom-right, 3 top-right).
//
// cvx_aug_images, per output pixel: bicubic tap (OpenCV's INTER_CUBIC in its uint8 fixed-point form, restated in tests/aug_restatement.py)
// -> RGB2HSV (8-bit integer form) -> three LUT look-ups -> HSV2RGB (float form) -> to_tensor.  cvx_aug_boxes: box scaling, flip, clamps,
// the w > 1 && h > 1 filter, merge_bboxes, normalisation to [image, cls, cx, cy, w, h], compacted in source order by a scan.
//
// Validation (DetectionDataset(train=False), get_random_data(random=False), :137-166) has no colour transform, and RGB -> HSV -> RGB is
// lossy in 8 bits even with identity tables, so the image kernel is a template on COLOUR: cvx_aug_images launches <true>,
// cvx_aug_images_plain <false> (paste + bicubic taps -> byte / 255).  A sibling entry point and not a bit in the job's reserved word: a
// loader never mixes training and validation pictures in one batch, and a per-job bit would put a branch, and the live range of the
// uncoloured bytes across it, into the colour instance that every existing caller runs; the template leaves that instance as it was.
// cvx_aug_boxes_padded is the box half for consumers that take (batch, max_boxes, 5) labels plus per-image counts (cvx_ssd_encode_targets,
// cvx_centernet_draw_targets): one workgroup per output image, the same box_row() arithmetic and the same scan as cvx_aug_boxes.
//
// Every fp32 step below is one rounded operation in the order written, so the whole file is compiled with contraction off; the host
// restatement (numpy fp32) then agrees to the byte.
#include "cvx_common.h"
#include "../../include/cvx_engine.h"
#include <limits.h>

#pragma clang fp contract(off)

namespace {

constexpr int TW = 64, TH = 16, MAXJ = 4;   // tile of one workgroup: 4 waves, wave w takes rows w, w + 4, w + 8, w + 12 (64 px = 256 B per plane store)
constexpr int OUTSIDE = INT_MIN;            // tap marker: this canvas row / column lies outside the pasted picture

// One destination coordinate r of a resize n_src -> n_dst: first tap and the four Keys weights (A = -0.75) in Q11.
__device__ __forceinline__ void cubic_tap(int r, int n_dst, int n_src, int* s, short* w) {
  const float f = (float)(((double)r + 0.5) * (double)n_src / (double)n_dst - 0.5);
  const float fl = floorf(f);
  const float t = f - fl;
  const float A = -0.75f;
  const float t1 = t + 1.0f, u = 1.0f - t;
  const float c0 = ((A * t1 - 5.0f * A) * t1 + 8.0f * A) * t1 - 4.0f * A;
  const float c1 = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  const float c2 = ((A + 2.0f) * u - (A + 3.0f)) * u * u + 1.0f;
  const float c3 = 1.0f - c0 - c1 - c2;
  *s = (int)fl - 1;
  w[0] = (short)rintf(c0 * 2048.0f);
  w[1] = (short)rintf(c1 * 2048.0f);
  w[2] = (short)rintf(c2 * 2048.0f);
  w[3] = (short)rintf(c3 * 2048.0f);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int sat_u8(float v) {   // saturate_cast<uchar>(float): round half to even, then clamp
  const float r = rintf(v);
  return r < 0.0f ? 0 : (r > 255.0f ? 255 : (int)r);
}

// cv2.cvtColor(RGB2HSV) on bytes -> LUTs -> cv2.cvtColor(HSV2RGB) on bytes (detection_dataset.py:195-205)
__device__ __forceinline__ void colour(int& r, int& g, int& b, const int* sdiv, const int* hdiv, const uint8_t* lut) {
  const int v = max(r, max(g, b)), mn = min(r, min(g, b));
  const int diff = v - mn;
  const int s = (diff * sdiv[v] + 2048) >> 12;
  int num;
  if (v == r) num = g - b;
  else if (v == g) num = b - r + 2 * diff;
  else num = r - g + 4 * diff;
  int h = (num * hdiv[diff] + 2048) >> 12;
  if (h < 0) h += 180;
  const int hb = lut[clampi(h, 0, 255)], sb = lut[256 + clampi(s, 0, 255)], vb = lut[512 + v];
  float hf = (float)hb * (6.0f / 180.0f);
  const float sf = (float)sb / 255.0f, vf = (float)vb / 255.0f;
  float fr = vf, fg = vf, fb = vf;
  if (sb != 0) {
    while (hf >= 6.0f) hf -= 6.0f;
    int sector = (int)floorf(hf);
    hf -= (float)sector;
    if ((unsigned)sector >= 6u) {
      sector = 0;
      hf = 0.0f;
    }
    const float t0 = vf, t1 = vf * (1.0f - sf), t2 = vf * (1.0f - sf * hf), t3 = vf * (1.0f - sf * (1.0f - hf));
    switch (sector) {   // OpenCV's sector table, (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}]
      case 0: fb = t1; fg = t3; fr = t0; break;
      case 1: fb = t1; fg = t0; fr = t2; break;
      case 2: fb = t3; fg = t0; fr = t1; break;
      case 3: fb = t0; fg = t2; fr = t1; break;
      case 4: fb = t0; fg = t1; fr = t3; break;
      default: fb = t2; fg = t1; fr = t0; break;
    }
  }
  r = sat_u8(fr * 255.0f);
  g = sat_u8(fg * 255.0f);
  b = sat_u8(fb * 255.0f);
}

template <bool COLOUR>
__global__ __launch_bounds__(256) void aug_images_kernel(const cvx_aug_job* __restrict__ jobs, const int32_t* __restrict__ job_start,
                                                         const uint8_t* __restrict__ luts, float* __restrict__ out, int H, int W) {
  __shared__ cvx_aug_job sjob[MAXJ];
  __shared__ int col_s[MAXJ][TW], row_s[MAXJ][TH];
  __shared__ short col_w[MAXJ][TW][4], row_w[MAXJ][TH][4];
  __shared__ int sdiv[256], hdiv[256];
  __shared__ uint8_t lut[768];
  const int tid = threadIdx.x, img = blockIdx.z;
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
  const int j0 = job_start[img];
  const int nj = min(job_start[img + 1] - j0, MAXJ);
  if (tid < nj) sjob[tid] = jobs[j0 + tid];
  // OpenCV's division tables: rint((255 << 12) / i) and rint((180 << 12) / (6 i)); no quotient is a tie for i < 256, so the rounded
  // integer division is the same number
  if constexpr (COLOUR) {
    sdiv[tid] = tid ? (2 * (255 << 12) + tid) / (2 * tid) : 0;
    hdiv[tid] = tid ? (2 * (180 << 12) + 6 * tid) / (12 * tid) : 0;
    for (int i = tid; i < 768; i += 256) lut[i] = luts[(size_t)img * 768 + i];
  }
  __syncthreads();
  for (int e = tid; e < nj * (TW + TH); e += 256) {
    const int s = e / (TW + TH), k = e - s * (TW + TH);
    const cvx_aug_job& jb = sjob[s];
    if (k < TW) {
      int x = tx0 + k;
      if (jb.quad < 0 && jb.flip) x = W - 1 - x;          // the canvas is mirrored after the paste
      const int rx = x - jb.dx;
      if (rx < 0 || rx >= jb.nw || x < 0) col_s[s][k] = OUTSIDE;
      else cubic_tap(rx, jb.nw, jb.iw, &col_s[s][k], col_w[s][k]);
    } else {
      const int ry = ty0 + (k - TW) - jb.dy;
      if (ry < 0 || ry >= jb.nh) row_s[s][k - TW] = OUTSIDE;
      else cubic_tap(ry, jb.nh, jb.ih, &row_s[s][k - TW], row_w[s][k - TW]);
    }
  }
  __syncthreads();
  const int lx = tid & 63, x = tx0 + lx;
  if (x >= W) return;
  const size_t plane = (size_t)H * W;
  for (int ly = tid >> 6; ly < TH; ly += 4) {
    const int y = ty0 + ly;
    if (y >= H) break;
    int s = -1;
    for (int q = 0; q < nj; ++q)
      if (x >= sjob[q].x0 && x < sjob[q].x1 && y >= sjob[q].y0 && y < sjob[q].y1) s = q;
    int r = 128, g = 128, b = 128;
    if (s >= 0 && col_s[s][lx] != OUTSIDE && row_s[s][ly] != OUTSIDE) {
      const cvx_aug_job& jb = sjob[s];
      const int iw = jb.iw, ih = jb.ih, cs = col_s[s][lx], rs = row_s[s][ly];
      const bool mirror = jb.quad >= 0 && jb.flip;           // mosaic: the source is mirrored before the resize
      int off[4], wx[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = clampi(cs + k, 0, iw - 1);
        off[k] = 3 * (mirror ? iw - 1 - c : c);
        wx[k] = col_w[s][lx][k];
      }
      int ar = 0, ag = 0, ab = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t* p = jb.src + (size_t)clampi(rs + j, 0, ih - 1) * iw * 3;
        int hr = 0, hg = 0, hb = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          hr += wx[k] * p[off[k]];
          hg += wx[k] * p[off[k] + 1];
          hb += wx[k] * p[off[k] + 2];
        }
        const int wy = row_w[s][ly][j];
        ar += wy * hr;
        ag += wy * hg;
        ab += wy * hb;
      }
      r = clampi((ar + (1 << 21)) >> 22, 0, 255);
      g = clampi((ag + (1 << 21)) >> 22, 0, 255);
      b = clampi((ab + (1 << 21)) >> 22, 0, 255);
    }
    if constexpr (COLOUR) colour(r, g, b, sdiv, hdiv, lut);
    float* o = out + (size_t)img * 3 * plane + (size_t)y * W + x;
    o[0] = (float)r / 255.0f;
    o[plane] = (float)g / 255.0f;
    o[2 * plane] = (float)b / 255.0f;
  }
}

// The last job in [lo, hi] whose first box is <= i (jobs without boxes are skipped over).
__device__ __forceinline__ int job_of_box(const int32_t* __restrict__ job_box_start, int lo, int hi, int i) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (job_box_start[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One source box (x1, y1, x2, y2, cls) of job jb -> o = [cls, cx, cy, w, h] normalised; returns whether the box is kept.  Both box kernels
// go through here, so their rows agree to the bit.
__device__ __forceinline__ bool box_row(const cvx_aug_job& jb, const float* __restrict__ bx, float fW, float fH, float* o) {
  float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
  const float fiw = (float)jb.iw, fih = (float)jb.ih, fnw = (float)jb.nw, fnh = (float)jb.nh, fdx = (float)jb.dx, fdy = (float)jb.dy;
  if (jb.quad >= 0 && jb.flip) {                        // mosaic_body :231, with iw = columns
    const float a = fiw - x2, c = fiw - x1;
    x1 = a;
    x2 = c;
  }
  x1 = x1 * fnw / fiw + fdx;
  x2 = x2 * fnw / fiw + fdx;
  y1 = y1 * fnh / fih + fdy;
  y2 = y2 * fnh / fih + fdy;
  if (jb.quad < 0 && jb.flip) {                         // get_random_data :212
    const float a = fW - x2, c = fW - x1;
    x1 = a;
    x2 = c;
  }
  if (x1 < 0.0f) x1 = 0.0f;
  if (y1 < 0.0f) y1 = 0.0f;
  if (x2 > fW) x2 = fW;
  if (y2 > fH) y2 = fH;
  bool keep = (x2 - x1 > 1.0f) && (y2 - y1 > 1.0f);
  if (keep && jb.quad >= 0) {                           // merge_bboxes :405-449
    const int q = jb.quad;
    const float cutx = (float)(q <= 1 ? jb.x1 : jb.x0), cuty = (float)((q == 0 || q == 3) ? jb.y1 : jb.y0);
    const bool sy = y2 >= cuty && y1 <= cuty, sx = x2 >= cutx && x1 <= cutx;
    if (q == 0) {
      if (y1 > cuty || x1 > cutx) keep = false;
      if (sy) y2 = cuty;
      if (sx) x2 = cutx;
    } else if (q == 1) {
      if (y2 < cuty || x1 > cutx) keep = false;
      if (sy) y1 = cuty;
      if (sx) x2 = cutx;
    } else if (q == 2) {
      if (y2 < cuty || x2 < cutx) keep = false;
      if (sy) y1 = cuty;
      if (sx) x1 = cutx;
    } else {
      if (y1 > cuty || x2 < cutx) keep = false;
      if (sy) y2 = cuty;
      if (sx) x1 = cutx;
    }
  }
  x1 = x1 / fW;                                         // detection_dataset.py:110-119
  x2 = x2 / fW;
  y1 = y1 / fH;
  y2 = y2 / fH;
  const float bw = x2 - x1, bh = y2 - y1;
  o[0] = bx[4];
  o[1] = x1 + bw / 2.0f;
  o[2] = y1 + bh / 2.0f;
  o[3] = bw;
  o[4] = bh;
  return keep;
}

// Rank of this thread's kept box among the 256 of the chunk, in thread order: ballot + popcount inside the wave, the four wave totals
// through LDS.  Returns the chunk's total in *total.  Ends on a barrier, so wave_tot may be written again right after.
__device__ __forceinline__ int chunk_rank(bool keep, int* wave_tot, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_tot[wave] = __popcll(m);
  __syncthreads();
  int pos = __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += wave_tot[w];
  *total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
  __syncthreads();
  return pos;
}

// One workgroup walks all boxes in chunks of 256; kept boxes take consecutive output rows in source order (ballot scan per wave, wave
// totals through LDS) -- no atomics, so the order and the result never depend on timing.
__global__ __launch_bounds__(256) void aug_boxes_kernel(const cvx_aug_job* __restrict__ jobs, const int32_t* __restrict__ job_box_start, int n_jobs,
                                                        const float* __restrict__ boxes, int n_boxes, int H, int W, float* __restrict__ targets,
                                                        int32_t* __restrict__ count) {
  __shared__ int wave_tot[4];
  const int tid = threadIdx.x;
  const float fW = (float)W, fH = (float)H;
  int base = 0;
  for (int c0 = 0; c0 < n_boxes; c0 += 256) {
    const int i = c0 + tid;
    bool keep = false;
    float image = 0, o[5] = {0, 0, 0, 0, 0};
    if (i < n_boxes) {
      const cvx_aug_job jb = jobs[job_of_box(job_box_start, 0, n_jobs - 1, i)];
      keep = box_row(jb, boxes + (size_t)i * 5, fW, fH, o);
      image = (float)jb.out;
    }
    int total;
    const int pos = base + chunk_rank(keep, wave_tot, &total);
    if (keep) {
      float* t = targets + (size_t)pos * 6;
      t[0] = image; t[1] = o[0]; t[2] = o[1]; t[3] = o[2]; t[4] = o[3]; t[5] = o[4];
    }
    base += total;
  }
  for (int i = base + tid; i < n_boxes; i += 256) {         // unused rows: image -1
    float* t = targets + (size_t)i * 6;
    t[0] = -1.0f; t[1] = 0.0f; t[2] = 0.0f; t[3] = 0.0f; t[4] = 0.0f; t[5] = 0.0f;
  }
  if (tid == 0) *count = base;
}

// One workgroup per output image: the boxes of its jobs (job_start[b] .. job_start[b+1]) in chunks of 256, kept ones to rows 0, 1, .. of
// labels[b] in source order; rows past max_boxes are dropped and reported, unused rows are zero.
__global__ __launch_bounds__(256) void aug_boxes_padded_kernel(const cvx_aug_job* __restrict__ jobs, const int32_t* __restrict__ job_start,
                                                               const int32_t* __restrict__ job_box_start, const float* __restrict__ boxes, int H, int W,
                                                               int max_boxes, float* __restrict__ labels, int32_t* __restrict__ counts,
                                                               int32_t* __restrict__ overflow) {
  __shared__ int wave_tot[4];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float fW = (float)W, fH = (float)H;
  const int j0 = job_start[b], j1 = job_start[b + 1];
  const int b0 = j1 > j0 ? job_box_start[j0] : 0, b1 = j1 > j0 ? job_box_start[j1] : 0;
  float* lab = labels + (size_t)b * max_boxes * 5;
  int base = 0;
  for (int c0 = b0; c0 < b1; c0 += 256) {
    const int i = c0 + tid;
    bool keep = false;
    float o[5] = {0, 0, 0, 0, 0};
    if (i < b1) {
      const cvx_aug_job jb = jobs[job_of_box(job_box_start, j0, j1 - 1, i)];
      keep = box_row(jb, boxes + (size_t)i * 5, fW, fH, o);
    }
    int total;
    const int pos = base + chunk_rank(keep, wave_tot, &total);
    if (keep && pos < max_boxes) {
      float* t = lab + (size_t)pos * 5;
      t[0] = o[0]; t[1] = o[1]; t[2] = o[2]; t[3] = o[3]; t[4] = o[4];
    }
    base += total;
  }
  const int kept = min(base, max_boxes);
  for (int i = kept * 5 + tid; i < max_boxes * 5; i += 256) lab[i] = 0.0f;
  if (tid == 0) {
    counts[b] = kept;
    if (base > max_boxes) *overflow = 1;                    // every workgroup that overflows stores the same word; the entry point cleared it
  }
}

}  // namespace

extern "C" int cvx_aug_images(const cvx_aug_job* jobs, const int32_t* job_start, const uint8_t* luts, int32_t batch, float* out_nchw, int32_t H,
                              int32_t W, void* hip_stream) {
  static_assert(sizeof(cvx_aug_job) == 64, "cvx_aug_job is 64 bytes on both sides of the ABI");
  CVX_CHECK(jobs && job_start && luts && out_nchw, "null pointer");
  CVX_CHECK(batch > 0 && batch <= 65535 && H > 0 && W > 0 && (long long)H * W * 3 < (1ll << 31), "bad shape");
  const dim3 grid(cvx_cdiv(W, TW), cvx_cdiv(H, TH), batch);
  CVX_CHECK(grid.y <= 65535, "output too tall");
  hipLaunchKernelGGL(aug_images_kernel<true>, grid, dim3(256), 0, (hipStream_t)hip_stream, jobs, job_start, luts, out_nchw, H, W);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_aug_images_plain(const cvx_aug_job* jobs, const int32_t* job_start, int32_t batch, float* out_nchw, int32_t H, int32_t W,
                                    void* hip_stream) {
  CVX_CHECK(jobs && job_start && out_nchw, "null pointer");
  CVX_CHECK(batch > 0 && batch <= 65535 && H > 0 && W > 0 && (long long)H * W * 3 < (1ll << 31), "bad shape");
  const dim3 grid(cvx_cdiv(W, TW), cvx_cdiv(H, TH), batch);
  CVX_CHECK(grid.y <= 65535, "output too tall");
  hipLaunchKernelGGL(aug_images_kernel<false>, grid, dim3(256), 0, (hipStream_t)hip_stream, jobs, job_start, (const uint8_t*)nullptr, out_nchw, H,
                     W);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_aug_boxes(const cvx_aug_job* jobs, const int32_t* job_box_start, int32_t n_jobs, const float* boxes, int32_t n_boxes, int32_t H,
                             int32_t W, float* targets, int32_t* count, void* hip_stream) {
  CVX_CHECK(jobs && job_box_start && count && n_jobs > 0 && n_boxes >= 0 && H > 0 && W > 0, "bad arguments");
  CVX_CHECK(n_boxes == 0 || (boxes && targets), "boxes without a buffer");
  hipLaunchKernelGGL(aug_boxes_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, jobs, job_box_start, n_jobs, boxes, n_boxes, H, W, targets,
                     count);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_aug_boxes_padded(const cvx_aug_job* jobs, const int32_t* job_start, const int32_t* job_box_start, int32_t batch,
                                    const float* boxes, int32_t n_boxes, int32_t H, int32_t W, int32_t max_boxes, float* labels, int32_t* counts,
                                    int32_t* overflow, void* hip_stream) {
  CVX_CHECK(jobs && job_start && job_box_start && labels && counts && overflow, "null pointer");
  CVX_CHECK(batch > 0 && n_boxes >= 0 && H > 0 && W > 0 && max_boxes > 0 && (long long)max_boxes * 5 < (1ll << 31), "bad arguments");
  CVX_CHECK(n_boxes == 0 || boxes, "boxes without a buffer");
  CVX_HIP(hipMemsetAsync(overflow, 0, sizeof(int32_t), (hipStream_t)hip_stream));
  hipLaunchKernelGGL(aug_boxes_padded_kernel, dim3(batch), dim3(256), 0, (hipStream_t)hip_stream, jobs, job_start, job_box_start, boxes, H, W,
                     max_boxes, labels, counts, overflow);
  CVX_HIP(hipGetLastError());
  return 0;
}

// ---- stage 2: affine / perspective warp, MixUp inside the batch, and the boxes that go with them ---------------------
// Stage 1 above writes its canvases and padded labels into scratch; two further launches turn them into the batch and the targets.  The
// rules are the project's own, modelled on YOLOv5's random_perspective / box_candidates / mixup, and tests/aug_warp_restatement.py holds
// both kernels to the bit.  The fp32 operation order, every step rounded on its own (contraction is off for the whole file):
//
//   pixel (x, y), integer coordinates, no half-pixel shift:
//     u' = (i0 * x + i1 * y) + i2,  v' = (i3 * x + i4 * y) + i5,  w = (i6 * x + i7 * y) + i8      (i = M^-1, row-major)
//     u = u' / w,  v = v' / w                                       (always divided)
//     if not (-1 < u < W and -1 < v < H): no tap can lie on the canvas, the value is the grey 128 / 255 itself
//     x0 = floor(u), lx = u - x0, y0 = floor(v), ly = v - y0; a tap outside the canvas is the grey
//     top = v00 * (1 - lx) + v01 * lx,  bot = v10 * (1 - lx) + v11 * lx,  value = top * (1 - ly) + bot * ly
//   MixUp: out = own * r + partner * r1 (both products rounded, then the sum); an output without a partner is `own` untouched
//   box [cls, cx, cy, w, h]: pcx = cx * W, pw = w * W, x1 = pcx - pw / 2, x2 = pcx + pw / 2 (y alike with H); the corners (x1, y1), (x2, y2),
//     (x1, y2), (x2, y1) through M as above ((m0 * x + m1 * y) + m2, ... , divided by the third row's value); min / max of the four,
//     clipped to [0, W] x [0, H]; w2 = X2 - X1, h2 = Y2 - Y1, w1 = x2 - x1, h1 = y2 - y1; kept iff w2 > min_wh and h2 > min_wh and
//     (w2 * h2) / ((w1 * s) * (h1 * s)) > min_area_ratio and fmax(w2 / h2, h2 / w2) < max_aspect; then the tail of box_row():
//     X / W, Y / H, bw = X2 - X1, cx = X1 + bw / 2.
namespace {

static_assert(sizeof(cvx_aug_view) == 96, "cvx_aug_view is 96 bytes on both sides of the ABI");

__device__ __forceinline__ void project(const float* __restrict__ m, float x, float y, float* px, float* py) {
  const float a = (m[0] * x + m[1] * y) + m[2];
  const float b = (m[3] * x + m[4] * y) + m[5];
  const float w = (m[6] * x + m[7] * y) + m[8];
  *px = a / w;
  *py = b / w;
}

// the three planes of output pixel (x, y) of one canvas seen through inv = M^-1
__device__ __forceinline__ void warp_pixel(const float* __restrict__ canvas, size_t plane, const float* __restrict__ inv, int x, int y, int H, int W,
                                           float* o) {
  const float grey = 128.0f / 255.0f;
  float u, v;
  project(inv, (float)x, (float)y, &u, &v);
  if (!(u > -1.0f && u < (float)W && v > -1.0f && v < (float)H)) {   // also every NaN
    o[0] = o[1] = o[2] = grey;
    return;
  }
  const float xf = floorf(u), yf = floorf(v);
  const float lx = u - xf, ly = v - yf, omx = 1.0f - lx, omy = 1.0f - ly;
  const int x0 = (int)xf, y0 = (int)yf;                              // -1 .. W - 1, -1 .. H - 1
  const bool xa = x0 >= 0, xb = x0 + 1 < W, ya = y0 >= 0, yb = y0 + 1 < H;
  const long long at = (long long)y0 * W + x0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = canvas + c * plane;
    const float v00 = (xa && ya) ? p[at] : grey, v01 = (xb && ya) ? p[at + 1] : grey;
    const float v10 = (xa && yb) ? p[at + W] : grey, v11 = (xb && yb) ? p[at + W + 1] : grey;
    const float top = v00 * omx + v01 * lx, bot = v10 * omx + v11 * lx;
    o[c] = top * omy + bot * ly;
  }
}

// The tile and the thread -> pixel map of aug_images_kernel: a wave stores 256 contiguous bytes per plane.  The view of an output is the
// same for the whole workgroup, so its matrix arrives through scalar loads and the partner branch never diverges.
__global__ __launch_bounds__(256) void aug_warp_mix_kernel(const float* __restrict__ canvases, const cvx_aug_view* __restrict__ views, int batch,
                                                           float* __restrict__ out, int H, int W) {
  const int tid = threadIdx.x, img = blockIdx.z;
  const int x = blockIdx.x * TW + (tid & 63), ty0 = blockIdx.y * TH;
  if (x >= W) return;
  const size_t plane = (size_t)H * W;
  const cvx_aug_view& vw = views[img];
  const int p = vw.partner;
  const bool mix = p >= 0 && p < batch;
  const float r = vw.r, r1 = vw.r1;
  for (int ly = tid >> 6; ly < TH; ly += 4) {
    const int y = ty0 + ly;
    if (y >= H) break;
    float a[3];
    warp_pixel(canvases + (size_t)img * 3 * plane, plane, vw.inv, x, y, H, W, a);
    if (mix) {
      float b[3];
      warp_pixel(canvases + (size_t)p * 3 * plane, plane, views[p].inv, x, y, H, W, b);
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c] = a[c] * r + b[c] * r1;
    }
    float* o = out + (size_t)img * 3 * plane + (size_t)y * W + x;
    o[0] = a[0];
    o[plane] = a[1];
    o[2 * plane] = a[2];
  }
}

// One stage-1 label l = [cls, cx, cy, w, h] through the view of its canvas -> o in the same form; returns whether the box is kept.
__device__ __forceinline__ bool warp_box_row(const cvx_aug_view& vw, const float* __restrict__ l, float fW, float fH, float min_wh, float min_area,
                                             float max_aspect, float* o) {
  const float pcx = l[1] * fW, pcy = l[2] * fH, pw = l[3] * fW, ph = l[4] * fH;
  const float x1 = pcx - pw / 2.0f, x2 = pcx + pw / 2.0f, y1 = pcy - ph / 2.0f, y2 = pcy + ph / 2.0f;
  float ax, ay, bx, by, cx, cy, dx, dy;
  project(vw.m, x1, y1, &ax, &ay);
  project(vw.m, x2, y2, &bx, &by);
  project(vw.m, x1, y2, &cx, &cy);
  project(vw.m, x2, y1, &dx, &dy);
  float X1 = fminf(fminf(ax, bx), fminf(cx, dx)), X2 = fmaxf(fmaxf(ax, bx), fmaxf(cx, dx));
  float Y1 = fminf(fminf(ay, by), fminf(cy, dy)), Y2 = fmaxf(fmaxf(ay, by), fmaxf(cy, dy));
  X1 = fminf(fmaxf(X1, 0.0f), fW);
  X2 = fminf(fmaxf(X2, 0.0f), fW);
  Y1 = fminf(fmaxf(Y1, 0.0f), fH);
  Y2 = fminf(fmaxf(Y2, 0.0f), fH);
  const float w2 = X2 - X1, h2 = Y2 - Y1, w1 = x2 - x1, h1 = y2 - y1;
  const float ratio = (w2 * h2) / ((w1 * vw.s) * (h1 * vw.s));
  const float aspect = fmaxf(w2 / h2, h2 / w2);
  const bool keep = w2 > min_wh && h2 > min_wh && ratio > min_area && aspect < max_aspect;
  const float nx1 = X1 / fW, nx2 = X2 / fW, ny1 = Y1 / fH, ny2 = Y2 / fH;
  const float bw = nx2 - nx1, bh = ny2 - ny1;
  o[0] = l[0];
  o[1] = nx1 + bw / 2.0f;
  o[2] = ny1 + bh / 2.0f;
  o[3] = bw;
  o[4] = bh;
  return keep;
}

// Output b takes the kept boxes of its own canvas in stage-1 order, then those of its partner's canvas, each through the view of the
// canvas it came from.  The padded form, one workgroup per output: labels[b] (cap_out, 5), counts[b] and the overflow word, the shape of
// aug_boxes_padded_kernel with its scan (chunk_rank), no atomics.
__global__ __launch_bounds__(256) void aug_boxes_warp_padded_kernel(const float* __restrict__ labels_in, const int32_t* __restrict__ counts_in,
                                                                    int cap_in, const cvx_aug_view* __restrict__ views, int batch, int H, int W,
                                                                    float min_wh, float min_area, float max_aspect, float* __restrict__ out,
                                                                    int cap_out, int32_t* __restrict__ counts, int32_t* __restrict__ overflow) {
  __shared__ int wave_tot[4];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float fW = (float)W, fH = (float)H;
  const int partner = views[b].partner;
  float* lab_out = out + (size_t)b * cap_out * 5;
  int base = 0;
  for (int seg = 0; seg < 2; ++seg) {
    const int c = seg ? partner : b;
    if (c < 0 || c >= batch) break;
    const cvx_aug_view vw = views[c];
    const int n = min(counts_in[c], cap_in);
    const float* lab = labels_in + (size_t)c * cap_in * 5;
    for (int c0 = 0; c0 < n; c0 += 256) {
      const int i = c0 + tid;
      bool keep = false;
      float o[5] = {0, 0, 0, 0, 0};
      if (i < n) keep = warp_box_row(vw, lab + (size_t)i * 5, fW, fH, min_wh, min_area, max_aspect, o);
      int total;
      const int pos = base + chunk_rank(keep, wave_tot, &total);
      if (keep && pos < cap_out) {
        float* t = lab_out + (size_t)pos * 5;
        t[0] = o[0]; t[1] = o[1]; t[2] = o[2]; t[3] = o[3]; t[4] = o[4];
      }
      base += total;
    }
  }
  const int kept = min(base, cap_out);
  for (int i = kept * 5 + tid; i < cap_out * 5; i += 256) lab_out[i] = 0.0f;
  if (tid == 0) {
    counts[b] = kept;
    if (base > cap_out) *overflow = 1;
  }
}

// The compact form, rows [image, cls, cx, cy, w, h] in image order from row 0 on, the rest of the cap_out rows with image -1, and the row
// count: the form of aug_boxes_kernel.  The rows of all outputs share one numbering, so one workgroup makes them, but not output after
// output (a batch of 32 with partners is 64 short lists, and a walk with two barriers per list took 50 - 90 us): each of its 16 waves
// takes every 16th output and walks that output's lists 64 boxes at a time with a ballot, once to count the kept boxes, and, after an
// integer scan of the counts in LDS, a second time to write them at their place.  The order is fixed by construction, no atomics.
constexpr int COMPACT_THREADS = 1024, COMPACT_MAX_BATCH = 4096;

// One pass over the lists of output b by one wave.  WRITE: rows from `base` on.  Returns the number of kept boxes.
template <bool WRITE>
__device__ __forceinline__ int compact_walk(const float* __restrict__ labels_in, const int32_t* __restrict__ counts_in, int cap_in,
                                            const cvx_aug_view* __restrict__ views, int batch, int b, float fW, float fH, float min_wh, float min_area,
                                            float max_aspect, float* __restrict__ out, int cap_out, int base) {
  const int lane = threadIdx.x & 63;
  const int partner = views[b].partner;
  int kept = 0;
  for (int seg = 0; seg < 2; ++seg) {
    const int c = seg ? partner : b;
    if (c < 0 || c >= batch) break;
    const cvx_aug_view vw = views[c];
    const int n = min(counts_in[c], cap_in);
    const float* lab = labels_in + (size_t)c * cap_in * 5;
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int i = c0 + lane;
      bool keep = false;
      float o[5] = {0, 0, 0, 0, 0};
      if (i < n) keep = warp_box_row(vw, lab + (size_t)i * 5, fW, fH, min_wh, min_area, max_aspect, o);
      const unsigned long long m = __ballot(keep);
      if (WRITE) {
        const int pos = base + kept + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < cap_out) {
          float* t = out + (size_t)pos * 6;
          t[0] = (float)b; t[1] = o[0]; t[2] = o[1]; t[3] = o[2]; t[4] = o[3]; t[5] = o[4];
        }
      }
      kept += __popcll(m);
    }
  }
  return kept;
}

__global__ __launch_bounds__(COMPACT_THREADS) void aug_boxes_warp_compact_kernel(const float* __restrict__ labels_in, const int32_t* __restrict__ counts_in,
                                                                                 int cap_in, const cvx_aug_view* __restrict__ views, int batch, int H,
                                                                                 int W, float min_wh, float min_area, float max_aspect,
                                                                                 float* __restrict__ out, int cap_out, int32_t* __restrict__ count) {
  __shared__ int start[COMPACT_MAX_BATCH + 1];               // start[b]: first row of output b; start[batch]: the number of rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = COMPACT_THREADS / 64;
  const float fW = (float)W, fH = (float)H;
  for (int b = wave; b < batch; b += waves) {
    const int kept = compact_walk<false>(labels_in, counts_in, cap_in, views, batch, b, fW, fH, min_wh, min_area, max_aspect, out, cap_out, 0);
    if (lane == 0) start[b + 1] = kept;
  }
  __syncthreads();
  if (wave == 0) {                                            // inclusive scan of the counts, 64 at a time
    int carry = 0;
    for (int c0 = 0; c0 < batch; c0 += 64) {
      int x = c0 + lane < batch ? start[c0 + lane + 1] : 0;
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
      }
      if (c0 + lane < batch) start[c0 + lane + 1] = carry + x;
      carry += __shfl(x, 63);
    }
    if (lane == 0) start[0] = 0;
  }
  __syncthreads();
  for (int b = wave; b < batch; b += waves)
    compact_walk<true>(labels_in, counts_in, cap_in, views, batch, b, fW, fH, min_wh, min_area, max_aspect, out, cap_out, start[b]);
  const int kept = min(start[batch], cap_out);
  for (int i = kept + tid; i < cap_out; i += COMPACT_THREADS) {   // unused rows: image -1
    float* t = out + (size_t)i * 6;
    t[0] = -1.0f; t[1] = 0.0f; t[2] = 0.0f; t[3] = 0.0f; t[4] = 0.0f; t[5] = 0.0f;
  }
  if (tid == 0) *count = kept;
}

}  // namespace

extern "C" int cvx_aug_warp_mix(const float* canvases, const cvx_aug_view* views, int32_t batch, float* out_nchw, int32_t H, int32_t W,
                                void* hip_stream) {
  CVX_CHECK(canvases && views && out_nchw && canvases != out_nchw, "null pointer, or the warp in place");
  CVX_CHECK(batch > 0 && batch <= 65535 && H > 0 && W > 0 && (long long)H * W * 3 < (1ll << 31), "bad shape");
  const dim3 grid(cvx_cdiv(W, TW), cvx_cdiv(H, TH), batch);
  CVX_CHECK(grid.y <= 65535, "output too tall");
  hipLaunchKernelGGL(aug_warp_mix_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, canvases, views, batch, out_nchw, H, W);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_aug_boxes_warp(const float* labels_in, const int32_t* counts_in, int32_t cap_in, const cvx_aug_view* views, int32_t batch,
                                  int32_t H, int32_t W, float min_wh, float min_area_ratio, float max_aspect, int32_t compact, float* out,
                                  int32_t cap_out, int32_t* counts, int32_t* overflow, void* hip_stream) {
  CVX_CHECK(labels_in && counts_in && views && out && counts, "null pointer");
  CVX_CHECK(batch > 0 && H > 0 && W > 0 && cap_in > 0 && cap_out > 0 && (long long)cap_in * 5 < (1ll << 31) && (long long)cap_out * 6 < (1ll << 31),
            "bad arguments");
  if (compact) {
    CVX_CHECK(batch <= COMPACT_MAX_BATCH, "the compact form takes a batch of at most 4096");
    hipLaunchKernelGGL(aug_boxes_warp_compact_kernel, dim3(1), dim3(COMPACT_THREADS), 0, (hipStream_t)hip_stream, labels_in, counts_in, cap_in, views,
                       batch, H, W, min_wh, min_area_ratio, max_aspect, out, cap_out, counts);
  } else {
    CVX_CHECK(overflow, "the padded form needs the overflow word");
    CVX_HIP(hipMemsetAsync(overflow, 0, sizeof(int32_t), (hipStream_t)hip_stream));
    hipLaunchKernelGGL(aug_boxes_warp_padded_kernel, dim3(batch), dim3(256), 0, (hipStream_t)hip_stream, labels_in, counts_in, cap_in, views, batch, H,
                       W, min_wh, min_area_ratio, max_aspect, out, cap_out, counts, overflow);
  }
  CVX_HIP(hipGetLastError());
  return 0;
}
