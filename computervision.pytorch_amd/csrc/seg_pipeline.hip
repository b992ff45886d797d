// Input path of the DeepLabv3+ trainer on gfx950: the reference's segmentation transforms (core/data/segmentation_dataset.py:82-293,
// get_voc_dataloader :256-293) as ONE launch per batch.
//
//   training    ToTensor -> RGB2idx -> Resize(base) -> RandomCrop(crop) -> RandomHorizontalFlip -> Normalize
//   validation  ToTensor -> RGB2idx -> Resize((H, W)) -> Normalize          (a job with rh = H, rw = W, no crop origin, no flip)
//
// The random draws stay on the host (seg_pipeline.draw_seg_params); what arrives here is one 64-byte job per output image.  No resized
// intermediate exists: an output pixel (y, x) maps back through the flip (x -> W - 1 - x) and the crop (+ (i, j)) to a pixel of the
// resized picture, and from there to the four bilinear taps of the source, with torch's fp32 coordinate arithmetic
// (upsample_bilinear2d, align_corners = False: scale = in / out, src = max(scale * (dst + 0.5) - 0.5, 0), upper tap clamped).
//
//   image   byte / 255 per tap, mixed along x in both rows, then along y, then (v - mean[c]) / std[c]
//   label   every tap of a colour mask -> class index by a search of the K-entry colour table (unlisted colour -> class 0, what the
//           reference's 2^24-entry table holds there); the four indices are mixed AS FLOATS and rounded half to even -- what
//           torchvision's F.resize does to an integer tensor (cast to fp32, interpolate, torch.round, cast back), so class boundaries get
//           in-between labels.  label_mode 1 offers nearest instead (F.interpolate(mode="nearest"): floor(dst * scale)).
//
// Every fp32 step is one rounded operation in the order torch's CPU kernel takes them, so the file is compiled with contraction off.
#include "cvx_common.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int SP_TW = 64, SP_TH = 4;   // one workgroup: 64 x 4 output pixels, a wave per row (256 B per plane store)
constexpr int SP_MAX_COLOURS = 256;

struct Tap {
  int i0, i1;
  float w0, w1;
};

// area_pixel_compute_source_index + guard_index_and_lambda (aten/src/ATen/native/UpSample.h)
__device__ __forceinline__ Tap linear_tap(int dst, int in_size, int out_size) {
  const float scale = (float)in_size / (float)out_size;
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  if (s < 0.0f) s = 0.0f;
  int a = (int)s;
  if (a > in_size - 1) a = in_size - 1;
  float lam = s - (float)a;
  lam = fminf(fmaxf(lam, 0.0f), 1.0f);
  Tap t;
  t.i0 = a;
  t.i1 = a + (a < in_size - 1 ? 1 : 0);
  t.w0 = 1.0f - lam;
  t.w1 = lam;
  return t;
}

// nearest_neighbor_compute_source_index: min(floor(dst * scale), in - 1)
__device__ __forceinline__ int nearest_tap(int dst, int in_size, int out_size) {
  const float scale = (float)in_size / (float)out_size;
  const int a = (int)floorf((float)dst * scale);
  return a < in_size - 1 ? a : in_size - 1;
}

__device__ __forceinline__ float mix4(float p00, float p01, float p10, float p11, const Tap& tx, const Tap& ty) {
  const float top = tx.w0 * p00 + tx.w1 * p01;
  const float bot = tx.w0 * p10 + tx.w1 * p11;
  return ty.w0 * top + ty.w1 * bot;
}

// class index of one mask pixel: channels == 1 -> the byte itself; channels == 3 -> its place in the colour table, 0 when unlisted
__device__ __forceinline__ float mask_class(const uint8_t* mask, int channels, long long pix, const int* table, int K) {
  if (channels == 1) return (float)mask[pix];
  const uint8_t* p = mask + pix * 3;
  const int key = ((int)p[0] << 16) | ((int)p[1] << 8) | (int)p[2];
  int cls = 0;
  for (int k = 0; k < K; ++k)
    if (table[k] == key) cls = k;       // a colour listed twice keeps its LAST index, as the reference's table fill does
  return (float)cls;
}

__global__ __launch_bounds__(256) void seg_pipeline_kernel(const cvx_seg_job* __restrict__ jobs, const uint8_t* __restrict__ colours, int K,
                                                           int label_mode, float m0, float m1, float m2, float s0, float s1, float s2,
                                                           float* __restrict__ out, long long* __restrict__ targets, int H, int W) {
  __shared__ int table[SP_MAX_COLOURS];
  __shared__ cvx_seg_job sjob;
  const int tid = threadIdx.x, img = blockIdx.z;
  if (tid == 0) sjob = jobs[img];
  for (int k = tid; k < K; k += 256) table[k] = ((int)colours[3 * k] << 16) | ((int)colours[3 * k + 1] << 8) | (int)colours[3 * k + 2];
  __syncthreads();
  const int x = blockIdx.x * SP_TW + (tid & 63), y = blockIdx.y * SP_TH + (tid >> 6);
  if (x >= W || y >= H) return;
  const cvx_seg_job& jb = sjob;
  const int ih = jb.ih, iw = jb.iw;
  const int ry = y + jb.i, rx = (jb.flip ? W - 1 - x : x) + jb.j;     // the pixel of the resized (rh, rw) picture
  const Tap ty = linear_tap(ry, ih, jb.rh), tx = linear_tap(rx, iw, jb.rw);
  const long long q00 = (long long)ty.i0 * iw + tx.i0, q01 = (long long)ty.i0 * iw + tx.i1;
  const long long q10 = (long long)ty.i1 * iw + tx.i0, q11 = (long long)ty.i1 * iw + tx.i1;
  const size_t plane = (size_t)H * W;
  float* o = out + (size_t)img * 3 * plane + (size_t)y * W + x;
  const uint8_t* src = jb.image;
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = mix4((float)src[q00 * 3 + c] / 255.0f, (float)src[q01 * 3 + c] / 255.0f, (float)src[q10 * 3 + c] / 255.0f,
                         (float)src[q11 * 3 + c] / 255.0f, tx, ty);
    o[c * plane] = (v - mean[c]) / stdv[c];
  }
  const int ch = jb.mask_channels;
  float label;
  if (label_mode == 0) {
    label = rintf(mix4(mask_class(jb.mask, ch, q00, table, K), mask_class(jb.mask, ch, q01, table, K), mask_class(jb.mask, ch, q10, table, K),
                       mask_class(jb.mask, ch, q11, table, K), tx, ty));
  } else {
    label = mask_class(jb.mask, ch, (long long)nearest_tap(ry, ih, jb.rh) * iw + nearest_tap(rx, iw, jb.rw), table, K);
  }
  targets[(size_t)img * plane + (size_t)y * W + x] = (long long)label;
}

// ---- the training recipe: zoom, rotation, padding, photometric distortion, Gaussian blur (cvx_seg_pipeline_aug) --------------------------
// The rules are those of the header comment of cvx_seg_pipeline_aug and DESIGN.md section 7r; tests/seg_aug_restatement.py states them
// operation by operation.  A neutral job (cos = 1, sin = 0, no flags, origin inside the picture) takes exactly the roundings of
// seg_pipeline_kernel above: u = x' + j + 0.5 is a half-integer below 2^22, exact in fp32.
// one workgroup: 32 x 16 output pixels, two per thread.  Measured against 32 x 32, 64 x 8 and 64 x 4: the smaller
// tile keeps 7 workgroups per CU by LDS (21888 bytes) where 32 x 32 keeps 4, and was the fastest with and without blur
constexpr int SA_TW = 32, SA_TH = 16;
constexpr int SA_ROWS = 256 / SA_TW, SA_PER = SA_TH / SA_ROWS;   // rows per pass of the 256 threads, output pixels per thread
constexpr int SA_RMAX = 4;                   // blur radius of the 9-tap kernel
constexpr int SA_EW = SA_TW + 2 * SA_RMAX, SA_EH = SA_TH + 2 * SA_RMAX;     // the tile with its halo
static_assert(256 % SA_TW == 0 && SA_TH % SA_ROWS == 0, "tile");

// linear_tap for a continuous coordinate u of the resized axis (u = dst + 0.5 at pixel centres)
__device__ __forceinline__ Tap linear_tap_at(float u, int in_size, int out_size) {
  const float scale = (float)in_size / (float)out_size;
  float s = scale * u - 0.5f;
  if (s < 0.0f) s = 0.0f;
  int a = (int)s;
  if (a > in_size - 1) a = in_size - 1;
  float lam = s - (float)a;
  lam = fminf(fmaxf(lam, 0.0f), 1.0f);
  Tap t;
  t.i0 = a;
  t.i1 = a + (a < in_size - 1 ? 1 : 0);
  t.w0 = 1.0f - lam;
  t.w1 = lam;
  return t;
}

// nearest_tap for a continuous coordinate: floor((u - 0.5) * in / out), clamped at both ends
__device__ __forceinline__ int nearest_tap_at(float u, int in_size, int out_size) {
  const float scale = (float)in_size / (float)out_size;
  int a = (int)floorf((u - 0.5f) * scale);
  if (a < 0) a = 0;
  return a < in_size - 1 ? a : in_size - 1;
}

__device__ __forceinline__ int mask_class_or(const uint8_t* mask, int channels, long long pix, const int* table, int K, int unlisted) {
  if (channels == 1) return (int)mask[pix];
  const uint8_t* p = mask + pix * 3;
  const int key = ((int)p[0] << 16) | ((int)p[1] << 8) | (int)p[2];
  int cls = unlisted;
  for (int k = 0; k < K; ++k)
    if (table[k] == key) cls = k;
  return cls;
}

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// step 1: output pixel (x, y) -- any integers, the halo of a blur tile lies outside the crop -- to (u, v) in the resized picture
__device__ __forceinline__ bool sa_coords(const cvx_seg_aug_job& jb, int x, int y, int H, int W, float& u, float& v) {
  const int xf = jb.flip ? W - 1 - x : x;
  const float hw = (float)W * 0.5f, hh = (float)H * 0.5f;
  const float px = ((float)xf + 0.5f) - hw, py = ((float)y + 0.5f) - hh;
  u = ((jb.cos * px + jb.sin * py) + hw) + (float)jb.j;
  v = ((jb.cos * py - jb.sin * px) + hh) + (float)jb.i;
  return u >= 0.0f && u < (float)jb.rw && v >= 0.0f && v < (float)jb.rh;
}

// the hexcone HSV step on one pixel: S scaled and clipped when `do_sat`, H shifted and wrapped when `do_hue`
__device__ __forceinline__ void sa_hsv(float& r, float& g, float& b, bool do_sat, float sat, bool do_hue, float hue) {
  const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b), d = mx - mn;
  float S = mx > 0.0f ? d / mx : 0.0f, Hd;
  if (d == 0.0f) {
    Hd = 0.0f;
  } else if (mx == r) {
    Hd = 60.0f * ((g - b) / d);
    if (Hd < 0.0f) Hd = Hd + 360.0f;
  } else if (mx == g) {
    Hd = 60.0f * ((b - r) / d) + 120.0f;
  } else {
    Hd = 60.0f * ((r - g) / d) + 240.0f;
  }
  if (do_sat) S = clip01(S * sat);
  if (do_hue) {
    Hd = Hd + hue;
    if (Hd >= 360.0f) Hd = Hd - 360.0f;
    if (Hd < 0.0f) Hd = Hd + 360.0f;
  }
  const float hh = Hd / 60.0f;
  int sector = (int)hh;
  const float f = hh - (float)sector;
  if (sector >= 6) sector -= 6;
  const float p = mx * (1.0f - S), q = mx * (1.0f - S * f), t = mx * (1.0f - S * (1.0f - f));
  switch (sector) {
    case 0: r = mx, g = t, b = p; break;
    case 1: r = q, g = mx, b = p; break;
    case 2: r = p, g = mx, b = t; break;
    case 3: r = p, g = q, b = mx; break;
    case 4: r = t, g = p, b = mx; break;
    default: r = mx, g = p, b = q; break;
  }
}

// steps 1-3: the [0, 1] colour of the extended plane at (x, y), before blur and normalisation
__device__ __forceinline__ void sa_colour(const cvx_seg_aug_job& jb, int x, int y, int H, int W, float f0, float f1, float f2, float rgb[3]) {
  float u, v;
  if (!sa_coords(jb, x, y, H, W, u, v)) {
    rgb[0] = f0, rgb[1] = f1, rgb[2] = f2;
    return;
  }
  const int iw = jb.iw;
  const Tap ty = linear_tap_at(v, jb.ih, jb.rh), tx = linear_tap_at(u, iw, jb.rw);
  const long long q00 = (long long)ty.i0 * iw + tx.i0, q01 = (long long)ty.i0 * iw + tx.i1;
  const long long q10 = (long long)ty.i1 * iw + tx.i0, q11 = (long long)ty.i1 * iw + tx.i1;
  const uint8_t* src = jb.image;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    rgb[c] = mix4((float)src[q00 * 3 + c] / 255.0f, (float)src[q01 * 3 + c] / 255.0f, (float)src[q10 * 3 + c] / 255.0f,
                  (float)src[q11 * 3 + c] / 255.0f, tx, ty);
  const int fl = jb.flags;
  if (fl & CVX_SEG_AUG_BRIGHTNESS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = clip01(rgb[c] + jb.beta);
  }
  if ((fl & CVX_SEG_AUG_CONTRAST) && !(fl & CVX_SEG_AUG_CONTRAST_LAST)) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = clip01(rgb[c] * jb.alpha);
  }
  if (fl & (CVX_SEG_AUG_SATURATION | CVX_SEG_AUG_HUE))
    sa_hsv(rgb[0], rgb[1], rgb[2], (fl & CVX_SEG_AUG_SATURATION) != 0, jb.sat, (fl & CVX_SEG_AUG_HUE) != 0, jb.hue);
  if ((fl & CVX_SEG_AUG_CONTRAST) && (fl & CVX_SEG_AUG_CONTRAST_LAST)) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = clip01(rgb[c] * jb.alpha);
  }
}

// steps 1-2 for the target of output pixel (x, y), never blurred
__device__ __forceinline__ long long sa_label(const cvx_seg_aug_job& jb, int x, int y, int H, int W, int label_mode, const int* table, int K,
                                              int unlisted, int ignore_index) {
  float u, v;
  if (!sa_coords(jb, x, y, H, W, u, v)) return (long long)ignore_index;
  const int iw = jb.iw, ch = jb.mask_channels;
  if (label_mode == 0) {
    const Tap ty = linear_tap_at(v, jb.ih, jb.rh), tx = linear_tap_at(u, iw, jb.rw);
    const long long q00 = (long long)ty.i0 * iw + tx.i0, q01 = (long long)ty.i0 * iw + tx.i1;
    const long long q10 = (long long)ty.i1 * iw + tx.i0, q11 = (long long)ty.i1 * iw + tx.i1;
    return (long long)rintf(mix4((float)mask_class_or(jb.mask, ch, q00, table, K, unlisted), (float)mask_class_or(jb.mask, ch, q01, table, K, unlisted),
                                 (float)mask_class_or(jb.mask, ch, q10, table, K, unlisted), (float)mask_class_or(jb.mask, ch, q11, table, K, unlisted),
                                 tx, ty));
  }
  return (long long)mask_class_or(jb.mask, ch, (long long)nearest_tap_at(v, jb.ih, jb.rh) * iw + nearest_tap_at(u, iw, jb.rw), table, K, unlisted);
}

__global__ __launch_bounds__(256) void seg_pipeline_aug_kernel(const cvx_seg_aug_job* __restrict__ jobs, const uint8_t* __restrict__ colours, int K,
                                                               int label_mode, int unlisted_mode, int ignore_index, float f0, float f1, float f2,
                                                               float m0, float m1, float m2, float s0, float s1, float s2,
                                                               float* __restrict__ out, long long* __restrict__ targets, int H, int W) {
  __shared__ int table[SP_MAX_COLOURS];
  __shared__ cvx_seg_aug_job sjob;
  __shared__ float tile[3][SA_EW * SA_EH];   // steps 1-3 with the halo; touched by blurred images only
  __shared__ float hrow[3][SA_EH * SA_TW];   // the horizontal pass
  const int tid = threadIdx.x, img = blockIdx.z;
  if (tid == 0) sjob = jobs[img];
  for (int k = tid; k < K; k += 256) table[k] = ((int)colours[3 * k] << 16) | ((int)colours[3 * k + 1] << 8) | (int)colours[3 * k + 2];
  __syncthreads();
  const cvx_seg_aug_job& jb = sjob;
  const int unlisted = unlisted_mode ? ignore_index : 0;
  const int lx0 = tid % SA_TW, ly0 = tid / SA_TW;
  const int x = blockIdx.x * SA_TW + lx0, y0 = blockIdx.y * SA_TH + ly0;
  const size_t plane = (size_t)H * W;
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  int bk = (jb.flags & CVX_SEG_AUG_BLUR) ? jb.blur_k : 0;             // one value for the whole workgroup: blockIdx.z is the image
  if (bk > 2 * SA_RMAX + 1) bk = 2 * SA_RMAX + 1;                     // the job table is device memory nobody checked: stay inside the tile
  if (bk <= 0) {                                                     // no blur: no tile, no further barrier
    if (x >= W) return;
#pragma unroll
    for (int m = 0; m < SA_PER; ++m) {
      const int y = y0 + SA_ROWS * m;
      if (y >= H) break;
      float rgb[3];
      sa_colour(jb, x, y, H, W, f0, f1, f2, rgb);
      float* o = out + (size_t)img * 3 * plane + (size_t)y * W + x;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane] = (rgb[c] - mean[c]) / stdv[c];
      targets[(size_t)img * plane + (size_t)y * W + x] = sa_label(jb, x, y, H, W, label_mode, table, K, unlisted, ignore_index);
    }
    return;
  }
  const int r = bk >> 1, ext = SA_TW + 2 * r, exth = SA_TH + 2 * r;   // bk is 3, 5, 7 or 9
  const int tx0 = blockIdx.x * SA_TW - r, ty0 = blockIdx.y * SA_TH - r;
  for (int idx = tid; idx < ext * exth; idx += 256) {
    const int ly = idx / ext, lx = idx - ly * ext;
    float rgb[3];
    sa_colour(jb, tx0 + lx, ty0 + ly, H, W, f0, f1, f2, rgb);
    tile[0][idx] = rgb[0], tile[1][idx] = rgb[1], tile[2][idx] = rgb[2];
  }
  __syncthreads();
  for (int idx = tid; idx < exth * SA_TW; idx += 256) {
    const int ly = idx / SA_TW, ox = idx % SA_TW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* row = &tile[c][ly * ext + ox];
      float acc = jb.taps[0] * row[0];
      for (int t = 1; t < bk; ++t) acc = acc + jb.taps[t] * row[t];
      hrow[c][idx] = acc;
    }
  }
  __syncthreads();
  if (x >= W) return;
  for (int m = 0; m < SA_PER; ++m) {
    const int oy = ly0 + SA_ROWS * m, y = blockIdx.y * SA_TH + oy;
    if (y >= H) break;
    float* o = out + (size_t)img * 3 * plane + (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* col = &hrow[c][oy * SA_TW + lx0];
      float acc = jb.taps[0] * col[0];
      for (int t = 1; t < bk; ++t) acc = acc + jb.taps[t] * col[t * SA_TW];
      o[c * plane] = (acc - mean[c]) / stdv[c];
    }
    targets[(size_t)img * plane + (size_t)y * W + x] = sa_label(jb, x, y, H, W, label_mode, table, K, unlisted, ignore_index);
  }
}

}  // namespace

extern "C" int cvx_seg_pipeline_aug(const cvx_seg_aug_job* jobs, int32_t batch, const uint8_t* colours, int32_t n_colours, int32_t label_mode,
                                    int32_t unlisted_mode, int32_t ignore_index, const float* fill3, const float* mean3, const float* std3,
                                    float* out_nchw, int64_t* targets, int32_t H, int32_t W, void* hip_stream) {
  static_assert(sizeof(cvx_seg_aug_job) == 128, "cvx_seg_aug_job is 128 bytes on both sides of the ABI");
  CVX_CHECK(jobs && fill3 && mean3 && std3 && out_nchw && targets, "null pointer");
  CVX_CHECK(batch > 0 && batch <= 65535 && H > 0 && W > 0 && (long long)H * W * 3 < (1ll << 31), "bad shape");
  CVX_CHECK(n_colours >= 0 && n_colours <= SP_MAX_COLOURS && (n_colours == 0 || colours), "colour table: at most 256 entries");
  CVX_CHECK(label_mode == 0 || label_mode == 1, "label_mode: 0 bilinear + round (the reference), 1 nearest");
  CVX_CHECK(unlisted_mode == 0 || (unlisted_mode == 1 && label_mode == 1), "unlisted_mode: 0 class 0, 1 ignore_index (nearest labels only)");
  const dim3 grid(cvx_cdiv(W, SA_TW), cvx_cdiv(H, SA_TH), batch);
  CVX_CHECK(grid.y <= 65535, "output too tall");
  hipLaunchKernelGGL(seg_pipeline_aug_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, jobs, colours, n_colours, label_mode, unlisted_mode,
                     ignore_index, fill3[0] / 255.0f, fill3[1] / 255.0f, fill3[2] / 255.0f, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
                     out_nchw, (long long*)targets, H, W);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_seg_pipeline(const cvx_seg_job* jobs, int32_t batch, const uint8_t* colours, int32_t n_colours, int32_t label_mode,
                                const float* mean3, const float* std3, float* out_nchw, int64_t* targets, int32_t H, int32_t W, void* hip_stream) {
  static_assert(sizeof(cvx_seg_job) == 64, "cvx_seg_job is 64 bytes on both sides of the ABI");
  CVX_CHECK(jobs && mean3 && std3 && out_nchw && targets, "null pointer");
  CVX_CHECK(batch > 0 && batch <= 65535 && H > 0 && W > 0 && (long long)H * W * 3 < (1ll << 31), "bad shape");
  CVX_CHECK(n_colours >= 0 && n_colours <= SP_MAX_COLOURS && (n_colours == 0 || colours), "colour table: at most 256 entries");
  CVX_CHECK(label_mode == 0 || label_mode == 1, "label_mode: 0 bilinear + round (the reference), 1 nearest");
  const dim3 grid(cvx_cdiv(W, SP_TW), cvx_cdiv(H, SP_TH), batch);
  CVX_CHECK(grid.y <= 65535, "output too tall");
  hipLaunchKernelGGL(seg_pipeline_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, jobs, colours, n_colours, label_mode, mean3[0], mean3[1],
                     mean3[2], std3[0], std3[1], std3[2], out_nchw, (long long*)targets, H, W);
  CVX_HIP(hipGetLastError());
  return 0;
}
