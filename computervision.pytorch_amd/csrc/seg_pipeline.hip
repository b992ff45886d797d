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

}  // namespace

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
