// Multi-scale and flip test-time augmentation for segmentation on gfx950: the network runs on the batch at several
// zooms and on its mirror image, and the per-pixel class scores of all views are fused at the picture's size.  Two launches per use, nothing
// is read by the host and no full-resolution logits exist in memory.
//
//   K1 seg_tta_inputs  a thread per output pixel, grid (cdiv(ow, 256), oh, batch * c): the bilinear resize of bilinear.h (align_corners =
//                      False, no antialiasing) of one plane, written to the plain half and, mirrored along x, to the flipped half.
//   K2 seg_fuse        a thread per PX neighbouring pixels of a row, grid (cdiv(ow, 256 * PX), oh, batch) -- the shape of
//                      seg_stitch_kernel (seg_tiles.hip).  The view table (at most 16 views of 24 bytes) is a kernel argument.  Per view:
//                      the taps of bilinear.h from the view's logit level straight to the output size (the number
//                      cvx_resize_bilinear_rows_to_nchw has for that view), read at the mirrored column for a flipped view.
//                      Mode 0: acc += z, one rounded add per view.  Mode 1: acc += softmax(z); a first pass over the taps leaves every
//                      view's (max, sum of exp) per pixel in LDS, the second pass accumulates.  Then the arg max (strict >, the lowest
//                      class wins a tie), the label byte, confusion[target][label] += 1 (LDS histogram or direct atomics, the split of
//                      cvx_seg_criterion_eval) and, in mode 1, the mean probabilities.  The logit chunk, the arg max and the LDS histogram are
//                      seg_tail.h's, shared with render.hip and seg_tiles.hip.
//                      The y taps of every view are the same for the whole workgroup: worked out once into LDS.  Classes go four at a time
//                      with the view loop inside, so no nc-sized register array exists.  PX is 4 in mode 0 and 2 in mode 1, where the
//                      per-view pairs cost 16 bytes of LDS per pixel and view.
// Every fp32 step is one rounded operation, so the file is compiled with contraction off (bilinear.h spells its fused steps out) and
// tests/seg_tta_restatement.py holds K1 and mode 0 of K2 to the bit.
#include "seg_tail.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int TTA_THREADS = 256;
constexpr int MAX_VIEWS = 16;
constexpr int HIST_LDS_CELLS = 8192;   // nc * nc uint32 cells a workgroup counts in (32 KB, nc <= 90): cvx_seg_criterion_eval's split
constexpr int YTAP_BYTES = MAX_VIEWS * 16;

struct ViewTable {
  cvx_seg_view v[MAX_VIEWS];
};
static_assert(sizeof(cvx_seg_view) == 24 && sizeof(ViewTable) == 384, "the view table is 16 entries of 24 bytes");

struct YTap {
  int i0, i1;
  float lam;
  int reserved;
};

__global__ __launch_bounds__(TTA_THREADS) void seg_tta_inputs_kernel(const float* __restrict__ in, int planes, int h, int w, int oh, int ow, int with_flip,
                                                                     float* __restrict__ out) {
  const int x = blockIdx.x * TTA_THREADS + threadIdx.x, y = blockIdx.y, plane = blockIdx.z;   // plane = image * c + channel
  if (x >= ow) return;
  int ya, yb, xa, xb;
  float ly, lx;
  bilinear_src(y, (float)h / (float)oh, h, &ya, &yb, &ly);
  bilinear_src(x, (float)w / (float)ow, w, &xa, &xb, &lx);
  const float* p = in + (long long)plane * h * w;
  const float *ra = p + (long long)ya * w, *rb = p + (long long)yb * w;
  const float v = bilinear_mix(ra[xa], ra[xb], rb[xa], rb[xb], lx, ly);
  float* q = out + ((long long)plane * oh + y) * ow;
  q[x] = v;
  if (with_flip) q[(long long)planes * oh * ow + (ow - 1 - x)] = v;   // the resize first, the mirror second
}

template <int MODE>
__global__ __launch_bounds__(TTA_THREADS) void seg_fuse_kernel(const ViewTable tab, int n_views, int ld, int nc, int oh, int ow, uint8_t* __restrict__ labels,
                                                               const long long* __restrict__ target, unsigned long long* __restrict__ confusion,
                                                               float* __restrict__ probs, int vec_ok, int lds_hist) {
  constexpr int PX = MODE ? 2 : 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  YTap* ytap = reinterpret_cast<YTap*>(smem);
  float2* stash = reinterpret_cast<float2*>(smem + YTAP_BYTES);                                   // mode 1: [n_views * PX][256] (max, sum)
  unsigned* hist = reinterpret_cast<unsigned*>(smem + YTAP_BYTES + (MODE ? n_views * PX * TTA_THREADS * 8 : 0));
  const int tid = threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  const int x0 = (blockIdx.x * TTA_THREADS + tid) * PX;
  const int npx = min(PX, ow - x0);   // <= 0: this thread has no pixel, it only helps with the histogram
  const bool count = confusion != nullptr, vec = vec_ok != 0;

  // ---- the y side, once per workgroup: the taps of every view for this row ----
  if (tid < n_views) {
    const int lh = tab.v[tid].lh;
    YTap t;
    bilinear_src(y, (float)lh / (float)oh, lh, &t.i0, &t.i1, &t.lam);
    t.reserved = 0;
    ytap[tid] = t;
  }
  if (count && lds_hist) hist_zero<TTA_THREADS>(hist, nc);
  __syncthreads();

  // ---- mode 1, first pass: (max, sum of exp) of every view at every pixel of this thread ----
  if (MODE == 1) {
    for (int k = 0; k < n_views; ++k) {
      const cvx_seg_view v = tab.v[k];
      const YTap t = ytap[k];
      const float sx = (float)v.lw / (float)ow;
      const float* ra = v.rows + ((long long)b * v.lh + t.i0) * v.lw * ld;
      const float* rb = v.rows + ((long long)b * v.lh + t.i1) * v.lw * ld;
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        if (j >= npx) continue;
        int xa, xb;
        float lx;
        bilinear_src(v.flip ? ow - 1 - (x0 + j) : x0 + j, sx, v.lw, &xa, &xb, &lx);
        float m = -INFINITY, s = 0.f, z[4];
        for (int c0 = 0; c0 < nc; c0 += 4) {
          logits4(ra + c0, rb + c0, xa, xb, lx, t.lam, ld, c0, nc, vec, z);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c0 + i < nc) m = fmaxf(m, z[i]);
        }
        for (int c0 = 0; c0 < nc; c0 += 4) {
          logits4(ra + c0, rb + c0, xa, xb, lx, t.lam, ld, c0, nc, vec, z);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c0 + i < nc) s += expf(z[i] - m);
        }
        stash[(k * PX + j) * TTA_THREADS + tid] = make_float2(m, s);   // this thread's own cells: no barrier
      }
    }
  }

  // ---- the fusion: classes four at a time, the view loop inside ----
  float best[PX];
  int arg[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) best[j] = 0.f, arg[j] = 0;
  for (int c0 = 0; c0 < nc; c0 += 4) {
    float acc[PX][4];
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
    for (int k = 0; k < n_views; ++k) {   // table order
      const cvx_seg_view v = tab.v[k];
      const YTap t = ytap[k];
      const float sx = (float)v.lw / (float)ow;
      const float* ra = v.rows + ((long long)b * v.lh + t.i0) * v.lw * ld + c0;
      const float* rb = v.rows + ((long long)b * v.lh + t.i1) * v.lw * ld + c0;
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        if (j >= npx) continue;
        int xa, xb;
        float lx, z[4];
        bilinear_src(v.flip ? ow - 1 - (x0 + j) : x0 + j, sx, v.lw, &xa, &xb, &lx);
        logits4(ra, rb, xa, xb, lx, t.lam, ld, c0, nc, vec, z);
        if (MODE == 0) {
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[j][i] = acc[j][i] + z[i];
        } else {
          const float2 ms = stash[(k * PX + j) * TTA_THREADS + tid];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[j][i] = acc[j][i] + expf(z[i] - ms.x) / ms.y;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) argmax4(acc[j], c0, nc, best[j], arg[j]);
    if (MODE == 1 && probs != nullptr) {
      const float n = (float)n_views;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (c0 + i >= nc) continue;
        float* q = probs + (((long long)b * nc + c0 + i) * oh + y) * ow + x0;
#pragma unroll
        for (int j = 0; j < PX; ++j)
          if (j < npx) q[j] = acc[j][i] / n;
      }
    }
  }

  if (npx > 0) {
    const long long at = ((long long)b * oh + y) * ow + x0;
    if (labels != nullptr)
      for (int j = 0; j < npx; ++j) labels[at + j] = (uint8_t)arg[j];
    if (count)
      for (int j = 0; j < npx; ++j) {
        const long long tg = target[at + j];
        if (tg < 0 || tg >= nc) continue;
        if (lds_hist) hist_add(hist, nc, (int)tg, arg[j]);
        else atomicAdd(confusion + (int)tg * nc + arg[j], 1ull);
      }
  }
  if (count && lds_hist) hist_flush<TTA_THREADS>(hist, nc, confusion);
}

}  // namespace

extern "C" int cvx_seg_tta_inputs(const float* images_nchw, int32_t batch, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t with_flip,
                                  float* out_nchw, void* hip_stream) {
  CVX_CHECK(images_nchw && out_nchw, "null arguments");
  CVX_CHECK(batch > 0 && c > 0 && (long long)batch * c <= 65535 && h > 0 && w > 0 && oh > 0 && oh <= 65535 && ow > 0, "bad sizes");
  CVX_CHECK(with_flip == 0 || with_flip == 1, "with_flip: 0 or 1");
  hipLaunchKernelGGL(seg_tta_inputs_kernel, dim3((unsigned)cvx_cdiv(ow, TTA_THREADS), (unsigned)oh, (unsigned)(batch * c)), dim3(TTA_THREADS), 0,
                     (hipStream_t)hip_stream, images_nchw, batch * c, h, w, oh, ow, with_flip, out_nchw);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_seg_fuse(const cvx_seg_view* views_host, int32_t n_views, int32_t ld, int32_t batch, int32_t nc, int32_t oh, int32_t ow, int32_t mode,
                            uint8_t* labels, const int64_t* target, int64_t* confusion, float* probs_nchw, void* hip_stream) {
  CVX_CHECK(views_host, "null arguments");
  CVX_CHECK(n_views >= 1 && n_views <= MAX_VIEWS, "1 <= n_views <= 16: the table is a kernel argument");
  CVX_CHECK(batch > 0 && batch <= 65535 && oh > 0 && oh <= 65535 && ow > 0, "bad sizes");
  CVX_CHECK(nc > 0 && nc <= 256 && ld >= nc && ld <= 4096, "bad logits shape (labels are bytes: nc <= 256)");
  CVX_CHECK(mode == 0 || mode == 1, "mode: 0 logits, 1 prob");
  CVX_CHECK((target == nullptr) == (confusion == nullptr), "targets and counts come together");
  CVX_CHECK(probs_nchw == nullptr || mode == 1, "probabilities are an output of mode 1 only");
  CVX_CHECK(labels || confusion || probs_nchw, "no output asked for");
  ViewTable tab = {};
  int vec = (ld & 3) == 0;
  for (int k = 0; k < n_views; ++k) {
    const cvx_seg_view v = views_host[k];
    CVX_CHECK(v.rows && v.lh > 0 && v.lw > 0 && (v.flip == 0 || v.flip == 1), "a view: rows, a positive level size, flip 0 or 1");
    vec = vec && (reinterpret_cast<uintptr_t>(v.rows) & 15) == 0;
    tab.v[k] = v;
    tab.v[k].reserved = 0;
  }
  const int lds_hist = nc * nc <= HIST_LDS_CELLS;
  const int hist_bytes = confusion && lds_hist ? nc * nc * 4 : 0;
  const dim3 block(TTA_THREADS);
  hipStream_t st = (hipStream_t)hip_stream;
  if (mode == 0) {
    hipLaunchKernelGGL(seg_fuse_kernel<0>, dim3((unsigned)cvx_cdiv(ow, TTA_THREADS * 4), (unsigned)oh, (unsigned)batch), block, (size_t)(YTAP_BYTES + hist_bytes),
                       st, tab, n_views, ld, nc, oh, ow, labels, (const long long*)target, reinterpret_cast<unsigned long long*>(confusion), probs_nchw, vec,
                       lds_hist);
  } else {
    const int lds = YTAP_BYTES + n_views * 2 * TTA_THREADS * 8 + hist_bytes;
    static unsigned long long optin_done = 0;
    if (lds > 48 * 1024)
      CVX_TRY(cvx_lds_optin((const void*)seg_fuse_kernel<1>, YTAP_BYTES + MAX_VIEWS * 2 * TTA_THREADS * 8 + HIST_LDS_CELLS * 4, &optin_done));
    hipLaunchKernelGGL(seg_fuse_kernel<1>, dim3((unsigned)cvx_cdiv(ow, TTA_THREADS * 2), (unsigned)oh, (unsigned)batch), block, (size_t)lds, st, tab, n_views,
                       ld, nc, oh, ow, labels, (const long long*)target, reinterpret_cast<unsigned long long*>(confusion), probs_nchw, vec, lds_hist);
  }
  CVX_HIP(hipGetLastError());
  return 0;
}
