// Cross-entropy with class weights, label smoothing and online hard example mining (OHEM, "bootstrapped" cross-entropy) for the
// DeepLabv3+ trainer on gfx950 -- the options of the fused criterion of loss_seg.hip, in the same launch chain: no (B, nc, H, W) logits
// tensor, no autograd tape, no sort, no host synchronisation.  This is not in the reference (its build_loss knows FocalLoss() and the
// unweighted nn.CrossEntropyLoss only); the definitions are torch's:
//
//   z_c   bilinearly interpolated logit of class c at a label pixel (PixelTaps, seg_loss_core.h), lse its log-sum-exp, t the target,
//         w the class weights (ones when absent), W = sum_c w_c, eps the smoothing, C = nc
//   l     = (1 - eps) w_t (lse - z_t) + (eps / C) sum_c w_c (lse - z_c)            sum_c w_c (lse - z_c) = W lse - sum_c w_c z_c
//   loss  = sum_{i in S} l_i / sum_{i in S} w_{t_i}      S: the valid pixels (t != ignore_index, 0 <= t < nc), or the kept ones under OHEM
//         = F.cross_entropy(logits, t, weight=w, ignore_index=, label_smoothing=eps, reduction="mean")
//   dl/dz_k = (1 - eps) w_t (p_k - [k == t]) + (eps / C) (W p_k - w_k),  p_k = exp(z_k - lse)
//
// OHEM: key = fp32 max(lse - z_t, 0) (the unweighted, unsmoothed cross-entropy), K = min_kept * batch, theta_t = -ln thresh,
// theta_min = the K-th largest key among the valid pixels (below every key when there are fewer than K).  A pixel is kept iff
// key > theta_t or key >= theta_min: ties at theta_min are all kept, so there is no tie order.  theta_min comes from an 8-bit radix
// select over the keys' bit patterns (non-negative floats order as uint32), the pattern of loss_multibox.hip.
//
//   K1 seg_opts_pixel      one thread per label pixel: the two class passes of seg_loss_pixel_kernel with the weighted terms; the per-pixel
//                          gradient (not yet normalised) -> dlogits (B, nc, OH, OW) fp32; block partials (sum l, sum w_t, valid pixels);
//                          under OHEM also the key plane and the per-pixel loss plane (4 bytes per pixel each)
//   without OHEM           K5 finalize, K6 resize_grad_rows_kernel (the adjoint of loss_seg.hip, norm_mode 1: divided by sum w_t)
//   with OHEM  K2 plan     valid pixels from the partials in a fixed order; rank K or "keep all"
//              K3 hist / pick (x4)   integer atomics only
//              K4 kept_sum  fixed-order block partials of (sum l, sum w_t, kept pixels) over the kept pixels; zeroes the gradients of
//                           the valid pixels that are not kept
//              K5 finalize  loss, the four stats
//              K6 resize_grad_rows_kernel   the same adjoint
// Every sum is a per-workgroup partial in a fixed tree plus one fixed-order pass over the partials: two runs give the same bits.
//
// Evaluation (cvx_seg_eval_opts): seg_eval_kernel of loss_seg.hip with the weighted, smoothed value; the arg max and the confusion
// counts are the same code, so the matrix is cvx_seg_eval's.  OHEM is a training device and is never applied here.
#include <math.h>

#include <algorithm>

#include "seg_loss_core.h"
#include "seg_loss_chain.h"
#include "../../include/cvx_engine.h"

namespace {

struct SegSelect {
  unsigned prefix, remaining;          // radix select state: key bits fixed so far, rank still to resolve inside the prefix bucket
  unsigned theta_t_bits, theta_min_bits;  // kept iff key bits > theta_t_bits or >= theta_min_bits (and the key is a valid pixel's)
  unsigned long long n_valid, k;
  int all;                             // fewer valid pixels than K: every valid pixel is kept, theta_min_bits = 0
  unsigned hist[256];
};

constexpr float SEG_KEY_INVALID = -1.f;  // the key plane's value at a pixel that is not valid: the sign bit marks it
__device__ __forceinline__ bool seg_kept(unsigned bits, unsigned theta_t_bits, unsigned theta_min_bits) {
  return (bits >> 31) == 0u && (bits > theta_t_bits || bits >= theta_min_bits);
}

// Block sums of three doubles; the first two go through block_pair_to_part's tree exactly (same partial bits as loss_seg.hip's).
__device__ __forceinline__ void block_triple_to_part(double a, double b, double c, double (*sm)[4], double* part) {
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    b += __shfl_xor(b, o);
    c += __shfl_xor(c, o);
  }
  if ((threadIdx.x & 63) == 0) {
    sm[0][threadIdx.x >> 6] = a;
    sm[1][threadIdx.x >> 6] = b;
    sm[2][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 0; q < 3; ++q) part[3 * (long long)blockIdx.x + q] = (sm[q][0] + sm[q][1]) + (sm[q][2] + sm[q][3]);
}

// What one label pixel contributes: the online softmax of seg_loss_pixel_kernel plus, with smoothing, W and sum_c w_c z_c.
struct PixelTerms {
  float lse, zt, wsum, swz;
  int arg;
};
__device__ __forceinline__ PixelTerms pixel_terms(const PixelTaps& tp, int nc, bool vec, long long tg, const float* cw, bool smooth) {
  float zmax = -INFINITY, se = 0.f, zt = 0.f, wsum = 0.f, swz = 0.f;
  int arg = 0;
  each_logit(tp, nc, vec, [&](int c, float z) {
    if (c == (int)tg) zt = z;
    if (z > zmax) {
      se = se * expf(zmax - z) + 1.f;
      zmax = z;
      arg = c;
    } else {
      se += expf(z - zmax);
    }
    if (smooth) {
      const float wc = cw ? cw[c] : 1.f;
      wsum += wc;
      swz = fmaf(wc, z, swz);
    }
  });
  return PixelTerms{zmax + logf(se), zt, wsum, swz, arg};
}
// l of a valid pixel; a = (1 - eps) w_t, s = eps / C
__device__ __forceinline__ float pixel_value(const PixelTerms& q, float a, float s, bool smooth) {
  const float ce = q.lse - q.zt;
  return smooth ? a * ce + s * (q.wsum * q.lse - q.swz) : a * ce;
}

template <bool OHEM>
__global__ __launch_bounds__(256) void seg_opts_pixel_kernel(const float* rows, int ld, int B, int nc, int ih, int iw, int OH, int OW,
                                                             const long long* target, const float* cw, float eps, long long ignore_index,
                                                             float* dlogits, double* part /* per block: sum l, sum w_t, valid pixels */, int* bad,
                                                             float* key, float* lplane) {
  __shared__ double sm[3][4];
  const long long n = (long long)B * OH * OW;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  double my_loss = 0.0, my_w = 0.0, my_cnt = 0.0;
  if (i < n) {
    const int ox = (int)(i % OW);
    long long t = i / OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    const PixelTaps tp(rows, ld, b, ih, iw, OH, OW, oy, ox);
    const long long tg = target[i];
    const bool ignored = tg == ignore_index;
    const bool valid = !ignored && tg >= 0 && tg < nc;
    if (!ignored && !valid) atomicOr(bad, 1);  // torch raises a device assert here
    const bool vec = (ld & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
    const bool smooth = eps > 0.f;
    const PixelTerms q = pixel_terms(tp, nc, vec, tg, cw, smooth);
    const float wt = valid ? (cw ? cw[tg] : 1.f) : 0.f;
    const float a = (1.f - eps) * wt, s = valid ? eps / (float)nc : 0.f;
    float l = 0.f;
    if (valid) {
      l = pixel_value(q, a, s, smooth);
      my_loss = (double)l;
      my_w = (double)wt;
      my_cnt = 1.0;
    }
    if (OHEM) {
      key[i] = valid ? fmaxf(q.lse - q.zt, 0.f) : SEG_KEY_INVALID;
      lplane[i] = l;
    }
    float* dl = dlogits + (long long)b * nc * OH * OW + (long long)oy * OW + ox;
    const float lse = q.lse, wsum = q.wsum;
    each_logit(tp, nc, vec, [&](int c, float z) {
      const float p = expf(z - lse);
      float g = a * (p - (c == (int)tg ? 1.f : 0.f));
      if (smooth) g += s * (wsum * p - (cw ? cw[c] : 1.f));
      dl[(long long)c * OH * OW] = valid ? g : 0.f;
    });
  }
  block_triple_to_part(my_loss, my_w, my_cnt, sm, part);
}

// fixed-order sum of n doubles at stride `stride` by one 256-thread workgroup (every thread returns the total)
__device__ double block_sum_256(const double* v, int n, int stride, double* sh) {
  double a = 0;
  for (int i = threadIdx.x; i < n; i += 256) a += v[(long long)i * stride];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double t = sh[0];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(256) void seg_opts_plan_kernel(const double* part, int nblocks, float theta_t, long long k, SegSelect* sel) {
  __shared__ double sh[256];
  const double nv = block_sum_256(part + 2, nblocks, 3, sh);  // counts: exact in any order
  sel->hist[threadIdx.x] = 0u;
  if (threadIdx.x != 0) return;
  sel->n_valid = (unsigned long long)nv;
  sel->k = (unsigned long long)k;
  sel->all = sel->n_valid < (unsigned long long)k;
  sel->prefix = 0u;
  sel->remaining = sel->all ? 0u : (unsigned)k;
  sel->theta_t_bits = __float_as_uint(theta_t);
  sel->theta_min_bits = 0u;
}

__global__ __launch_bounds__(256) void seg_opts_hist_kernel(const unsigned* key, long long N, int shift, SegSelect* sel) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  if (sel->all) return;  // uniform: nothing to select
  const unsigned prefix = sel->prefix;
  const unsigned hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
    const unsigned kx = key[i];
    if ((kx >> 31) == 0u && (kx & hi_mask) == (prefix & hi_mask)) atomicAdd(&h[(kx >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&sel->hist[threadIdx.x], h[threadIdx.x]);
}

__global__ void seg_opts_pick_kernel(int shift, SegSelect* sel) {  // one thread: the bucket (from the top) that holds the rank still looked for
  if (!sel->all) {
    unsigned rem = sel->remaining;
    int b = 255;
    for (; b > 0; --b) {
      if (sel->hist[b] >= rem) break;
      rem -= sel->hist[b];
    }
    sel->prefix |= (unsigned)b << shift;
    sel->remaining = rem;
  }
  for (int q = 0; q < 256; ++q) sel->hist[q] = 0;
  if (shift == 0) sel->theta_min_bits = sel->all ? 0u : sel->prefix;
}

// (sum l, sum w_t, kept pixels) over the kept pixels: KS_PIX chunks of 256 consecutive pixels per workgroup, a fixed assignment.  A valid
// pixel that is not kept has its nc gradients in dlogits zeroed here (an ignored pixel's are zero already), so the adjoint that follows
// is loss_seg.hip's, unchanged: testing the keys inside the adjoint doubled its loads and its time (0.86 against 0.44 ms at batch 16).
constexpr int KS_PIX = 8;
__global__ __launch_bounds__(256) void seg_opts_kept_sum_kernel(const unsigned* key, const float* lplane, const long long* target, const float* cw,
                                                                long long N, const SegSelect* sel, double* part, float* dlogits, int nc,
                                                                long long plane /* OH * OW */) {
  __shared__ double sm[3][4];
  const unsigned tt = sel->theta_t_bits, tm = sel->theta_min_bits;
  double my_loss = 0.0, my_w = 0.0, my_cnt = 0.0;
  for (int it = 0; it < KS_PIX; ++it) {
    const long long i = ((long long)blockIdx.x * KS_PIX + it) * 256 + threadIdx.x;
    if (i >= N) break;
    const unsigned kx = key[i];
    if (seg_kept(kx, tt, tm)) {  // a kept pixel is valid: its target is a class
      my_loss += (double)lplane[i];
      my_w += (double)(cw ? cw[target[i]] : 1.f);
      my_cnt += 1.0;
    } else if ((kx >> 31) == 0u) {
      float* dl = dlogits + (i / plane) * nc * plane + i % plane;
      for (int c = 0; c < nc; ++c) dl[(long long)c * plane] = 0.f;
    }
  }
  block_triple_to_part(my_loss, my_w, my_cnt, sm, part);
}

// loss = sum l / sum w_t over the partials in index order; acc[0..1] for the adjoint; stats: kept pixels, valid pixels, theta_min, denominator.
__global__ __launch_bounds__(256) void seg_opts_finalize_kernel(const double* part, int nblocks, const SegSelect* sel /* null: no OHEM */, double* acc,
                                                                float* loss, double* stats) {
  __shared__ double s[3][256];
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nblocks; i += 256)
    for (int q = 0; q < 3; ++q) v[q] += part[3 * (long long)i + q];
  for (int q = 0; q < 3; ++q) s[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      for (int q = 0; q < 3; ++q) s[q][threadIdx.x] += s[q][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    acc[0] = s[0][0];
    acc[1] = s[1][0];
    loss[0] = (float)(s[0][0] / s[1][0]);  // an empty set: 0 / 0 = nan, as torch
    stats[0] = s[2][0];
    stats[1] = sel ? (double)sel->n_valid : s[2][0];
    stats[2] = sel && !sel->all ? (double)__uint_as_float(sel->theta_min_bits) : -(double)INFINITY;
    stats[3] = s[1][0];
  }
}

// seg_eval_kernel (loss_seg.hip) with the weighted, smoothed value: part = per block (sum l, sum w_t); the confusion counts are the same code.
template <bool LDS_HIST>
__global__ __launch_bounds__(256) void seg_eval_opts_kernel(const float* rows, int ld, int B, int nc, int ih, int iw, int OH, int OW,
                                                            const long long* target, const float* cw, float eps, long long ignore_index,
                                                            unsigned long long* confusion, double* part) {
  extern __shared__ unsigned int hist[];
  __shared__ double s_sum[4], s_cnt[4];
  if (LDS_HIST) {
    hist_zero<256>(hist, nc);
    __syncthreads();
  }
  const long long n = (long long)B * OH * OW;
  const bool vec = (ld & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
  const bool smooth = eps > 0.f;
  double my_loss = 0.0, my_w = 0.0;
  for (int it = 0; it < EV_PIX; ++it) {
    const long long i = ((long long)blockIdx.x * EV_PIX + it) * 256 + threadIdx.x;
    if (i >= n) break;
    const int ox = (int)(i % OW);
    const long long t = i / OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    const PixelTaps tp(rows, ld, b, ih, iw, OH, OW, oy, ox);
    const long long tg = target[i];
    const bool in_range = tg >= 0 && tg < nc;
    const bool valid = in_range && tg != ignore_index;
    const PixelTerms q = pixel_terms(tp, nc, vec, tg, cw, smooth);
    if (valid) {
      const float wt = cw ? cw[tg] : 1.f;
      my_loss += (double)pixel_value(q, (1.f - eps) * wt, eps / (float)nc, smooth);
      my_w += (double)wt;
    }
    if (in_range) {
      if (LDS_HIST) hist_add(hist, nc, (int)tg, q.arg);
      else atomicAdd(confusion + (int)tg * nc + q.arg, 1ull);
    }
  }
  if (LDS_HIST) hist_flush<256>(hist, nc, confusion);
  block_pair_to_part(my_loss, my_w, s_sum, s_cnt, part);
}

inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }
inline long long pixel_blocks(long long npix) { return cvx_cdiv(npix, 256); }
inline long long kept_sum_blocks(long long npix) { return cvx_cdiv(npix, 256 * KS_PIX); }

}  // namespace

static_assert(sizeof(SegSelect) + 64 <= CVX_SEG_OPTS_KEY_OFFSET, "the totals and the selection state sit in front of the key plane");

extern "C" int64_t cvx_seg_loss_opts_workspace_bytes(int32_t batch, int32_t nc, int32_t oh, int32_t ow, int32_t ohem) {
  // totals and selection state; [key plane, loss plane]; the pixel kernel's and the kept sum's partial triples; the NCHW logit gradients
  const long long npix = (long long)batch * oh * ow;
  int64_t n = CVX_SEG_OPTS_KEY_OFFSET;
  if (ohem) n += 2 * al16((size_t)npix * 4);
  n += al16((size_t)pixel_blocks(npix) * 24) + al16((size_t)kept_sum_blocks(npix) * 24);
  return n + (int64_t)batch * nc * oh * ow * 4;
}

// The chain half of cvx_seg_loss_opts (seg_loss_chain.h): K1 .. K5, which leave the gradient plane and its normaliser on the device.
void seg_opts_chain(const float* rows_f32, int ld, int batch, int nc, int ih, int iw, int oh, int ow, const int64_t* target, const float* class_weight,
                    float label_smoothing, int64_t ignore_index, float ohem_theta, int64_t ohem_min_kept, float* loss_out, int32_t* bad_target,
                    double* stats_out, void* workspace, hipStream_t st, SegChainOut* out) {
  const bool ohem = !(ohem_theta < 0.f);  // -ln thresh >= 0; negative: off
  const long long npix = (long long)batch * oh * ow;
  const long long nblk = pixel_blocks(npix), nks = kept_sum_blocks(npix);
  char* w = (char*)workspace;
  double* acc = (double*)w;
  SegSelect* sel = (SegSelect*)(w + 64);
  w += CVX_SEG_OPTS_KEY_OFFSET;
  float *key = nullptr, *lplane = nullptr;
  if (ohem) {
    key = (float*)w;
    w += al16((size_t)npix * 4);
    lplane = (float*)w;
    w += al16((size_t)npix * 4);
  }
  double* part = (double*)w;
  w += al16((size_t)nblk * 24);
  double* part_kept = (double*)w;
  w += al16((size_t)nks * 24);
  float* dlogits = (float*)w;
  const long long* tg = (const long long*)target;
  if (!ohem) {
    hipLaunchKernelGGL(seg_opts_pixel_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, st, rows_f32, ld, batch, nc, ih, iw, oh, ow, tg, class_weight,
                       label_smoothing, (long long)ignore_index, dlogits, part, bad_target, key, lplane);
    hipLaunchKernelGGL(seg_opts_finalize_kernel, dim3(1), dim3(256), 0, st, part, (int)nblk, (const SegSelect*)nullptr, acc, loss_out, stats_out);
  } else {
    const float theta = ohem_theta == 0.f ? 0.f : ohem_theta;  // -0.0 (thresh = 1) has the sign bit set
    hipLaunchKernelGGL(seg_opts_pixel_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, st, rows_f32, ld, batch, nc, ih, iw, oh, ow, tg, class_weight,
                       label_smoothing, (long long)ignore_index, dlogits, part, bad_target, key, lplane);
    hipLaunchKernelGGL(seg_opts_plan_kernel, dim3(1), dim3(256), 0, st, part, (int)nblk, theta, (long long)ohem_min_kept, sel);
    const int hb = (int)std::min<long long>(512, nblk);
    for (int shift = 24; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(seg_opts_hist_kernel, dim3(hb), dim3(256), 0, st, (const unsigned*)key, npix, shift, sel);
      hipLaunchKernelGGL(seg_opts_pick_kernel, dim3(1), dim3(1), 0, st, shift, sel);
    }
    hipLaunchKernelGGL(seg_opts_kept_sum_kernel, dim3((unsigned)nks), dim3(256), 0, st, (const unsigned*)key, lplane, tg, class_weight, npix, sel,
                       part_kept, dlogits, nc, (long long)oh * ow);
    hipLaunchKernelGGL(seg_opts_finalize_kernel, dim3(1), dim3(256), 0, st, part_kept, (int)nks, (const SegSelect*)sel, acc, loss_out, stats_out);
  }
  *out = SegChainOut{dlogits, acc, 1, 1.0};
}

extern "C" int cvx_seg_loss_opts(const float* rows_f32, int32_t ld, int32_t batch, int32_t nc, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                                 const int64_t* target, const float* class_weight, float label_smoothing, int64_t ignore_index, float ohem_theta,
                                 int64_t ohem_min_kept, float loss_scale, float* loss_out, void* dpred_f16, int32_t* bad_target, double* stats_out,
                                 void* workspace, void* hip_stream) {
  CVX_CHECK(rows_f32 && target && loss_out && dpred_f16 && bad_target && stats_out && workspace, "null arguments");
  CVX_CHECK(batch > 0 && nc > 0 && nc <= SEG_MAX_NC && nc <= ld && ih > 0 && iw > 0 && oh > 0 && ow > 0, "bad sizes");
  CVX_CHECK(label_smoothing >= 0.f && label_smoothing < 1.f, "label_smoothing in [0, 1)");
  CVX_CHECK(loss_scale > 0.f, "loss_scale must be positive");
  const bool ohem = !(ohem_theta < 0.f);  // -ln thresh >= 0; negative: off
  CVX_CHECK(!ohem || (ohem_min_kept >= 1 && isfinite(ohem_theta)), "OHEM: thresh in (0, 1], min_kept >= 1");
  hipStream_t st = (hipStream_t)hip_stream;
  const long long npix = (long long)batch * oh * ow;
  CVX_CHECK(pixel_blocks(npix) < (1LL << 31) && ld <= 4096, "too many pixels / columns");
  CVX_CHECK(!ohem || npix < (1LL << 31), "OHEM counts pixels in 32 bits");
  CVX_HIP(hipMemsetAsync(bad_target, 0, 4, st));
  SegChainOut ch;
  seg_opts_chain(rows_f32, ld, batch, nc, ih, iw, oh, ow, target, class_weight, label_smoothing, ignore_index, ohem_theta, ohem_min_kept, loss_out,
                 bad_target, stats_out, workspace, st, &ch);
  const long long nlow = (long long)batch * ih * iw;
  hipLaunchKernelGGL(resize_grad_rows_kernel, dim3((unsigned)cvx_cdiv(nlow, RG_PIX)), dim3(256), (size_t)RG_PIX * ld * 2, st, ch.dlogits, batch, nc, ih, iw,
                     oh, ow, loss_scale, ch.norm_mode, ch.norm_const, ch.acc, (half_t*)dpred_f16, ld);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_seg_eval_opts(const float* rows_f32, int32_t ld, int32_t batch, int32_t nc, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                                 const int64_t* target, const float* class_weight, float label_smoothing, int64_t ignore_index, int64_t* confusion,
                                 float* loss_out, void* workspace, void* hip_stream) {
  CVX_CHECK(rows_f32 && target && confusion && loss_out && workspace, "null arguments");
  CVX_CHECK(batch > 0 && nc > 0 && nc <= SEG_MAX_NC && nc <= ld && ld <= 4096 && ih > 0 && iw > 0 && oh > 0 && ow > 0, "bad sizes");
  CVX_CHECK(label_smoothing >= 0.f && label_smoothing < 1.f, "label_smoothing in [0, 1)");
  hipStream_t st = (hipStream_t)hip_stream;
  const long long npix = (long long)batch * oh * ow;
  const long long nblk = cvx_cdiv(npix, 256 * EV_PIX);  // cvx_seg_eval's grid: the workspace is cvx_seg_eval_workspace_bytes()
  CVX_CHECK(nblk < (1LL << 31), "too many pixels");
  double* acc = (double*)workspace;
  double* part = (double*)((char*)workspace + 64);
  if (nc * nc <= EV_LDS_CELLS)
    hipLaunchKernelGGL(seg_eval_opts_kernel<true>, dim3((unsigned)nblk), dim3(256), (size_t)nc * nc * 4, st, rows_f32, ld, batch, nc, ih, iw, oh, ow,
                       (const long long*)target, class_weight, label_smoothing, (long long)ignore_index, (unsigned long long*)confusion, part);
  else
    hipLaunchKernelGGL(seg_eval_opts_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, st, rows_f32, ld, batch, nc, ih, iw, oh, ow,
                       (const long long*)target, class_weight, label_smoothing, (long long)ignore_index, (unsigned long long*)confusion, part);
  hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(256), 0, st, part, (int)nblk, acc, 1, 1.0, loss_out);
  CVX_HIP(hipGetLastError());
  return 0;
}
