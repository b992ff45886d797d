// Dice / Tversky / focal-Tversky region losses for the DeepLabv3+ trainer on gfx950, inside the fused criterion chain of loss_seg.hip and
// loss_seg_opts.hip: no (B, nc, H, W) logits or probability tensor beyond the fp32 gradient plane the chain already has, no autograd tape,
// no host read.  Not in the reference (its build_loss knows FocalLoss() and nn.CrossEntropyLoss only).  The rules:
//
//   z_c  bilinearly interpolated logit of class c at a label pixel (PixelTaps), p_c = softmax(z)_c, t the target, y_c = [t == c];
//        valid pixels as in cvx_seg_loss; a group is the whole batch or one image (per_image); every sum runs over a group's valid pixels
//   I_c = sum p_c y_c     P_c = sum p_c     Y_c = sum y_c
//   D_c = (1 - al - be) I_c + al P_c + be Y_c + smooth         T_c = (I_c + smooth) / D_c, 1 when D_c == 0        L_c = (1 - T_c)^gamma
//   m_c = [Y_c > 0] with skip_absent, else 1; v the region class weights (ones when absent)
//   group loss = sum_c m_c v_c L_c / sum_c m_c v_c (0 when that is 0);  region = mean of the group losses over the G groups
//   k_c = (1/G) m_c v_c / sum m v * (-gamma (1 - T_c)^(gamma - 1)), 0 where 1 - T_c <= 0
//   a_c = k_c (D_c - (I_c + smooth)(1 - al - be)) / D_c^2       b_c = -k_c (I_c + smooth) al / D_c^2        g_c = a_c y_c + b_c
//   d region / d z_k = p_k (g_k - sum_c p_c g_c) at a valid pixel, 0 elsewhere
//   loss = base_weight * base + weight * region
//
//   base   the chain half of cvx_seg_loss or cvx_seg_loss_opts (seg_loss_chain.h), kernels untouched: the gradient plane, not yet
//          normalised, and its normaliser stay on the device
//   R1 seg_region_sums    RS_PIX label pixels per thread, a workgroup inside one image: the online softmax, then eight classes at a time
//                         (I, P, Y) summed over the workgroup in a fixed tree -> one triple per class and workgroup, in double
//   R2 seg_region_reduce  the triples of a group in index order (16 interleaved slices, joined in order) -> (G, nc, 3) sums
//   R3 seg_region_solve   one workgroup: T_c, the group losses, a_c, b_c (times weight), region_stats, the combined loss, the base's scale
//   R4 seg_region_grad    one thread per label pixel: the softmax again, with sum_c p_c g_c carried through the same online pass;
//                         base_weight * g_base / normaliser + weight * d region / d z -> the gradient plane (in place with a base)
//   R5 resize_grad_rows_kernel   the unchanged adjoint, norm_mode 0 with norm_const 1
// No floating-point atomics: every sum is a fixed tree per workgroup plus a fixed-order pass, so two calls give the same bits.
#include <math.h>

#include "seg_loss_core.h"
#include "seg_loss_chain.h"
#include "../../include/cvx_engine.h"

namespace {

constexpr int REGION_MAX_NC = 1024;  // the kernels loop over the classes; the bound keeps the one-workgroup solve short
constexpr int RS_PIX = 8;            // R1: label pixels per thread
constexpr int RS_ROW = 256 + 8;      // R1: LDS row stride in floats: rows q and q + 1 start 8 banks apart

struct RegionCfg {
  double alpha, beta, gamma, smooth, weight, base_weight;
  int skip_absent;
};

// lse of the interpolated logits (the online softmax of seg_loss_pixel_kernel)
__device__ __forceinline__ float pixel_lse(const PixelTaps& tp, int nc, bool vec) {
  float zmax = -INFINITY, se = 0.f;
  each_logit(tp, nc, vec, [&](int, float z) {
    if (z > zmax) {
      se = se * expf(zmax - z) + 1.f;
      zmax = z;
    } else {
      se += expf(z - zmax);
    }
  });
  return zmax + logf(se);
}

// Workgroup blk of image b owns the pixels [blk * 256 * RS_PIX, ...) of that image: it never straddles two images, so the partials of an
// image are the bpi consecutive triples b * bpi .. and a group (image or batch) is a contiguous run of them.
__global__ __launch_bounds__(256) void seg_region_sums_kernel(const float* rows, int ld, int nc, int ih, int iw, int OH, int OW,
                                                              const long long* target, long long ignore_index, int bpi,
                                                              double* part /* [workgroup][nc][I, P, Y] */, int* bad) {
  __shared__ float s[24][RS_ROW];
  const int b = blockIdx.x / bpi, blk = blockIdx.x % bpi;
  const long long plane = (long long)OH * OW;
  const bool vec = (ld & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
  float lse[RS_PIX];
  int tgt[RS_PIX];  // -1: not a valid pixel (or past the image's end)
#pragma unroll
  for (int it = 0; it < RS_PIX; ++it) {
    const long long i = ((long long)blk * RS_PIX + it) * 256 + threadIdx.x;
    tgt[it] = -1;
    lse[it] = 0.f;
    if (i < plane) {
      const long long tg = target[(long long)b * plane + i];
      const bool ignored = tg == ignore_index;
      const bool valid = !ignored && tg >= 0 && tg < nc;
      if (!ignored && !valid) atomicOr(bad, 1);
      if (valid) {
        const PixelTaps tp(rows, ld, b, ih, iw, OH, OW, (int)(i / OW), (int)(i % OW));
        lse[it] = pixel_lse(tp, nc, vec);
        tgt[it] = (int)tg;
      }
    }
  }
  for (int c0 = 0; c0 < nc; c0 += 8) {
    float aI[8], aP[8], aY[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) aI[k] = aP[k] = aY[k] = 0.f;
#pragma unroll
    for (int it = 0; it < RS_PIX; ++it) {
      if (tgt[it] < 0) continue;
      const long long i = ((long long)blk * RS_PIX + it) * 256 + threadIdx.x;
      const PixelTaps tp(rows, ld, b, ih, iw, OH, OW, (int)(i / OW), (int)(i % OW));
      float z[8];
      if (vec) {
        tp.logits8(c0, z);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) z[k] = c0 + k < nc ? tp.logit(c0 + k) : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (c0 + k < nc) {
          const float p = expf(z[k] - lse[it]);
          aP[k] += p;
          if (tgt[it] == c0 + k) {
            aI[k] += p;
            aY[k] += 1.f;
          }
        }
      }
    }
    __syncthreads();  // the readers of the previous eight classes are done
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s[k][threadIdx.x] = aI[k];
      s[8 + k][threadIdx.x] = aP[k];
      s[16 + k][threadIdx.x] = aY[k];
    }
    __syncthreads();
    if (threadIdx.x < 192) {  // three whole waves: 24 quantities x 8 lanes, each lane 32 threads' values in index order, then a fixed tree
      const int q = threadIdx.x >> 3, j = threadIdx.x & 7;
      double a = 0.0;
      for (int i = 0; i < 32; ++i) a += (double)s[q][i * 8 + j];
      a += __shfl_xor(a, 4);
      a += __shfl_xor(a, 2);
      a += __shfl_xor(a, 1);
      const int c = c0 + (q & 7);
      if (j == 0 && c < nc) part[((long long)blockIdx.x * nc + c) * 3 + (q >> 3)] = a;
    }
  }
}

// sums[g][e] = the group's partials part[(g * ppg + p) * E + e], p = 0 .. ppg - 1: slice sl takes p = sl, sl + 16, ... in order, the 16 slices
// are then added in order.  E = 3 * nc.  grid (cdiv(E, 16), G).
__global__ __launch_bounds__(256) void seg_region_reduce_kernel(const double* part, int ppg, int E, double* sums) {
  __shared__ double s[16][17];
  const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el, g = blockIdx.y;
  double a = 0.0;
  if (e < E)
    for (int p = sl; p < ppg; p += 16) a += part[((long long)g * ppg + p) * E + e];
  s[sl][el] = a;
  __syncthreads();
  if (sl == 0 && e < E) {
    double t = 0.0;
    for (int q = 0; q < 16; ++q) t += s[q][el];
    sums[(long long)g * E + e] = t;
  }
}

// fixed-tree sums of two per-thread values over the 256 threads; every thread gets both totals
__device__ __forceinline__ void block_sum2_256(double& a, double& b, double* s0, double* s1) {
  s0[threadIdx.x] = a;
  s1[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      s0[threadIdx.x] += s0[threadIdx.x + o];
      s1[threadIdx.x] += s1[threadIdx.x + o];
    }
    __syncthreads();
  }
  a = s0[0];
  b = s1[0];
  __syncthreads();
}

struct ClassTerms {
  double I, P, Y, D, T, L, w;  // w = m_c v_c
};
__device__ __forceinline__ ClassTerms class_terms(const double* sums, int c, const RegionCfg& cfg, const float* v) {
  ClassTerms t;
  t.I = sums[3 * c];
  t.P = sums[3 * c + 1];
  t.Y = sums[3 * c + 2];
  t.D = (1.0 - cfg.alpha - cfg.beta) * t.I + cfg.alpha * t.P + cfg.beta * t.Y + cfg.smooth;
  t.T = t.D == 0.0 ? 1.0 : (t.I + cfg.smooth) / t.D;
  const double om = 1.0 - t.T;
  t.L = om > 0.0 ? pow(om, cfg.gamma) : 0.0;
  t.w = (cfg.skip_absent && !(t.Y > 0.0)) ? 0.0 : (v ? (double)v[c] : 1.0);
  return t;
}

// base_loss: the base's value (null: no base term); base_acc / norm_mode / norm_const: its gradient's normaliser (SegChainOut), used
// when hdr is not null (training).  coef: (G, nc, 2) floats = weight * (a_c, b_c); hdr[0] = base_weight / normaliser.
__global__ __launch_bounds__(256) void seg_region_solve_kernel(const double* sums, int G, int nc, RegionCfg cfg, const float* v, const float* base_loss,
                                                               const double* base_acc, int norm_mode, double norm_const, float* coef, float* hdr,
                                                               double* stats /* (G, nc, 4): I, P, Y, T */, float* loss_out) {
  __shared__ double s0[256], s1[256];
  double total = 0.0;
  for (int g = 0; g < G; ++g) {
    const double* sg = sums + (long long)g * 3 * nc;
    double mv = 0.0, mvl = 0.0;
    for (int c = threadIdx.x; c < nc; c += 256) {
      const ClassTerms t = class_terms(sg, c, cfg, v);
      mv += t.w;
      mvl += t.w * t.L;
    }
    block_sum2_256(mv, mvl, s0, s1);
    total += mv > 0.0 ? mvl / mv : 0.0;
    for (int c = threadIdx.x; c < nc; c += 256) {
      const ClassTerms t = class_terms(sg, c, cfg, v);
      const double om = 1.0 - t.T;
      double a = 0.0, b = 0.0;
      if (mv > 0.0 && om > 0.0 && t.D != 0.0) {
        const double k = (1.0 / (double)G) * (t.w / mv) * (-cfg.gamma * pow(om, cfg.gamma - 1.0));
        a = k * (t.D - (t.I + cfg.smooth) * (1.0 - cfg.alpha - cfg.beta)) / (t.D * t.D);
        b = -k * (t.I + cfg.smooth) * cfg.alpha / (t.D * t.D);
      }
      const long long o = (long long)g * nc + c;
      if (coef) {
        coef[2 * o] = (float)(cfg.weight * a);
        coef[2 * o + 1] = (float)(cfg.weight * b);
      }
      stats[4 * o] = t.I;
      stats[4 * o + 1] = t.P;
      stats[4 * o + 2] = t.Y;
      stats[4 * o + 3] = t.T;
    }
  }
  if (threadIdx.x == 0) {
    const double region = total / (double)G;
    loss_out[0] = base_loss ? (float)(cfg.base_weight * (double)base_loss[0] + cfg.weight * region) : (float)(cfg.weight * region);
    if (hdr) {
      const double denom = norm_mode == 0 ? norm_const : (base_acc && base_acc[1] > 0.0 ? base_acc[1] : 1.0);
      hdr[0] = (float)(cfg.base_weight / denom);
    }
  }
}

// One thread per label pixel, as the base chains' pixel kernels (a wave writes a class plane along x).  With g_c = a_c [t == c] + b_c,
// sum_c p_c g_c = (sum_c e_c g_c) / (sum_c e_c) rides the online softmax's rescaling.
__global__ __launch_bounds__(256) void seg_region_grad_kernel(const float* rows, int ld, int B, int nc, int ih, int iw, int OH, int OW,
                                                              const long long* target, long long ignore_index, const float* coef, int per_image,
                                                              const float* hdr, int has_base, float* dlogits) {
  const long long plane = (long long)OH * OW;
  const long long n = (long long)B * plane;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ox = (int)(i % OW);
  const long long t = i / OW;
  const int oy = (int)(t % OH);
  const int b = (int)(t / OH);
  const long long tg = target[i];
  const bool valid = tg != ignore_index && tg >= 0 && tg < nc;
  float* dl = dlogits + (long long)b * nc * plane + (long long)oy * OW + ox;
  if (!valid) {  // with a base the plane holds the base's zero here already
    if (!has_base)
      for (int c = 0; c < nc; ++c) dl[(long long)c * plane] = 0.f;
    return;
  }
  const float* cf = coef + (long long)(per_image ? b : 0) * nc * 2;
  const PixelTaps tp(rows, ld, b, ih, iw, OH, OW, oy, ox);
  const bool vec = (ld & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
  float zmax = -INFINITY, se = 0.f, sg = 0.f;
  each_logit(tp, nc, vec, [&](int c, float z) {
    const float g = cf[2 * c + 1] + (c == (int)tg ? cf[2 * c] : 0.f);
    if (z > zmax) {
      const float r = expf(zmax - z);
      se = se * r + 1.f;
      sg = sg * r + g;
      zmax = z;
    } else {
      const float e = expf(z - zmax);
      se += e;
      sg = fmaf(e, g, sg);
    }
  });
  const float lse = zmax + logf(se), S = sg / se;
  const float sb = has_base ? hdr[0] : 0.f;
  auto term = [&](int c, float z) {
    const float g = cf[2 * c + 1] + (c == (int)tg ? cf[2 * c] : 0.f);
    return expf(z - lse) * (g - S);
  };
  if (vec) {  // eight classes at a time: the base's eight gradients are loaded together, ahead of the eight stores
    for (int c0 = 0; c0 < nc; c0 += 8) {
      float z[8], old[8];
      tp.logits8(c0, z);
#pragma unroll
      for (int k = 0; k < 8; ++k) old[k] = has_base && c0 + k < nc ? dl[(long long)(c0 + k) * plane] : 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c0 + k < nc) dl[(long long)(c0 + k) * plane] = fmaf(sb, old[k], term(c0 + k, z[k]));
    }
  } else {
    for (int c = 0; c < nc; ++c) {
      float* o = dl + (long long)c * plane;
      *o = fmaf(sb, has_base ? *o : 0.f, term(c, tp.logit(c)));
    }
  }
}

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int region_bpi(int oh, int ow) { return cvx_cdiv((long long)oh * ow, 256 * RS_PIX); }

struct RegionLayout {
  size_t sums, coef, part, rest, total;
};
inline RegionLayout region_layout(int batch, int nc, int oh, int ow, int base, int ohem, int per_image, int value_only) {
  const size_t G = per_image ? (size_t)batch : 1, nparts = (size_t)batch * region_bpi(oh, ow);
  RegionLayout l;
  l.sums = 256;  // the header: hdr[0] the base's scale, hdr[1] the base's value
  l.coef = l.sums + al256(G * 3 * nc * 8);
  l.part = l.coef + al256(G * 2 * nc * 4);
  l.rest = l.part + al256(nparts * 3 * nc * 8);
  size_t rest = 0;  // the base chain's whole workspace (its last part is the gradient plane), or the plane alone
  if (!value_only)
    rest = base == 0   ? (size_t)batch * nc * oh * ow * 4
           : base == 3 ? (size_t)cvx_seg_loss_opts_workspace_bytes(batch, nc, oh, ow, ohem)
                       : (size_t)cvx_seg_loss_workspace_bytes(batch, nc, oh, ow);
  l.total = l.rest + rest;
  return l;
}

}  // namespace

extern "C" int64_t cvx_seg_loss_region_workspace_bytes(int32_t batch, int32_t nc, int32_t oh, int32_t ow, int32_t base, int32_t ohem, int32_t per_image,
                                                       int32_t value_only) {
  return (int64_t)region_layout(batch, nc, oh, ow, base, ohem, per_image, value_only).total;
}

extern "C" int cvx_seg_loss_region(const float* rows_f32, int32_t ld, int32_t batch, int32_t nc, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                                   const int64_t* target, int32_t base, float focal_alpha, float focal_gamma, const float* class_weight,
                                   float label_smoothing, int64_t ignore_index, float ohem_theta, int64_t ohem_min_kept, double base_weight, double weight,
                                   double alpha, double beta, double gamma, double smooth, int32_t per_image, int32_t skip_absent,
                                   const float* region_class_weight, float loss_scale, const float* base_value, float* loss_out, void* dpred_f16,
                                   int32_t* bad_target, double* base_stats_out, double* region_stats_out, void* workspace, void* hip_stream) {
  CVX_CHECK(rows_f32 && target && loss_out && bad_target && region_stats_out && workspace, "null arguments");
  CVX_CHECK(batch > 0 && nc > 0 && nc <= ld && ld <= 4096 && ih > 0 && iw > 0 && oh > 0 && ow > 0, "bad sizes");
  CVX_CHECK(nc <= REGION_MAX_NC, "the region losses take at most 1024 classes");
  CVX_CHECK(base >= 0 && base <= 3, "base: 0 none, 1 focal, 2 cross-entropy, 3 cross-entropy with options");
  CVX_CHECK(isfinite(weight) && weight > 0.0 && isfinite(base_weight) && base_weight >= 0.0, "weight > 0, base_weight >= 0");
  CVX_CHECK(isfinite(alpha) && alpha >= 0.0 && isfinite(beta) && beta >= 0.0 && isfinite(gamma) && gamma > 0.0 && isfinite(smooth) && smooth >= 0.0,
            "alpha, beta, smooth >= 0 and gamma > 0");
  const bool value_only = dpred_f16 == nullptr;
  const bool ohem = base == 3 && !(ohem_theta < 0.f);
  if (!value_only) {
    CVX_CHECK(loss_scale > 0.f, "loss_scale must be positive");
    CVX_CHECK((base != 0) == (base_weight > 0.0), "a base term needs base_weight > 0, and base_weight = 0 takes base = 0");
    CVX_CHECK(base != 3 || (base_stats_out && label_smoothing >= 0.f && label_smoothing < 1.f), "options: stats and label_smoothing in [0, 1)");
    CVX_CHECK(!ohem || (ohem_min_kept >= 1 && isfinite(ohem_theta)), "OHEM: thresh in (0, 1], min_kept >= 1");
  }
  hipStream_t st = (hipStream_t)hip_stream;
  const long long plane = (long long)oh * ow, npix = (long long)batch * plane;
  const int bpi = region_bpi(oh, ow);
  const long long nparts = (long long)batch * bpi;
  CVX_CHECK((npix + 255) / 256 < (1LL << 31) && nparts < (1LL << 31), "too many pixels");
  CVX_CHECK(!ohem || npix < (1LL << 31), "OHEM counts pixels in 32 bits");
  const int G = per_image ? batch : 1, ppg = per_image ? bpi : (int)nparts, E = 3 * nc;
  const RegionLayout lay = region_layout(batch, nc, oh, ow, value_only ? 0 : base, ohem, per_image, value_only);
  char* w = (char*)workspace;
  float* hdr = (float*)w;
  double* sums = (double*)(w + lay.sums);
  float* coef = (float*)(w + lay.coef);
  double* part = (double*)(w + lay.part);
  const RegionCfg cfg{alpha, beta, gamma, smooth, weight, base_weight, skip_absent != 0};
  const long long* tg = (const long long*)target;
  CVX_HIP(hipMemsetAsync(bad_target, 0, 4, st));
  SegChainOut ch{(float*)(w + lay.rest), nullptr, 0, 1.0};
  const float* base_loss = value_only ? base_value : nullptr;
  if (!value_only && base != 0) {
    if (base == 3)
      seg_opts_chain(rows_f32, ld, batch, nc, ih, iw, oh, ow, target, class_weight, label_smoothing, ignore_index, ohem_theta, ohem_min_kept, hdr + 1,
                     bad_target, base_stats_out, w + lay.rest, st, &ch);
    else
      seg_plain_chain(rows_f32, ld, batch, nc, ih, iw, oh, ow, target, base == 1 ? 0 : 1, focal_alpha, focal_gamma, ignore_index, hdr + 1, bad_target,
                      w + lay.rest, st, &ch);
    base_loss = hdr + 1;
  }
  hipLaunchKernelGGL(seg_region_sums_kernel, dim3((unsigned)nparts), dim3(256), 0, st, rows_f32, ld, nc, ih, iw, oh, ow, tg, (long long)ignore_index, bpi,
                     part, bad_target);
  hipLaunchKernelGGL(seg_region_reduce_kernel, dim3((unsigned)cvx_cdiv(E, 16), (unsigned)G), dim3(256), 0, st, part, ppg, E, sums);
  hipLaunchKernelGGL(seg_region_solve_kernel, dim3(1), dim3(256), 0, st, sums, G, nc, cfg, region_class_weight, base_loss, ch.acc, ch.norm_mode,
                     ch.norm_const, value_only ? nullptr : coef, value_only ? nullptr : hdr, region_stats_out, loss_out);
  if (!value_only) {
    hipLaunchKernelGGL(seg_region_grad_kernel, dim3((unsigned)cvx_cdiv(npix, 256)), dim3(256), 0, st, rows_f32, ld, batch, nc, ih, iw, oh, ow, tg,
                       (long long)ignore_index, coef, per_image, hdr, base != 0, ch.dlogits);
    const long long nlow = (long long)batch * ih * iw;
    hipLaunchKernelGGL(resize_grad_rows_kernel, dim3((unsigned)cvx_cdiv(nlow, RG_PIX)), dim3(256), (size_t)RG_PIX * ld * 2, st, ch.dlogits, batch, nc, ih, iw,
                       oh, ow, loss_scale, 0, 1.0, (const double*)nullptr, (half_t*)dpred_f16, ld);
  }
  CVX_HIP(hipGetLastError());
  return 0;
}
