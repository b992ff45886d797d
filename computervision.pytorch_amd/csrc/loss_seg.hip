// The fused segmentation criterion of the DeepLabv3+ trainer on gfx950 (cvx_seg_criterion_loss / cvx_seg_criterion_eval): bilinear
// upsampling of the decoder's logits to the label resolution, the loss per pixel, and the gradient w.r.t. the LOW-RESOLUTION logits rows
// the engine's backward pass starts from -- value and gradient in one launch chain, no autograd tape, no (B, nc, H, W) logits tensor in
// HBM, no host read.  One criterion = a base term (none / focal / cross-entropy, the latter with options) plus an optional
// region term (Dice / Tversky, or Lovasz-Softmax -- the one term that sorts):   loss = base_weight * base + weight * region   (base alone: loss = base).
//
// Reference semantics (file:line under the reference tree):
//   DeeplabV3Plus.forward        core/models/deeplabv3plus.py:143-148   x = F.interpolate(classifier(features), size=input, bilinear,
//                                                                       align_corners=False)
//   FocalLoss.forward            core/loss/focal_loss.py:14-22          ce = F.cross_entropy(x, t, ignore_index, reduction="none");
//                                                                       pt = exp(-ce); loss = alpha * (1 - pt)^gamma * ce; mean()
//   DeeplabV3PlusA.build_loss    core/algorithms/segmentation_2d.py:59-64  "focal" -> FocalLoss() (alpha 0.25, gamma 2, ignore -100),
//                                                                       "ce" -> nn.CrossEntropyLoss(reduction="mean")
//   train_loop / evaluate_loop   core/trainer/segmentation_trainer.py:114-131, 133-159
// The options and the region term are not in the reference; their definitions are torch's (F.cross_entropy(weight=, label_smoothing=))
// and the usual one-hot Dice / Tversky loss.
//
// Base.  z_c the bilinearly interpolated logit of class c at a label pixel (PixelTaps), lse its log-sum-exp, t the target, p = softmax(z);
// valid pixels: t != ignore_index and 0 <= t < nc (another t that is not ignore_index raises the bad-label flag and is skipped).
//   Focal      alpha (1 - pt)^gamma ce, ce = lse - z_t, pt = exp(-ce); mean over ALL pixels (ignored ones count in the denominator)
//   Ce<false>  ce; mean over the valid pixels
//   Ce<true>   w the class weights (ones when absent), W = sum_c w_c, eps the smoothing, C = nc
//              l = (1 - eps) w_t ce + (eps / C) (W lse - sum_c w_c z_c);  loss = sum_{i in S} l_i / sum_{i in S} w_{t_i}
//              dl/dz_k = (1 - eps) w_t (p_k - [k == t]) + (eps / C) (W p_k - w_k);  S: the valid pixels, or the kept ones under OHEM
// The three are compile-time policies of one pixel kernel and one evaluation kernel: Ce<false> loads no weight and carries no W.
// OHEM: key = fp32 max(ce, 0), K = min_kept * batch, theta_t = -ln thresh, theta_min = the K-th largest key among the valid pixels (below
// every key when there are fewer than K).  A pixel is kept iff key > theta_t or key >= theta_min: ties at theta_min are all kept, so there
// is no tie order.  theta_min comes from an 8-bit radix select over the keys' bit patterns (non-negative floats order as uint32).
//
//   K1 seg_pixel        one thread per label pixel: the class loop twice (online softmax, then the gradient); the per-pixel gradient, not
//                       yet normalised -> dlogits (B, nc, OH, OW) fp32; block partials (sum l, sum w_t[, valid pixels]); under OHEM also the
//                       key plane and the per-pixel loss plane
//   with OHEM  K2 plan, K3 hist / pick (x4, integer atomics only), K4 kept_sum (fixed-order partials over the kept pixels; zeroes the
//              gradients of the valid pixels that are not kept)
//   K5 finalize         loss = sum / normaliser; the four stats of Ce<true>
//   K6 resize_grad_rows adjoint of the bilinear resize as a gather (deterministic) -> dpred (B, ih*iw, ld) fp16
//   launches: 3 (no OHEM), 13 (OHEM)
//
// Region (Dice / Tversky / focal Tversky).  A group is the whole batch or one image (per_image); every sum runs over a group's valid pixels,
// y_c = [t == c]:
//   I_c = sum p_c y_c     P_c = sum p_c     Y_c = sum y_c
//   D_c = (1 - al - be) I_c + al P_c + be Y_c + smooth         T_c = (I_c + smooth) / D_c, 1 when D_c == 0        L_c = (1 - T_c)^gamma
//   m_c = [Y_c > 0] with skip_absent, else 1; v the region class weights (ones when absent)
//   group loss = sum_c m_c v_c L_c / sum_c m_c v_c (0 when that is 0);  region = mean of the group losses over the G groups
//   k_c = (1/G) m_c v_c / sum m v * (-gamma (1 - T_c)^(gamma - 1)), 0 where 1 - T_c <= 0
//   a_c = k_c (D_c - (I_c + smooth)(1 - al - be)) / D_c^2       b_c = -k_c (I_c + smooth) al / D_c^2        g_c = a_c y_c + b_c
//   d region / d z_k = p_k (g_k - sum_c p_c g_c) at a valid pixel, 0 elsewhere
//
//   the base's K1 .. K5 (none with base 0): the gradient plane, not yet normalised, and its normaliser stay on the device
//   R1 seg_region_sums    RS_PIX label pixels per thread, a workgroup inside one image: the online softmax, then eight classes at a time
//                         (I, P, Y) summed over the workgroup in a fixed tree -> one triple per class and workgroup, in double
//   R2 seg_region_reduce  the triples of a group in index order (16 interleaved slices, joined in order) -> (G, nc, 3) sums
//   R3 seg_region_solve   one workgroup: T_c, the group losses, a_c, b_c (times weight), region_stats, the combined loss, the base's scale
//   R4 seg_region_grad    one thread per label pixel: the softmax again, with sum_c p_c g_c carried through the same online pass;
//                         base_weight * g_base / normaliser + weight * d region / d z -> the gradient plane (in place with a base)
//   K6 the adjoint, with scale 1
//   launches: 5 (region alone), 7 (plain base + region)
//
// Lovasz-Softmax (region 2; the rules are the header's).  Per group and class the errors e = [t == c] ? 1 - p_c : p_c of the valid pixels,
// sorted descending with ties by ascending pixel index, weighted by the increments of the Jaccard loss along that order:
//   the base's K1 .. K5 as above
//   L1 count, L2 offsets  the valid pixels per block of 1024 and their exclusive offsets per group: invalid pixels never enter a segment
//   L3 keys               online softmax, then eight classes at a time: the fp32 bits of e and (pixel index | flag << 31) into segment
//                         (group, class) at the pixel's compacted place; G_c by integer atomics
//   L4 plan               coef = weight (1/G) m_c v_c / sum m v, the segment table of the sorted view
//   L5 sort               lovasz_sort.h: four stable 8-bit passes of histogram / scan / scatter, ranks from ballots and counts
//   L6 flagsum, L7 flagscan, L8 value   integer prefix counts of the flags, Delta from the closed form in double, sum e Delta in
//                         fixed-order partials; in training coef * s * Delta scattered to a plane laid out like the gradient plane
//   L9 reduce, solve      L_c, the stats, the combined loss, the base's scale
//   L10 seg_lovasz_grad   R4 with h_c read from the plane;   K6 the adjoint, with scale 1
//   launches: 22 and a memset for the term; evaluation stops after L9 with a one-byte payload (21)
//
// Evaluation: seg_eval_kernel walks the label pixels the same way -- the same taps, the same online softmax, the same policies -- and
// keeps the arg max instead of a gradient: confusion[target][argmax] += 1 and the batch's base value (K5 finishes its sum); then R1 .. R3
// for a region term.  OHEM is a training device and is never applied here.  The LDS histogram is seg_tail.h's.
//
// No floating-point atomics: every sum is a fixed tree per workgroup plus one fixed-order pass over the partials, so two calls give the
// same bits.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "cvx_common.h"
#include "lovasz_sort.h"
#include "seg_tail.h"
#include "../../include/cvx_engine.h"

static_assert(sizeof(cvx_seg_dims) == CVX_SEG_DIMS_BYTES && sizeof(cvx_seg_criterion) == CVX_SEG_CRITERION_BYTES,
              "the ctypes mirrors of the two structs are checked against these sizes");

namespace {

constexpr int SEG_MAX_NC = 4096;     // sanity bound only: the kernels loop over the classes
constexpr int REGION_MAX_NC = 1024;  // the bound keeps the one-workgroup solve short
constexpr int EV_PIX = 8, EV_LDS_CELLS = 8192;  // seg_eval_kernel: label pixels per thread, and the LDS histogram's cells (nc <= 90)
constexpr int KS_PIX = 8;            // K4: chunks of 256 consecutive pixels per workgroup
constexpr int RS_PIX = 8;            // R1: label pixels per thread
constexpr int RS_ROW = 256 + 8;      // R1: LDS row stride in floats: rows q and q + 1 start 8 banks apart
constexpr int RG_PIX = 32;           // K6: source pixels per workgroup

// ---- one label pixel -----------------------------------------------------------------------------------------------------------------------

// The four source rows of one label pixel and its weights; logit(c) is the value cvx_resize_bilinear_rows_to_nchw writes for class c
// there (bilinear_src / bilinear_mix, bilinear.h).
struct PixelTaps {
  const float *r00, *r01, *r10, *r11;
  float lx, ly;
  __device__ __forceinline__ PixelTaps(const float* rows, const cvx_seg_dims& d, int b, int oy, int ox) {
    int y0, y1, x0, x1;
    bilinear_src(oy, (float)d.ih / (float)d.oh, d.ih, &y0, &y1, &ly);
    bilinear_src(ox, (float)d.iw / (float)d.ow, d.iw, &x0, &x1, &lx);
    const float* base = rows + (long long)b * d.ih * d.iw * d.ld;
    r00 = base + ((long long)y0 * d.iw + x0) * d.ld;
    r01 = base + ((long long)y0 * d.iw + x1) * d.ld;
    r10 = base + ((long long)y1 * d.iw + x0) * d.ld;
    r11 = base + ((long long)y1 * d.iw + x1) * d.ld;
  }
  // The same taps with the two weights taken from a source coordinate formed in double (sy = ih / oh, sx = iw / ow as doubles): the
  // fp32 coordinate of bilinear_src is a number of magnitude up to ih, so its weight carries half an ulp of THAT -- 5e-7 at 8 .. 16 --
  // which a difference of 6 between neighbouring logits turns into 3e-6 on the logit.  Only the Lovasz keys, which are held to 1e-6 of
  // float64, take their logits this way; everything else keeps the values cvx_resize_bilinear_rows_to_nchw writes.
  __device__ __forceinline__ PixelTaps(const float* rows, const cvx_seg_dims& d, int b, int oy, int ox, double sy, double sx) {
    int y0, y1, x0, x1;
    src_f64(oy, sy, d.ih, &y0, &y1, &ly);
    src_f64(ox, sx, d.iw, &x0, &x1, &lx);
    const float* base = rows + (long long)b * d.ih * d.iw * d.ld;
    r00 = base + ((long long)y0 * d.iw + x0) * d.ld;
    r01 = base + ((long long)y0 * d.iw + x1) * d.ld;
    r10 = base + ((long long)y1 * d.iw + x0) * d.ld;
    r11 = base + ((long long)y1 * d.iw + x1) * d.ld;
  }
  static __device__ __forceinline__ void src_f64(int o, double scale, int in_size, int* i0, int* i1, float* lam) {
    double s = ((double)o + 0.5) * scale - 0.5;
    if (s < 0.0) s = 0.0;
    int a = (int)s;
    if (a > in_size - 1) a = in_size - 1;
    *i0 = a;
    *i1 = a + (a < in_size - 1 ? 1 : 0);
    *lam = (float)(s - (double)a);
  }
  __device__ __forceinline__ float logit(int c) const { return bilinear_mix(r00[c], r01[c], r10[c], r11[c], lx, ly); }
  // eight classes at a time with 16-byte loads issued together (rows with ld % 8 == 0 on a 16-byte boundary)
  __device__ __forceinline__ void logits8(int c0, float* z) const {
    float a[8], bq[8], cq[8], d[8];
    *reinterpret_cast<float4*>(a) = *reinterpret_cast<const float4*>(r00 + c0);
    *reinterpret_cast<float4*>(a + 4) = *reinterpret_cast<const float4*>(r00 + c0 + 4);
    *reinterpret_cast<float4*>(bq) = *reinterpret_cast<const float4*>(r01 + c0);
    *reinterpret_cast<float4*>(bq + 4) = *reinterpret_cast<const float4*>(r01 + c0 + 4);
    *reinterpret_cast<float4*>(cq) = *reinterpret_cast<const float4*>(r10 + c0);
    *reinterpret_cast<float4*>(cq + 4) = *reinterpret_cast<const float4*>(r10 + c0 + 4);
    *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(r11 + c0);
    *reinterpret_cast<float4*>(d + 4) = *reinterpret_cast<const float4*>(r11 + c0 + 4);
#pragma unroll
    for (int k = 0; k < 8; ++k) z[k] = bilinear_mix(a[k], bq[k], cq[k], d[k], lx, ly);
  }
};

__device__ __forceinline__ bool rows_vec(const float* rows, int ld) { return (ld & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0; }

// f(c, logit) for every class in order.  Rows with ld % 8 == 0 (the engine's: 16-byte aligned, padded to 8 columns) take logits8; a class
// loop of scalar loads waits for memory 4 * nc times per pass.
template <class F>
__device__ __forceinline__ void each_logit(const PixelTaps& tp, int nc, bool vec, F f) {
  if (vec) {
    for (int c0 = 0; c0 < nc; c0 += 8) {
      float z[8];
      tp.logits8(c0, z);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c0 + k < nc) f(c0 + k, z[k]);
    }
  } else {
    for (int c = 0; c < nc; ++c) f(c, tp.logit(c));
  }
}

// Where a label pixel is and what its target is worth, under the one rule: in_range 0 <= t < nc (it counts in the confusion matrix);
// valid: in_range and not ignore_index (it counts in the criterion); neither in range nor ignore_index: the bad-label flag (torch raises
// a device assert there), unless bad is null.
struct SegPixel {
  int b, oy, ox;
  long long tg;
  bool valid, in_range;
  // i: the pixel's index in (b, oy, ox) order
  __device__ __forceinline__ SegPixel(long long i, const cvx_seg_dims& d, const long long* target, long long ignore_index, int* bad) {
    ox = (int)(i % d.ow);
    const long long t = i / d.ow;
    oy = (int)(t % d.oh);
    b = (int)(t / d.oh);
    classify(target[i], d.nc, ignore_index, bad);
  }
  // in_image: the pixel's index inside image b
  __device__ __forceinline__ SegPixel(int b_, long long in_image, const cvx_seg_dims& d, const long long* target, long long ignore_index, int* bad)
      : b(b_), oy((int)(in_image / d.ow)), ox((int)(in_image % d.ow)) {
    classify(target[(long long)b_ * d.oh * d.ow + in_image], d.nc, ignore_index, bad);
  }

 private:
  __device__ __forceinline__ void classify(long long t, int nc, long long ignore_index, int* bad) {
    tg = t;
    in_range = t >= 0 && t < nc;
    valid = in_range && t != ignore_index;
    if (bad && !in_range && t != ignore_index) atomicOr(bad, 1);
  }
};

// The online softmax over the classes (no per-thread array: the class count is a run-time value): running maximum and rescaled sum of
// exponentials.  arg: strict >, so the lowest class wins a tie, like torch.argmax.  g(c, z) is evaluated once per class, ahead of the
// branch (so its loads are issued with the logits'), and its values ride the same rescaling: sg / se = sum_c p_c g_c.
struct Softmax {
  float lse, zt, se, sg;
  int arg;
};
template <class G>
__device__ __forceinline__ Softmax online_softmax(const PixelTaps& tp, int nc, bool vec, int tg, G g) {
  float zmax = -INFINITY, se = 0.f, sg = 0.f, zt = 0.f;
  int arg = 0;
  each_logit(tp, nc, vec, [&](int c, float z) {
    const float gc = g(c, z);
    if (c == tg) zt = z;
    if (z > zmax) {
      const float r = expf(zmax - z);
      se = se * r + 1.f;
      sg = sg * r + gc;
      zmax = z;
      arg = c;
    } else {
      const float e = expf(z - zmax);
      se += e;
      sg = fmaf(e, gc, sg);
    }
  });
  return Softmax{zmax + logf(se), zt, se, sg, arg};
}

// ---- fixed-order sums ----------------------------------------------------------------------------------------------------------------------

// N per-thread doubles summed over the workgroup in a fixed tree (shfl_xor 32..1, then the four waves as (w0 + w1) + (w2 + w3)): one
// record of N per workgroup, summed in index order by partials_sum_256 (deterministic, no same-address atomics).
template <int N>
__device__ __forceinline__ void block_to_part(double (&v)[N], double (*sm)[4], double* part) {
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] += __shfl_xor(v[q], o);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) sm[q][threadIdx.x >> 6] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) part[N * (long long)blockIdx.x + q] = (sm[q][0] + sm[q][1]) + (sm[q][2] + sm[q][3]);
  }
}

// N per-thread doubles summed over the 256 threads by the 128..1 LDS tree; every thread gets the totals.
template <int N>
__device__ __forceinline__ void block_tree_256(double (&v)[N], double (*sh)[256]) {
#pragma unroll
  for (int q = 0; q < N; ++q) sh[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int q = 0; q < N; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = sh[q][0];
  __syncthreads();
}

// The first N doubles of n records of `stride` doubles, by one 256-thread workgroup: thread j takes records j, j + 256, ... in order, then the tree.
template <int N>
__device__ __forceinline__ void partials_sum_256(const double* part, int n, int stride, double (&v)[N], double (*sh)[256]) {
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] += part[(long long)i * stride + q];
  }
  block_tree_256<N>(v, sh);
}

// ---- the base term's per-pixel policies -------------------------------------------------------------------------------------------------------
// Sums / accumulate: what rides the online softmax pass; terms(): value and weight of a VALID pixel plus what grad() needs;
// grad(): d value / d z_c from p_c.  NPART: the pixel kernel's partials per workgroup -- (sum value, sum weight[, valid pixels]).

struct NoSums {};

struct Focal {
  float alpha, gamma;
  static constexpr int NPART = 2;
  static constexpr int NORM_MODE = 0;  // the mean runs over all pixels
  using Sums = NoSums;
  struct Terms {
    float value, weight, coef;  // coef: d value / d ce
  };
  __device__ __forceinline__ void accumulate(Sums&, int, float) const {}
  __device__ __forceinline__ Terms terms(const Softmax& q, const Sums&, long long, int) const {
    const float ce = q.lse - q.zt;
    const float pt = expf(-ce);
    const float om = fmaxf(1.f - pt, 0.f);
    const float w = powf(om, gamma);
    // d/dce [alpha (1 - pt)^gamma ce], d pt / d ce = -pt
    return Terms{alpha * w * ce, 1.f, alpha * (w + (gamma > 0.f ? gamma * powf(om, gamma - 1.f) * pt * ce : 0.f))};
  }
  __device__ __forceinline__ float grad(const Terms& t, const Sums&, float p, int, bool target) const { return t.coef * (p - (target ? 1.f : 0.f)); }
};

template <bool OPTS>
struct Ce;

template <>
struct Ce<false> {
  static constexpr int NPART = 2;
  static constexpr int NORM_MODE = 1;  // the mean runs over the valid pixels: the second partial
  using Sums = NoSums;
  struct Terms {
    float value, weight;
  };
  __device__ __forceinline__ void accumulate(Sums&, int, float) const {}
  __device__ __forceinline__ Terms terms(const Softmax& q, const Sums&, long long, int) const { return Terms{q.lse - q.zt, 1.f}; }
  __device__ __forceinline__ float grad(const Terms&, const Sums&, float p, int, bool target) const { return p - (target ? 1.f : 0.f); }
};

template <>
struct Ce<true> {
  const float* cw;  // null: ones
  float eps;
  static constexpr int NPART = 3;
  static constexpr int NORM_MODE = 1;  // divided by sum w_t
  struct Sums {
    float wsum = 0.f, swz = 0.f;  // with smoothing: W and sum_c w_c z_c
  };
  struct Terms {
    float value, weight, a, s;  // a = (1 - eps) w_t, s = eps / C
  };
  __device__ __forceinline__ void accumulate(Sums& m, int c, float z) const {
    if (eps > 0.f) {
      const float wc = cw ? cw[c] : 1.f;
      m.wsum += wc;
      m.swz = fmaf(wc, z, m.swz);
    }
  }
  __device__ __forceinline__ Terms terms(const Softmax& q, const Sums& m, long long tg, int nc) const {
    const float wt = cw ? cw[tg] : 1.f;
    const float a = (1.f - eps) * wt, s = eps / (float)nc;
    const float ce = q.lse - q.zt;
    return Terms{eps > 0.f ? a * ce + s * (m.wsum * q.lse - m.swz) : a * ce, wt, a, s};
  }
  __device__ __forceinline__ float grad(const Terms& t, const Sums& m, float p, int c, bool target) const {
    float g = t.a * (p - (target ? 1.f : 0.f));
    if (eps > 0.f) g += t.s * (m.wsum * p - (cw ? cw[c] : 1.f));
    return g;
  }
};

// ---- K1, evaluation -----------------------------------------------------------------------------------------------------------------------------

constexpr float SEG_KEY_INVALID = -1.f;  // the key plane's value at a pixel that is not valid: the sign bit marks it

template <class P, bool OHEM>
__global__ __launch_bounds__(256) void seg_pixel_kernel(const float* rows, cvx_seg_dims d, const long long* target, P pol, long long ignore_index,
                                                        float* dlogits, double* part /* per block: NPART sums */, int* bad, float* key, float* lplane) {
  __shared__ double sm[P::NPART][4];
  const long long plane = (long long)d.oh * d.ow, n = d.batch * plane;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  double my[P::NPART] = {};
  if (i < n) {
    const SegPixel px(i, d, target, ignore_index, bad);
    const PixelTaps tp(rows, d, px.b, px.oy, px.ox);
    const bool vec = rows_vec(rows, d.ld);
    const int tg = (int)px.tg;
    typename P::Sums sums;
    const Softmax q = online_softmax(tp, d.nc, vec, tg, [&](int c, float z) {
      pol.accumulate(sums, c, z);
      return 0.f;
    });
    typename P::Terms t{};
    if (px.valid) {
      t = pol.terms(q, sums, px.tg, d.nc);
      my[0] = (double)t.value;
      my[1] = (double)t.weight;
      if (P::NPART == 3) my[P::NPART - 1] = 1.0;
    }
    if (OHEM) {
      key[i] = px.valid ? fmaxf(q.lse - q.zt, 0.f) : SEG_KEY_INVALID;
      lplane[i] = t.value;
    }
    float* dl = dlogits + px.b * d.nc * plane + (long long)px.oy * d.ow + px.ox;
    each_logit(tp, d.nc, vec, [&](int c, float z) {
      const float g = pol.grad(t, sums, expf(z - q.lse), c, c == tg);  // unconditional: its loads are issued with the logits'
      dl[c * plane] = px.valid ? g : 0.f;
    });
  }
  block_to_part<P::NPART>(my, sm, part);
}

// Evaluation: EV_PIX label pixels per thread (chunks of 256 consecutive pixels, so a wave still reads along x), the arg max of the
// interpolated logits counted against the target, and the policy's value as in seg_pixel_kernel: part = per block (sum value, sum weight).
// LDS_HIST: the workgroup counts in nc * nc uint32 cells of LDS (nc <= 90: 32 KB) and adds its non-zero cells to the global int64 matrix
// once at the end; otherwise every pixel goes to the global matrix directly.  7 waves per SIMD (72 VGPRs) is what every instantiation needs;
// said here because left alone the compiler spends 78 on <Ce<false>, false> and loses a wave.
template <class P, bool LDS_HIST>
__global__ __launch_bounds__(256, 7) void seg_eval_kernel(const float* rows, cvx_seg_dims d, const long long* target, P pol, long long ignore_index,
                                                       unsigned long long* confusion, double* part) {
  extern __shared__ unsigned int hist[];
  __shared__ double sm[2][4];
  const int nc = d.nc;
  if (LDS_HIST) {
    hist_zero<256>(hist, nc);
    __syncthreads();
  }
  const long long n = (long long)d.batch * d.oh * d.ow;
  const bool vec = rows_vec(rows, d.ld);
  double my[2] = {0.0, 0.0};
  for (int it = 0; it < EV_PIX; ++it) {
    const long long i = ((long long)blockIdx.x * EV_PIX + it) * 256 + threadIdx.x;
    if (i >= n) break;
    const SegPixel px(i, d, target, ignore_index, nullptr);
    const PixelTaps tp(rows, d, px.b, px.oy, px.ox);
    typename P::Sums sums;
    const Softmax q = online_softmax(tp, nc, vec, (int)px.tg, [&](int c, float z) {
      pol.accumulate(sums, c, z);
      return 0.f;
    });
    if (px.valid) {
      const typename P::Terms t = pol.terms(q, sums, px.tg, nc);
      my[0] += (double)t.value;
      my[1] += (double)t.weight;
    }
    if (px.in_range) {
      if (LDS_HIST) hist_add(hist, nc, (int)px.tg, q.arg);
      else atomicAdd(confusion + (int)px.tg * nc + q.arg, 1ull);
    }
  }
  if (LDS_HIST) hist_flush<256>(hist, nc, confusion);
  block_to_part<2>(my, sm, part);
}

// ---- OHEM: K2 .. K4 -----------------------------------------------------------------------------------------------------------------------------

struct SegSelect {
  unsigned prefix, remaining;          // radix select state: key bits fixed so far, rank still to resolve inside the prefix bucket
  unsigned theta_t_bits, theta_min_bits;  // kept iff key bits > theta_t_bits or >= theta_min_bits (and the key is a valid pixel's)
  unsigned long long n_valid, k;
  int all;                             // fewer valid pixels than K: every valid pixel is kept, theta_min_bits = 0
  unsigned hist[256];
};

__device__ __forceinline__ bool seg_kept(unsigned bits, unsigned theta_t_bits, unsigned theta_min_bits) {
  return (bits >> 31) == 0u && (bits > theta_t_bits || bits >= theta_min_bits);
}

__global__ __launch_bounds__(256) void seg_ohem_plan_kernel(const double* part, int nblocks, float theta_t, long long k, SegSelect* sel) {
  __shared__ double sh[1][256];
  double nv[1];
  partials_sum_256<1>(part + 2, nblocks, 3, nv, sh);  // counts: exact in any order
  sel->hist[threadIdx.x] = 0u;
  if (threadIdx.x != 0) return;
  sel->n_valid = (unsigned long long)nv[0];
  sel->k = (unsigned long long)k;
  sel->all = sel->n_valid < (unsigned long long)k;
  sel->prefix = 0u;
  sel->remaining = sel->all ? 0u : (unsigned)k;
  sel->theta_t_bits = __float_as_uint(theta_t);
  sel->theta_min_bits = 0u;
}

__global__ __launch_bounds__(256) void seg_ohem_hist_kernel(const unsigned* key, long long N, int shift, SegSelect* sel) {
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

__global__ void seg_ohem_pick_kernel(int shift, SegSelect* sel) {  // one thread: the bucket (from the top) that holds the rank still looked for
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
// is the one every path uses: testing the keys inside the adjoint doubled its loads and its time (0.86 against 0.44 ms at batch 16).
__global__ __launch_bounds__(256) void seg_ohem_kept_sum_kernel(const unsigned* key, const float* lplane, const long long* target, const float* cw,
                                                                long long N, const SegSelect* sel, double* part, float* dlogits, int nc,
                                                                long long plane /* OH * OW */) {
  __shared__ double sm[3][4];
  const unsigned tt = sel->theta_t_bits, tm = sel->theta_min_bits;
  double my[3] = {0.0, 0.0, 0.0};
  for (int it = 0; it < KS_PIX; ++it) {
    const long long i = ((long long)blockIdx.x * KS_PIX + it) * 256 + threadIdx.x;
    if (i >= N) break;
    const unsigned kx = key[i];
    if (seg_kept(kx, tt, tm)) {  // a kept pixel is valid: its target is a class
      my[0] += (double)lplane[i];
      my[1] += (double)(cw ? cw[target[i]] : 1.f);
      my[2] += 1.0;
    } else if ((kx >> 31) == 0u) {
      float* dl = dlogits + (i / plane) * nc * plane + i % plane;
      for (int c = 0; c < nc; ++c) dl[(long long)c * plane] = 0.f;
    }
  }
  block_to_part<3>(my, sm, part);
}

// ---- K5, K6 -------------------------------------------------------------------------------------------------------------------------------------

// The partials in index order: acc[0..1] = (sum value, sum weight) for the adjoint; loss = sum value / normaliser, norm_mode 0:
// norm_const, 1: sum weight (an empty set: 0 / 0 = nan, as torch).  N == 3 (Ce<true>): stats = kept pixels, valid pixels, theta_min, the
// denominator; sel null: no OHEM.
template <int N>
__global__ __launch_bounds__(256) void seg_finalize_kernel(const double* part, int nblocks, const SegSelect* sel, double* acc, int norm_mode,
                                                           double norm_const, float* loss, double* stats) {
  __shared__ double sh[N][256];
  double v[N];
  partials_sum_256<N>(part, nblocks, N, v, sh);
  if (threadIdx.x == 0) {
    acc[0] = v[0];
    acc[1] = v[1];
    loss[0] = (float)(v[0] / (norm_mode == 0 ? norm_const : v[1]));
    if (N == 3) {
      stats[0] = v[N - 1];
      stats[1] = sel ? (double)sel->n_valid : v[N - 1];
      stats[2] = sel && !sel->all ? (double)__uint_as_float(sel->theta_min_bits) : -(double)INFINITY;
      stats[3] = v[1];
    }
  }
}

__device__ __forceinline__ void bilinear_dst_range(int s, float scale, int out_size, int* lo, int* hi) {
  const float a = ((float)s - 0.5f) / scale - 0.5f, b = ((float)s + 1.5f) / scale - 0.5f;
  int l = (int)floorf(a) - 1, h = (int)ceilf(b) + 1;
  *lo = l < 0 ? 0 : l;
  *hi = h > out_size - 1 ? out_size - 1 : h;
}

// dpred[b][y*iw + x][c] = scale * sum over label pixels of w(oy, y) * w(ox, x) * g[b][c][oy][ox]; columns nc..ld-1 are zeroed.
// norm_mode 0: scale = grad_scale / norm_const; 1: scale = grad_scale / acc[1] (the pixel kernel's sum of weights; 1 where that is not positive).
// A workgroup owns 32 consecutive pixels of the flattened (b, y, x) order and all ld columns: thread = (pixel lane, class lane of 8), so a
// wave reads two class planes along x (contiguous), and the 32 x ld results leave through LDS as whole rows (one contiguous run of
// 32 * ld halves) -- a thread per (class, pixel) would write single halves 2 * ld bytes apart from workgroups on different XCDs.
__global__ __launch_bounds__(256) void resize_grad_rows_kernel(const float* g, int B, int nc, int ih, int iw, int OH, int OW, float grad_scale,
                                                               int norm_mode, double norm_const, const double* acc, half_t* dpred, int ld) {
  extern __shared__ __attribute__((aligned(16))) half_t tile[];  // [RG_PIX][ld]
  const long long npix = (long long)B * ih * iw;
  const long long p0 = (long long)blockIdx.x * RG_PIX;
  const int pl = threadIdx.x & (RG_PIX - 1), cl = threadIdx.x >> 5;
  const long long pidx = p0 + pl;
  const bool live = pidx < npix;
  const int x = live ? (int)(pidx % iw) : 0;
  const long long t = live ? pidx / iw : 0;
  const int y = (int)(t % ih);
  const int b = (int)(t / ih);
  const float sh = (float)ih / (float)OH, sw = (float)iw / (float)OW;
  int oy0, oy1, ox0, ox1;
  bilinear_dst_range(y, sh, OH, &oy0, &oy1);
  bilinear_dst_range(x, sw, OW, &ox0, &ox1);
  const double denom = norm_mode == 0 ? norm_const : (acc[1] > 0.0 ? acc[1] : 1.0);
  const float scale = (float)((double)grad_scale / denom);
  constexpr int XC = 12;  // label columns per chunk (the whole range at DeepLab's 4x upsampling)
  for (int c = cl; c < ld; c += 8) {
    float accv = 0.f;
    if (live && c < nc) {
      const float* gp = g + ((long long)b * nc + c) * OH * OW;
      for (int oxc = ox0; oxc <= ox1; oxc += XC) {  // the column weights of a chunk once, then every label row against them
        float wx[XC];
        int xo[XC];
#pragma unroll
        for (int j = 0; j < XC; ++j) {
          int x0, x1;
          float lx;
          bilinear_src(oxc + j, sw, iw, &x0, &x1, &lx);
          wx[j] = oxc + j <= ox1 ? (x0 == x ? 1.f - lx : 0.f) + (x1 == x ? lx : 0.f) : 0.f;
          xo[j] = oxc + j <= ox1 ? oxc + j : ox1;  // clamped: the loads below are unconditional (issued together), the weight is 0 there
        }
        for (int oy = oy0; oy <= oy1; ++oy) {
          int y0, y1;
          float ly;
          bilinear_src(oy, sh, ih, &y0, &y1, &ly);
          const float wy = (y0 == y ? 1.f - ly : 0.f) + (y1 == y ? ly : 0.f);
          if (wy == 0.f) continue;
          const float* gr = gp + (long long)oy * OW;
          float gv[XC];
#pragma unroll
          for (int j = 0; j < XC; ++j) gv[j] = gr[xo[j]];
          float row = 0.f;
#pragma unroll
          for (int j = 0; j < XC; ++j) row = fmaf(wx[j], gv[j], row);
          accv = fmaf(wy, row, accv);
        }
      }
    }
    tile[pl * ld + c] = (half_t)(accv * scale);
  }
  __syncthreads();
  const long long nlive = npix - p0 < RG_PIX ? npix - p0 : RG_PIX;
  const int nhalf = (int)nlive * ld;
  half_t* dst = dpred + p0 * ld;
  if ((ld & 7) == 0 && (reinterpret_cast<uintptr_t>(dpred) & 15) == 0) {
    for (int i = threadIdx.x * 8; i < nhalf; i += 256 * 8) *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(tile + i);
  } else {
    for (int i = threadIdx.x; i < nhalf; i += 256) dst[i] = tile[i];
  }
}

// ---- the region term: R1 .. R4 ------------------------------------------------------------------------------------------------------------------

struct RegionCfg {
  double alpha, beta, gamma, smooth, weight, base_weight;
  int skip_absent;
};

// Workgroup blk of image b owns the pixels [blk * 256 * RS_PIX, ...) of that image: it never straddles two images, so the partials of an
// image are the bpi consecutive triples b * bpi .. and a group (image or batch) is a contiguous run of them.
__global__ __launch_bounds__(256) void seg_region_sums_kernel(const float* rows, cvx_seg_dims d, const long long* target, long long ignore_index, int bpi,
                                                              double* part /* [workgroup][nc][I, P, Y] */, int* bad) {
  __shared__ float s[24][RS_ROW];
  const int b = blockIdx.x / bpi, blk = blockIdx.x % bpi, nc = d.nc;
  const long long plane = (long long)d.oh * d.ow;
  const bool vec = rows_vec(rows, d.ld);
  float lse[RS_PIX];
  int tgt[RS_PIX];  // -1: not a valid pixel (or past the image's end)
#pragma unroll
  for (int it = 0; it < RS_PIX; ++it) {
    const long long i = ((long long)blk * RS_PIX + it) * 256 + threadIdx.x;
    tgt[it] = -1;
    lse[it] = 0.f;
    if (i < plane) {
      const SegPixel px(b, i, d, target, ignore_index, bad);
      if (px.valid) {
        lse[it] = online_softmax(PixelTaps(rows, d, b, px.oy, px.ox), nc, vec, -1, [](int, float) { return 0.f; }).lse;
        tgt[it] = (int)px.tg;
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
      const PixelTaps tp(rows, d, b, (int)(i / d.ow), (int)(i % d.ow));
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

// base_loss: the base's value (null: no base term); base_acc / norm_mode / norm_const: its gradient's normaliser (the adjoint's rule), used
// when hdr is not null (training).  coef: (G, nc, 2) floats = weight * (a_c, b_c); hdr[0] = base_weight / normaliser.
__global__ __launch_bounds__(256) void seg_region_solve_kernel(const double* sums, int G, int nc, RegionCfg cfg, const float* v, const float* base_loss,
                                                               const double* base_acc, int norm_mode, double norm_const, float* coef, float* hdr,
                                                               double* stats /* (G, nc, 4): I, P, Y, T */, float* loss_out) {
  __shared__ double sh[2][256];
  double total = 0.0;
  for (int g = 0; g < G; ++g) {
    const double* sg = sums + (long long)g * 3 * nc;
    double m[2] = {0.0, 0.0};  // sum m v, sum m v L
    for (int c = threadIdx.x; c < nc; c += 256) {
      const ClassTerms t = class_terms(sg, c, cfg, v);
      m[0] += t.w;
      m[1] += t.w * t.L;
    }
    block_tree_256<2>(m, sh);
    const double mv = m[0], mvl = m[1];
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

// One thread per label pixel, as seg_pixel_kernel (a wave writes a class plane along x).  With g_c = a_c [t == c] + b_c,
// sum_c p_c g_c = (sum_c e_c g_c) / (sum_c e_c) rides the online softmax's rescaling.
__global__ __launch_bounds__(256) void seg_region_grad_kernel(const float* rows, cvx_seg_dims d, const long long* target, long long ignore_index,
                                                              const float* coef, int per_image, const float* hdr, int has_base, float* dlogits) {
  const int nc = d.nc;
  const long long plane = (long long)d.oh * d.ow;
  const long long n = (long long)d.batch * plane;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const SegPixel px(i, d, target, ignore_index, nullptr);
  float* dl = dlogits + (long long)px.b * nc * plane + (long long)px.oy * d.ow + px.ox;
  if (!px.valid) {  // with a base the plane holds the base's zero here already
    if (!has_base)
      for (int c = 0; c < nc; ++c) dl[(long long)c * plane] = 0.f;
    return;
  }
  const int tg = (int)px.tg;
  const float* cf = coef + (long long)(per_image ? px.b : 0) * nc * 2;
  const PixelTaps tp(rows, d, px.b, px.oy, px.ox);
  const bool vec = rows_vec(rows, d.ld);
  const Softmax q = online_softmax(tp, nc, vec, tg, [&](int c, float) { return cf[2 * c + 1] + (c == tg ? cf[2 * c] : 0.f); });
  const float lse = q.lse, S = q.sg / q.se;
  const float sb = has_base ? hdr[0] : 0.f;
  auto term = [&](int c, float z) {
    const float g = cf[2 * c + 1] + (c == tg ? cf[2 * c] : 0.f);
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

// ---- the Lovasz-Softmax term: L1 .. L9 ----------------------------------------------------------------------------------------------------------
// (the rules: include/cvx_engine.h; the sort: lovasz_sort.h).  A group's valid pixels are compacted in index order, so segment
// (group, class) holds nvalid[group] keys and every bit pattern is free to be a key.

// The payload that travels with a key: training keeps the pixel's index inside its group (bits 0..30) and the foreground flag (bit 31);
// the value-only chain of validation needs the flag alone, one byte.
template <class PL>
struct LvPay;
template <>
struct LvPay<unsigned> {
  static __device__ __forceinline__ unsigned make(unsigned idx, bool fg) { return idx | (fg ? 0x80000000u : 0u); }
  static __device__ __forceinline__ bool fg(unsigned v) { return (v >> 31) != 0u; }
  static __device__ __forceinline__ unsigned idx(unsigned v) { return v & 0x7FFFFFFFu; }
};
template <>
struct LvPay<unsigned char> {
  static __device__ __forceinline__ unsigned char make(unsigned, bool fg) { return fg ? 1 : 0; }
  static __device__ __forceinline__ bool fg(unsigned char v) { return v != 0; }
  static __device__ __forceinline__ unsigned idx(unsigned char) { return 0u; }
};

// L1: the valid pixels of each block of LV_TILE consecutive pixels of an image (block blk of image b = workgroup b * bpk + blk).
__global__ __launch_bounds__(256) void seg_lovasz_count_kernel(const long long* target, cvx_seg_dims d, long long ignore_index, int bpk, int* blkcnt) {
  __shared__ unsigned sh[16];
  const int b = blockIdx.x / bpk, blk = blockIdx.x % bpk;
  const long long plane = (long long)d.oh * d.ow;
  bool f[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const long long i = ((long long)blk * 4 + it) * 256 + threadIdx.x;
    f[it] = i < plane && SegPixel(b, i, d, target, ignore_index, nullptr).valid;
  }
  unsigned rank[4], total;
  lv_rank4(f, sh, rank, &total);
  if (threadIdx.x == 0) blkcnt[blockIdx.x] = (int)total;
}

// L2: one workgroup per group: the exclusive running count over the group's ppg blocks in order -> blkoff; the total -> nvalid[group].
__global__ __launch_bounds__(256) void seg_lovasz_offsets_kernel(const int* blkcnt, int ppg, int* blkoff, int* nvalid) {
  __shared__ unsigned sh[256];
  const int g = blockIdx.x, per = (ppg + 255) / 256;
  const long long lo = (long long)threadIdx.x * per, hi = lo + per < ppg ? lo + per : ppg;
  const int* cnt = blkcnt + (long long)g * ppg;
  unsigned mine = 0u;
  for (long long i = lo; i < hi; ++i) mine += (unsigned)cnt[i];
  unsigned total;
  unsigned run = lv_excl_scan_256(mine, sh, &total);
  for (long long i = lo; i < hi; ++i) {
    blkoff[(long long)g * ppg + i] = (int)run;
    run += (unsigned)cnt[i];
  }
  if (threadIdx.x == 0) nvalid[g] = (int)total;
}

// L3: the keys.  The workgroup's pixels as in L1; per valid pixel the log-sum-exp, then the classes eight at a time as in R1 (with the
// interpolation weights from a double coordinate, see PixelTaps): the error e = [t == c] ? 1 - p_c : p_c in fp32, its bit pattern and the payload to place blkoff + (rank among the block's valid pixels) of
// segment (group, class).  G_c: counted in LDS, then integer atomics (exact in any order).
template <class PL>
__global__ __launch_bounds__(256) void seg_lovasz_keys_kernel(const float* rows, cvx_seg_dims d, const long long* target, long long ignore_index, int bpk,
                                                              int per_image, const int* blkoff, unsigned* keys, PL* pay, int* gc, int* bad) {
  __shared__ unsigned sh[16];
  __shared__ int hist[REGION_MAX_NC];
  const int b = blockIdx.x / bpk, blk = blockIdx.x % bpk, nc = d.nc;
  const long long plane = (long long)d.oh * d.ow;
  const int g = per_image ? b : 0;
  const long long ng = per_image ? plane : (long long)d.batch * plane;
  const bool vec = rows_vec(rows, d.ld);
  const double sy = (double)d.ih / (double)d.oh, sx = (double)d.iw / (double)d.ow;  // the keys' own interpolation weights: PixelTaps
  for (int c = threadIdx.x; c < nc; c += 256) hist[c] = 0;
  float lse[4];
  int tgt[4];  // -1: not a valid pixel (or past the image's end)
  bool f[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const long long i = ((long long)blk * 4 + it) * 256 + threadIdx.x;
    tgt[it] = -1;
    lse[it] = 0.f;
    if (i < plane) {
      const SegPixel px(b, i, d, target, ignore_index, bad);
      if (px.valid) {
        lse[it] = online_softmax(PixelTaps(rows, d, b, px.oy, px.ox, sy, sx), nc, vec, -1, [](int, float) { return 0.f; }).lse;
        tgt[it] = (int)px.tg;
      }
    }
    f[it] = tgt[it] >= 0;
  }
  unsigned rank[4], total;
  lv_rank4(f, sh, rank, &total);  // its barrier also covers the zeroing of hist
  const long long first = blkoff[blockIdx.x];
#pragma unroll
  for (int it = 0; it < 4; ++it)
    if (f[it]) atomicAdd(&hist[tgt[it]], 1);
  for (int c0 = 0; c0 < nc; c0 += 8) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      if (!f[it]) continue;
      const long long i = ((long long)blk * 4 + it) * 256 + threadIdx.x;
      const PixelTaps tp(rows, d, b, (int)(i / d.ow), (int)(i % d.ow), sy, sx);
      float z[8];
      if (vec) {
        tp.logits8(c0, z);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) z[k] = c0 + k < nc ? tp.logit(c0 + k) : 0.f;
      }
      const long long at = first + rank[it];
      const unsigned idx = (unsigned)(per_image ? i : (long long)b * plane + i);
      if (at >= ng) continue;  // never: the offsets count the same pixels
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (c0 + k < nc) {
          const float p = expf(z[k] - lse[it]);
          const bool fg = tgt[it] == c0 + k;
          const float e = fg ? fmaxf(1.f - p, 0.f) : p;
          const long long o = ((long long)g * nc + c0 + k) * ng + at;
          keys[o] = __float_as_uint(e);
          pay[o] = LvPay<PL>::make(idx, fg);
        }
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nc; c += 256)
    if (hist[c]) atomicAdd(&gc[(long long)g * nc + c], hist[c]);
}

struct LovaszCfg {
  double weight, base_weight;
  int skip_absent;
};
__device__ __forceinline__ double lovasz_mv(const LovaszCfg& cfg, const int* gc, const float* v, int c) {
  return (cfg.skip_absent && gc[c] == 0) ? 0.0 : (v ? (double)v[c] : 1.0);
}

// L4: one workgroup, once the counts are known: coef[g][c] = weight (1/G) m_c v_c / sum m v -- what a pixel's s * Delta is scaled by --
// and the segment table (element offset, length) of the sorted view; a segment the sort skips has length 0.
__global__ __launch_bounds__(256) void seg_lovasz_plan_kernel(const int* gc, const int* nvalid, int G, int nc, long long ng, LovaszCfg cfg, const float* v,
                                                              double* coef, long long* segtab) {
  __shared__ double sh[1][256];
  for (int g = 0; g < G; ++g) {
    const int* gg = gc + (long long)g * nc;
    double m[1] = {0.0};
    for (int c = threadIdx.x; c < nc; c += 256) m[0] += lovasz_mv(cfg, gg, v, c);
    block_tree_256<1>(m, sh);
    for (int c = threadIdx.x; c < nc; c += 256) {
      const long long s = (long long)g * nc + c;
      coef[s] = m[0] > 0.0 ? cfg.weight * (1.0 / (double)G) * lovasz_mv(cfg, gg, v, c) / m[0] : 0.0;
      segtab[2 * s] = s * ng;
      segtab[2 * s + 1] = (cfg.skip_absent && gg[c] == 0) ? 0 : nvalid[g];
    }
  }
}

// L6: the foreground flags of a tile of the sorted segment.
template <class PL>
__global__ __launch_bounds__(256) void seg_lovasz_flagsum_kernel(const PL* pay, LvGeom q, const int* nvalid, const int* gc, unsigned* tilefg) {
  __shared__ unsigned sh[16];
  const LvTile t = lv_tile(q, nvalid, gc);
  if (!t.live) return;
  bool f[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long i = (long long)t.tile * LV_TILE + j * 256 + threadIdx.x;
    f[j] = i < t.n && LvPay<PL>::fg(pay[t.base + i]);
  }
  unsigned rank[4], total;
  lv_rank4(f, sh, rank, &total);
  if (threadIdx.x == 0) tilefg[blockIdx.x] = total;
}

// L7: one workgroup per segment: the exclusive running count of the tiles' flags, in place.
__global__ __launch_bounds__(256) void seg_lovasz_flagscan_kernel(LvGeom q, const int* nvalid, const int* gc, unsigned* tilefg) {
  __shared__ unsigned sh[256];
  const int seg = blockIdx.x;
  int nt;
  if (!lv_segment_live(q, nvalid, gc, seg, &nt)) return;
  unsigned* tf = tilefg + (long long)seg * q.tps;
  const int per = (nt + 255) / 256;
  const int lo = min(threadIdx.x * per, (unsigned)nt), hi = min(lo + per, nt);
  unsigned mine = 0u;
  for (int i = lo; i < hi; ++i) mine += tf[i];
  unsigned total;
  unsigned run = lv_excl_scan_256(mine, sh, &total);
  for (int i = lo; i < hi; ++i) {
    const unsigned v = tf[i];
    tf[i] = run;
    run += v;
  }
}

// L8: the element of rank k of a segment has fb foreground and k - fb background elements in front of it (integers: the tile's offset
// plus a ballot count), so I = G_c - fb, U = G_c + k - fb and Delta = 1 / U at a foreground element, I / (U (U + 1)) at a background
// one (1 for the first element of a class without a target pixel): one division in double.  sum e Delta -> one partial per tile;
// TRAIN: coef * s * Delta -> the plane, at the pixel's place in the gradient plane's layout (b, c, y, x).
template <class PL, bool TRAIN>
__global__ __launch_bounds__(256) void seg_lovasz_value_kernel(const unsigned* keys, const PL* pay, LvGeom q, const int* nvalid, const int* gc,
                                                               const unsigned* tilefg, const double* coef, int per_image, long long plane, float* hplane,
                                                               double* part) {
  __shared__ unsigned sh[16];
  __shared__ double sm[1][4];
  const LvTile t = lv_tile(q, nvalid, gc);
  if (!t.live) return;
  bool f[4], ok[4];
  unsigned key[4];
  PL pl[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long i = (long long)t.tile * LV_TILE + j * 256 + threadIdx.x;
    ok[j] = i < t.n;
    key[j] = ok[j] ? keys[t.base + i] : 0u;
    pl[j] = ok[j] ? pay[t.base + i] : PL(0);
    f[j] = ok[j] && LvPay<PL>::fg(pl[j]);
  }
  unsigned rank[4], total;
  lv_rank4(f, sh, rank, &total);
  const long long Gc = gc[t.seg], F0 = tilefg[blockIdx.x];
  const double cf = TRAIN ? coef[t.seg] : 0.0;
  const int g = t.seg / q.nc, c = t.seg % q.nc;
  double my[1] = {0.0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!ok[j]) continue;
    const long long k = (long long)t.tile * LV_TILE + j * 256 + threadIdx.x;
    const long long fb = F0 + rank[j], I = Gc - fb, U = Gc + (k - fb);
    const double dl = U <= 0 ? 1.0 : f[j] ? 1.0 / (double)U : (double)I / ((double)U * (double)(U + 1));
    my[0] += (double)__uint_as_float(key[j]) * dl;
    if (TRAIN) {
      const long long idx = (long long)LvPay<PL>::idx(pl[j]);
      const long long b = per_image ? g : idx / plane, in = per_image ? idx : idx % plane;
      if (idx < q.ng) hplane[(b * q.nc + c) * plane + in] = (float)(cf * (f[j] ? -dl : dl));  // idx < ng always: the keys kernel wrote it
    }
  }
  block_to_part<1>(my, sm, part);
}

// L9a: one workgroup per segment: L_c = the tiles' partials in order (0 for a segment the sort skipped).
__global__ __launch_bounds__(256) void seg_lovasz_reduce_kernel(const double* part, LvGeom q, const int* nvalid, const int* gc, double* L) {
  __shared__ double sh[1][256];
  const int seg = blockIdx.x;
  int nt;
  if (!lv_segment_live(q, nvalid, gc, seg, &nt)) nt = 0;
  double v[1];
  partials_sum_256<1>(part + (long long)seg * q.tps, nt, 1, v, sh);
  if (threadIdx.x == 0) L[seg] = v[0];
}

// L9b: one workgroup: the group losses, the stats (0, 0, Y_c, L_c), the combined loss and, in training (hdr not null), the base's scale --
// seg_region_solve_kernel's tail.
__global__ __launch_bounds__(256) void seg_lovasz_solve_kernel(const double* L, const int* gc, int G, int nc, LovaszCfg cfg, const float* v,
                                                               const float* base_loss, const double* base_acc, int norm_mode, double norm_const, float* hdr,
                                                               double* stats, float* loss_out) {
  __shared__ double sh[2][256];
  double total = 0.0;
  for (int g = 0; g < G; ++g) {
    const int* gg = gc + (long long)g * nc;
    double m[2] = {0.0, 0.0};
    for (int c = threadIdx.x; c < nc; c += 256) {
      const double w = lovasz_mv(cfg, gg, v, c);
      m[0] += w;
      m[1] += w * L[(long long)g * nc + c];
    }
    block_tree_256<2>(m, sh);
    total += m[0] > 0.0 ? m[1] / m[0] : 0.0;
    for (int c = threadIdx.x; c < nc; c += 256) {
      const long long o = (long long)g * nc + c;
      stats[4 * o] = 0.0;
      stats[4 * o + 1] = 0.0;
      stats[4 * o + 2] = (double)gg[c];
      stats[4 * o + 3] = L[o];
    }
  }
  if (threadIdx.x == 0) {
    const double lov = total / (double)G;
    loss_out[0] = base_loss ? (float)(cfg.base_weight * (double)base_loss[0] + cfg.weight * lov) : (float)(cfg.weight * lov);
    if (hdr) {
      const double denom = norm_mode == 0 ? norm_const : (base_acc && base_acc[1] > 0.0 ? base_acc[1] : 1.0);
      hdr[0] = (float)(cfg.base_weight / denom);
    }
  }
}

// L10: seg_region_grad_kernel with h_c read from the plane L8 wrote (0 where coef is 0: the sort skipped the class and wrote nothing):
// base_weight * g_base / normaliser + p_k (h_k - sum_c p_c h_c) -> the gradient plane, in place with a base.
__global__ __launch_bounds__(256) void seg_lovasz_grad_kernel(const float* rows, cvx_seg_dims d, const long long* target, long long ignore_index,
                                                              const float* hplane, const double* coef, int per_image, const float* hdr, int has_base,
                                                              float* dlogits) {
  const int nc = d.nc;
  const long long plane = (long long)d.oh * d.ow;
  const long long n = (long long)d.batch * plane;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const SegPixel px(i, d, target, ignore_index, nullptr);
  const long long at = (long long)px.b * nc * plane + (long long)px.oy * d.ow + px.ox;
  float* dl = dlogits + at;
  if (!px.valid) {  // with a base the plane holds the base's zero here already
    if (!has_base)
      for (int c = 0; c < nc; ++c) dl[(long long)c * plane] = 0.f;
    return;
  }
  const int tg = (int)px.tg;
  const float* hp = hplane + at;
  const double* cf = coef + (long long)(per_image ? px.b : 0) * nc;
  const PixelTaps tp(rows, d, px.b, px.oy, px.ox);
  const bool vec = rows_vec(rows, d.ld);
  auto h = [&](int c) {
    const float x = hp[(long long)c * plane];
    return cf[c] != 0.0 ? x : 0.f;
  };
  const Softmax q = online_softmax(tp, nc, vec, tg, [&](int c, float) { return h(c); });
  const float lse = q.lse, S = q.sg / q.se;
  const float sb = has_base ? hdr[0] : 0.f;
  if (vec) {  // eight classes at a time: the base's eight gradients and the eight coefficients are loaded together, ahead of the eight stores
    for (int c0 = 0; c0 < nc; c0 += 8) {
      float z[8], old[8], hc[8];
      tp.logits8(c0, z);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        old[k] = has_base && c0 + k < nc ? dl[(long long)(c0 + k) * plane] : 0.f;
        hc[k] = c0 + k < nc ? h(c0 + k) : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c0 + k < nc) dl[(long long)(c0 + k) * plane] = fmaf(sb, old[k], expf(z[k] - lse) * (hc[k] - S));
    }
  } else {
    for (int c = 0; c < nc; ++c) {
      float* o = dl + (long long)c * plane;
      *o = fmaf(sb, has_base ? *o : 0.f, expf(tp.logit(c) - lse) * (h(c) - S));
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------

inline bool seg_ohem(const cvx_seg_criterion& c) { return !(c.ohem_theta < 0.f); }  // -ln thresh >= 0; negative: off
inline bool seg_with_options(const cvx_seg_criterion& c) { return c.class_weight != nullptr || c.label_smoothing > 0.f || seg_ohem(c); }
inline long long seg_npix(const cvx_seg_dims& d) { return (long long)d.batch * d.oh * d.ow; }
inline long long seg_pixel_blocks(long long npix) { return cvx_cdiv(npix, 256); }
inline long long seg_eval_blocks(long long npix) { return cvx_cdiv(npix, 256 * EV_PIX); }
inline long long seg_kept_sum_blocks(long long npix) { return cvx_cdiv(npix, 256 * KS_PIX); }
inline int seg_region_bpi(const cvx_seg_dims& d) { return cvx_cdiv((long long)d.oh * d.ow, 256 * RS_PIX); }
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int seg_lovasz_bpk(const cvx_seg_dims& d) { return cvx_cdiv((long long)d.oh * d.ow, LV_TILE); }
inline long long seg_lovasz_ng(const cvx_seg_dims& d, const cvx_seg_criterion& c) { return (c.per_image ? 1LL : (long long)d.batch) * d.oh * d.ow; }

// Every offset into the workspace.  The first CVX_SEG_OPTS_KEY_OFFSET bytes hold the small state -- the totals acc[2] at 0, the OHEM
// selection at 64, the region header at SEG_HDR (hdr[0] the base's scale, hdr[1] the base's value, then evaluation's bad-label flag) --
// so the key plane starts at that constant in every configuration.  Then, each a multiple of 256 bytes and present only when used:
// [key plane, loss plane] (OHEM); the base's partials [and the kept sum's]; the region's sums, coefficients and partials (its size does
// not depend on the base or on for_eval); the Lovasz term's state (region 2: the block counts and offsets, the counts per group and
// class, the coefficients, L_c, the segment table, the sort's tables, the tiles' flag counts and partials, then the two ping-pong
// buffers of keys and payload -- the payload is one byte in evaluation, four in training); last the gradient plane (training).
constexpr size_t SEG_SELECT = 64, SEG_HDR = 2048;
static_assert(SEG_SELECT + sizeof(SegSelect) <= SEG_HDR && SEG_HDR + 256 <= CVX_SEG_OPTS_KEY_OFFSET,
              "the totals, the selection state and the region header sit in front of the key plane");
struct SegLayout {
  size_t key, lplane, part, part_kept, sums, coef, rpart, dlogits, total;
  size_t lv_blkcnt, lv_blkoff, lv_nvalid, lv_gc, lv_coef, lv_L, lv_segtab, lv_binbase, lv_tilehist, lv_tilefg, lv_part, lv_key[2], lv_pay[2];
  SegLayout(const cvx_seg_dims& d, const cvx_seg_criterion& c, bool for_eval) {
    const size_t npix = (size_t)seg_npix(d);
    size_t o = CVX_SEG_OPTS_KEY_OFFSET;
    auto take = [&o](size_t bytes) {
      const size_t at = o;
      o += al256(bytes);
      return at;
    };
    const bool ohem = !for_eval && c.base == 2 && seg_ohem(c);
    key = take(ohem ? npix * 4 : 0);
    lplane = take(ohem ? npix * 4 : 0);
    part = take(for_eval ? (size_t)seg_eval_blocks(npix) * 16 : c.base == 0 ? 0 : (size_t)seg_pixel_blocks(npix) * 24);
    part_kept = take(ohem ? (size_t)seg_kept_sum_blocks(npix) * 24 : 0);
    const size_t G = c.per_image ? (size_t)d.batch : 1, nc = (size_t)d.nc;
    sums = take(c.region == 1 ? G * 3 * nc * 8 : 0);
    coef = take(c.region == 1 ? G * 2 * nc * 4 : 0);
    rpart = take(c.region == 1 ? (size_t)d.batch * seg_region_bpi(d) * 3 * nc * 8 : 0);
    const bool lv = c.region == 2;
    const size_t nblk = lv ? (size_t)d.batch * seg_lovasz_bpk(d) : 0, nseg = lv ? G * nc : 0, ng = lv ? (size_t)seg_lovasz_ng(d, c) : 0;
    const size_t tiles = nseg * (size_t)cvx_cdiv((long long)ng, LV_TILE), pay = for_eval ? 1 : 4;
    lv_blkcnt = take(nblk * 4);
    lv_blkoff = take(nblk * 4);
    lv_nvalid = take(lv ? G * 4 : 0);
    lv_gc = take(nseg * 4);
    lv_coef = take(nseg * 8);
    lv_L = take(nseg * 8);
    lv_segtab = take(nseg * 16);
    lv_binbase = take(nseg * 256 * 4);
    lv_tilehist = take(tiles * 256 * 4);
    lv_tilefg = take(tiles * 4);
    lv_part = take(tiles * 8);
    for (int q = 0; q < 2; ++q) {
      lv_key[q] = take(nseg * ng * 4);
      lv_pay[q] = take(nseg * ng * pay);
    }
    dlogits = o;
    total = o + (for_eval ? 0 : npix * nc * 4);
  }
};

// What the base chain leaves on the device: the fp32 gradient plane (batch, nc, oh, ow), not yet normalised, and its normaliser (the
// adjoint's rule).
struct SegChain {
  float* dlogits;
  const double* acc;
  int norm_mode;
  double norm_const;
};

void launch_adjoint(const SegChain& ch, const cvx_seg_dims& d, float scale, void* dpred_f16, hipStream_t st) {
  const long long nlow = (long long)d.batch * d.ih * d.iw;
  hipLaunchKernelGGL(resize_grad_rows_kernel, dim3((unsigned)cvx_cdiv(nlow, RG_PIX)), dim3(256), (size_t)RG_PIX * d.ld * 2, st, ch.dlogits, d.batch, d.nc, d.ih,
                     d.iw, d.oh, d.ow, scale, ch.norm_mode, ch.norm_const, ch.acc, (half_t*)dpred_f16, d.ld);
}

// f(policy) with the base term's policy; base 0 (evaluation of a region term alone, where only the matrix is kept) counts with Ce<false>.
template <class F>
void with_policy(const cvx_seg_criterion& c, F f) {
  if (c.base == 1) f(Focal{c.focal_alpha, c.focal_gamma});
  else if (c.base == 2 && seg_with_options(c)) f(Ce<true>{c.class_weight, c.label_smoothing});
  else f(Ce<false>{});
}

// The base term's launches up to and including the finalize, which leaves the value in loss_out.  confusion null: training (K1 .. K5);
// else evaluation (seg_eval_kernel, K5).
SegChain seg_base_chain(const float* rows, const cvx_seg_dims& d, const long long* tg, const cvx_seg_criterion& c, const SegLayout& lay, char* w,
                        unsigned long long* confusion, float* loss_out, int32_t* bad, double* stats_out, hipStream_t st) {
  const bool eval = confusion != nullptr, ohem = !eval && c.base == 2 && seg_ohem(c);
  const long long npix = seg_npix(d), nblk = eval ? seg_eval_blocks(npix) : seg_pixel_blocks(npix), nks = seg_kept_sum_blocks(npix);
  const long long ig = (long long)c.ignore_index;
  double *acc = (double*)w, *part = (double*)(w + lay.part), *part_kept = (double*)(w + lay.part_kept);
  SegSelect* sel = (SegSelect*)(w + SEG_SELECT);
  float *key = ohem ? (float*)(w + lay.key) : nullptr, *lplane = ohem ? (float*)(w + lay.lplane) : nullptr;
  float* dlogits = (float*)(w + lay.dlogits);
  SegChain ch{dlogits, acc, 1, 1.0};
  with_policy(c, [&](auto pol) {
    using P = decltype(pol);
    if (P::NORM_MODE == 0) ch = SegChain{dlogits, acc, 0, (double)npix};
    if (eval) {
      if (d.nc * d.nc <= EV_LDS_CELLS)
        hipLaunchKernelGGL((seg_eval_kernel<P, true>), dim3((unsigned)nblk), dim3(256), (size_t)d.nc * d.nc * 4, st, rows, d, tg, pol, ig, confusion, part);
      else
        hipLaunchKernelGGL((seg_eval_kernel<P, false>), dim3((unsigned)nblk), dim3(256), 0, st, rows, d, tg, pol, ig, confusion, part);
      hipLaunchKernelGGL(seg_finalize_kernel<2>, dim3(1), dim3(256), 0, st, part, (int)nblk, (const SegSelect*)nullptr, acc, ch.norm_mode, ch.norm_const,
                         loss_out, (double*)nullptr);
      return;
    }
    if constexpr (std::is_same_v<P, Ce<true>>) {
      if (ohem) {
        const float theta = c.ohem_theta == 0.f ? 0.f : c.ohem_theta;  // -0.0 (thresh = 1) has the sign bit set
        hipLaunchKernelGGL((seg_pixel_kernel<P, true>), dim3((unsigned)nblk), dim3(256), 0, st, rows, d, tg, pol, ig, dlogits, part, bad, key, lplane);
        hipLaunchKernelGGL(seg_ohem_plan_kernel, dim3(1), dim3(256), 0, st, part, (int)nblk, theta, (long long)c.ohem_min_kept, sel);
        const int hb = (int)std::min<long long>(512, nblk);
        for (int shift = 24; shift >= 0; shift -= 8) {
          hipLaunchKernelGGL(seg_ohem_hist_kernel, dim3(hb), dim3(256), 0, st, (const unsigned*)key, npix, shift, sel);
          hipLaunchKernelGGL(seg_ohem_pick_kernel, dim3(1), dim3(1), 0, st, shift, sel);
        }
        hipLaunchKernelGGL(seg_ohem_kept_sum_kernel, dim3((unsigned)nks), dim3(256), 0, st, (const unsigned*)key, lplane, tg, c.class_weight, npix, sel,
                           part_kept, dlogits, d.nc, (long long)d.oh * d.ow);
        hipLaunchKernelGGL(seg_finalize_kernel<3>, dim3(1), dim3(256), 0, st, part_kept, (int)nks, (const SegSelect*)sel, acc, 1, 1.0, loss_out, stats_out);
        return;
      }
    }
    hipLaunchKernelGGL((seg_pixel_kernel<P, false>), dim3((unsigned)nblk), dim3(256), 0, st, rows, d, tg, pol, ig, dlogits, part, bad, key, lplane);
    hipLaunchKernelGGL(seg_finalize_kernel<P::NPART>, dim3(1), dim3(256), 0, st, part, (int)nblk, (const SegSelect*)nullptr, acc, ch.norm_mode, ch.norm_const,
                       loss_out, stats_out);
  });
  return ch;
}

// R1 .. R3 and, in training (ch not null), R4 on the gradient plane the base chain left (ch->acc null: no base).
void seg_region_chain(const float* rows, const cvx_seg_dims& d, const long long* tg, const cvx_seg_criterion& c, const SegLayout& lay, char* w,
                      const float* base_loss, const SegChain* ch, int32_t* bad, double* region_stats_out, float* loss_out, hipStream_t st) {
  const int bpi = seg_region_bpi(d);
  const long long nparts = (long long)d.batch * bpi, ig = (long long)c.ignore_index;
  const int G = c.per_image ? d.batch : 1, ppg = c.per_image ? bpi : (int)nparts, E = 3 * d.nc;
  float *hdr = (float*)(w + SEG_HDR), *coef = (float*)(w + lay.coef);
  double *sums = (double*)(w + lay.sums), *part = (double*)(w + lay.rpart);
  const RegionCfg cfg{c.alpha, c.beta, c.gamma, c.smooth, c.weight, c.base_weight, c.skip_absent != 0};
  hipLaunchKernelGGL(seg_region_sums_kernel, dim3((unsigned)nparts), dim3(256), 0, st, rows, d, tg, ig, bpi, part, bad);
  hipLaunchKernelGGL(seg_region_reduce_kernel, dim3((unsigned)cvx_cdiv(E, 16), (unsigned)G), dim3(256), 0, st, part, ppg, E, sums);
  hipLaunchKernelGGL(seg_region_solve_kernel, dim3(1), dim3(256), 0, st, sums, G, d.nc, cfg, c.region_class_weight, base_loss, ch ? ch->acc : nullptr,
                     ch ? ch->norm_mode : 0, ch ? ch->norm_const : 1.0, ch ? coef : nullptr, ch ? hdr : nullptr, region_stats_out, loss_out);
  if (ch)
    hipLaunchKernelGGL(seg_region_grad_kernel, dim3((unsigned)seg_pixel_blocks(seg_npix(d))), dim3(256), 0, st, rows, d, tg, ig, coef, c.per_image, hdr,
                       ch->acc != nullptr, ch->dlogits);
}

// L1 .. L9 and, in training (ch not null), L10 on the gradient plane the base chain left (ch->acc null: no base).  PL: the payload.
// The plane of L8 lies in the second key buffer, which the sort has left by then; the sorted keys and payload stay in the first.
template <class PL>
void seg_lovasz_chain(const float* rows, const cvx_seg_dims& d, const long long* tg, const cvx_seg_criterion& c, const SegLayout& lay, char* w,
                      const float* base_loss, const SegChain* ch, int32_t* bad, double* region_stats_out, float* loss_out, hipStream_t st) {
  const int bpk = seg_lovasz_bpk(d), G = c.per_image ? d.batch : 1, nseg = G * d.nc, nblk = d.batch * bpk, ppg = c.per_image ? bpk : nblk;
  const long long ig = (long long)c.ignore_index, plane = (long long)d.oh * d.ow;
  const LvGeom q{seg_lovasz_ng(d, c), cvx_cdiv(seg_lovasz_ng(d, c), LV_TILE), d.nc, c.skip_absent != 0};
  const unsigned tiles = (unsigned)nseg * (unsigned)q.tps;
  int *blkcnt = (int*)(w + lay.lv_blkcnt), *blkoff = (int*)(w + lay.lv_blkoff), *nvalid = (int*)(w + lay.lv_nvalid), *gc = (int*)(w + lay.lv_gc);
  double *coef = (double*)(w + lay.lv_coef), *L = (double*)(w + lay.lv_L), *part = (double*)(w + lay.lv_part);
  unsigned *binbase = (unsigned*)(w + lay.lv_binbase), *tilehist = (unsigned*)(w + lay.lv_tilehist), *tilefg = (unsigned*)(w + lay.lv_tilefg);
  unsigned *ka = (unsigned*)(w + lay.lv_key[0]), *kb = (unsigned*)(w + lay.lv_key[1]);
  PL *pa = (PL*)(w + lay.lv_pay[0]), *pb = (PL*)(w + lay.lv_pay[1]);
  float *hdr = (float*)(w + SEG_HDR), *hplane = (float*)kb;
  const LovaszCfg cfg{c.weight, c.base_weight, c.skip_absent != 0};
  hipMemsetAsync(gc, 0, (size_t)nseg * 4, st);
  hipLaunchKernelGGL(seg_lovasz_count_kernel, dim3((unsigned)nblk), dim3(256), 0, st, tg, d, ig, bpk, blkcnt);
  hipLaunchKernelGGL(seg_lovasz_offsets_kernel, dim3((unsigned)G), dim3(256), 0, st, (const int*)blkcnt, ppg, blkoff, nvalid);
  hipLaunchKernelGGL(seg_lovasz_keys_kernel<PL>, dim3((unsigned)nblk), dim3(256), 0, st, rows, d, tg, ig, bpk, c.per_image, (const int*)blkoff, ka, pa, gc, bad);
  hipLaunchKernelGGL(seg_lovasz_plan_kernel, dim3(1), dim3(256), 0, st, (const int*)gc, (const int*)nvalid, G, d.nc, q.ng, cfg, c.region_class_weight, coef,
                     (long long*)(w + lay.lv_segtab));
  lv_sort<PL>(ka, pa, kb, pb, q, nseg, nvalid, gc, tilehist, binbase, st);
  hipLaunchKernelGGL(seg_lovasz_flagsum_kernel<PL>, dim3(tiles), dim3(256), 0, st, (const PL*)pa, q, (const int*)nvalid, (const int*)gc, tilefg);
  hipLaunchKernelGGL(seg_lovasz_flagscan_kernel, dim3((unsigned)nseg), dim3(256), 0, st, q, (const int*)nvalid, (const int*)gc, tilefg);
  if (ch)
    hipLaunchKernelGGL((seg_lovasz_value_kernel<PL, true>), dim3(tiles), dim3(256), 0, st, (const unsigned*)ka, (const PL*)pa, q, (const int*)nvalid,
                       (const int*)gc, (const unsigned*)tilefg, (const double*)coef, c.per_image, plane, hplane, part);
  else
    hipLaunchKernelGGL((seg_lovasz_value_kernel<PL, false>), dim3(tiles), dim3(256), 0, st, (const unsigned*)ka, (const PL*)pa, q, (const int*)nvalid,
                       (const int*)gc, (const unsigned*)tilefg, (const double*)coef, c.per_image, plane, (float*)nullptr, part);
  hipLaunchKernelGGL(seg_lovasz_reduce_kernel, dim3((unsigned)nseg), dim3(256), 0, st, (const double*)part, q, (const int*)nvalid, (const int*)gc, L);
  hipLaunchKernelGGL(seg_lovasz_solve_kernel, dim3(1), dim3(256), 0, st, (const double*)L, (const int*)gc, G, d.nc, cfg, c.region_class_weight, base_loss,
                     ch ? ch->acc : nullptr, ch ? ch->norm_mode : 0, ch ? ch->norm_const : 1.0, ch ? hdr : nullptr, region_stats_out, loss_out);
  if (ch)
    hipLaunchKernelGGL(seg_lovasz_grad_kernel, dim3((unsigned)seg_pixel_blocks(seg_npix(d))), dim3(256), 0, st, rows, d, tg, ig, (const float*)hplane,
                       (const double*)coef, c.per_image, (const float*)hdr, ch->acc != nullptr, ch->dlogits);
}

// The checks every entry makes; null when the arguments are good.
const char* seg_check(const cvx_seg_dims* dp, const cvx_seg_criterion* cp, bool for_eval) {
  if (!dp || !cp) return "null arguments";
  const cvx_seg_dims& d = *dp;
  const cvx_seg_criterion& c = *cp;
  if (!(d.batch > 0 && d.nc > 0 && d.nc <= SEG_MAX_NC && d.nc <= d.ld && d.ld <= 4096 && d.ih > 0 && d.iw > 0 && d.oh > 0 && d.ow > 0)) return "bad sizes";
  if (!(seg_pixel_blocks(seg_npix(d)) < (1LL << 31))) return "too many pixels / columns";
  if (!(c.base >= 0 && c.base <= 2)) return "base: 0 none, 1 focal, 2 cross-entropy";
  if (seg_with_options(c) && c.base != 2) return "class_weight, label_smoothing and OHEM are options of base 2 (cross-entropy)";
  if (!(c.label_smoothing >= 0.f && c.label_smoothing < 1.f)) return "label_smoothing in [0, 1)";
  if (!for_eval && seg_ohem(c)) {
    if (!(c.ohem_min_kept >= 1 && isfinite(c.ohem_theta))) return "OHEM: thresh in (0, 1], min_kept >= 1";
    if (!(seg_npix(d) < (1LL << 31))) return "OHEM counts pixels in 32 bits";
  }
  if (!c.region) return c.base != 0 ? nullptr : "base 0 takes a region term";
  if (!(d.nc <= REGION_MAX_NC)) return "the region losses take at most 1024 classes";
  if (!(c.region == 1 || c.region == 2)) return "region: 0 none, 1 Dice / Tversky, 2 Lovasz-Softmax";
  if (!(isfinite(c.weight) && c.weight > 0.0 && isfinite(c.base_weight) && c.base_weight >= 0.0)) return "weight > 0, base_weight >= 0";
  if (c.region == 2) {
    if ((c.base != 0) != (c.base_weight > 0.0)) return "a base term needs base_weight > 0, and base_weight = 0 takes base = 0";
    const long long ng = seg_lovasz_ng(d, c);
    if (!(ng < (1LL << 31))) return "the Lovasz term takes groups of fewer than 2^31 pixels";
    if (!((long long)(c.per_image ? d.batch : 1) * d.nc * cvx_cdiv(ng, LV_TILE) < (1LL << 31))) return "too many sort tiles";
    return nullptr;
  }
  if (!(isfinite(c.alpha) && c.alpha >= 0.0 && isfinite(c.beta) && c.beta >= 0.0 && isfinite(c.gamma) && c.gamma > 0.0 && isfinite(c.smooth) && c.smooth >= 0.0))
    return "alpha, beta, smooth >= 0 and gamma > 0";
  if ((c.base != 0) != (c.base_weight > 0.0)) return "a base term needs base_weight > 0, and base_weight = 0 takes base = 0";
  if (!((long long)d.batch * seg_region_bpi(d) < (1LL << 31))) return "too many pixels";
  return nullptr;
}

}  // namespace

extern "C" int64_t cvx_seg_criterion_workspace_bytes(const cvx_seg_dims* dims, const cvx_seg_criterion* crit, int32_t for_eval) {
  if (seg_check(dims, crit, for_eval != 0)) return 0;
  return (int64_t)SegLayout(*dims, *crit, for_eval != 0).total;
}

extern "C" int cvx_seg_criterion_lovasz_view(const cvx_seg_dims* dims, const cvx_seg_criterion* crit, int64_t offsets_out[3]) {
  CVX_CHECK(offsets_out != nullptr, "null arguments");
  const char* why = seg_check(dims, crit, false);
  CVX_CHECK(why == nullptr, why);
  CVX_CHECK(crit->region == 2, "the criterion has no Lovasz term");
  const SegLayout lay(*dims, *crit, false);
  offsets_out[0] = (int64_t)lay.lv_key[0];
  offsets_out[1] = (int64_t)lay.lv_pay[0];
  offsets_out[2] = (int64_t)lay.lv_segtab;
  return 0;
}

extern "C" int cvx_seg_criterion_loss(const float* rows_f32, const cvx_seg_dims* dims, const int64_t* target, const cvx_seg_criterion* crit,
                                      float loss_scale, float* loss_out, void* dpred_f16, int32_t* bad_target, double* stats_out,
                                      double* region_stats_out, void* workspace, void* hip_stream) {
  CVX_CHECK(rows_f32 && target && loss_out && dpred_f16 && bad_target && workspace, "null arguments");
  const char* why = seg_check(dims, crit, false);
  CVX_CHECK(why == nullptr, why);
  const cvx_seg_dims d = *dims;
  const cvx_seg_criterion c = *crit;
  CVX_CHECK(loss_scale > 0.f, "loss_scale must be positive");
  CVX_CHECK(!(c.base == 2 && seg_with_options(c)) || stats_out, "cross-entropy with options writes stats_out");
  CVX_CHECK(!c.region || region_stats_out, "a region term writes region_stats_out");
  hipStream_t st = (hipStream_t)hip_stream;
  const SegLayout lay(d, c, false);
  char* w = (char*)workspace;
  float* hdr = (float*)(w + SEG_HDR);
  const long long* tg = (const long long*)target;
  CVX_HIP(hipMemsetAsync(bad_target, 0, 4, st));
  SegChain ch{(float*)(w + lay.dlogits), nullptr, 0, 1.0};
  if (c.base != 0) ch = seg_base_chain(rows_f32, d, tg, c, lay, w, nullptr, c.region ? hdr + 1 : loss_out, bad_target, stats_out, st);
  if (c.region) {
    if (c.region == 2) seg_lovasz_chain<unsigned>(rows_f32, d, tg, c, lay, w, c.base != 0 ? hdr + 1 : nullptr, &ch, bad_target, region_stats_out, loss_out, st);
    else seg_region_chain(rows_f32, d, tg, c, lay, w, c.base != 0 ? hdr + 1 : nullptr, &ch, bad_target, region_stats_out, loss_out, st);
    ch = SegChain{ch.dlogits, nullptr, 0, 1.0};  // R4 / L10 left the plane normalised
  }
  launch_adjoint(ch, d, loss_scale, dpred_f16, st);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_seg_criterion_eval(const float* rows_f32, const cvx_seg_dims* dims, const int64_t* target, const cvx_seg_criterion* crit,
                                      int64_t* confusion, float* loss_out, double* region_stats_out, void* workspace, void* hip_stream) {
  CVX_CHECK(rows_f32 && target && confusion && loss_out && workspace, "null arguments");
  const char* why = seg_check(dims, crit, true);
  CVX_CHECK(why == nullptr, why);
  const cvx_seg_dims d = *dims;
  const cvx_seg_criterion c = *crit;
  CVX_CHECK(!c.region || region_stats_out, "a region term writes region_stats_out");
  hipStream_t st = (hipStream_t)hip_stream;
  const SegLayout lay(d, c, true);
  char* w = (char*)workspace;
  const long long* tg = (const long long*)target;
  seg_base_chain(rows_f32, d, tg, c, lay, w, (unsigned long long*)confusion, loss_out, nullptr, nullptr, st);
  if (c.region) {
    int32_t* bad = (int32_t*)(w + SEG_HDR + 8);  // R1 raises it; evaluation does not report it
    CVX_HIP(hipMemsetAsync(bad, 0, 4, st));
    if (c.region == 2) seg_lovasz_chain<unsigned char>(rows_f32, d, tg, c, lay, w, c.base != 0 ? loss_out : nullptr, nullptr, bad, region_stats_out, loss_out, st);
    else seg_region_chain(rows_f32, d, tg, c, lay, w, c.base != 0 ? loss_out : nullptr, nullptr, bad, region_stats_out, loss_out, st);
  }
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_resize_bilinear_nchw_grad_to_rows(const float* grad_nchw, int32_t batch, int32_t nc, int32_t ih, int32_t iw, int32_t oh,
                                                     int32_t ow, float scale, void* dpred_f16, int32_t ld, void* hip_stream) {
  CVX_CHECK(grad_nchw && dpred_f16 && batch > 0 && nc > 0 && nc <= ld && ih > 0 && iw > 0 && oh > 0 && ow > 0, "bad arguments");
  CVX_CHECK(ld <= 4096, "too many columns");
  launch_adjoint(SegChain{const_cast<float*>(grad_nchw), nullptr, 0, 1.0}, cvx_seg_dims{ld, batch, nc, ih, iw, oh, ow}, scale, dpred_f16,
                 (hipStream_t)hip_stream);
  CVX_HIP(hipGetLastError());
  return 0;
}
