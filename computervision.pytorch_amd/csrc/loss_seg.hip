// Segmentation loss of the DeepLabv3+ trainer on gfx950: bilinear upsampling of the decoder's logits to the label resolution,
// cross-entropy / focal loss per pixel, and the gradient w.r.t. the LOW-RESOLUTION logits rows the engine's backward pass starts
// from -- value and gradient in one pass chain, no autograd tape and no (B, nc, H, W) logits tensor in HBM.
//
// Reference semantics (file:line under the reference tree):
//   DeeplabV3Plus.forward        core/models/deeplabv3plus.py:143-148   x = F.interpolate(classifier(features), size=input, bilinear,
//                                                                       align_corners=False)
//   FocalLoss.forward            core/loss/focal_loss.py:14-22          ce = F.cross_entropy(x, t, ignore_index, reduction="none");
//                                                                       pt = exp(-ce); loss = alpha * (1 - pt)^gamma * ce; mean()
//   DeeplabV3PlusA.build_loss    core/algorithms/segmentation_2d.py:59-64  "focal" -> FocalLoss() (alpha 0.25, gamma 2, ignore -100),
//                                                                       "ce" -> nn.CrossEntropyLoss(reduction="mean")
//   train_loop                   core/trainer/segmentation_trainer.py:114-131
//
//   K1 seg_loss_pixel   one thread per label pixel: interpolate the nc logits from the four source rows (fp32, the forward
//                       kernel's arithmetic), log-softmax, loss value -> block partial sums, d loss / d logit (times
//                       grad_scale / normaliser) -> dlogits (B, nc, OH, OW) fp32
//   K2 resize_grad_rows adjoint of the bilinear resize as a gather (deterministic): one thread per (image, class, source pixel)
//                       collects the label pixels that interpolate from it -> dpred (B, ih*iw, ld) fp16
//   K3 finalize         loss = sum / normaliser
//
// Evaluation (cvx_seg_eval, the reference's evaluate_loop, segmentation_trainer.py:133-159, and evaluate_on_voc,
// segmentation_2d.py:146-157): seg_eval_kernel walks the label pixels the same way -- the same taps, the same online softmax, the same
// loss definitions -- and keeps the arg max instead of a gradient: confusion[target][argmax] += 1 and the batch's criterion value, with
// no (B, nc, H, W) tensor and no gradient written.  K3 finishes its loss sum.  The LDS histogram is seg_tail.h's.
//
// The taps, the class loop, the block sums, K2 and K3 live in seg_loss_core.h, which loss_seg_opts.hip (class weights, label smoothing,
// hard-pixel mining) includes too.
#include "seg_loss_core.h"
#include "seg_loss_chain.h"
#include "../../include/cvx_engine.h"

namespace {

// The criterion's value of one valid pixel from its cross-entropy, and d loss / d ce.
__device__ __forceinline__ float pixel_loss(float ce, int mode, float alpha, float gamma, float* coef) {
  if (mode == 0) {
    const float pt = expf(-ce);
    const float om = fmaxf(1.f - pt, 0.f);
    const float w = powf(om, gamma);
    // d/dce [alpha (1 - pt)^gamma ce], d pt / d ce = -pt
    *coef = alpha * (w + (gamma > 0.f ? gamma * powf(om, gamma - 1.f) * pt * ce : 0.f));
    return alpha * w * ce;
  }
  *coef = 1.f;
  return ce;
}

// mode 0: focal (alpha, gamma), mean over ALL pixels (ignored ones count in the denominator: focal_loss.mean());
// mode 1: cross-entropy, mean over the non-ignored pixels (nn.CrossEntropyLoss(reduction="mean")): normalised by K3 / K2's scale
__global__ __launch_bounds__(256) void seg_loss_pixel_kernel(const float* rows, int ld, int B, int nc, int ih, int iw, int OH, int OW,
                                                             const long long* target, int mode, float alpha, float gamma, long long ignore_index,
                                                             float* dlogits, double* part /* per block: loss sum, valid pixels */, int* bad) {
  __shared__ double s_sum[4], s_cnt[4];
  const long long n = (long long)B * OH * OW;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  double my_loss = 0.0, my_cnt = 0.0;
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
    // pass 1: running maximum and rescaled sum of exponentials (no per-thread array: the class count is a run-time value)
    const bool vec = (ld & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
    float zmax = -INFINITY, se = 0.f, zt = 0.f;
    auto online = [&](int c, float z) {
      if (c == (int)tg) zt = z;
      if (z > zmax) {
        se = se * expf(zmax - z) + 1.f;
        zmax = z;
      } else {
        se += expf(z - zmax);
      }
    };
    each_logit(tp, nc, vec, online);
    const float lse = zmax + logf(se);
    float coef = 0.f;  // d loss / d ce
    if (valid) {
      my_loss = (double)pixel_loss(lse - zt, mode, alpha, gamma, &coef);
      my_cnt = 1.0;
    }
    float* dl = dlogits + (long long)b * nc * OH * OW + (long long)oy * OW + ox;
    auto emit = [&](int c, float z) {
      const float p = expf(z - lse);
      dl[(long long)c * OH * OW] = valid ? coef * (p - (c == (int)tg ? 1.f : 0.f)) : 0.f;
    };
    each_logit(tp, nc, vec, emit);
  }
  block_pair_to_part(my_loss, my_cnt, s_sum, s_cnt, part);
}

// Evaluation: EV_PIX label pixels per thread (chunks of 256 consecutive pixels, so a wave still reads along x), the arg max of the
// interpolated logits (strict >, so the lowest class wins a tie, like torch.argmax) counted against the target, and the criterion's
// value as in seg_loss_pixel_kernel.  LDS_HIST: the workgroup counts in nc * nc uint32 cells of LDS (nc <= 90: 32 KB) and adds its
// non-zero cells to the global int64 matrix once at the end; otherwise every pixel goes to the global matrix directly.
template <bool LDS_HIST>
__global__ __launch_bounds__(256) void seg_eval_kernel(const float* rows, int ld, int B, int nc, int ih, int iw, int OH, int OW,
                                                       const long long* target, int mode, float alpha, float gamma, long long ignore_index,
                                                       unsigned long long* confusion, double* part) {
  extern __shared__ unsigned int hist[];
  __shared__ double s_sum[4], s_cnt[4];
  if (LDS_HIST) {
    hist_zero<256>(hist, nc);
    __syncthreads();
  }
  const long long n = (long long)B * OH * OW;
  const bool vec = (ld & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;
  double my_loss = 0.0, my_cnt = 0.0;
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
    float zmax = -INFINITY, se = 0.f, zt = 0.f;
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
    });
    if (valid) {
      float coef;
      my_loss += (double)pixel_loss(zmax + logf(se) - zt, mode, alpha, gamma, &coef);
      my_cnt += 1.0;
    }
    if (in_range) {
      if (LDS_HIST) hist_add(hist, nc, (int)tg, arg);
      else atomicAdd(confusion + (int)tg * nc + arg, 1ull);
    }
  }
  if (LDS_HIST) hist_flush<256>(hist, nc, confusion);
  block_pair_to_part(my_loss, my_cnt, s_sum, s_cnt, part);
}

}  // namespace

static long long seg_pixel_blocks(long long npix) { return cvx_cdiv(npix, 256); }
extern "C" int64_t cvx_seg_loss_workspace_bytes(int32_t batch, int32_t nc, int32_t oh, int32_t ow) {
  // 64 B of totals, the per-workgroup (loss, count) pairs, the NCHW logit gradients
  return 64 + seg_pixel_blocks((long long)batch * oh * ow) * 16 + (int64_t)batch * nc * oh * ow * 4;
}

// The chain half of cvx_seg_loss (seg_loss_chain.h): K1 and K3, which leave the gradient plane and its normaliser on the device.
void seg_plain_chain(const float* rows_f32, int ld, int batch, int nc, int ih, int iw, int oh, int ow, const int64_t* target, int mode, float alpha,
                     float gamma, int64_t ignore_index, float* loss_out, int32_t* bad_target, void* workspace, hipStream_t st, SegChainOut* out) {
  const long long npix = (long long)batch * oh * ow;
  const long long nblk = seg_pixel_blocks(npix);
  double* acc = (double*)workspace;
  double* part = (double*)((char*)workspace + 64);
  float* dlogits = (float*)((char*)workspace + 64 + nblk * 16);
  hipLaunchKernelGGL(seg_loss_pixel_kernel, dim3((unsigned)nblk), dim3(256), 0, st, rows_f32, ld, batch, nc, ih, iw, oh, ow,
                     (const long long*)target, mode, alpha, gamma, (long long)ignore_index, dlogits, part, bad_target);
  hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(256), 0, st, part, (int)nblk, acc, mode, (double)npix, loss_out);
  *out = SegChainOut{dlogits, acc, mode, (double)npix};
}

extern "C" int cvx_seg_loss(const float* rows_f32, int32_t ld, int32_t batch, int32_t nc, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                            const int64_t* target, int32_t mode, float alpha, float gamma, int64_t ignore_index, float loss_scale,
                            float* loss_out, void* dpred_f16, int32_t* bad_target, void* workspace, void* hip_stream) {
  CVX_CHECK(rows_f32 && target && loss_out && dpred_f16 && bad_target && workspace, "null arguments");
  CVX_CHECK(batch > 0 && nc > 0 && nc <= SEG_MAX_NC && nc <= ld && ih > 0 && iw > 0 && oh > 0 && ow > 0, "bad sizes");
  CVX_CHECK(mode == 0 || mode == 1, "mode: 0 focal, 1 cross-entropy");
  CVX_CHECK(loss_scale > 0.f, "loss_scale must be positive");
  hipStream_t st = (hipStream_t)hip_stream;
  CVX_CHECK(seg_pixel_blocks((long long)batch * oh * ow) < (1LL << 31) && ld <= 4096, "too many pixels / columns");
  CVX_HIP(hipMemsetAsync(bad_target, 0, 4, st));
  SegChainOut ch;
  seg_plain_chain(rows_f32, ld, batch, nc, ih, iw, oh, ow, target, mode, alpha, gamma, ignore_index, loss_out, bad_target, workspace, st, &ch);
  const long long nlow = (long long)batch * ih * iw;
  hipLaunchKernelGGL(resize_grad_rows_kernel, dim3((unsigned)cvx_cdiv(nlow, RG_PIX)), dim3(256), (size_t)RG_PIX * ld * 2, st, ch.dlogits, batch, nc, ih, iw, oh,
                     ow, loss_scale, ch.norm_mode, ch.norm_const, ch.acc, (half_t*)dpred_f16, ld);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_resize_bilinear_nchw_grad_to_rows(const float* grad_nchw, int32_t batch, int32_t nc, int32_t ih, int32_t iw, int32_t oh,
                                                     int32_t ow, float scale, void* dpred_f16, int32_t ld, void* hip_stream) {
  CVX_CHECK(grad_nchw && dpred_f16 && batch > 0 && nc > 0 && nc <= ld && ih > 0 && iw > 0 && oh > 0 && ow > 0, "bad arguments");
  CVX_CHECK(ld <= 4096, "too many columns");
  const long long nlow = (long long)batch * ih * iw;
  hipLaunchKernelGGL(resize_grad_rows_kernel, dim3((unsigned)cvx_cdiv(nlow, RG_PIX)), dim3(256), (size_t)RG_PIX * ld * 2, (hipStream_t)hip_stream, grad_nchw,
                     batch, nc, ih, iw, oh, ow, scale, 0, 1.0, nullptr, (half_t*)dpred_f16, ld);
  CVX_HIP(hipGetLastError());
  return 0;
}

static long long seg_eval_blocks(long long npix) { return cvx_cdiv(npix, 256 * EV_PIX); }
extern "C" int64_t cvx_seg_eval_workspace_bytes(int32_t batch, int32_t oh, int32_t ow) {
  return 64 + seg_eval_blocks((long long)batch * oh * ow) * 16;  // totals, the per-workgroup (loss, count) pairs
}

extern "C" int cvx_seg_eval(const float* rows_f32, int32_t ld, int32_t batch, int32_t nc, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                            const int64_t* target, int32_t mode, float alpha, float gamma, int64_t ignore_index, int64_t* confusion,
                            float* loss_out, void* workspace, void* hip_stream) {
  CVX_CHECK(rows_f32 && target && confusion && loss_out && workspace, "null arguments");
  CVX_CHECK(batch > 0 && nc > 0 && nc <= SEG_MAX_NC && nc <= ld && ld <= 4096 && ih > 0 && iw > 0 && oh > 0 && ow > 0, "bad sizes");
  CVX_CHECK(mode == 0 || mode == 1, "mode: 0 focal, 1 cross-entropy");
  hipStream_t st = (hipStream_t)hip_stream;
  const long long npix = (long long)batch * oh * ow;
  const long long nblk = seg_eval_blocks(npix);
  CVX_CHECK(nblk < (1LL << 31), "too many pixels");
  double* acc = (double*)workspace;
  double* part = (double*)((char*)workspace + 64);
  if (nc * nc <= EV_LDS_CELLS)
    hipLaunchKernelGGL(seg_eval_kernel<true>, dim3((unsigned)nblk), dim3(256), (size_t)nc * nc * 4, st, rows_f32, ld, batch, nc, ih, iw, oh, ow,
                       (const long long*)target, mode, alpha, gamma, (long long)ignore_index, (unsigned long long*)confusion, part);
  else
    hipLaunchKernelGGL(seg_eval_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, st, rows_f32, ld, batch, nc, ih, iw, oh, ow,
                       (const long long*)target, mode, alpha, gamma, (long long)ignore_index, (unsigned long long*)confusion, part);
  hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(256), 0, st, part, (int)nblk, acc, mode, (double)npix, loss_out);
  CVX_HIP(hipGetLastError());
  return 0;
}
