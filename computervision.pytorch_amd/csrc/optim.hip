// The optimiser steps of the library (gfx950): Adam as FlatAdam runs it (cvx_adam_step, cvx_adam_step_dev, cvx_adam_ema_step_dev), and the
// steps that know about parameter groups (cvx_optim_step): SGD with momentum / Nesterov and coupled weight decay, Adam with decoupled weight
// decay (AdamW), frozen groups, clipping by the global gradient norm.  All of them are ONE streaming kernel body over the flat fp32 arenas,
// optim_step_kernel<KIND, EMA, GROUPED>: 16-byte accesses, a scalar tail for n % 4 != 0, the weight average in the same pass when EMA.  The
// per-element arithmetic is optim_core.h's.  The average as a pass of its own (cvx_ema_update) and the finite check (cvx_check_finite) live
// here too.
//
// GROUPED: which group an element belongs to comes from one byte per 16-byte chunk (arena offsets and sizes are multiples of 4 floats, so a
// chunk belongs to at most one parameter): a group id below n_groups, or anything else (255 by convention) for "no trainable parameter here:
// do not touch".  The per-group hyper-parameters live in a device table the host writes only when a learning rate changes, the step count in
// the device step state, so a captured graph of the whole train step replays without a changed kernel argument.
// Not GROUPED (Adam only): every element is live, there is no map, no table, no decay and no clip state; lr/(1-b1^t) and 1/sqrt(1-b2^t) come
// from the device state, or by value when there is none (cvx_adam_step).
#include <algorithm>
#include "optim_core.h"
#include "../../include/cvx_engine.h"

namespace {

constexpr int GS = CVX_OPTIM_GROUP_FLOATS;
enum { G_LR = 0, G_DECAY_COUPLED = 1, G_DECAY_FACTOR = 2, G_FROZEN = 3, G_MOMENTUM = 4, G_NESTEROV = 5, G_LR_BC1 = 6 };

__device__ __forceinline__ bool step_skipped(const int* found_inf, const float* clip) {
  return (found_inf && *found_inf != 0) || (clip && clip[2] != 0.f);
}

// state[0] = lr (host-written; with groups, group 0's), state[1] = step count (all groups share it), state[2] = state[0]/(1-b1^t),
// state[3] = 1/sqrt(1-b2^t); per group lr/(1-b1^t) in the table.  G = 0: no groups.  A one-group ADAM run keeps the state an ungrouped one keeps.
__global__ void optim_advance_kernel(float* state, float* gs, int G, int kind, float b1, float b2, const int* found_inf, const float* clip) {
  if (step_skipped(found_inf, clip)) return;  // a skipped step does not advance the bias correction
  const float t = state[1] + 1.f;
  state[1] = t;
  if (kind != CVX_OPTIM_ADAM) return;
  const float bc1 = 1.f - powf(b1, t);
  for (int k = 0; k < G; ++k) gs[k * GS + G_LR_BC1] = gs[k * GS + G_LR] / bc1;
  if (G) state[0] = gs[G_LR];
  state[2] = state[0] / bc1;
  state[3] = rsqrtf(1.f - powf(b2, t));
}

// g1 = rn(g * grad_scale); with a clip state g2 = rn(g1 * coef)
__device__ __forceinline__ float scaled_grad(float g, float gscale, bool clipped, float coef) {
#pragma clang fp contract(off)
  float x = g * gscale;
  if (clipped) x = x * coef;
  return x;
}

// torch.optim.SGD with dampening 0, every operation rounded on its own:
// g3 = rn(g2 + rn(lam*p)); b = rn(rn(mu*b) + g3); d = nesterov ? rn(g3 + rn(mu*b)) : b; p = rn(p - rn(lr*d))
__device__ __forceinline__ void sgd_step(float& p, float& b, float g2, float lr, float lam, float mu, bool nesterov) {
#pragma clang fp contract(off)
  const float dp = lam * p;
  const float g3 = g2 + dp;
  const float mb = mu * b;
  b = mb + g3;
  const float mb2 = mu * b;
  const float look = g3 + mb2;
  const float d = nesterov ? look : b;
  const float upd = lr * d;
  p = p - upd;
}

// AdamW's param.mul_(1 - lr * wd): one rounded multiply by the factor the host formed in double
__device__ __forceinline__ float decay_mul(float p, float factor) {
#pragma clang fp contract(off)
  return p * factor;
}

// q: the element's row of the group table (GROUPED), else unused: lr_over_bc1 is the learning rate over the bias correction then
template <int KIND, bool GROUPED, bool TAIL>
__device__ __forceinline__ void elem_step(float& p, float& a, float& b, float g, const float* q, float gscale, bool clipped, float coef, float b1,
                                          float b2, float eps, float lr_over_bc1, float inv_sqrt_bc2) {
  const float g2 = scaled_grad(g, gscale, GROUPED && clipped, coef);
  if (KIND == CVX_OPTIM_SGD) {
    sgd_step(p, a, g2, q[G_LR], q[G_DECAY_COUPLED], q[G_MOMENTUM], q[G_NESTEROV] != 0.f);
  } else {
    if (GROUPED) {
      p = decay_mul(p, q[G_DECAY_FACTOR]);
      lr_over_bc1 = q[G_LR_BC1];
    }
    if (TAIL)
      adam_step1(p, a, b, g2, b1, b2, eps, lr_over_bc1, inv_sqrt_bc2);
    else
      adam_step4(p, a, b, g2, b1, b2, eps, lr_over_bc1, inv_sqrt_bc2);
  }
}

// a = momentum buffer (SGD) or exp_avg (ADAM), b = exp_avg_sq (ADAM only).  One 16-byte chunk per thread.  Not GROUPED: map, gs and clip are
// not read, and lr_over_bc1 / inv_sqrt_bc2 hold when state is null.  A skipped step leaves p, a, b alone, still zeroes g when asked and still
// moves the average (toward the unchanged p).
template <int KIND, bool EMA, bool GROUPED>
__global__ __launch_bounds__(256) void optim_step_kernel(float* p, float* g, float* a, float* b, long long n, const uint8_t* map, const float* gs,
                                                         int G, const float* state, float lr_over_bc1, float inv_sqrt_bc2, float b1, float b2,
                                                         float eps, const int* found_inf, int zero_grad, float gscale, const float* clip, float* e,
                                                         float d, float omd) {
  static_assert(GROUPED || KIND == CVX_OPTIM_ADAM, "SGD keeps its hyper-parameters in the group table");
  __shared__ float sg[GROUPED ? CVX_OPTIM_MAX_GROUPS * GS : 1];
  if (GROUPED) {
    if ((int)threadIdx.x < G * GS) sg[threadIdx.x] = gs[threadIdx.x];
    __syncthreads();
  }
  const bool skip = step_skipped(found_inf, GROUPED ? clip : nullptr);
  const bool clipped = GROUPED && clip != nullptr;
  const float coef = clipped ? clip[1] : 1.f;
  if (KIND == CVX_OPTIM_ADAM && state) {  // device-resident step state (hipGraph replay: no host-side arguments change between steps)
    lr_over_bc1 = state[2];
    inv_sqrt_bc2 = state[3];
  }
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  const int k = GROUPED ? map[i >> 2] : 0;
  const bool mapped = !GROUPED || k < G;  // 255, and any id the host failed to refuse, is left alone
  const float* q = sg + (mapped ? k : 0) * GS;
  const bool live = mapped && (!GROUPED || q[G_FROZEN] == 0.f) && !skip;
  const bool avg = EMA && mapped;
  if (i + 4 <= n) {
    if (live || avg) {
      f4 pp = *reinterpret_cast<f4*>(p + i);
      if (live) {
        const f4 gg = *reinterpret_cast<f4*>(g + i);
        f4 aa = *reinterpret_cast<f4*>(a + i), bb = f4{0.f, 0.f, 0.f, 0.f};
        if (KIND == CVX_OPTIM_ADAM) bb = *reinterpret_cast<f4*>(b + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float pj = pp[j], aj = aa[j], bj = bb[j];
          elem_step<KIND, GROUPED, false>(pj, aj, bj, gg[j], q, gscale, clipped, coef, b1, b2, eps, lr_over_bc1, inv_sqrt_bc2);
          pp[j] = pj;
          aa[j] = aj;
          bb[j] = bj;
        }
        *reinterpret_cast<f4*>(p + i) = pp;
        *reinterpret_cast<f4*>(a + i) = aa;
        if (KIND == CVX_OPTIM_ADAM) *reinterpret_cast<f4*>(b + i) = bb;
      }
      if (avg) {
        f4 ee = *reinterpret_cast<f4*>(e + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) ee[j] = ema_mix(ee[j], pp[j], d, omd);
        *reinterpret_cast<f4*>(e + i) = ee;
      }
    }
    if (zero_grad) *reinterpret_cast<f4*>(g + i) = f4{0.f, 0.f, 0.f, 0.f};
  } else {
    for (; i < n; ++i) {
      if (live || avg) {
        float pj = p[i];
        if (live) {
          float aj = a[i], bj = KIND == CVX_OPTIM_ADAM ? b[i] : 0.f;
          elem_step<KIND, GROUPED, true>(pj, aj, bj, g[i], q, gscale, clipped, coef, b1, b2, eps, lr_over_bc1, inv_sqrt_bc2);
          p[i] = pj;
          a[i] = aj;
          if (KIND == CVX_OPTIM_ADAM) b[i] = bj;
        }
        if (avg) e[i] = ema_mix(e[i], pj, d, omd);
      }
      if (zero_grad) g[i] = 0.f;
    }
  }
}

// The average as a pass of its own (BatchNorm statistics; parameters when no optimiser step is fused with it): 16-byte vectors, scalar tail.
__global__ __launch_bounds__(256) void ema_update_kernel(float* e, const float* p, long long n, float d, float omd) {
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n) {
    f4 ee = *reinterpret_cast<f4*>(e + i);
    const f4 pp = *reinterpret_cast<const f4*>(p + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) ee[k] = ema_mix(ee[k], pp[k], d, omd);
    *reinterpret_cast<f4*>(e + i) = ee;
  } else {
    for (; i < n; ++i) e[i] = ema_mix(e[i], p[i], d, omd);
  }
}

__global__ __launch_bounds__(256) void check_finite_kernel(const float* g, long long n, int* found_inf) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  bool bad = false;
  for (; i < n; i += stride) {
    float x = g[i];
    bad |= !(fabsf(x) <= 3.0e38f);
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) *found_inf = 1;
}

// ---- global gradient norm: sum of squares of grad_scale * g over the live chunks, two stages, no floating-point atomics -------------------
// Stage 1: a grid that depends on n alone, every workgroup strides over the chunks and leaves ONE partial; stage 2: one workgroup adds the
// partials in a fixed order.  The partition and both trees are fixed, so two runs over the same input give the same bits.
constexpr int NORM_MAX_BLOCKS = 1024, NORM_CHUNKS_PER_THREAD = 4;

int norm_blocks(long long n) {
  const long long chunks = (n + 3) / 4, per_block = 256LL * NORM_CHUNKS_PER_THREAD;
  const long long blocks = (chunks + per_block - 1) / per_block;
  return (int)(blocks < 1 ? 1 : blocks > NORM_MAX_BLOCKS ? NORM_MAX_BLOCKS : blocks);
}

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* g, long long n, const uint8_t* map, const float* gs, int G, float gscale,
                                                                float* partials) {
  __shared__ float frozen[CVX_OPTIM_MAX_GROUPS];
  __shared__ float wsum[4];
  if (threadIdx.x < CVX_OPTIM_MAX_GROUPS) frozen[threadIdx.x] = (int)threadIdx.x < G ? gs[threadIdx.x * GS + G_FROZEN] : 1.f;
  __syncthreads();
  const long long chunks = (n + 3) >> 2, stride = (long long)gridDim.x * blockDim.x;
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
    const int k = map[c];
    if (k >= G || frozen[k] != 0.f) continue;
    long long i = c * 4;
    if (i + 4 <= n) {
      const f4 x = *reinterpret_cast<const f4*>(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float s = x[j] * gscale;
        acc[j] = __builtin_fmaf(s, s, acc[j]);
      }
    } else {
      for (int j = 0; i < n; ++i, ++j) {
        const float s = g[i] * gscale;
        acc[j] = __builtin_fmaf(s, s, acc[j]);
      }
    }
  }
  float t = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  t = cvx_wave_sum64(t);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// clip[0] = norm, clip[1] = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), clip[2] = 1 when the norm is not finite
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const float* partials, int nparts, float max_norm, float* clip, int* found_inf) {
  __shared__ float s[256];
  float acc = 0.f;
  for (int j = threadIdx.x; j < nparts; j += 256) acc += partials[j];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float norm = sqrtf(s[0]);
  const bool bad = !(norm <= 3.0e38f);
  const float den = norm + 1e-6f;
  clip[0] = norm;
  clip[1] = bad ? 0.f : fminf(1.f, max_norm / den);
  clip[2] = bad ? 1.f : 0.f;
  if (bad && found_inf) *found_inf = 1;
}

template <typename K, typename... Args>
int launch_chunks(K kern, long long n, hipStream_t st, Args... args) {
  hipLaunchKernelGGL(kern, dim3(cvx_cdiv((n + 3) / 4, 256)), dim3(256), 0, st, args...);
  CVX_HIP(hipGetLastError());
  return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// the ungrouped Adam step: with a device state one advance launch in front of it, without one the two factors by value
int adam_ungrouped(float* p, float* g, float* m, float* v, long long n, float* state, float lr_over_bc1, float inv_sqrt_bc2, float b1, float b2,
                   float eps, const int* found_inf, int zero_grad, float gscale, float* e, float d, float omd, hipStream_t st) {
  if (state)
    hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, st, state, (float*)nullptr, 0, (int)CVX_OPTIM_ADAM, b1, b2, found_inf,
                       (const float*)nullptr);
#define CVX_ADAM_LAUNCH(E)                                                                                                                  \
  return launch_chunks(optim_step_kernel<CVX_OPTIM_ADAM, E, false>, n, st, p, g, m, v, n, (const uint8_t*)nullptr, (const float*)nullptr, 0, \
                       (const float*)state, lr_over_bc1, inv_sqrt_bc2, b1, b2, eps, found_inf, zero_grad, gscale, (const float*)nullptr, e, d, omd)
  if (e) CVX_ADAM_LAUNCH(true);
  CVX_ADAM_LAUNCH(false);
#undef CVX_ADAM_LAUNCH
}

}  // namespace

// Adam (torch.optim.Adam defaults semantics, no weight decay / amsgrad), fp32 state; optionally skipped when *found_inf != 0; zeroes the
// gradient arena afterwards when zero_grad != 0.
extern "C" int cvx_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                             float eps, int32_t step, const int32_t* found_inf, int32_t zero_grad, void* hip_stream) {
  CVX_CHECK(params && grads && exp_avg && exp_avg_sq && n > 0, "bad arguments");
  CVX_CHECK(aligned16(params) && aligned16(grads) && aligned16(exp_avg) && aligned16(exp_avg_sq), "adam arenas must be 16-byte aligned");
  CVX_CHECK(step >= 1, "adam: step starts at 1");
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  return adam_ungrouped(params, grads, exp_avg, exp_avg_sq, n, nullptr, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)), beta1, beta2, eps, found_inf,
                        zero_grad, 1.0f, nullptr, 0.f, 0.f, (hipStream_t)hip_stream);
}
// same update with the step state on the device (state[0]=lr, [1]=step, [2],[3] derived): replayable from a hipGraph
extern "C" int cvx_adam_step_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1, float beta2, float eps,
                                 float* state, const int32_t* found_inf, int32_t zero_grad, float grad_scale, void* hip_stream) {
  CVX_CHECK(params && grads && exp_avg && exp_avg_sq && state && n > 0, "bad arguments");
  return adam_ungrouped(params, grads, exp_avg, exp_avg_sq, n, state, 0.f, 0.f, beta1, beta2, eps, found_inf, zero_grad, grad_scale, nullptr, 0.f,
                        0.f, (hipStream_t)hip_stream);
}
// cvx_adam_step_dev plus the weight average in the same pass: e <- rn(rn(e * d) + rn(omd * p_new)); on a skipped step e moves toward the unchanged p
extern "C" int cvx_adam_ema_step_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1, float beta2,
                                     float eps, float* state, const int32_t* found_inf, int32_t zero_grad, float grad_scale, float* ema, float d,
                                     float one_minus_d, void* hip_stream) {
  CVX_CHECK(params && grads && exp_avg && exp_avg_sq && state && ema && n > 0, "bad arguments");
  CVX_CHECK(ema != params, "the average must not be the arena it follows");
  CVX_CHECK(aligned16(params) && aligned16(grads) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(ema),
            "adam arenas must be 16-byte aligned");
  return adam_ungrouped(params, grads, exp_avg, exp_avg_sq, n, state, 0.f, 0.f, beta1, beta2, eps, found_inf, zero_grad, grad_scale, ema, d,
                        one_minus_d, (hipStream_t)hip_stream);
}
// the average alone: ema <- rn(rn(ema * d) + rn(one_minus_d * src)) over n floats
extern "C" int cvx_ema_update(float* ema, const float* src, int64_t n, float d, float one_minus_d, void* hip_stream) {
  CVX_CHECK(ema && src && n > 0, "bad arguments");
  CVX_CHECK(ema != src, "the average must not be the arena it follows");
  CVX_CHECK(aligned16(ema) && aligned16(src), "ema arenas must be 16-byte aligned");
  return launch_chunks(ema_update_kernel, n, (hipStream_t)hip_stream, ema, src, (long long)n, d, one_minus_d);
}
// sets *found_inf = 1 if any gradient is non-finite
extern "C" int cvx_check_finite(const float* grads, int64_t n, int32_t* found_inf, void* hip_stream) {
  CVX_CHECK(grads && found_inf, "bad arguments");
  if (n <= 0) return 0;
  const int blocks = (int)std::min<long long>(1024, (n + 255) / 256);
  hipLaunchKernelGGL(check_finite_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, grads, (long long)n, found_inf);
  CVX_HIP(hipGetLastError());
  return 0;
}

extern "C" int cvx_optim_step(int32_t kind, float* params, float* grads, float* buf1, float* buf2, int64_t n, const uint8_t* group_map,
                              float* group_state, int32_t n_groups, float* state, float beta1, float beta2, float eps, const int32_t* found_inf,
                              int32_t zero_grad, float grad_scale, const float* clip_state, float* ema, float d, float one_minus_d,
                              void* hip_stream) {
  CVX_CHECK(kind == CVX_OPTIM_SGD || kind == CVX_OPTIM_ADAM, "kind: CVX_OPTIM_SGD or CVX_OPTIM_ADAM");
  CVX_CHECK(params && grads && buf1 && group_map && group_state && state && n > 0, "bad arguments");
  CVX_CHECK(n_groups >= 1 && n_groups <= CVX_OPTIM_MAX_GROUPS, "1 <= n_groups <= 16: the group table is staged in LDS and ids are bytes");
  CVX_CHECK(kind != CVX_OPTIM_ADAM || buf2, "the ADAM kind needs buf2 (exp_avg_sq)");
  CVX_CHECK(aligned16(params) && aligned16(grads) && aligned16(buf1) && aligned16(buf2) && aligned16(ema), "optimiser arenas must be 16-byte aligned");
  CVX_CHECK(ema != params, "the average must not be the arena it follows");
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, st, state, group_state, n_groups, kind, beta1, beta2, found_inf, clip_state);
#define CVX_OPTIM_LAUNCH(K, E)                                                                                                                  \
  return launch_chunks(optim_step_kernel<K, E, true>, n, st, params, grads, buf1, buf2, (long long)n, group_map, (const float*)group_state, n_groups, \
                       (const float*)state, 0.f, 0.f, beta1, beta2, eps, found_inf, zero_grad, grad_scale, clip_state, ema, d, one_minus_d)
  if (kind == CVX_OPTIM_SGD) {
    if (ema) CVX_OPTIM_LAUNCH(CVX_OPTIM_SGD, true);
    CVX_OPTIM_LAUNCH(CVX_OPTIM_SGD, false);
  }
  if (ema) CVX_OPTIM_LAUNCH(CVX_OPTIM_ADAM, true);
  CVX_OPTIM_LAUNCH(CVX_OPTIM_ADAM, false);
#undef CVX_OPTIM_LAUNCH
}

extern "C" int64_t cvx_grad_norm_workspace(int64_t n) { return n > 0 ? norm_blocks(n) : 0; }

extern "C" int cvx_grad_norm(const float* grads, int64_t n, const uint8_t* group_map, const float* group_state, int32_t n_groups, float grad_scale,
                             float max_norm, float* clip_state, int32_t* found_inf, float* workspace, int64_t workspace_floats, void* hip_stream) {
  CVX_CHECK(grads && group_map && group_state && clip_state && workspace && n > 0, "bad arguments");
  CVX_CHECK(n_groups >= 1 && n_groups <= CVX_OPTIM_MAX_GROUPS, "1 <= n_groups <= 16: the group table is staged in LDS and ids are bytes");
  CVX_CHECK(aligned16(grads), "the gradient arena must be 16-byte aligned");
  CVX_CHECK(max_norm > 0.f, "max_norm must be positive");
  const int blocks = norm_blocks(n);
  CVX_CHECK(workspace_floats >= blocks, "workspace too small: cvx_grad_norm_workspace(n) = " + std::to_string(blocks) + " floats");
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(blocks), dim3(256), 0, st, grads, (long long)n, group_map, group_state, n_groups, grad_scale,
                     workspace);
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, blocks, max_norm, clip_state, found_inf);
  CVX_HIP(hipGetLastError());
  return 0;
}
