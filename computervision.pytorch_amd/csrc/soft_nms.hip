// Soft-NMS on gfx950 (Bodla et al., ICCV 2017): the score of a box that overlaps a better one decays instead of the box disappearing.
// cvx_soft_nms is a sibling of cvx_nms_variant (nms.hip) with the same inputs and outputs; include/cvx_engine.h states the rules and
// tests/soft_nms_restatement.py restates them in numpy float32.  DESIGN.md section 7w has the budget and the timings.
//
// The decay makes the pick order depend on the scores as they change, so the suppression bit matrix and the single greedy walk of
// mask_nms.h do not apply.  One 1024-thread workgroup per block of the batch:
//     1. candidates (best class score > conf) into the LDS key array, 2. lds_sort_keys by (score desc, anchor asc), 3. gather of the
//        sorted candidates into the workspace -- the front end of nms_kernel, in line in both: behind one helper both kernels measured
//        slower (nms_common.h holds what they state once; profiles/suppress_refactor_ab.txt has the figures).
//     4. a second in-LDS sort by (class, position) gives the segments (box_fusion.hip's construction, in line in both for the same
//        reason: a ballot per 64 positions, a prefix over the mask words).  The key array is dead after it: its 8 bytes per candidate
//        become the live score s (fp32) and the position (int32), both in segment order.  The segment-ordered boxes go to the workspace.
//     5. the walk: the 16 waves take the segments round-robin.  Candidate a + l + 64 q of a segment that starts at a belongs to lane l,
//        which alone reads and writes its s: there is no cross-lane traffic through LDS, so no fence inside a segment.  One sweep per
//        pick applies M's decay to the lane's live candidates and tracks the lane's (largest s, lowest position); six shuffles reduce
//        that to the next M.  An emitted candidate keeps -s (s > 0 at emission) and a flag in its position word; a candidate hard mode
//        removes keeps -1.
//     6. the merge: the emitted candidates' (final score desc, position asc) keys are sorted in the same LDS array; the first max_det
//        leave.
// Nothing depends on the arrival order of an atomic except the slots of step 1, which the first sort re-orders: two calls give the same
// bits.  Vector stores only.
#include "box_overlap.h"
#include "cvx_common.h"
#include "det_rows.h"
#include "lds_sort.h"
#include "nms_common.h"
#include "../../include/cvx_engine.h"

namespace {

constexpr int SNMS_CAP = NMS_CAP;  // candidates per block the LDS sort holds (nms_common.h)
constexpr int SNMS_THREADS = 1024;
constexpr int SNMS_WAVES = SNMS_THREADS / 64;
constexpr int SNMS_PER_THREAD = SNMS_CAP / SNMS_THREADS;
constexpr unsigned SNMS_EMITTED = 0x80000000u;
#ifndef SNMS_FLY
#define SNMS_FLY 4  // candidates a lane has in flight per trip of the sweep
#endif

// E(x) = exp(-x) as a fixed sequence of fp32 operations, each rounded on its own: k = rint(-x log2 e), a two-constant Cody-Waite
// reduction (k * 0.693359375 is exact for |k| < 2^15), the degree-6 Taylor polynomial in Horner form without fma, an exact scaling by
// 2^k.  x >= 80 gives 0; below that 2^k p is a normal number.  Within 1e-6 relative of exp(-x) on [0, 20].
__device__ __forceinline__ float snms_exp_neg(float x) {
#pragma clang fp contract(off)
  if (x >= 80.0f) return 0.0f;
  const float t = -x;
  const float k = rintf(t * 1.44269504088896341f);
  float r = t - k * 0.693359375f;
  r = r - k * -2.12194440e-4f;
  float p = 1.0f / 720.0f;
  p = p * r + 1.0f / 120.0f;
  p = p * r + 1.0f / 24.0f;
  p = p * r + 1.0f / 6.0f;
  p = p * r + 0.5f;
  p = p * r + 1.0f;
  p = p * r + 1.0f;
  return ldexpf(p, (int)k);
}
__device__ __forceinline__ float snms_linear(float s, float o) {
#pragma clang fp contract(off)
  return s * (1.0f - o);
}
__device__ __forceinline__ float snms_gaussian(float s, float o, float sigma) {
#pragma clang fp contract(off)
  const float x = (o * o) / sigma;
  return s * snms_exp_neg(x);
}

struct SnmsWs {
  float4* box;   // [B][cap] boxes (xyxy) by position
  float4* bseg;  // [B][cap] the same boxes in segment order
  float* score;  // [B][cap]
  int* cls;      // [B][cap]
  int* aidx;     // [B][cap]
};

// position of the sg-th segment start: the mask word that holds it (the last whose prefix does not exceed sg), then its bit
__device__ __forceinline__ int snms_seg_start(const unsigned long long* mask, const int* wpre, int nw, int sg) {
  int lo = 0, hi = nw - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (wpre[mid] <= sg) lo = mid;
    else hi = mid - 1;
  }
  unsigned long long m = mask[lo];
  for (int k = sg - wpre[lo]; k > 0; --k) m &= m - 1;
  return lo * 64 + __ffsll((long long)m) - 1;
}

__global__ __launch_bounds__(SNMS_THREADS) void soft_nms_kernel(const float* __restrict__ y, int A, int nc, float conf_thres, float iou_thres,
                                                                int max_det, int cap, int method, float sigma, float min_score, int flags,
                                                                SnmsWs ws, float* __restrict__ out_rows, int* __restrict__ out_index,
                                                                int* __restrict__ counts) {
  const bool xyxy = (flags & CVX_NMS_BOXES_XYXY) != 0, agnostic = (flags & CVX_SOFT_NMS_CLASS_AGNOSTIC) != 0;
  extern __shared__ unsigned long long keys[];                 // cap entries while a sort runs
  float* s_live = reinterpret_cast<float*>(keys);              // [cap] during the walk, segment order
  unsigned* s_pos = reinterpret_cast<unsigned*>(keys) + cap;   // [cap] position | SNMS_EMITTED
  __shared__ int s_n, s_nseg, s_nemit;
  __shared__ unsigned long long s_mask[SNMS_CAP / 64];
  __shared__ int s_wpre[SNMS_CAP / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* yb = y + (long long)b * (4 + nc) * A;
  float* orow = out_rows + (long long)b * max_det * 6;
  int* oidx = out_index + (long long)b * max_det;
  if (tid == 0) s_n = s_nemit = 0;
  __syncthreads();
  // ---- 1. candidates: best class score > conf ----
  for (int a0 = 0; a0 < A; a0 += SNMS_THREADS) {
    const int a = a0 + tid;
    float best = -1.f;
    if (a < A)
      for (int c = 0; c < nc; ++c) best = fmaxf(best, yb[(long long)(4 + c) * A + a]);
    if (a < A && best > conf_thres) {
      const int slot = atomicAdd(&s_n, 1);
      if (slot < cap) keys[slot] = score_key(best, (unsigned)a);
    }
  }
  __syncthreads();
  if (s_n > cap) {  // more candidates than the in-LDS sort holds: signalled, never truncated
    zero_rows<SNMS_THREADS>(orow, 0, max_det, oidx, 0);
    if (tid == 0) counts[b] = -1;
    return;
  }
  const int n = s_n;
  if (n == 0) {
    zero_rows<SNMS_THREADS>(orow, 0, max_det, oidx, 0);
    if (tid == 0) counts[b] = 0;
    return;
  }
  // ---- 2. (score desc, anchor asc) ----
  lds_sort_keys<SNMS_THREADS>(keys, n);
  // ---- 3. gather the sorted candidates ----
  float4* box = ws.box + (long long)b * cap;
  float4* bseg = ws.bseg + (long long)b * cap;
  float* score = ws.score + (long long)b * cap;
  int* cls = ws.cls + (long long)b * cap;
  int* aidx = ws.aidx + (long long)b * cap;
  for (int i = tid; i < n; i += SNMS_THREADS) {
    const int a = (int)(keys[i] & 0xFFFFFFFFu);
    const float cx = yb[a], cy = yb[(long long)A + a], w = yb[2LL * A + a], h = yb[3LL * A + a];
    box[i] = xyxy ? make_float4(cx, cy, w, h) : box_corners(cx, cy, w, h);
    float best = -1.f;
    int bc = 0;
    for (int c = 0; c < nc; ++c) {
      const float s = yb[(long long)(4 + c) * A + a];
      if (s > best) {
        best = s;
        bc = c;
      }
    }
    score[i] = best;
    cls[i] = bc;
    aidx[i] = a;
  }
  __syncthreads();  // the keys are dead; this workgroup's workspace writes are visible to it
  // ---- 4. segment order: (class, position), or the positions as they are ----
  if (!agnostic) {
    for (int i = tid; i < n; i += SNMS_THREADS) keys[i] = ((unsigned long long)(unsigned)cls[i] << 32) | (unsigned)i;
    lds_sort_keys<SNMS_THREADS>(keys, n);
  }
  {
    unsigned pj[SNMS_PER_THREAD];
#pragma unroll
    for (int q = 0; q < SNMS_PER_THREAD; ++q) {
      const int j = tid + q * SNMS_THREADS;
      pj[q] = j < n ? (agnostic ? (unsigned)j : (unsigned)(keys[j] & 0xFFFFFFFFu)) : 0u;
    }
    __syncthreads();  // every key is in a register before the array is rewritten as s | position
#pragma unroll
    for (int q = 0; q < SNMS_PER_THREAD; ++q) {
      const int j = tid + q * SNMS_THREADS;
      if (j < n) {
        s_live[j] = score[pj[q]];
        s_pos[j] = pj[q];
        bseg[j] = box[pj[q]];
      }
    }
  }
  __syncthreads();
  // segment starts: a change of class (the construction of box_fusion.hip, step 3)
  for (int p0 = 0; p0 < n; p0 += SNMS_THREADS) {
    const int p = p0 + tid;
    const bool start = p < n && (p == 0 || (!agnostic && cls[s_pos[p]] != cls[s_pos[p - 1]]));
    const unsigned long long m = __ballot(start);
    if (lane == 0) s_mask[p >> 6] = m;
  }
  __syncthreads();
  const int nw = (n + 63) / 64;
  if (tid == 0) {
    int acc = 0;
    for (int w = 0; w < nw; ++w) {
      s_wpre[w] = acc;
      acc += __popcll(s_mask[w]);
    }
    s_nseg = acc;
  }
  __syncthreads();
  // ---- 5. the walk: a wave per segment, candidate a + l + 64 q on lane l ----
  const int nseg = s_nseg;
  int emitted_by_wave = 0;
  for (int sg = wave; sg < nseg; sg += SNMS_WAVES) {
    const int a = snms_seg_start(s_mask, s_wpre, nw, sg);
    const int e = sg + 1 < nseg ? snms_seg_start(s_mask, s_wpre, nw, sg + 1) : n;
    bool have = false;
    float4 bm = make_float4(0.f, 0.f, 0.f, 0.f);
    float am = 0.f;
    int emitted = 0;
    for (;;) {
      unsigned long long best = 0;  // (s bits, ~j) of the lane's best live candidate: s >= 0, its bits order like the value
      // SNMS_FLY of the lane's candidates at a time: their scores, then the boxes of the live ones, are all requested before the first
      // is used -- one candidate per trip waited for every box on its own
      for (int j0 = a + lane; j0 < e; j0 += 64 * SNMS_FLY) {
        float sv[SNMS_FLY];
        float4 bv[SNMS_FLY];
#pragma unroll
        for (int u = 0; u < SNMS_FLY; ++u) {
          const int j = j0 + 64 * u;
          sv[u] = j < e ? s_live[j] : -1.f;
        }
#pragma unroll
        for (int u = 0; u < SNMS_FLY; ++u) {
          bv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (have && sv[u] >= 0.f) bv[u] = bseg[j0 + 64 * u];
        }
#pragma unroll
        for (int u = 0; u < SNMS_FLY; ++u) {
          const int j = j0 + 64 * u;
          float s = sv[u];
          if (!(s >= 0.f)) continue;  // past the end, emitted, removed, or decayed below zero by a degenerate overlap: never taken
          if (have) {
            const float o = iou_value(bm, am, bv[u], box_area(bv[u]));
            if (method == CVX_SOFT_NMS_HARD) {
              if (o > iou_thres) {
                s_live[j] = -1.f;
                continue;
              }
            } else if (method == CVX_SOFT_NMS_LINEAR) {
              if (o > iou_thres) {
                s = snms_linear(s, o);
                s_live[j] = s;
              }
            } else if (o > 0.f) {
              s = snms_gaussian(s, o, sigma);
              s_live[j] = s;
            }
            if (!(s >= 0.f)) continue;
          }
          const unsigned long long key = ((unsigned long long)__float_as_uint(s) << 32) | (0xFFFFFFFFu - (unsigned)j);
          if (key > best) best = key;
        }
      }
      for (int off = 32; off; off >>= 1) {
        const unsigned long long other = __shfl_xor(best, off);
        if (other > best) best = other;
      }
      if (best == 0) break;  // nothing live
      const float sm = __uint_as_float((unsigned)(best >> 32));
      if (method != CVX_SOFT_NMS_HARD && !(sm > min_score)) break;
      const int jm = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu));  // the largest s, the lowest position among equals
      if (lane == ((jm - a) & 63)) {
        s_live[jm] = -sm;
        s_pos[jm] |= SNMS_EMITTED;
      }
      ++emitted;
      if (method == CVX_SOFT_NMS_HARD && emitted >= max_det) break;  // scores untouched: a segment's later picks rank behind these
      bm = bseg[jm];
      am = box_area(bm);
      have = true;
    }
    emitted_by_wave += emitted;
  }
  if (lane == 0 && emitted_by_wave) atomicAdd(&s_nemit, emitted_by_wave);  // a sum: the same whatever the order
  __syncthreads();
  // ---- 6. merge the segments' emissions by (final score desc, position asc) ----
  {
    unsigned long long kq[SNMS_PER_THREAD];
#pragma unroll
    for (int q = 0; q < SNMS_PER_THREAD; ++q) {
      const int j = tid + q * SNMS_THREADS;
      kq[q] = ~0ull;
      if (j < n) {
        const unsigned p = s_pos[j];
        if (p & SNMS_EMITTED) kq[q] = score_key(-s_live[j], p & ~SNMS_EMITTED);
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SNMS_PER_THREAD; ++q) {
      const int j = tid + q * SNMS_THREADS;
      if (j < n) keys[j] = kq[q];
    }
  }
  lds_sort_keys<SNMS_THREADS>(keys, n);  // the candidates that were not emitted carry the padding key: they sort last
  const int nk = min(s_nemit, max_det);
  for (int r = tid; r < nk; r += SNMS_THREADS) {
    const unsigned long long k = keys[r];
    const int p = (int)(k & 0xFFFFFFFFu);
    const float4 bx = box[p];
    float* o = orow + (long long)r * 6;
    o[0] = bx.x;
    o[1] = bx.y;
    o[2] = bx.z;
    o[3] = bx.w;
    o[4] = __uint_as_float(0xFFFFFFFFu - (unsigned)(k >> 32));
    o[5] = (float)cls[p];
    oidx[r] = aidx[p];
  }
  zero_rows<SNMS_THREADS>(orow, nk, max_det, oidx, 0);
  if (tid == 0) counts[b] = nk;
}

SnmsWs snms_layout(cvx_carver& c, long long B, long long cap) {
  SnmsWs ws;
  ws.box = c.take<float4>(B * cap);
  ws.bseg = c.take<float4>(B * cap);
  ws.score = c.take<float>(B * cap);
  ws.cls = c.take<int>(B * cap);
  ws.aidx = c.take<int>(B * cap);
  return ws;
}

}  // namespace

extern "C" int64_t cvx_soft_nms_workspace_bytes(int32_t B, int32_t A) {
  if (B <= 0 || A <= 0) return 0;
  cvx_carver c(nullptr);
  snms_layout(c, B, nms_cap_for(A));
  return c.total();
}

extern "C" int cvx_soft_nms(const float* y, int32_t B, int32_t A, int32_t nc, float conf_thres, float iou_thres, int32_t max_det, int32_t method,
                            float sigma, float min_score, int32_t flags, float* out_rows, int32_t* out_index, int32_t* counts, void* workspace,
                            int64_t workspace_bytes, void* hip_stream) {
  CVX_CHECK(y && out_rows && out_index && counts && workspace, "null arguments");
  CVX_CHECK(B > 0 && A > 0 && nc > 0, "bad sizes");
  CVX_CHECK(method >= CVX_SOFT_NMS_HARD && method <= CVX_SOFT_NMS_GAUSSIAN, "unknown soft-NMS method");
  CVX_CHECK((flags & ~(CVX_NMS_BOXES_XYXY | CVX_SOFT_NMS_CLASS_AGNOSTIC)) == 0, "unknown soft-NMS flags");
  CVX_CHECK(conf_thres >= 0.f && conf_thres <= 1.f && iou_thres >= 0.f && iou_thres <= 1.f, "thresholds must lie in [0,1]");
  CVX_CHECK(sigma >= 0.05f && sigma <= 10.f, "sigma must lie in [0.05,10]");
  CVX_CHECK(min_score >= 0.f && min_score < 1.f, "min_score must lie in [0,1)");
  CVX_CHECK(max_det >= 1 && max_det <= SNMS_CAP, "max_det must lie in [1,16384]");
  CVX_CHECK(workspace_bytes >= cvx_soft_nms_workspace_bytes(B, A), "workspace too small");
  const int cap = nms_cap_for(A);
  cvx_carver carver(workspace);
  const SnmsWs ws = snms_layout(carver, B, cap);
  static unsigned long long optin = 0;  // 128 KB of keys at capacity: beyond the default dynamic LDS limit
  CVX_TRY(cvx_lds_optin((const void*)soft_nms_kernel, SNMS_CAP * 8, &optin));
  hipLaunchKernelGGL(soft_nms_kernel, dim3(B), dim3(SNMS_THREADS), (size_t)cap * 8, (hipStream_t)hip_stream, y, A, nc, conf_thres, iou_thres, max_det,
                     cap, (int)method, sigma, min_score, (int)flags, ws, out_rows, out_index, counts);
  CVX_HIP(hipGetLastError());
  return 0;
}
