// Weighted Boxes Fusion (Solovyev et al., 2021) of the rows several sources report for a frame, on gfx950.  The
// sources are the views of a test-time augmentation or the members of a detector ensemble; the inputs are those of cvx_det_fuse_views
// (det_tta.hip): slot k * frames + f holds what source k reports for frame f, and a per-slot affine map brings it to the picture.
//
//   wbf_kernel   one workgroup of 1024 threads per frame.
//     1. thread 0 walks the frame's (at most 32) counts: the prefix of the valid ones gives every row a frame-local id below 8192 that
//        rises with its ordinal, so the id stands in for the ordinal in every key and the ordinal is rebuilt from it at the end.
//     2. every row goes through its slot's map and the clamp (view_box.h, shared with fuse_kernel), the skipped ones drop out, and the
//        rest are sorted twice with lds_sort.h: by (weighted score desc, id asc), whose position is a rank below 8192, then by (class
//        bits, rank).  The sorted candidates go to the workspace.  class_agnostic needs the first sort alone.
//     3. segment starts (a change of class) are found with a ballot per 64 positions and numbered by a prefix over the 128 mask words.
//     4. the walk: the 16 waves take the segments round-robin.  A wave walks its segment's candidates in order; for each one its lanes
//        stride over the segment's clusters, lane c & 63 scanning cluster c against the broadcast candidate, and a wave reduction picks
//        the best match above the threshold, ties to the lower index.  Cluster c of the segment that starts at a lives in slot a + c (a
//        segment of L candidates has at most L clusters): its fused box in LDS, its sums in the workspace.  Lane c & 63 is the only lane
//        that ever reads or writes slot a + c -- it scans it, it alone updates or opens it --, so nothing one lane writes is read by
//        another, the only cross-lane traffic is the reduction, and the walk needs no fence and no barrier.
//     5. after a barrier the clusters of the frame are sorted by (score desc, first id asc) and the first max_det are written out.
// No floating-point atomics, nothing depends on arrival order: the two atomicAdd fills of the key array are followed by a sort of unique
// keys.  Every fp32 step is one rounded operation: the file is compiled with contraction off, and tests/box_fusion_restatement.py holds
// the kernel to the bit.
#include "box_overlap.h"
#include "det_rows.h"
#include "lds_sort.h"
#include "view_box.h"
#include "../../include/cvx_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int WBF_CAP = 8192;   // candidates per frame: what the in-LDS sort holds, and the fused boxes of as many clusters fill 128 KB of LDS
constexpr int WBF_THREADS = 1024;
constexpr int WBF_WAVES = WBF_THREADS / 64;
constexpr int WBF_MAX_SOURCES = 32;
constexpr int WBF_BOX_BYTES = WBF_CAP * 16;                    // the fused boxes; its first half holds the keys while a sort runs
constexpr int WBF_LDS_BYTES = WBF_BOX_BYTES + (WBF_CAP + 8) * 2;   // + the segment starts, 16 bits each, one more than segments

struct WbfCand {   // [frames][WBF_CAP] candidates in sorted order
  float4* box;     // in picture coordinates
  float* s;        // score * weight of the source
  float* cls;
  int* meta;       // id | source << 16
};
struct WbfWs {
  WbfCand a, b;    // a: by (s, id); b: by (class, s, id)
  float4* sx;      // per cluster slot: the weighted corner sums, ...
  float4* fused;   // ... the fused box as the walk leaves it, ...
  float* sw;       // ... the weight sum, the first (largest) weighted score, the class of the first member, the score, ...
  float* smax;
  float* ccls;
  float* score;
  int* cnt;        // ... the members (0: the slot holds no cluster) and the meta word of the first member
  int* first;
};

__global__ __launch_bounds__(WBF_THREADS) void wbf_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int max_det_in,
                                                          const float* __restrict__ view_map, const int* __restrict__ frame_hw, int frames, int sources,
                                                          const float* __restrict__ weights, float iou_thr, float skip_score, int class_agnostic,
                                                          int conf_mode, int rescale, int max_det, WbfWs ws, float* __restrict__ out_rows,
                                                          int* __restrict__ out_counts, int* __restrict__ out_source, int* __restrict__ out_members,
                                                          int* overflow) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(lds);   // while a sort runs
  float4* fused = reinterpret_cast<float4*>(lds);                         // during the walk
  unsigned short* seg_start = reinterpret_cast<unsigned short*>(lds + WBF_BOX_BYTES);
  __shared__ int s_pre[WBF_MAX_SOURCES + 1];
  __shared__ int s_fill, s_nseg, s_ncl;
  __shared__ float s_W;
  __shared__ unsigned long long s_mask[WBF_CAP / 64];
  __shared__ int s_wpre[WBF_CAP / 64];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* orow = out_rows + (long long)f * max_det * 6;
  int* osrc = out_source + (long long)f * max_det;
  int* omem = out_members + (long long)f * max_det;
  // ---- 1. the ids: the prefix of the frame's valid counts; a count outside [0, max_det_in] contributes nothing and is flagged ----
  if (tid == 0) {
    int at = 0, bad = 0;
    float W = 0.f;
    for (int k = 0; k < sources; ++k) {
      const int c = counts[k * frames + f];
      s_pre[k] = at;
      if (c < 0 || c > max_det_in) ++bad;
      else at += c;
      W = W + weights[k];
    }
    s_pre[sources] = at;
    if (bad) atomicAdd(overflow, bad);
    s_W = W;
    s_fill = s_ncl = 0;
  }
  __syncthreads();
  const int n_raw = s_pre[sources];
  if (n_raw > WBF_CAP) {  // more than the in-LDS sort holds: flagged, never truncated
    zero_rows<WBF_THREADS>(orow, 0, max_det, osrc, -1, omem, 0);
    if (tid == 0) {
      out_counts[f] = -1;
      atomicAdd(overflow, 1);
    }
    return;
  }
  const int fh = frame_hw[2 * f], fw = frame_hw[2 * f + 1];
  // ---- 2. keys of the rows that are not skipped: (weighted score desc, id asc); then the sort ----
  for (int id = tid; id < n_raw; id += WBF_THREADS) {
    int k = 0;
    while (s_pre[k + 1] <= id) ++k;   // id < s_pre[sources]: ends inside the table
    const int slot = k * frames + f;
    const float* row = rows + ((long long)slot * max_det_in + (id - s_pre[k])) * 6;
    const float4 b = mapped_box(row, view_map + 4 * slot, fh, fw);
    if (row[4] < skip_score || !(b.z > b.x && b.w > b.y)) continue;
    keys[atomicAdd(&s_fill, 1)] = score_key(row[4] * weights[k], (unsigned)id);
  }
  __syncthreads();
  const int n = s_fill;
  if (n == 0) {
    zero_rows<WBF_THREADS>(orow, 0, max_det, osrc, -1, omem, 0);
    if (tid == 0) out_counts[f] = 0;
    return;
  }
  lds_sort_keys<WBF_THREADS>(keys, n);
  const long long base = (long long)f * WBF_CAP;
  const WbfCand A = {ws.a.box + base, ws.a.s + base, ws.a.cls + base, ws.a.meta + base};
  const WbfCand Bc = {ws.b.box + base, ws.b.s + base, ws.b.cls + base, ws.b.meta + base};
  for (int i = tid; i < n; i += WBF_THREADS) {
    const int id = (int)(keys[i] & 0xFFFFFFFFu);
    int k = 0;
    while (s_pre[k + 1] <= id) ++k;
    const int slot = k * frames + f;
    const float* row = rows + ((long long)slot * max_det_in + (id - s_pre[k])) * 6;
    A.box[i] = mapped_box(row, view_map + 4 * slot, fh, fw);
    A.s[i] = row[4] * weights[k];
    A.cls[i] = row[5];
    A.meta[i] = id | (k << 16);
  }
  __syncthreads();
  if (!class_agnostic) {  // (class bits asc, rank asc): the bits of a non-negative fp32 order like the value
    for (int i = tid; i < n; i += WBF_THREADS) keys[i] = ((unsigned long long)__float_as_uint(A.cls[i]) << 32) | (unsigned)i;
    lds_sort_keys<WBF_THREADS>(keys, n);
    for (int p = tid; p < n; p += WBF_THREADS) {
      const int r = (int)(keys[p] & 0xFFFFFFFFu);
      Bc.box[p] = A.box[r];
      Bc.s[p] = A.s[r];
      Bc.cls[p] = A.cls[r];
      Bc.meta[p] = A.meta[r];
    }
    __syncthreads();   // the keys are dead from here; the sorted candidates are in the workspace
  }
  const WbfCand C = class_agnostic ? A : Bc;
  // ---- 3. the segments: a start where the class changes ----
  for (int p0 = 0; p0 < n; p0 += WBF_THREADS) {
    const int p = p0 + tid;
    const bool start = p < n && (p == 0 || (!class_agnostic && __float_as_uint(C.cls[p]) != __float_as_uint(C.cls[p - 1])));
    const unsigned long long m = __ballot(start);
    if (lane == 0) s_mask[p >> 6] = m;
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int w = 0; w < (n + 63) / 64; ++w) {
      s_wpre[w] = acc;
      acc += __popcll(s_mask[w]);
    }
    s_nseg = acc;
    seg_start[acc] = (unsigned short)n;   // n <= 8192 fits 16 bits
  }
  __syncthreads();
  for (int p = tid; p < n; p += WBF_THREADS) {
    const unsigned long long m = s_mask[p >> 6];
    if ((m >> (p & 63)) & 1ull) seg_start[s_wpre[p >> 6] + __popcll(m & ((1ull << (p & 63)) - 1ull))] = (unsigned short)p;
  }
  __syncthreads();
  // ---- 4. the walk: a wave per segment, a lane per cluster (lane c & 63 alone touches cluster c) ----
  const float W = s_W;
  const int nseg = s_nseg;
  float4* sx = ws.sx + base;
  float4* fusedg = ws.fused + base;
  float *sw = ws.sw + base, *smax = ws.smax + base, *ccls = ws.ccls + base, *score = ws.score + base;
  int *cnt = ws.cnt + base, *first = ws.first + base;
  for (int sg = wave; sg < nseg; sg += WBF_WAVES) {
    const int a = seg_start[sg], e = seg_start[sg + 1];
    int nc = 0;
    float4 nb = C.box[a];
    float ns = C.s[a], ncl = C.cls[a];
    int nm = C.meta[a];
    for (int j = a; j < e; ++j) {
      const float4 b = nb;
      const float s = ns, cl = ncl;
      const int meta = nm;
      if (j + 1 < e) {   // the next candidate's loads fly during this one's scan
        nb = C.box[j + 1];
        ns = C.s[j + 1];
        ncl = C.cls[j + 1];
        nm = C.meta[j + 1];
      }
      const float ab = box_area(b);
      unsigned long long best = 0;   // (IoU bits, ~c): above the threshold the IoU is positive, and its bits order like the value
      for (int c = lane; c < nc; c += 64) {
        const float4 fb = fused[a + c];
        const float v = iou_value(fb, box_area(fb), b, ab);
        if (v > iou_thr) {   // a NaN never matches
          const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (0xFFFFFFFFu - (unsigned)c);
          if (key > best) best = key;
        }
      }
      if (__ballot(best != 0) == 0) {   // no match: cluster nc opens, its box the candidate's bit for bit
        if (lane == (nc & 63)) {
          const int slot = a + nc;
          fused[slot] = b;
          sw[slot] = s;
          sx[slot] = make_float4(s * b.x, s * b.y, s * b.z, s * b.w);
          cnt[slot] = 1;
          smax[slot] = s;
          first[slot] = meta;
          ccls[slot] = cl;
        }
        ++nc;
      } else {
        for (int off = 32; off; off >>= 1) {
          const unsigned long long other = __shfl_xor(best, off);
          if (other > best) best = other;
        }
        const int win = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu));   // the largest IoU, the lowest index among equals
        if (lane == (win & 63)) {
          const int slot = a + win;
          const float t = sw[slot] + s;
          float4 x = sx[slot];
          x.x = x.x + s * b.x;
          x.y = x.y + s * b.y;
          x.z = x.z + s * b.z;
          x.w = x.w + s * b.w;
          sw[slot] = t;
          sx[slot] = x;
          cnt[slot] = cnt[slot] + 1;
          fused[slot] = make_float4(x.x / t, x.y / t, x.z / t, x.w / t);
        }
      }
    }
    // the segment's clusters leave LDS with their scores, each by its own lane; the slots behind them hold none
    for (int c = lane; c < e - a; c += 64) {
      const int slot = a + c;
      if (c < nc) {
        const float nf = (float)cnt[slot];
        const float own = conf_mode == 1 ? smax[slot] : sw[slot] / nf;
        score[slot] = rescale ? (own * fminf(nf, W)) / W : own;
        fusedg[slot] = fused[slot];
      } else {
        cnt[slot] = 0;
      }
    }
  }
  __syncthreads();
  // ---- 5. the clusters of the frame by (score desc, first asc): the id of the first member, the slot behind it to find the cluster again ----
  for (int slot = tid; slot < n; slot += WBF_THREADS)
    if (cnt[slot] > 0) keys[atomicAdd(&s_ncl, 1)] = score_key(score[slot], ((unsigned)(first[slot] & 0xFFFF) << 13) | (unsigned)slot);
  __syncthreads();
  const int clusters = s_ncl;
  lds_sort_keys<WBF_THREADS>(keys, clusters);
  const int nk = min(clusters, max_det);
  for (int r = tid; r < nk; r += WBF_THREADS) {
    const int slot = (int)(keys[r] & (WBF_CAP - 1));
    const float4 b = fusedg[slot];
    const int meta = first[slot], k = meta >> 16;
    store_row(orow + (long long)r * 6, b, score[slot], ccls[slot]);
    osrc[r] = (k * frames + f) * max_det_in + ((meta & 0xFFFF) - s_pre[k]);
    omem[r] = cnt[slot];
  }
  zero_rows<WBF_THREADS>(orow, nk, max_det, osrc, -1, omem, 0);
  if (tid == 0) out_counts[f] = nk;
}

// per frame: two candidate tables of 28 bytes an entry, the cluster slots of 56
WbfWs wbf_layout(cvx_carver& c, long long frames) {
  const long long n = frames * WBF_CAP;
  WbfWs ws;
  for (WbfCand* t : {&ws.a, &ws.b}) {
    t->box = c.take<float4>(n);
    t->s = c.take<float>(n);
    t->cls = c.take<float>(n);
    t->meta = c.take<int>(n);
  }
  ws.sx = c.take<float4>(n);
  ws.fused = c.take<float4>(n);
  ws.sw = c.take<float>(n);
  ws.smax = c.take<float>(n);
  ws.ccls = c.take<float>(n);
  ws.score = c.take<float>(n);
  ws.cnt = c.take<int>(n);
  ws.first = c.take<int>(n);
  return ws;
}

}  // namespace

extern "C" int64_t cvx_det_wbf_workspace_bytes(int32_t frames) {
  if (frames <= 0) return 0;
  cvx_carver c(nullptr);
  wbf_layout(c, frames);
  return c.total();
}

extern "C" int cvx_det_fuse_wbf(const float* rows, const int32_t* counts, int32_t max_det_in, const float* view_map, const int32_t* frame_hw,
                                int32_t frames, int32_t sources, const float* weights, float iou_thr, float skip_score, int32_t class_agnostic,
                                int32_t conf_mode, int32_t rescale, int32_t max_det_out, float* out_rows, int32_t* out_counts, int32_t* out_source,
                                int32_t* out_members, int32_t* overflow, void* workspace, int64_t workspace_bytes, void* hip_stream) {
  CVX_CHECK(rows && counts && view_map && frame_hw && weights && out_rows && out_counts && out_source && out_members && overflow && workspace,
            "null arguments");
  CVX_CHECK(sources >= 1 && sources <= WBF_MAX_SOURCES, "1 <= sources <= 32");
  CVX_CHECK(max_det_in > 0 && frames > 0 && (long long)sources * frames * max_det_in < (1LL << 31), "bad sizes: the ordinal is 32 bits");
  CVX_CHECK(iou_thr >= 0.f && iou_thr <= 1.f, "iou_thr must lie in [0,1]");
  CVX_CHECK(skip_score >= 0.f && skip_score < INFINITY, "skip_score is finite and not negative: the score key orders non-negative scores");
  CVX_CHECK(conf_mode == 0 || conf_mode == 1, "conf_mode: 0 avg, 1 max");
  CVX_CHECK(rescale == 0 || rescale == 1, "rescale: 0 or 1");
  CVX_CHECK(max_det_out >= 1 && max_det_out <= WBF_CAP, "max_det_out must lie in [1,8192]");
  CVX_CHECK(workspace_bytes >= cvx_det_wbf_workspace_bytes(frames), "workspace too small");
  cvx_carver carver(workspace);
  const WbfWs ws = wbf_layout(carver, frames);
  static unsigned long long optin = 0;  // 128 KB of fused boxes + 16 KB of segment starts: beyond the default dynamic LDS limit
  CVX_TRY(cvx_lds_optin((const void*)wbf_kernel, WBF_LDS_BYTES, &optin));
  hipLaunchKernelGGL(wbf_kernel, dim3(frames), dim3(WBF_THREADS), (size_t)WBF_LDS_BYTES, (hipStream_t)hip_stream, rows, counts, max_det_in, view_map,
                     frame_hw, frames, sources, weights, iou_thr, skip_score, class_agnostic, conf_mode, rescale, max_det_out, ws, out_rows,
                     out_counts, out_source, out_members, overflow);
  CVX_HIP(hipGetLastError());
  return 0;
}
