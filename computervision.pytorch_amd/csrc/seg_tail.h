// The per-pixel tail of the segmentation output kernels, shared by seg_overlay_kernel (render.hip), seg_stitch_kernel (seg_tiles.hip;
// it keeps the logit chunk in line, see there), both modes of seg_fuse_kernel (seg_tta.hip) and, for the histogram, seg_eval_kernel
// (loss_seg.hip): four classes of interpolated logits, the arg max over them, four RGB pixels of a frame row, and the workgroup's
// confusion counts in LDS.  The suite holds these kernels to the bit against each other (same taps, same tie rule, same blend), so the
// blocks live in one place.  How a kernel accumulates the logits (fma(w, z, acc), acc + z, acc + softmax) stays in the kernel.  No
// helper here does fp32 arithmetic of its own: the taps are bilinear_mix's, whose roundings are spelled out.  Each translation unit
// gets its own copy (anonymous namespace).
#pragma once
#include "bilinear.h"
#include "pixel_blend.h"

namespace {

// The logits of classes c0 .. c0 + 3 at one pixel from feature rows ra (weight 1 - ly) and rb (ly), both already advanced to class c0,
// at columns xa (1 - lx) and xb (lx).  vec: ld % 4 == 0 and a 16-byte aligned base, then one 16-byte load per tap.  Classes past nc are
// 0 on the scalar path and whatever the padding holds on the vector path -- argmax4 and the callers never look at them.
__device__ __forceinline__ void logits4(const float* ra, const float* rb, int xa, int xb, float lx, float ly, int ld, int c0, int nc, bool vec,
                                        float z[4]) {
  const float *r00 = ra + (long long)xa * ld, *r01 = ra + (long long)xb * ld;
  const float *r10 = rb + (long long)xa * ld, *r11 = rb + (long long)xb * ld;
  if (vec && c0 + 4 <= ld) {
    const f4 a = *reinterpret_cast<const f4*>(r00), b = *reinterpret_cast<const f4*>(r01);
    const f4 c = *reinterpret_cast<const f4*>(r10), d = *reinterpret_cast<const f4*>(r11);
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = bilinear_mix(a[i], b[i], c[i], d[i], lx, ly);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = c0 + i < nc ? bilinear_mix(r00[i], r01[i], r10[i], r11[i], lx, ly) : 0.f;
  }
}

// (best, arg) updated with classes c0 .. c0 + 3: strict >, so the lowest class wins a tie, like torch.argmax; class 0 always enters.
__device__ __forceinline__ void argmax4(const float z[4], int c0, int nc, float& best, int& arg) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c0 + i < nc && (c0 + i == 0 || z[i] > best)) {
      best = z[i];
      arg = c0 + i;
    }
}

// Up to four RGB pixels at p (npx of them) of a frame row: three 32-bit words when the thread has all four and the frame's base and
// stride are 4-byte aligned (p is then 12-byte granular), bytes otherwise.  The twelve bytes are one vector value, not a byte array:
// an array that passes through these functions is read back as words by the time they are inlined and no longer fits registers
// (16 bytes of scratch per lane in both callers); a vector is loaded and stored whole, whatever the index.
typedef uint8_t pixel_quad __attribute__((ext_vector_type(12)));
__device__ __forceinline__ bool quad_is_wide(const uint8_t* data, int stride, int npx) {
  return npx == 4 && ((reinterpret_cast<uintptr_t>(data) | (uintptr_t)stride) & 3) == 0;
}
__device__ __forceinline__ void quad_load(const uint8_t* p, int npx, bool wide, pixel_quad& px) {
  if (wide) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    const uint32_t a = q[0], b = q[1], c = q[2];
    for (int k = 0; k < 4; ++k) {
      px[k] = (uint8_t)(a >> 8 * k);
      px[4 + k] = (uint8_t)(b >> 8 * k);
      px[8 + k] = (uint8_t)(c >> 8 * k);
    }
  } else {
    for (int k = 0; k < 3 * npx; ++k) px[k] = p[k];
  }
}
// pixel k takes the 50/50 blend with the palette colour col (RGB); bgr_out: the frame's bytes are B, G, R
__device__ __forceinline__ void quad_blend(pixel_quad& px, int k, const uint8_t* col, int bgr_out) {
  const unsigned r = blend_half(px[3 * k + 0], col[0]), g = blend_half(px[3 * k + 1], col[1]), b = blend_half(px[3 * k + 2], col[2]);
  px[3 * k + 0] = (uint8_t)(bgr_out ? b : r);
  px[3 * k + 1] = (uint8_t)g;
  px[3 * k + 2] = (uint8_t)(bgr_out ? r : b);
}
__device__ __forceinline__ void quad_store(uint8_t* p, int npx, bool wide, const pixel_quad& px) {
  if (wide) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = px[0] | px[1] << 8 | px[2] << 16 | (uint32_t)px[3] << 24;
    q[1] = px[4] | px[5] << 8 | px[6] << 16 | (uint32_t)px[7] << 24;
    q[2] = px[8] | px[9] << 8 | px[10] << 16 | (uint32_t)px[11] << 24;
  } else {
    for (int k = 0; k < 3 * npx; ++k) p[k] = px[k];
  }
}

// confusion[target][label] += 1 through nc * nc uint32 cells of LDS per workgroup of THREADS threads: zeroed (the caller's next barrier
// publishes that), one LDS atomic per pixel, then -- after a barrier of its own -- one 64-bit global atomic per non-zero cell.
template <int THREADS>
__device__ __forceinline__ void hist_zero(unsigned* hist, int nc) {
  for (int i = threadIdx.x; i < nc * nc; i += THREADS) hist[i] = 0u;
}
__device__ __forceinline__ void hist_add(unsigned* hist, int nc, int target, int label) { atomicAdd(&hist[target * nc + label], 1u); }
template <int THREADS>
__device__ __forceinline__ void hist_flush(const unsigned* hist, int nc, unsigned long long* confusion) {
  __syncthreads();
  for (int i = threadIdx.x; i < nc * nc; i += THREADS) {
    const unsigned v = hist[i];
    if (v) atomicAdd(confusion + i, (unsigned long long)v);
  }
}

}  // namespace
