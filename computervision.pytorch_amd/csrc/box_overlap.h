// The overlap arithmetic the suite pins bit for bit, shared by the NMS (nms.hip), Soft-NMS (soft_nms.hip), the tile merge (tiles.hip), the
// two fusions of views (det_tta.hip, box_fusion.hip) and the tracker (track.hip):
// plain operators with contraction switched off in each helper, every operation rounded on its own (the pragma does not reach into the
// _rn intrinsics' own bodies, so they are not used here).  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "cvx_common.h"

namespace {

__device__ __forceinline__ float box_area(const float4& b) {
#pragma clang fp contract(off)
  return (b.z - b.x) * (b.w - b.y);
}
// fp32 IoU exactly as torchvision's nms_kernel / oracle.nms_ref.greedy_nms_per_class
__device__ __forceinline__ bool iou_gt(const float4& a, float area_a, const float4& b, float area_b, float thr) {
#pragma clang fp contract(off)
  const float w = fmaxf(0.f, fminf(a.z, b.z) - fmaxf(a.x, b.x));
  const float h = fmaxf(0.f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
  const float inter = w * h;
  const float sum = area_a + area_b;
  const float ovr = inter / (sum - inter);
  return ovr > thr;
}
// the value iou_gt compares: the same operations in the same order (the tracker ranks its pairs by it, track.hip)
__device__ __forceinline__ float iou_value(const float4& a, float area_a, const float4& b, float area_b) {
#pragma clang fp contract(off)
  const float w = fmaxf(0.f, fminf(a.z, b.z) - fmaxf(a.x, b.x));
  const float h = fmaxf(0.f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
  const float inter = w * h;
  const float sum = area_a + area_b;
  return inter / (sum - inter);
}
// intersection over the smaller box, the same `inter`: a box cut by a tile border lies inside the whole box of the neighbouring tile
__device__ __forceinline__ bool ios_gt(const float4& a, float area_a, const float4& b, float area_b, float thr) {
#pragma clang fp contract(off)
  const float w = fmaxf(0.f, fminf(a.z, b.z) - fmaxf(a.x, b.x));
  const float h = fmaxf(0.f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
  const float inter = w * h;
  const float ovr = inter / fminf(area_a, area_b);
  return ovr > thr;
}

}  // namespace
