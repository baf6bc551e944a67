// nms.hip -- horizontal (axis-aligned) NMS for the Mask R-CNN config (the reference's mmdet/ops/nms: nms / batched_nms, the RPN proposals and the test-time
// multiclass NMS): lmv_nms (+ _workspace_bytes).  include/lemevit_hip.h has the semantics.  nms_frame.h, shared with lmv_obb_nms (csrc/obb.hip), has the mask launch,
// the reduce launch and the host side; this file has the box record, the candidate rule and the pair rule.
#include "common.h"
#include "nms_frame.h"
#include <math.h>

// No implicit fused multiply-adds: the pair rule rounds as nms_cpu.cpp's float32 build does, operation by operation.
#pragma clang fp contract(off)

namespace {

constexpr int HB_CAND = 1;          // record flag: NMS candidate

struct HbRec { float x1, y1, x2, y2, area; int flags, group; };

__device__ __forceinline__ HbRec hb_none() {
  HbRec r; r.x1 = r.y1 = r.x2 = r.y2 = r.area = 0.f; r.flags = 0; r.group = 0;
  return r;
}

// candidate: score > score_thr and four finite coordinates; an `order` entry outside [0, N) names no box
__device__ __forceinline__ bool hb_candidate(const NmsArgs& a, int rank, int64_t* index) {
  if (rank >= a.N) return false;
  const int64_t idx = a.order[rank];
  if (idx < 0 || idx >= a.N) return false;
  *index = idx;
  const float* b = a.boxes + idx * a.stride;
  return isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]) && a.scores[idx] > a.score_thr;
}

__device__ __forceinline__ HbRec hb_load(const NmsArgs& a, int rank) {
  int64_t idx = 0;
  if (!hb_candidate(a, rank, &idx)) return hb_none();
  const float* b = a.boxes + idx * a.stride;
  HbRec r;
  r.x1 = b[0]; r.y1 = b[1]; r.x2 = b[2]; r.y2 = b[3];
  r.area = (r.x2 - r.x1) * (r.y2 - r.y1);
  r.flags = HB_CAND;
  r.group = a.groups ? a.groups[idx] : 0;
  return r;
}

// THE pair rule (nms_cpu.cpp): a NaN quotient (two zero-area boxes) is not above any threshold
__device__ __forceinline__ bool hb_suppresses(const HbRec& p, const HbRec& q, float thr) {
  const float w = fmaxf(0.f, fminf(p.x2, q.x2) - fmaxf(p.x1, q.x1));
  const float h = fmaxf(0.f, fminf(p.y2, q.y2) - fmaxf(p.y1, q.y1));
  const float inter = w * h;
  return inter / (p.area + q.area - inter) > thr;
}

__global__ __launch_bounds__(256) void nms_mask_kernel(NmsArgs a) {
  lmv_nms_mask<HbRec, HB_CAND>(a, [](const NmsArgs& a, int rank) { return hb_load(a, rank); },
                               [&](const HbRec& p, const HbRec& q) { return hb_suppresses(p, q, a.iou_thr); });
}

struct HbCandidate {
  __device__ __forceinline__ bool operator()(const NmsArgs& a, int rank) const { int64_t idx; return hb_candidate(a, rank, &idx); }
};

__global__ __launch_bounds__(256) void nms_reduce_kernel(NmsArgs a) { lmv_nms_reduce(a, HbCandidate()); }

constexpr NmsOp HB_OP = {"nms", 4, "x1, y1, x2, y2", LMV_NMS_MAX, "lmv_nms_workspace_bytes", nms_mask_kernel, nms_reduce_kernel};

}  // namespace

extern "C" size_t lmv_nms_workspace_bytes(int N) { return lmv_nms_bytes(N, LMV_NMS_MAX); }

extern "C" int lmv_nms(const float* boxes, int stride, const float* scores, const int64_t* order, const int32_t* groups, int N, float iou_thr, float score_thr,
                       int max_num, int phases, void* workspace, size_t workspace_bytes, int64_t* keep, int64_t* count, void* stream) {
  return lmv_nms_run(HB_OP, boxes, stride, scores, order, groups, N, iou_thr, score_thr, max_num, phases, workspace, workspace_bytes, keep, count, stream);
}

