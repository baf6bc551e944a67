// nms.hip -- horizontal (axis-aligned) NMS for the Mask R-CNN config (the reference's mmdet/ops/nms: nms / batched_nms, the RPN proposals and the test-time
// multiclass NMS): lmv_nms (+ _workspace_bytes).  include/lemevit_hip.h has the semantics.  The structure is that of lmv_obb_nms (csrc/obb.hip):
//
//   mask launch    64 x 64 tiles of the rank-ordered boxes, upper triangle; a wave owns 16 rows of the tile, lane j evaluates (row, column j) and the ballot is the row's
//                  word.  Different groups never reach the pair rule.
//   reduce launch  nms_reduce.h, the reduce launch of the rotated NMS with this file's candidate rule.
#include "common.h"
#include "nms_reduce.h"
#include <math.h>

// No implicit fused multiply-adds: the pair rule rounds as nms_cpu.cpp's float32 build does, operation by operation.
#pragma clang fp contract(off)

namespace {

constexpr int HB_CAND = 1;          // record flag: NMS candidate

struct HbRec { float x1, y1, x2, y2, area; int flags, group; };

struct HbArgs {
  const float* boxes; int stride; const float* scores; const int64_t* order; const int32_t* groups;
  int N, nb; float iou_thr, score_thr; int cap; unsigned long long* mask; int64_t* keep; int64_t* count;
};

__device__ __forceinline__ HbRec hb_none() {
  HbRec r; r.x1 = r.y1 = r.x2 = r.y2 = r.area = 0.f; r.flags = 0; r.group = 0;
  return r;
}

// candidate: score > score_thr and four finite coordinates; an `order` entry outside [0, N) names no box
__device__ __forceinline__ bool hb_candidate(const HbArgs& a, int rank, int64_t* index) {
  if (rank >= a.N) return false;
  const int64_t idx = a.order[rank];
  if (idx < 0 || idx >= a.N) return false;
  *index = idx;
  const float* b = a.boxes + idx * a.stride;
  return isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]) && a.scores[idx] > a.score_thr;
}

__device__ __forceinline__ HbRec hb_load(const HbArgs& a, int rank) {
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

__global__ __launch_bounds__(256) void nms_mask_kernel(HbArgs a) {
  const int rb = blockIdx.y, cb = blockIdx.x;
  if (cb < rb) return;          // below the diagonal: never read
  __shared__ HbRec rows[64], cols[64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < 64) rows[tid] = hb_load(a, rb * 64 + tid);
  else if (tid < 128) cols[tid - 64] = hb_load(a, cb * 64 + tid - 64);
  __syncthreads();
  const HbRec q = cols[lane];
  const int qrank = cb * 64 + lane;
#pragma unroll 1
  for (int i = 0; i < 16; ++i) {
    const int r = wv * 16 + i, rrank = rb * 64 + r;
    if (rrank >= a.N) break;          // (wave-uniform)
    const HbRec p = rows[r];
    bool sup = false;
    if ((p.flags & q.flags & HB_CAND) && qrank > rrank && p.group == q.group) sup = hb_suppresses(p, q, a.iou_thr);
    const unsigned long long word = __ballot(sup);
    if (lane == 0) a.mask[(int64_t)rrank * a.nb + cb] = word;
  }
}

struct HbCandidate {
  __device__ __forceinline__ bool operator()(const HbArgs& a, int rank) const { int64_t idx; return hb_candidate(a, rank, &idx); }
};

__global__ __launch_bounds__(256) void nms_reduce_kernel(HbArgs a) { lmv_nms_reduce(a, HbCandidate()); }

}  // namespace

extern "C" size_t lmv_nms_workspace_bytes(int N) {
  if (N < 0 || N > LMV_NMS_MAX) return 0;
  return (size_t)N * (size_t)((N + 63) / 64) * 8;
}

extern "C" int lmv_nms(const float* boxes, int stride, const float* scores, const int64_t* order, const int32_t* groups, int N, float iou_thr, float score_thr,
                       int max_num, int phases, void* workspace, size_t workspace_bytes, int64_t* keep, int64_t* count, void* stream) {
  const char* fn = "nms";
  if (N < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: %d boxes (a negative size)", fn, N);
  if (stride < 4) LMV_FAIL(LMV_ERR_SHAPE, "%s: a row stride of %d floats (at least 4: x1, y1, x2, y2)", fn, stride);
  if (N > 0 && !boxes) LMV_FAIL(LMV_ERR_SHAPE, "%s: null boxes", fn);
  if (N > LMV_NMS_MAX) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = %d boxes, at most %d", fn, N, LMV_NMS_MAX);
  if (max_num < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: max_num = %d < 0 (0: no limit)", fn, max_num);
  if (iou_thr != iou_thr || score_thr != score_thr) LMV_FAIL(LMV_ERR_SHAPE, "%s: a NaN threshold (iou_thr = %g, score_thr = %g)", fn, iou_thr, score_thr);
  if (phases < 1 || phases > 3) LMV_FAIL(LMV_ERR_SHAPE, "%s: phases = %d outside 1 .. 3 (1: mask launch, 2: reduce launch, 3: both)", fn, phases);
  if (N > 0 && (!scores || !order)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null scores / order", fn);
  if (!count) LMV_FAIL(LMV_ERR_SHAPE, "%s: null count", fn);
  const int cap = max_num > 0 ? max_num : N;
  if (cap > 0 && !keep) LMV_FAIL(LMV_ERR_SHAPE, "%s: null keep", fn);
  if ((((uintptr_t)boxes) & 3u) || (((uintptr_t)scores) & 3u) || (((uintptr_t)groups) & 3u) || (((uintptr_t)order) & 7u) || (((uintptr_t)keep) & 7u) ||
      (((uintptr_t)count) & 7u) || (((uintptr_t)workspace) & 7u))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  const size_t need = lmv_nms_workspace_bytes(N);
  if (workspace_bytes < need || (need > 0 && !workspace)) LMV_FAIL(LMV_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (lmv_nms_workspace_bytes)", fn, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {          // no launch: count = 0, keep = -1 throughout
    if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot clear count", fn);
    if (cap > 0 && hipMemsetAsync(keep, 0xff, (size_t)cap * sizeof(int64_t), st) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot fill keep", fn);
    return LMV_OK;
  }
  HbArgs a;
  a.boxes = boxes; a.stride = stride; a.scores = scores; a.order = order; a.groups = groups;
  a.N = N; a.nb = (N + 63) / 64; a.iou_thr = iou_thr; a.score_thr = score_thr; a.cap = cap;
  a.mask = reinterpret_cast<unsigned long long*>(workspace); a.keep = keep; a.count = count;
  if (phases & 1) hipLaunchKernelGGL(nms_mask_kernel, dim3((unsigned)a.nb, (unsigned)a.nb), dim3(256), 0, st, a);
  if (phases & 2) hipLaunchKernelGGL(nms_reduce_kernel, dim3(1), dim3(256), 0, st, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}
