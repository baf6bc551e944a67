// obb.hip -- rotated IoU and rotated NMS for the Oriented R-CNN configs (the reference's mmdet/ops/box_iou_rotated: obb_overlaps and mmdet/ops/nms_rotated: obb_nms /
// arb_batched_nms): lmv_obb_overlaps, lmv_obb_nms (+ _workspace_bytes).  include/lemevit_hip.h has the semantics; obb_pair.h has the pair function, this file the mappings.
//
//   pair      ONE device function, obb_pair, in fp32 from per-box records (cx, cy, w/2, h/2, cos, sin, half diagonal, flags, group) that are built once per box.
//             The corners of box A are expressed in the frame of box B (from the centre difference and the sine / cosine of the angle difference), where B is the
//             rectangle |u| <= W, |v| <= H, and the intersection area is the boundary integral
//                 I = sum over the four edges of A (counter-clockwise) of  INT (clamp(u, -W, W) - k) dv   over the part of the edge with v in [-H, H]
//             (for a fixed v the slice of A is an interval [uL, uR], its part inside the rectangle has length clamp(uR) - clamp(uL)).  On an edge the integrand is
//             piecewise linear with breakpoints where u crosses -W and +W, so three trapezoids give it exactly.  There is no polygon, no vertex count and no
//             decision about topology: min / max / select only, nothing indexed at run time (0 bytes of scratch), and the value is continuous in the boxes -- a
//             duplicate, its theta + pi twin, and its theta + pi / 2 twin with w and h swapped give I = w h to rounding.  Which box plays A is decided by a total order
//             on the records, so pair(p, q) == pair(q, p) bit for bit.
//   overlaps  a workgroup owns a 16 x 64 tile of the [N, M] matrix and stages its 16 + 64 records in LDS; a lane owns a column, so the stores run along M.
//   nms       nms_frame.h (shared with the horizontal NMS of nms.hip) has the mask launch, the reduce launch and the host side; this file has the record at a rank and
//             the candidate rule.  Different groups and pairs whose bounding circles are apart never reach the pair function.
#include "common.h"
#include "nms_frame.h"
#include <math.h>

// No implicit fused multiply-adds in this file (the explicit fmaf calls stay): the pair function then rounds the same way in every kernel it is inlined into, so the
// aligned pairs equal the diagonal of the matrix and the NMS decides on exactly the values the overlaps kernel reports.
#pragma clang fp contract(off)

#include "obb_pair.h"          // ObbRec, obb_load and THE pair function, obb_pair (shared with assign.hip)

namespace {

constexpr int OB_TN = 16, OB_TM = 64;          // overlaps: rows x columns of a workgroup's tile

// ---- overlaps ----------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void obb_overlaps_kernel(const float* __restrict__ b1, int s1, int N, const float* __restrict__ b2, int s2, int M, int mode,
                                                           float* __restrict__ out) {
  __shared__ ObbRec rows[OB_TN], cols[OB_TM];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n0 = blockIdx.x * OB_TN, m0 = blockIdx.y * OB_TM;
  if (tid < OB_TM) {
    const int m = m0 + tid;
    cols[tid] = m < M ? obb_load(b2 + (int64_t)m * s2) : obb_none();
  } else if (tid < OB_TM + OB_TN) {
    const int n = n0 + tid - OB_TM;
    rows[tid - OB_TM] = n < N ? obb_load(b1 + (int64_t)n * s1) : obb_none();
  }
  __syncthreads();
  const ObbRec q = cols[lane];
  const int m = m0 + lane;
#pragma unroll 1
  for (int i = 0; i < OB_TN / 4; ++i) {
    const int r = wv * (OB_TN / 4) + i, n = n0 + r;
    if (n >= N) break;
    const float v = obb_pair(rows[r], q, mode);
    if (m < M) out[(int64_t)n * M + m] = v;
  }
}

__global__ __launch_bounds__(256) void obb_overlaps_aligned_kernel(const float* __restrict__ b1, int s1, const float* __restrict__ b2, int s2, int N, int mode,
                                                                   float* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const ObbRec p = obb_load(b1 + (int64_t)n * s1), q = obb_load(b2 + (int64_t)n * s2);
  out[n] = obb_pair(p, q, mode);
}

// ---- NMS ---------------------------------------------------------------------------------------------------------------------------------------------------------
// the record of the box at a rank; an `order` entry outside [0, N) reads nothing and is no candidate
__device__ __forceinline__ ObbRec nms_load(const NmsArgs& a, int rank) {
  if (rank >= a.N) return obb_none();
  const int64_t idx = a.order[rank];
  if (idx < 0 || idx >= a.N) return obb_none();
  ObbRec r = obb_load(a.boxes + idx * a.stride);
  const float sc = a.scores[idx];
  if ((r.flags & OB_VALID) ? sc > a.score_thr : false) r.flags |= OB_CAND;
  r.group = a.groups ? a.groups[idx] : 0;
  return r;
}

// candidate test alone (the reduce launch): score > score_thr and both sides >= 0.001, the rule of nms_load's flag for finite boxes; a non-finite box has no IoU
// with anything and is no candidate either
__device__ __forceinline__ bool nms_candidate(const NmsArgs& a, int rank) {
  if (rank >= a.N) return false;
  const int64_t idx = a.order[rank];
  if (idx < 0 || idx >= a.N) return false;
  const float* b = a.boxes + idx * a.stride;
  const float cx = b[0], cy = b[1], w = b[2], h = b[3], th = b[4];
  const float hw = 0.5f * w, hh = 0.5f * h;
  const bool finite = isfinite(cx) && isfinite(cy) && isfinite(w) && isfinite(h) && isfinite(th) && isfinite(sqrtf(hw * hw + hh * hh));
  return finite && w >= OB_MIN_SIDE && h >= OB_MIN_SIDE && a.scores[idx] > a.score_thr;
}

__global__ __launch_bounds__(256) void obb_nms_mask_kernel(NmsArgs a) {
  lmv_nms_mask<ObbRec, OB_CAND>(a, [](const NmsArgs& a, int rank) { return nms_load(a, rank); },
                                [&](const ObbRec& p, const ObbRec& q) { return obb_pair(p, q, LMV_OBB_IOU) > a.iou_thr; });
}

struct ObbCandidate {
  __device__ __forceinline__ bool operator()(const NmsArgs& a, int rank) const { return nms_candidate(a, rank); }
};

__global__ __launch_bounds__(256) void obb_nms_reduce_kernel(NmsArgs a) { lmv_nms_reduce(a, ObbCandidate()); }

constexpr NmsOp OB_OP = {"obb_nms", 5, "cx, cy, w, h, theta", LMV_OBB_NMS_MAX, "lmv_obb_nms_workspace_bytes", obb_nms_mask_kernel, obb_nms_reduce_kernel};

int obb_check_boxes(const char* fn, const char* what, const float* b, int stride, int n) {
  if (n < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: %d %s (a negative size)", fn, n, what);
  if (stride < 5) LMV_FAIL(LMV_ERR_SHAPE, "%s: %s: a row stride of %d floats (at least 5: cx, cy, w, h, theta)", fn, what, stride);
  if (n > 0 && !b) LMV_FAIL(LMV_ERR_SHAPE, "%s: null %s", fn, what);
  if (((uintptr_t)b) & 3u) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned %s", fn, what);
  return LMV_OK;
}

}  // namespace

extern "C" int lmv_obb_overlaps(const float* b1, int stride1, int N, const float* b2, int stride2, int M, int mode, int aligned, float* out, void* stream) {
  const char* fn = "obb_overlaps";
  if (int rc = obb_check_boxes(fn, "boxes1", b1, stride1, N)) return rc;
  if (int rc = obb_check_boxes(fn, "boxes2", b2, stride2, M)) return rc;
  if (mode != LMV_OBB_IOU && mode != LMV_OBB_IOF) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown mode %d (LMV_OBB_IOU / LMV_OBB_IOF)", fn, mode);
  if (aligned != 0 && aligned != 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: aligned = %d is neither 0 nor 1", fn, aligned);
  if (aligned && N != M) LMV_FAIL(LMV_ERR_SHAPE, "%s: aligned pairs need N == M, got %d and %d", fn, N, M);
  if (N > LMV_OBB_MAX_BOXES || M > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: %d x %d boxes: more than %d on a side", fn, N, M, LMV_OBB_MAX_BOXES);
  if (((uintptr_t)out) & 3u) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned out", fn);
  if (N == 0 || M == 0) return LMV_OK;
  if (!out) LMV_FAIL(LMV_ERR_SHAPE, "%s: null out", fn);
  if (aligned) {
    hipLaunchKernelGGL(obb_overlaps_aligned_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, b1, stride1, b2, stride2, N, mode, out);
  } else {
    const dim3 grid((unsigned)((N + OB_TN - 1) / OB_TN), (unsigned)((M + OB_TM - 1) / OB_TM));
    hipLaunchKernelGGL(obb_overlaps_kernel, grid, dim3(256), 0, (hipStream_t)stream, b1, stride1, N, b2, stride2, M, mode, out);
  }
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" size_t lmv_obb_nms_workspace_bytes(int N) { return lmv_nms_bytes(N, LMV_OBB_NMS_MAX); }

extern "C" int lmv_obb_nms(const float* boxes, int stride, const float* scores, const int64_t* order, const int32_t* groups, int N, float iou_thr, float score_thr,
                           int max_num, int phases, void* workspace, size_t workspace_bytes, int64_t* keep, int64_t* count, void* stream) {
  return lmv_nms_run(OB_OP, boxes, stride, scores, order, groups, N, iou_thr, score_thr, max_num, phases, workspace, workspace_bytes, keep, count, stream);
}
