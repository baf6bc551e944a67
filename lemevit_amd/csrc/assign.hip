// assign.hip -- max-IoU target assignment without the [boxes x ground truths] matrix, for horizontal and rotated boxes (upstream mmdet 2.x MaxIoUAssigner, used twice
// per image by the Oriented R-CNN configs), and the horizontal overlaps matrix (upstream bbox_overlaps): lmv_max_iou_assign (+ _workspace_bytes), lmv_bbox_overlaps.
// The sources of MaxIoUAssigner and bbox_overlaps are not part of the reference tree: the rules restate upstream.  include/lemevit_hip.h has the semantics.
//
//   pair      ONE function per box kind: obb_pair (obb_pair.h, shared with obb.hip) for rotated boxes, hbx_pair below for horizontal ones.  The assignment's
//             v[j, n] is pair(box n, ground truth j), the argument order of the overlaps kernels: it equals their [n, j] element bit for bit.
//   overlaps  lmv_bbox_overlaps: the mapping of lmv_obb_overlaps -- a workgroup owns a 16 x 64 tile, a lane owns a column, stores run along M.
//   assign    a workgroup owns 256 boxes of one image, one record per thread in registers, and stages the image's ground-truth records through LDS in chunks of
//             LMV_ASSIGN_GT_CHUNK.
//               launch 1 (only with match_low_quality): the per-ground-truth maximum over the boxes.  IoU >= 0, so its bit pattern orders as an unsigned integer:
//                 lanes with v > 0 (few: most pairs are exactly 0) issue an LDS integer max on the 64-bit key (value bits << 32) | ~n, and the workgroup sends one
//                 global integer atomicMax per ground truth whose LDS key is non-zero into a table that a memset node zeroed.  The key's low word makes the LOWEST n
//                 win among equal values.  Integer maxima do not depend on arrival order: no floating-point atomics, two calls agree bit for bit.
//               launch 2: recomputes v with the same function; row maximum and argmax (lowest j) in registers; with gt_max_assign_all the largest j + 1 with
//                 v == gt_max[j] >= min_pos_iou; without it, the table's holders that fall into the workgroup's 256 boxes are gathered through LDS.  Writes every
//                 output element once.  The [N, G] values are never stored.
#include "common.h"
#include <math.h>

// No implicit fused multiply-adds (the rule of obb.hip): a pair rounds the same way in every kernel it is inlined into.
#pragma clang fp contract(off)

#include "obb_pair.h"

namespace {

constexpr int AS_TN = 16, AS_TM = 64;          // overlaps: rows x columns of a workgroup's tile
constexpr int AS_BOXES = 256;                  // assignment: boxes of a workgroup, one per thread
constexpr int AS_CHUNK = LMV_ASSIGN_GT_CHUNK;  // ground truths staged in LDS at a time
static_assert(AS_CHUNK <= AS_BOXES, "a chunk is loaded by one thread per ground truth");

// ---- the horizontal record and THE horizontal pair function ------------------------------------------------------------------------------------------------------
struct HbxRec { float x1, y1, x2, y2, area; int valid; };

__device__ __forceinline__ HbxRec hbx_none() {
  HbxRec r; r.x1 = r.y1 = r.x2 = r.y2 = r.area = 0.f; r.valid = 0;
  return r;
}

__device__ __forceinline__ HbxRec hbx_load(const float* b) {
  HbxRec r;
  r.x1 = b[0]; r.y1 = b[1]; r.x2 = b[2]; r.y2 = b[3];
  r.area = (r.x2 - r.x1) * (r.y2 - r.y1);
  r.valid = (isfinite(r.x1) && isfinite(r.y1) && isfinite(r.x2) && isfinite(r.y2)) ? 1 : 0;
  return r;
}

// upstream bbox_overlaps (no "+ 1"), eps = 1e-6: symmetric to the bit for iou (min, max and the sum of the areas commute); never negative, never NaN
__device__ __forceinline__ float hbx_pair(const HbxRec& p, const HbxRec& q, int mode) {
  if (!(p.valid & q.valid)) return 0.f;
  const float w = fmaxf(fminf(p.x2, q.x2) - fmaxf(p.x1, q.x1), 0.f);
  const float h = fmaxf(fminf(p.y2, q.y2) - fmaxf(p.y1, q.y1), 0.f);
  const float inter = w * h;
  const float v = mode == LMV_OBB_IOU ? inter / fmaxf(p.area + q.area - inter, 1e-6f) : inter / fmaxf(p.area, 1e-6f);
  return (isfinite(v) && v > 0.f) ? v : 0.f;
}

struct Horizontal {
  using Rec = HbxRec;
  static __device__ __forceinline__ Rec load(const float* b) { return hbx_load(b); }
  static __device__ __forceinline__ Rec none() { return hbx_none(); }
  static __device__ __forceinline__ float pair(const Rec& p, const Rec& q, int mode) { return hbx_pair(p, q, mode); }
};

struct Rotated {
  using Rec = ObbRec;
  static __device__ __forceinline__ Rec load(const float* b) { return obb_load(b); }
  static __device__ __forceinline__ Rec none() { return obb_none(); }
  static __device__ __forceinline__ float pair(const Rec& p, const Rec& q, int mode) { return obb_pair(p, q, mode); }
};

// ---- horizontal overlaps (the mapping of obb_overlaps_kernel) --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bbox_overlaps_kernel(const float* __restrict__ b1, int s1, int N, const float* __restrict__ b2, int s2, int M, int mode,
                                                            float* __restrict__ out) {
  __shared__ HbxRec rows[AS_TN], cols[AS_TM];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n0 = blockIdx.x * AS_TN, m0 = blockIdx.y * AS_TM;
  if (tid < AS_TM) {
    const int m = m0 + tid;
    cols[tid] = m < M ? hbx_load(b2 + (int64_t)m * s2) : hbx_none();
  } else if (tid < AS_TM + AS_TN) {
    const int n = n0 + tid - AS_TM;
    rows[tid - AS_TM] = n < N ? hbx_load(b1 + (int64_t)n * s1) : hbx_none();
  }
  __syncthreads();
  const HbxRec q = cols[lane];
  const int m = m0 + lane;
#pragma unroll 1
  for (int i = 0; i < AS_TN / 4; ++i) {
    const int r = wv * (AS_TN / 4) + i, n = n0 + r;
    if (n >= N) break;
    const float v = hbx_pair(rows[r], q, mode);
    if (m < M) out[(int64_t)n * M + m] = v;
  }
}

__global__ __launch_bounds__(256) void bbox_overlaps_aligned_kernel(const float* __restrict__ b1, int s1, const float* __restrict__ b2, int s2, int N, int mode,
                                                                    float* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const HbxRec p = hbx_load(b1 + (int64_t)n * s1), q = hbx_load(b2 + (int64_t)n * s2);
  out[n] = hbx_pair(p, q, mode);
}

// ---- assignment --------------------------------------------------------------------------------------------------------------------------------------------------
struct AsgArgs {
  const float* boxes; int box_stride; int64_t box_batch;          // box_batch: floats between the images' box sets; 0: one set shared by all images
  int N;
  const float* gts; int gt_stride; int Gmax;
  const int32_t* gt_counts; const int64_t* gt_labels; const uint8_t* ignore;
  float pos, neg_lo, neg_hi, min_pos; int low_quality, assign_all;
  unsigned long long* table;          // [B, Gmax + 1] keys; entry Gmax of an image: (1 << 32) | ~(its lowest box index that is not ignored)
  int64_t* gt_inds; float* max_overlaps; int64_t* labels;
};

__device__ __forceinline__ int asg_count(const AsgArgs& a, int b) {
  return a.gt_counts ? min(max(a.gt_counts[b], 0), a.Gmax) : a.Gmax;
}

// launch 1: table[b, j] = max over the boxes n that are not ignored and have v[j, n] > 0 of (bits of v << 32) | ~n
template <typename Kind>
__global__ __launch_bounds__(AS_BOXES) void assign_colmax_kernel(AsgArgs a) {
  using Rec = typename Kind::Rec;
  __shared__ Rec gt[AS_CHUNK];
  __shared__ unsigned long long key[AS_CHUNK];
  __shared__ unsigned first;          // ~(lowest index of a box of this workgroup that is not ignored); 0: none
  const int tid = threadIdx.x, b = blockIdx.y, n = blockIdx.x * AS_BOXES + tid;
  const int g = asg_count(a, b);
  if (g == 0) return;          // (uniform over the workgroup)
  const bool live = n < a.N && !(a.ignore && a.ignore[(int64_t)b * a.N + n]);
  const Rec box = n < a.N ? Kind::load(a.boxes + b * a.box_batch + (int64_t)n * a.box_stride) : Kind::none();
  if (tid == 0) first = 0u;
  const float* gts = a.gts + (int64_t)b * a.Gmax * a.gt_stride;
  unsigned long long* tab = a.table + (int64_t)b * (a.Gmax + 1);
  for (int j0 = 0; j0 < g; j0 += AS_CHUNK) {
    const int cnt = min(AS_CHUNK, g - j0);
    __syncthreads();          // the previous chunk's keys have been sent
    if (tid < AS_CHUNK) {
      gt[tid] = tid < cnt ? Kind::load(gts + (int64_t)(j0 + tid) * a.gt_stride) : Kind::none();
      key[tid] = 0ull;
    }
    __syncthreads();
    if (live) {
      for (int jj = 0; jj < cnt; ++jj) {
        const float v = Kind::pair(box, gt[jj], LMV_OBB_IOU);
        if (v > 0.f) atomicMax(&key[jj], ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(~(unsigned)n));
      }
    }
    __syncthreads();
    if (tid < cnt && key[tid] != 0ull) atomicMax(&tab[j0 + tid], key[tid]);
  }
  if (!a.assign_all) {          // a ground truth that overlaps nothing is held by the image's first box that is not ignored (the argmax of a row of zeros)
    if (live) atomicMax(&first, ~(unsigned)n);
    __syncthreads();
    if (tid == 0 && first != 0u) atomicMax(&tab[a.Gmax], (1ull << 32) | (unsigned long long)first);
  }
}

// launch 2 (the only one without match_low_quality): every output element, once
template <typename Kind>
__global__ __launch_bounds__(AS_BOXES) void assign_final_kernel(AsgArgs a) {
  using Rec = typename Kind::Rec;
  __shared__ Rec gt[AS_CHUNK];
  __shared__ float gmax[AS_CHUNK];
  __shared__ int own[AS_BOXES];
  const int tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * AS_BOXES, n = n0 + tid;
  const int g = asg_count(a, b);
  const bool inside = n < a.N;
  const bool live = inside && !(a.ignore && a.ignore[(int64_t)b * a.N + n]);
  const Rec box = inside ? Kind::load(a.boxes + b * a.box_batch + (int64_t)n * a.box_stride) : Kind::none();
  const float* gts = a.gts + (int64_t)b * a.Gmax * a.gt_stride;
  const unsigned long long* tab = a.table + (int64_t)b * (a.Gmax + 1);
  const bool all = a.low_quality && a.assign_all;
  float best = -1.f;
  int arg = 0, low = 0;          // low: the low-quality match, j + 1 (0: none)
  for (int j0 = 0; j0 < g; j0 += AS_CHUNK) {
    const int cnt = min(AS_CHUNK, g - j0);
    __syncthreads();
    if (tid < AS_CHUNK) {
      gt[tid] = tid < cnt ? Kind::load(gts + (int64_t)(j0 + tid) * a.gt_stride) : Kind::none();
      gmax[tid] = (all && tid < cnt) ? __uint_as_float((unsigned)(tab[j0 + tid] >> 32)) : 0.f;
    }
    __syncthreads();
    if (live) {
      for (int jj = 0; jj < cnt; ++jj) {
        float v = Kind::pair(box, gt[jj], LMV_OBB_IOU);
        v = v > 0.f ? v : 0.f;
        if (v > best) { best = v; arg = j0 + jj; }
        if (all && gmax[jj] >= a.min_pos && v == gmax[jj]) low = j0 + jj + 1;          // j ascending: the largest one stays
      }
    }
  }
  if (a.low_quality && !a.assign_all && g > 0) {          // gather the table's holders that are boxes of this workgroup
    own[tid] = 0;
    __syncthreads();
    const unsigned long long fkey = tab[a.Gmax];
    for (int j = tid; j < g; j += AS_BOXES) {
      const unsigned long long k = tab[j];
      if (!(__uint_as_float((unsigned)(k >> 32)) >= a.min_pos)) continue;
      const unsigned long long hk = k != 0ull ? k : fkey;
      if (hk == 0ull) continue;          // every box of the image is ignored
      const unsigned holder = ~(unsigned)hk;
      if (holder >= (unsigned)n0 && holder < (unsigned)n0 + AS_BOXES) atomicMax(&own[holder - (unsigned)n0], j + 1);
    }
    __syncthreads();
    low = own[tid];
  }
  if (!inside) return;
  int64_t ind;
  float mo;
  if (!live) { ind = -1; mo = -1.f; }
  else if (g == 0) { ind = 0; mo = 0.f; }
  else {
    mo = best;
    ind = mo >= a.pos ? arg + 1 : ((mo >= a.neg_lo && mo < a.neg_hi) ? 0 : -1);
    if (low > 0) ind = low;
  }
  const int64_t o = (int64_t)b * a.N + n;
  a.gt_inds[o] = ind;
  a.max_overlaps[o] = mo;
  if (a.labels) a.labels[o] = ind > 0 ? a.gt_labels[(int64_t)b * a.Gmax + (ind - 1)] : -1;
}

template <typename Kind>
void assign_launch(const AsgArgs& a, int B, bool two, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + AS_BOXES - 1) / AS_BOXES), (unsigned)B);
  if (two) hipLaunchKernelGGL(assign_colmax_kernel<Kind>, grid, dim3(AS_BOXES), 0, st, a);
  hipLaunchKernelGGL(assign_final_kernel<Kind>, grid, dim3(AS_BOXES), 0, st, a);
}

int hbx_check_boxes(const char* fn, const char* what, const float* b, int stride, int n) {
  if (n < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: %d %s (a negative size)", fn, n, what);
  if (stride < 4) LMV_FAIL(LMV_ERR_SHAPE, "%s: %s: a row stride of %d floats (at least 4: x1, y1, x2, y2)", fn, what, stride);
  if (n > 0 && !b) LMV_FAIL(LMV_ERR_SHAPE, "%s: null %s", fn, what);
  if (((uintptr_t)b) & 3u) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned %s", fn, what);
  return LMV_OK;
}

}  // namespace

extern "C" int lmv_bbox_overlaps(const float* b1, int stride1, int N, const float* b2, int stride2, int M, int mode, int aligned, float* out, void* stream) {
  const char* fn = "bbox_overlaps";
  if (int rc = hbx_check_boxes(fn, "boxes1", b1, stride1, N)) return rc;
  if (int rc = hbx_check_boxes(fn, "boxes2", b2, stride2, M)) return rc;
  if (mode != LMV_OBB_IOU && mode != LMV_OBB_IOF) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown mode %d (LMV_OBB_IOU / LMV_OBB_IOF)", fn, mode);
  if (aligned != 0 && aligned != 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: aligned = %d is neither 0 nor 1", fn, aligned);
  if (aligned && N != M) LMV_FAIL(LMV_ERR_SHAPE, "%s: aligned pairs need N == M, got %d and %d", fn, N, M);
  if (N > LMV_OBB_MAX_BOXES || M > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: %d x %d boxes: more than %d on a side", fn, N, M, LMV_OBB_MAX_BOXES);
  if (((uintptr_t)out) & 3u) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned out", fn);
  if (N == 0 || M == 0) return LMV_OK;
  if (!out) LMV_FAIL(LMV_ERR_SHAPE, "%s: null out", fn);
  if (aligned) {
    hipLaunchKernelGGL(bbox_overlaps_aligned_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, b1, stride1, b2, stride2, N, mode, out);
  } else {
    const dim3 grid((unsigned)((N + AS_TN - 1) / AS_TN), (unsigned)((M + AS_TM - 1) / AS_TM));
    hipLaunchKernelGGL(bbox_overlaps_kernel, grid, dim3(256), 0, (hipStream_t)stream, b1, stride1, N, b2, stride2, M, mode, out);
  }
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" size_t lmv_max_iou_assign_workspace_bytes(int B, int Gmax) {
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH || Gmax < 0 || Gmax > LMV_ASSIGN_MAX_GT) return 0;
  return (size_t)B * (size_t)(Gmax + 1) * 8;
}

extern "C" int lmv_max_iou_assign(int kind, const float* boxes, int box_stride, int64_t box_batch_stride, int N, const float* gts, int gt_stride, int B, int Gmax,
                                  const int32_t* gt_counts, const int64_t* gt_labels, const uint8_t* ignore, float pos_iou_thr, float neg_lo, float neg_hi,
                                  float min_pos_iou, int match_low_quality, int gt_max_assign_all, void* workspace, size_t workspace_bytes, int64_t* gt_inds,
                                  float* max_overlaps, int64_t* labels, void* stream) {
  const char* fn = "assign";
  if (kind != LMV_ASSIGN_HORIZONTAL && kind != LMV_ASSIGN_ROTATED) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown kind %d (LMV_ASSIGN_HORIZONTAL / LMV_ASSIGN_ROTATED)", fn, kind);
  const int k = kind == LMV_ASSIGN_ROTATED ? 5 : 4;
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH) LMV_FAIL(LMV_ERR_SHAPE, "%s: B = %d images outside 1 .. %d", fn, B, LMV_ASSIGN_MAX_BATCH);
  if (N < 0 || Gmax < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = %d boxes, Gmax = %d ground truths (a negative size)", fn, N, Gmax);
  if (N > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = %d boxes, at most %d", fn, N, LMV_OBB_MAX_BOXES);
  if (Gmax > LMV_ASSIGN_MAX_GT) LMV_FAIL(LMV_ERR_SHAPE, "%s: Gmax = %d ground truths, at most %d", fn, Gmax, LMV_ASSIGN_MAX_GT);
  if (box_stride < k || gt_stride < k) LMV_FAIL(LMV_ERR_SHAPE, "%s: row strides of %d (boxes) and %d (ground truths) floats, at least %d", fn, box_stride, gt_stride, k);
  if (box_batch_stride < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: a negative batch stride of the boxes (0: one set shared by all images)", fn);
  if (pos_iou_thr != pos_iou_thr || neg_lo != neg_lo || neg_hi != neg_hi || min_pos_iou != min_pos_iou)
    LMV_FAIL(LMV_ERR_SHAPE, "%s: a NaN threshold (pos_iou_thr = %g, neg = %g .. %g, min_pos_iou = %g)", fn, pos_iou_thr, neg_lo, neg_hi, min_pos_iou);
  if (neg_lo > neg_hi) LMV_FAIL(LMV_ERR_SHAPE, "%s: neg_lo = %g > neg_hi = %g", fn, neg_lo, neg_hi);
  if ((match_low_quality != 0 && match_low_quality != 1) || (gt_max_assign_all != 0 && gt_max_assign_all != 1))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: match_low_quality = %d, gt_max_assign_all = %d: flags are 0 or 1", fn, match_low_quality, gt_max_assign_all);
  if (N > 0 && !boxes) LMV_FAIL(LMV_ERR_SHAPE, "%s: null boxes", fn);
  if (Gmax > 0 && !gts) LMV_FAIL(LMV_ERR_SHAPE, "%s: null ground truths", fn);
  if (N > 0 && (!gt_inds || !max_overlaps)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null gt_inds / max_overlaps", fn);
  if (N > 0 && gt_labels && !labels) LMV_FAIL(LMV_ERR_SHAPE, "%s: null labels with gt_labels given", fn);
  if (labels && !gt_labels && Gmax > 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: labels without gt_labels (only with Gmax = 0, where every label is -1)", fn);
  if ((((uintptr_t)boxes) & 3u) || (((uintptr_t)gts) & 3u) || (((uintptr_t)gt_counts) & 3u) || (((uintptr_t)max_overlaps) & 3u) || (((uintptr_t)gt_labels) & 7u) ||
      (((uintptr_t)gt_inds) & 7u) || (((uintptr_t)labels) & 7u) || (((uintptr_t)workspace) & 7u))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  const size_t need = lmv_max_iou_assign_workspace_bytes(B, Gmax);
  if (workspace_bytes < need || !workspace) LMV_FAIL(LMV_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (lmv_max_iou_assign_workspace_bytes)", fn, workspace_bytes, need);
  if (N == 0) return LMV_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool two = match_low_quality && Gmax > 0;
  if (two && hipMemsetAsync(workspace, 0, need, st) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot clear the table", fn);
  AsgArgs a;
  a.boxes = boxes; a.box_stride = box_stride; a.box_batch = box_batch_stride; a.N = N;
  a.gts = gts; a.gt_stride = gt_stride; a.Gmax = Gmax; a.gt_counts = gt_counts; a.gt_labels = gt_labels; a.ignore = ignore;
  a.pos = pos_iou_thr; a.neg_lo = neg_lo; a.neg_hi = neg_hi; a.min_pos = min_pos_iou; a.low_quality = two ? 1 : 0; a.assign_all = gt_max_assign_all;
  a.table = reinterpret_cast<unsigned long long*>(workspace);
  a.gt_inds = gt_inds; a.max_overlaps = max_overlaps; a.labels = labels;          // (null gt_labels: Gmax = 0, no index is positive)
  if (kind == LMV_ASSIGN_ROTATED) assign_launch<Rotated>(a, B, two, st);
  else assign_launch<Horizontal>(a, B, two, st);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}
