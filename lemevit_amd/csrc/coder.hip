// coder.hip -- the box coders of the Oriented R-CNN configs: MidpointOffsetCoder (RPN head) and OBB2OBBDeltaXYWHTCoder (R-CNN head), encode and decode:
// lmv_box_encode, lmv_box_decode, lmv_box_decode_map.  The coders' sources are not part of the reference tree: the rules restate upstream (OBBDetection on mmdet 2.x).
// include/lemevit_hip.h has the rules and the semantics.
//
//   rule      ONE device function per rule (cd_midpoint_encode, cd_midpoint_decode, cd_obb_encode, cd_obb_decode), inlined into every kernel: the aligned and the
//             gathering encode, the plain, the class-specific and the map decode agree bit for bit on the same operands.
//   mapping   one thread per output row (decode: per (row, delta set)), 256 threads per workgroup; boxes, ground truths, deltas and the regression map are read in
//             place through their strides; every output element is written once.  No LDS, no atomics, no synchronisation.
#include "coder_rules.h"

namespace {

constexpr int CD_THREADS = 256;

struct Midpoint {
  static constexpr int K = 4, D = 6;
  static __device__ __forceinline__ void encode(const float* p, const float* g, const CdNorm& nm, float* d) { cd_midpoint_encode(p, g, nm, d); }
  static __device__ __forceinline__ void decode(const float* p, const float* d, const CdNorm& nm, float mr, float* o) { cd_midpoint_decode(p, d, nm, mr, o); }
};

struct Obb2Obb {
  static constexpr int K = 5, D = 5;
  static __device__ __forceinline__ void encode(const float* p, const float* g, const CdNorm& nm, float* d) { cd_obb_encode(p, g, nm, d); }
  static __device__ __forceinline__ void decode(const float* p, const float* d, const CdNorm& nm, float mr, float* o) { cd_obb_decode(p, d, nm, mr, o); }
};

// ---- kernels -------------------------------------------------------------------------------------------------------------------------------------------------------
struct EncArgs {
  const float* boxes; int box_stride; int64_t box_batch; int N;
  const float* gts; int gt_stride; int Gmax;
  const int32_t* gt_counts; const int64_t* gt_inds; const uint8_t* sampled;
  CdNorm nm;
  float* targets; float* weights;
};

template <typename Coder>
__global__ __launch_bounds__(CD_THREADS) void box_encode_kernel(EncArgs a) {
  const int n = blockIdx.x * CD_THREADS + threadIdx.x, b = blockIdx.y;
  if (n >= a.N) return;
  const int64_t o = (int64_t)b * a.N + n;
  const int count = a.gt_counts ? min(max(a.gt_counts[b], 0), a.Gmax) : a.Gmax;
  const int64_t ind = a.gt_inds ? a.gt_inds[o] : (int64_t)n + 1;          // null: the aligned form
  const bool live = ind >= 1 && ind <= (int64_t)count && !(a.sampled && a.sampled[o] == 0);
  float d[Coder::D];
#pragma unroll
  for (int i = 0; i < Coder::D; ++i) d[i] = 0.f;
  if (live) {          // (only then is a ground-truth row read: ind - 1 < count <= Gmax)
    const float* pb = a.boxes + b * a.box_batch + (int64_t)n * a.box_stride;
    const float* gb = a.gts + ((int64_t)b * a.Gmax + (ind - 1)) * a.gt_stride;
    float p[Coder::K], g[5];
#pragma unroll
    for (int i = 0; i < Coder::K; ++i) p[i] = pb[i];
#pragma unroll
    for (int i = 0; i < 5; ++i) g[i] = gb[i];
    Coder::encode(p, g, a.nm, d);
  }
  float* t = a.targets + o * Coder::D;
#pragma unroll
  for (int i = 0; i < Coder::D; ++i) t[i] = d[i];
  a.weights[o] = live ? 1.f : 0.f;
}

// one thread per (row n, delta set c): i = n C + c, also the output row
template <typename Coder>
__global__ __launch_bounds__(CD_THREADS) void box_decode_kernel(const float* __restrict__ boxes, int box_stride, const float* __restrict__ deltas, int64_t delta_stride,
                                                                int64_t rows, int C, CdNorm nm, float max_ratio, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * CD_THREADS + threadIdx.x;
  if (i >= rows) return;
  const int64_t n = i / C;
  const int c = (int)(i - n * C);
  const float* pb = boxes + n * box_stride;
  const float* db = deltas + n * delta_stride + (int64_t)c * Coder::D;
  float p[Coder::K], d[Coder::D], o[5];
#pragma unroll
  for (int j = 0; j < Coder::K; ++j) p[j] = pb[j];
#pragma unroll
  for (int j = 0; j < Coder::D; ++j) d[j] = db[j];
  Coder::decode(p, d, nm, max_ratio, o);
  float* t = out + i * 5;
#pragma unroll
  for (int j = 0; j < 5; ++j) t[j] = o[j];
}

struct MapArgs {
  const float* boxes; int box_stride; int gathered;
  const float* map; int A, H, W; int64_t sc, sh, sw;
  const int64_t* index; int K;
  CdNorm nm; float max_ratio;
  float* out;
};

template <typename Coder>
__global__ __launch_bounds__(CD_THREADS) void box_decode_map_kernel(MapArgs a) {
  const int i = blockIdx.x * CD_THREADS + threadIdx.x;
  if (i >= a.K) return;
  const int64_t r = a.index[i], total = (int64_t)a.H * a.W * a.A;
  float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (r >= 0 && r < total) {          // (only then is anything else read)
    const int64_t pos = r / a.A;
    const int an = (int)(r - pos * a.A), h = (int)(pos / a.W), w = (int)(pos - (int64_t)h * a.W);
    const float* pb = a.boxes + (a.gathered ? (int64_t)i : r) * a.box_stride;
    const float* db = a.map + (int64_t)an * Coder::D * a.sc + h * a.sh + w * a.sw;
    float p[Coder::K], d[Coder::D];
#pragma unroll
    for (int j = 0; j < Coder::K; ++j) p[j] = pb[j];
#pragma unroll
    for (int j = 0; j < Coder::D; ++j) d[j] = db[j * a.sc];
    Coder::decode(p, d, a.nm, a.max_ratio, o);
  }
  float* t = a.out + (int64_t)i * 5;
#pragma unroll
  for (int j = 0; j < 5; ++j) t[j] = o[j];
}

// ---- host checks -----------------------------------------------------------------------------------------------------------------------------------------------------
int cd_kind(const char* fn, int kind, int* k, int* D) {
  if (kind != LMV_CODER_MIDPOINT && kind != LMV_CODER_OBB2OBB) LMV_FAIL(LMV_ERR_SHAPE, "%s: unknown kind %d (LMV_CODER_MIDPOINT / LMV_CODER_OBB2OBB)", fn, kind);
  *k = kind == LMV_CODER_MIDPOINT ? 4 : 5;
  *D = kind == LMV_CODER_MIDPOINT ? 6 : 5;
  return LMV_OK;
}

int cd_norm(const char* fn, const float* means, const float* stds, int D, CdNorm* nm) {
  if (!means || !stds) LMV_FAIL(LMV_ERR_SHAPE, "%s: null means / stds (host arrays of %d floats)", fn, D);
  for (int i = 0; i < CD_MAX_D; ++i) {
    nm->mean[i] = i < D ? means[i] : 0.f;
    nm->std[i] = i < D ? stds[i] : 1.f;
    if (nm->mean[i] != nm->mean[i] || nm->std[i] != nm->std[i]) LMV_FAIL(LMV_ERR_SHAPE, "%s: a NaN mean or std (entry %d)", fn, i);
  }
  return LMV_OK;
}

int cd_clip(const char* fn, float wh_ratio_clip, float* max_ratio) {
  if (!(wh_ratio_clip > 0.f) || !isfinite(wh_ratio_clip)) LMV_FAIL(LMV_ERR_SHAPE, "%s: wh_ratio_clip = %g is not a positive finite number", fn, wh_ratio_clip);
  *max_ratio = (float)fabs(log((double)wh_ratio_clip));
  return LMV_OK;
}

}  // namespace

extern "C" int lmv_box_encode(int kind, const float* boxes, int box_stride, int64_t box_batch_stride, int N, const float* gts, int gt_stride, int B, int Gmax,
                              const int32_t* gt_counts, const int64_t* gt_inds, const uint8_t* sampled, const float* means, const float* stds, float* targets,
                              float* weights, void* stream) {
  const char* fn = "box_encode";
  int k, D;
  if (int rc = cd_kind(fn, kind, &k, &D)) return rc;
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH) LMV_FAIL(LMV_ERR_SHAPE, "%s: B = %d images outside 1 .. %d", fn, B, LMV_ASSIGN_MAX_BATCH);
  if (N < 0 || Gmax < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = %d boxes, Gmax = %d ground truths (a negative size)", fn, N, Gmax);
  if (N > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = %d boxes, at most %d", fn, N, LMV_OBB_MAX_BOXES);
  if (Gmax > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: Gmax = %d ground truths, at most %d", fn, Gmax, LMV_OBB_MAX_BOXES);
  if (box_stride < k || gt_stride < 5) LMV_FAIL(LMV_ERR_SHAPE, "%s: row strides of %d (boxes, at least %d) and %d (ground truths, at least 5) floats", fn, box_stride, k, gt_stride);
  if (box_batch_stride < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: a negative batch stride of the boxes (0: one set shared by all images)", fn);
  if (!gt_inds && Gmax != N) LMV_FAIL(LMV_ERR_SHAPE, "%s: the aligned form (null gt_inds) pairs row n with ground truth n: Gmax = %d is not N = %d", fn, Gmax, N);
  CdNorm nm;
  if (int rc = cd_norm(fn, means, stds, D, &nm)) return rc;
  if (N > 0 && !boxes) LMV_FAIL(LMV_ERR_SHAPE, "%s: null boxes", fn);
  if (N > 0 && Gmax > 0 && !gts) LMV_FAIL(LMV_ERR_SHAPE, "%s: null ground truths", fn);
  if (N > 0 && (!targets || !weights)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null targets / weights", fn);
  if ((((uintptr_t)boxes) & 3u) || (((uintptr_t)gts) & 3u) || (((uintptr_t)gt_counts) & 3u) || (((uintptr_t)targets) & 3u) || (((uintptr_t)weights) & 3u) ||
      (((uintptr_t)gt_inds) & 7u))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  if (N == 0) return LMV_OK;
  EncArgs a;
  a.boxes = boxes; a.box_stride = box_stride; a.box_batch = box_batch_stride; a.N = N;
  a.gts = gts; a.gt_stride = gt_stride; a.Gmax = Gmax; a.gt_counts = gt_counts; a.gt_inds = gt_inds; a.sampled = sampled;
  a.nm = nm; a.targets = targets; a.weights = weights;
  const dim3 grid((unsigned)((N + CD_THREADS - 1) / CD_THREADS), (unsigned)B);
  if (kind == LMV_CODER_MIDPOINT) hipLaunchKernelGGL(box_encode_kernel<Midpoint>, grid, dim3(CD_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(box_encode_kernel<Obb2Obb>, grid, dim3(CD_THREADS), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_box_decode(int kind, const float* boxes, int box_stride, const float* deltas, int64_t delta_stride, int N, int C, const float* means,
                              const float* stds, float wh_ratio_clip, float* out, void* stream) {
  const char* fn = "box_decode";
  int k, D;
  if (int rc = cd_kind(fn, kind, &k, &D)) return rc;
  if (N < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = %d rows (a negative size)", fn, N);
  if (N > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = %d rows, at most %d", fn, N, LMV_OBB_MAX_BOXES);
  if (C < 1 || C > LMV_CODER_MAX_SETS) LMV_FAIL(LMV_ERR_SHAPE, "%s: C = %d delta sets per row outside 1 .. %d", fn, C, LMV_CODER_MAX_SETS);
  if (box_stride < k) LMV_FAIL(LMV_ERR_SHAPE, "%s: a box row stride of %d floats, at least %d", fn, box_stride, k);
  if (delta_stride < (int64_t)D * C) LMV_FAIL(LMV_ERR_SHAPE, "%s: a delta row stride of %lld floats, at least D C = %d", fn, (long long)delta_stride, D * C);
  CdNorm nm;
  float max_ratio;
  if (int rc = cd_norm(fn, means, stds, D, &nm)) return rc;
  if (int rc = cd_clip(fn, wh_ratio_clip, &max_ratio)) return rc;
  if (N > 0 && (!boxes || !deltas || !out)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null boxes / deltas / out", fn);
  if ((((uintptr_t)boxes) & 3u) || (((uintptr_t)deltas) & 3u) || (((uintptr_t)out) & 3u)) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  if (N == 0) return LMV_OK;
  const int64_t rows = (int64_t)N * C;
  const dim3 grid((unsigned)((rows + CD_THREADS - 1) / CD_THREADS));
  if (kind == LMV_CODER_MIDPOINT)
    hipLaunchKernelGGL(box_decode_kernel<Midpoint>, grid, dim3(CD_THREADS), 0, (hipStream_t)stream, boxes, box_stride, deltas, delta_stride, rows, C, nm, max_ratio, out);
  else
    hipLaunchKernelGGL(box_decode_kernel<Obb2Obb>, grid, dim3(CD_THREADS), 0, (hipStream_t)stream, boxes, box_stride, deltas, delta_stride, rows, C, nm, max_ratio, out);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_box_decode_map(int kind, const float* boxes, int box_stride, int gathered, const float* map, int A, int H, int W, int64_t map_stride_c,
                                  int64_t map_stride_h, int64_t map_stride_w, const int64_t* index, int K, const float* means, const float* stds, float wh_ratio_clip,
                                  float* out, void* stream) {
  const char* fn = "box_decode_map";
  int k, D;
  if (int rc = cd_kind(fn, kind, &k, &D)) return rc;
  if (K < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: K = %d rows (a negative size)", fn, K);
  if (K > LMV_OBB_MAX_BOXES) LMV_FAIL(LMV_ERR_SHAPE, "%s: K = %d rows, at most %d", fn, K, LMV_OBB_MAX_BOXES);
  if (A < 1 || H < 1 || W < 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: a map of %d anchors x %d x %d positions (each at least 1)", fn, A, H, W);
  if ((int64_t)H * W > 2147483647ll / A) LMV_FAIL(LMV_ERR_SHAPE, "%s: H W A = %d x %d x %d rows, at most 2^31 - 1", fn, H, W, A);
  if (gathered != 0 && gathered != 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: gathered = %d is neither 0 nor 1", fn, gathered);
  if (box_stride < k) LMV_FAIL(LMV_ERR_SHAPE, "%s: a box row stride of %d floats, at least %d", fn, box_stride, k);
  CdNorm nm;
  float max_ratio;
  if (int rc = cd_norm(fn, means, stds, D, &nm)) return rc;
  if (int rc = cd_clip(fn, wh_ratio_clip, &max_ratio)) return rc;
  if (K > 0 && (!boxes || !map || !index || !out)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null boxes / map / index / out", fn);
  if ((((uintptr_t)boxes) & 3u) || (((uintptr_t)map) & 3u) || (((uintptr_t)out) & 3u) || (((uintptr_t)index) & 7u)) LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  if (K == 0) return LMV_OK;
  MapArgs a;
  a.boxes = boxes; a.box_stride = box_stride; a.gathered = gathered;
  a.map = map; a.A = A; a.H = H; a.W = W; a.sc = map_stride_c; a.sh = map_stride_h; a.sw = map_stride_w;
  a.index = index; a.K = K; a.nm = nm; a.max_ratio = max_ratio; a.out = out;
  const dim3 grid((unsigned)((K + CD_THREADS - 1) / CD_THREADS));
  if (kind == LMV_CODER_MIDPOINT) hipLaunchKernelGGL(box_decode_map_kernel<Midpoint>, grid, dim3(CD_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(box_decode_map_kernel<Obb2Obb>, grid, dim3(CD_THREADS), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}
