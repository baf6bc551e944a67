// nms_frame.h -- the frame that rotated NMS (obb.hip) and horizontal NMS (nms.hip) share; the box record, its loader, the pair rule and the candidate rule stay in
// their files, behind the named kernels.
//
//   mask launch    64 x 64 tiles of the rank-ordered boxes, upper triangle; a wave owns 16 rows of the tile, lane j evaluates (row, column j) and the ballot is the row's
//                  word, written by lane 0.  Non-candidates, different groups and the lower triangle of a diagonal tile never reach the pair rule.
//   reduce launch  from the suppression words to keep[] and count: one workgroup, thread c owns word c of the `removed` bit vector in a register.  Per block of 64
//                  ranks: every thread loads the 64 row words of its own column block (independent loads, issued before the serial part), wave 0 resolves the diagonal
//                  word serially on the scalar unit (row r's word is read out of lane r's registers: no memory access in the 64-step chain), and every thread ORs the
//                  rows that were kept into its word.  Then a scan over the popcounts places the kept ranks in keep[], the tail is -1, count is written.
//   host           one validation, the N == 0 memsets and the `phases` launch pair (NmsOp holds what differs: names, row stride, limit, kernels).
//
// No floating-point arithmetic lives here; the files that include it switch contraction off for their pair rules.
#pragma once
#include "common.h"

namespace {

struct NmsArgs {
  const float* boxes; int stride; const float* scores; const int64_t* order; const int32_t* groups;
  int N, nb; float iou_thr, score_thr; int cap; unsigned long long* mask; int64_t* keep; int64_t* count;
};

// Rec: the box record with `flags` (CAND: the bit of an NMS candidate) and `group`; load(a, rank) -> Rec; suppresses(p, q): THE pair rule of the box type against a.iou_thr
template <typename Rec, int CAND, typename Load, typename Pair>
__device__ __forceinline__ void lmv_nms_mask(const NmsArgs& a, Load load, Pair suppresses) {
  const int rb = blockIdx.y, cb = blockIdx.x;
  if (cb < rb) return;          // below the diagonal: never read
  __shared__ Rec rows[64], cols[64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < 64) rows[tid] = load(a, rb * 64 + tid);
  else if (tid < 128) cols[tid - 64] = load(a, cb * 64 + tid - 64);
  __syncthreads();
  const Rec q = cols[lane];
  const int qrank = cb * 64 + lane;
#pragma unroll 1
  for (int i = 0; i < 16; ++i) {
    const int r = wv * 16 + i, rrank = rb * 64 + r;
    if (rrank >= a.N) break;          // (wave-uniform)
    const Rec p = rows[r];
    bool sup = false;
    if ((p.flags & q.flags & CAND) && qrank > rrank && p.group == q.group) sup = suppresses(p, q);
    const unsigned long long word = __ballot(sup);
    if (lane == 0) a.mask[(int64_t)rrank * a.nb + cb] = word;
  }
}

// Cand: bool operator()(const NmsArgs&, int rank), the candidate rule of the box type
template <typename Cand>
__device__ __forceinline__ void lmv_nms_reduce(const NmsArgs& a, Cand candidate) {
  __shared__ unsigned long long cur_sh, kept_sh;
  __shared__ int scan[256];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = a.N, nb = a.nb;
  // removed bits to start with: ranks past N and non-candidates.  Wave w builds words w, w + 4, ...; thread c then takes word c.
  __shared__ unsigned long long init[256];
  for (int w = wv; w < nb; w += 4) {
    const unsigned long long word = __ballot(!candidate(a, w * 64 + lane));
    if (lane == 0) init[w] = word;
  }
  __syncthreads();
  unsigned long long mine = tid < nb ? init[tid] : ~0ull;
  for (int b = 0; b < nb; ++b) {
    const int nrows = min(64, N - b * 64);
    // this thread's column of the block's rows: independent loads, in flight during the serial part
    unsigned long long wrow[64];
    const bool active = tid > b && tid < nb;
    const unsigned long long* src = a.mask + (int64_t)b * 64 * nb + tid;
#pragma unroll
    for (int r = 0; r < 64; ++r) wrow[r] = (active && r < nrows) ? src[(int64_t)r * nb] : 0ull;
    if (tid == b) cur_sh = mine;
    unsigned long long dword = 0ull;          // wave 0: lane r holds the diagonal word of row r
    if (tid < nrows) dword = a.mask[((int64_t)b * 64 + tid) * nb + b];
    __syncthreads();
    if (wv == 0) {
      // the serial part on the scalar unit: `cur` is wave-uniform, row r's word comes out of lane r's registers (a constant lane: v_readlane), no memory in the chain
      const unsigned long long c0 = cur_sh;
      // (the builtins return int: every half goes through `unsigned` before it is widened, or a set bit 31 would smear over the upper word)
      unsigned long long cur = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(c0 >> 32)) << 32) |
                               (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)c0);
      const int dlo = (int)(unsigned)dword, dhi = (int)(unsigned)(dword >> 32);
#pragma unroll
      for (int r = 0; r < 64; ++r) {
        const unsigned long long w = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, r) << 32) | (unsigned long long)(unsigned)__builtin_amdgcn_readlane(dlo, r);
        if (!((cur >> r) & 1ull)) cur |= w;          // row r is kept: it removes what it overlaps (bits above r only)
      }
      if (lane == 0) kept_sh = ~cur;
    }
    __syncthreads();
    const unsigned long long kept = kept_sh;
    if (tid == b) mine = ~kept;
    unsigned long long acc = 0ull;
#pragma unroll
    for (int r = 0; r < 64; ++r) acc |= ((kept >> r) & 1ull) ? wrow[r] : 0ull;
    mine |= acc;
  }
  // kept ranks in rank order -> keep[0 .. count), -1 behind
  const unsigned long long keptw = tid < nb ? ~mine : 0ull;
  scan[tid] = __popcll(keptw);
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const int total = scan[255];
  int pos = scan[tid] - __popcll(keptw);
  unsigned long long k = keptw;
  while (k) {
    const int r = __ffsll((long long)k) - 1;
    k &= k - 1;
    if (pos < a.cap) a.keep[pos] = a.order[tid * 64 + r];
    ++pos;
  }
  const int written = min(total, a.cap);
  for (int i = written + tid; i < a.cap; i += 256) a.keep[i] = -1;
  if (tid == 0) *a.count = written;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------------------------
struct NmsOp {          // what differs between the two operators
  const char* fn;                          // the prefix of every message
  int min_stride; const char* columns;     // of a box row
  int max_n;
  const char* sizer;                       // the exported workspace-size function
  void (*mask)(NmsArgs); void (*reduce)(NmsArgs);
};

// the suppression words: N rows of ceil(N / 64) words; 0 for an N no call accepts
size_t lmv_nms_bytes(int N, int max_n) {
  if (N < 0 || N > max_n) return 0;
  return (size_t)N * (size_t)((N + 63) / 64) * 8;
}

int lmv_nms_run(const NmsOp& op, const float* boxes, int stride, const float* scores, const int64_t* order, const int32_t* groups, int N, float iou_thr, float score_thr,
                int max_num, int phases, void* workspace, size_t workspace_bytes, int64_t* keep, int64_t* count, void* stream) {
  const char* fn = op.fn;
  if (N < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: %d boxes (a negative size)", fn, N);
  if (stride < op.min_stride) LMV_FAIL(LMV_ERR_SHAPE, "%s: boxes: a row stride of %d floats (at least %d: %s)", fn, stride, op.min_stride, op.columns);
  if (N > 0 && !boxes) LMV_FAIL(LMV_ERR_SHAPE, "%s: null boxes", fn);
  if (N > op.max_n) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = %d boxes, at most %d", fn, N, op.max_n);
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
  const size_t need = lmv_nms_bytes(N, op.max_n);
  if (workspace_bytes < need || (need > 0 && !workspace)) LMV_FAIL(LMV_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (%s)", fn, workspace_bytes, need, op.sizer);
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {          // no launch: count = 0, keep = -1 throughout
    if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot clear count", fn);
    if (cap > 0 && hipMemsetAsync(keep, 0xff, (size_t)cap * sizeof(int64_t), st) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot fill keep", fn);
    return LMV_OK;
  }
  NmsArgs a;
  a.boxes = boxes; a.stride = stride; a.scores = scores; a.order = order; a.groups = groups;
  a.N = N; a.nb = (N + 63) / 64; a.iou_thr = iou_thr; a.score_thr = score_thr; a.cap = cap;
  a.mask = reinterpret_cast<unsigned long long*>(workspace); a.keep = keep; a.count = count;
  if (phases & 1) hipLaunchKernelGGL(op.mask, dim3((unsigned)a.nb, (unsigned)a.nb), dim3(256), 0, st, a);
  if (phases & 2) hipLaunchKernelGGL(op.reduce, dim3(1), dim3(256), 0, st, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

}  // namespace
