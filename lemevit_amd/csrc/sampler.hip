// sampler.hip -- the samplers of both heads of the Oriented R-CNN configs (upstream mmdet 2.x RandomSampler / OBBRandomSampler: their sources are not part of the
// reference tree, the rules restate upstream): lmv_random_sample (+ _workspace_bytes) picks, for B images at once, up to `num` boxes per image from what
// lmv_max_iou_assign wrote -- no nonzero, no randperm, no cat of the ground truths, no host round trip -- and lmv_sample_gather builds the R-CNN head's inputs from
// the picks.  include/lemevit_hip.h has the rules and the semantics.
//
//   choice    a class's k chosen are the k smallest 64-bit words (priority << 32) | element: an exact radix select (four 8-bit digits of the priority, then the
//             element order) -- no sort, and no value depends on the order in which an atomic lands (integer counters only): two calls agree bit for bit.
//   launch 1  grid-wide, 1024 elements per workgroup: class byte and priority of every element into the workspace (rows padded to 16 elements, so that launch 2
//             reads them 16 at a time), the histograms of the priority's top byte per class in LDS, flushed with integer atomics into a table a memset node zeroed.
//   launch 2  one workgroup of 1024 threads per image: the quotas from the bin totals; for an oversubscribed class three more digit sweeps over the workspace give
//             the threshold priority t and how many elements equal to t to take; one ordered sweep (16 consecutive elements per thread, block prefix scans of the
//             packed per-class counts) writes inds, mask and the counts.  Every output element is written exactly once.
#include "common.h"
#include "philox.h"
#include "select_frame.h"
#include <math.h>

namespace {

constexpr int SM_CHUNK = 1024;          // elements per workgroup of launch 1
constexpr int SM_T1 = 256;
constexpr int SM_T2 = 1024, SM_WAVES = SM_T2 / LMV_WAVE;
constexpr int SM_VEC = 16;              // consecutive elements per thread of launch 2; the workspace rows are padded to it
constexpr int SM_SPAN = SM_T2 * SM_VEC;
constexpr uint32_t SM_TAG = 0x53414d50u;          // counter word 3 of the priorities ("SAMP")
constexpr int SM_NONE = 0, SM_POS = 1, SM_NEG = 2;          // the class byte; also the mask's values
constexpr int SM_TAKE_NONE = 0, SM_TAKE_ALL = 1, SM_TAKE_SOME = 2;
constexpr size_t SM_HIST_BYTES = 2 * 256 * sizeof(uint32_t);          // per image

static_assert(SM_T1 == 256, "launch 1 clears and flushes one histogram bin per thread");
static_assert(LMV_SAMPLE_MAX_NUM <= 65535 && SM_SPAN <= 65535, "launch 2 scans two 16-bit counts in one word");

__host__ __device__ inline int sm_padded(int M) { return (M + SM_VEC - 1) / SM_VEC * SM_VEC; }

struct SmArgs {
  const int64_t* gt_inds; const int32_t* gt_counts; const uint32_t* priorities; const uint32_t* key;
  int N, Gmax, off, M, Mp;          // off: the ground-truth elements in front of the boxes (add_gt ? Gmax : 0); Mp: the padded row of the workspace
  int num, P; float ub;
  uint32_t* hist; uint32_t* prio; uint8_t* cls;          // the workspace: [B, 2, 256], [B, Mp], [B, Mp]
  int64_t* inds; int32_t* num_pos; int32_t* num_neg; uint8_t* mask;
};

__global__ __launch_bounds__(SM_T1) void sample_classify_kernel(SmArgs a) {
  __shared__ uint32_t h[2][256];
  const int tid = threadIdx.x, b = blockIdx.y;
  h[0][tid] = 0u; h[1][tid] = 0u;
  __syncthreads();
  const int count = a.off ? (a.gt_counts ? min(max(a.gt_counts[b], 0), a.Gmax) : a.Gmax) : 0;
  uint32_t k0 = 0u, k1 = 0u;
  if (!a.priorities) { k0 = a.key[0]; k1 = a.key[1]; }
  const int64_t wrow = (int64_t)b * a.Mp;
#pragma unroll
  for (int i = 0; i < SM_CHUNK / SM_T1; ++i) {
    const int e = blockIdx.x * SM_CHUNK + i * SM_T1 + tid;
    if (e < a.Mp) {
      int c = SM_NONE;
      uint32_t p = 0u;
      if (e < a.off) c = e < count ? SM_POS : SM_NONE;          // ground truth e: a candidate below the count, and then a positive
      else if (e < a.M) {
        const int64_t g = a.gt_inds[(int64_t)b * a.N + (e - a.off)];
        c = g > 0 ? SM_POS : g == 0 ? SM_NEG : SM_NONE;
      }
      if (c != SM_NONE) {
        if (a.priorities) p = a.priorities[(int64_t)b * a.M + e];
        else {
          uint32_t r[4];
          philox4x32_10((uint32_t)e, (uint32_t)b, 0u, SM_TAG, k0, k1, r);
          p = r[0];
        }
        atomicAdd(&h[c - 1][p >> 24], 1u);
      }
      a.prio[wrow + e] = p;
      a.cls[wrow + e] = (uint8_t)c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const uint32_t v = h[c][tid];
    if (v) atomicAdd(&a.hist[((int64_t)b * 2 + c) * 256 + tid], v);
  }
}

// elements e0 .. e0 + 15 of a padded workspace row (e0 % 16 == 0): one 16-byte load of class bytes, four of priorities
__device__ __forceinline__ void sm_load(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ prio, int e0, int* c, uint32_t* p) {
  const uint4 cv = *reinterpret_cast<const uint4*>(cls + e0);
  const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
  for (int j = 0; j < SM_VEC; ++j) c[j] = (int)((cw[j >> 2] >> (8 * (j & 3))) & 0xffu);
#pragma unroll
  for (int q = 0; q < SM_VEC / 4; ++q) {
    const uint4 pv = reinterpret_cast<const uint4*>(prio + e0)[q];
    p[4 * q] = pv.x; p[4 * q + 1] = pv.y; p[4 * q + 2] = pv.z; p[4 * q + 3] = pv.w;
  }
}

__global__ __launch_bounds__(SM_T2) void sample_select_kernel(SmArgs a) {
  __shared__ uint32_t h[2][256];
  __shared__ uint32_t wt[2][2][SM_WAVES];          // [parity of the iteration][scan][wave]
  __shared__ uint32_t s_cnt[2], s_take[2], s_mode[2], s_pref[2], s_rest[2];
  const int tid = threadIdx.x, lane = tid & (LMV_WAVE - 1), wave = tid >> 6, b = blockIdx.x;
  const uint32_t* prio = a.prio + (int64_t)b * a.Mp;
  const uint8_t* cls = a.cls + (int64_t)b * a.Mp;
  if (tid < 512) h[tid >> 8][tid & 255] = a.hist[(int64_t)b * 512 + tid];
  __syncthreads();
  if (wave < 2) {          // the bin totals are the candidates of the class
    uint32_t s = (h[wave][4 * lane] + h[wave][4 * lane + 1]) + (h[wave][4 * lane + 2] + h[wave][4 * lane + 3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, LMV_WAVE);
    if (lane == 0) s_cnt[wave] = s;
  }
  __syncthreads();
  if (tid == 0) {          // the quotas: upstream's arithmetic
    const int c_pos = (int)s_cnt[0], c_neg = (int)s_cnt[1];
    const int n_pos = min(c_pos, a.P);
    int E = a.num - n_pos;
    if (a.ub >= 0.f) {
      const double cap = floor((double)a.ub * (double)max(1, n_pos));
      if (cap < (double)E) E = (int)cap;
    }
    const int n_neg = min(c_neg, E);
    s_take[0] = (uint32_t)n_pos; s_take[1] = (uint32_t)n_neg;
    s_mode[0] = n_pos == 0 ? SM_TAKE_NONE : c_pos <= n_pos ? SM_TAKE_ALL : SM_TAKE_SOME;
    s_mode[1] = n_neg == 0 ? SM_TAKE_NONE : c_neg <= n_neg ? SM_TAKE_ALL : SM_TAKE_SOME;
    s_pref[0] = s_pref[1] = 0u;
    s_rest[0] = (uint32_t)n_pos; s_rest[1] = (uint32_t)n_neg;
  }
  __syncthreads();
  const int mode0 = (int)s_mode[0], mode1 = (int)s_mode[1];
  const bool some = mode0 == SM_TAKE_SOME || mode1 == SM_TAKE_SOME;
  if (some) {          // the threshold of an oversubscribed class, digit by digit; s_rest: how many to take among the elements that share the digits so far
    if (wave < 2 && (int)s_mode[wave] == SM_TAKE_SOME) {
      uint32_t bin = 0u, rest = 0u;
      const uint32_t r = s_rest[wave];
      lmv_select_pick(h[wave], r, lane, &bin, &rest);
      if (rest) { s_pref[wave] = bin << 24; s_rest[wave] = rest; }          // (the finding lane alone: rest >= 1 there, 0 elsewhere)
    }
    for (int shift = 16; shift >= 0; shift -= 8) {
      __syncthreads();
      if (tid < 512) h[tid >> 8][tid & 255] = 0u;
      __syncthreads();
      const uint32_t pf0 = s_pref[0] >> (shift + 8), pf1 = s_pref[1] >> (shift + 8);
      for (int e0 = tid * SM_VEC; e0 < a.Mp; e0 += SM_SPAN) {
        int c[SM_VEC];
        uint32_t p[SM_VEC];
        sm_load(cls, prio, e0, c, p);
#pragma unroll
        for (int j = 0; j < SM_VEC; ++j) {
          const bool hit = (c[j] == SM_POS && mode0 == SM_TAKE_SOME && (p[j] >> (shift + 8)) == pf0) ||
                           (c[j] == SM_NEG && mode1 == SM_TAKE_SOME && (p[j] >> (shift + 8)) == pf1);
          if (hit) atomicAdd(&h[c[j] - 1][(p[j] >> shift) & 0xffu], 1u);
        }
      }
      __syncthreads();
      if (wave < 2 && (int)s_mode[wave] == SM_TAKE_SOME) {
        uint32_t bin = 0u, rest = 0u;
        const uint32_t r = s_rest[wave];
        lmv_select_pick(h[wave], r, lane, &bin, &rest);
        if (rest) { s_pref[wave] |= bin << shift; s_rest[wave] = rest; }
      }
    }
    __syncthreads();
  }
  const uint32_t t0 = s_pref[0], t1 = s_pref[1];
  const int r0 = (int)s_rest[0], r1 = (int)s_rest[1];
  const int n_pos = (int)s_take[0], n_neg = (int)s_take[1];
  int64_t* inds = a.inds + (int64_t)b * a.num;
  uint8_t* mask = a.mask ? a.mask + (int64_t)b * a.M : nullptr;
  int eq0 = 0, eq1 = 0;          // the elements equal to the threshold in front of this sweep position, per class
  int out0 = 0, out1 = 0;        // the chosen ones in front of it
  int parity = 0;
  for (int base = 0; base < a.Mp; base += SM_SPAN, parity ^= 1) {
    const int e0 = base + tid * SM_VEC;
    int c[SM_VEC];
    uint32_t p[SM_VEC];
    if (e0 < a.Mp) sm_load(cls, prio, e0, c, p);
    else {
#pragma unroll
      for (int j = 0; j < SM_VEC; ++j) { c[j] = SM_NONE; p[j] = 0u; }
    }
    int my0 = eq0, my1 = eq1;
    if (some) {
      uint32_t mine = 0u, total;
#pragma unroll
      for (int j = 0; j < SM_VEC; ++j) {
        if (c[j] == SM_POS && mode0 == SM_TAKE_SOME && p[j] == t0) mine += 1u;
        if (c[j] == SM_NEG && mode1 == SM_TAKE_SOME && p[j] == t1) mine += 1u << 16;
      }
      const uint32_t ex = lmv_select_scan<SM_WAVES>(mine, wt[parity][0], lane, wave, &total);
      my0 += (int)(ex & 0xffffu); my1 += (int)(ex >> 16);
      eq0 += (int)(total & 0xffffu); eq1 += (int)(total >> 16);
    }
    uint32_t chosen = 0u, mine = 0u, total;          // bit j: element e0 + j is chosen
#pragma unroll
    for (int j = 0; j < SM_VEC; ++j) {
      bool take = false;
      if (c[j] == SM_POS) {
        if (mode0 == SM_TAKE_ALL) take = true;
        else if (mode0 == SM_TAKE_SOME) {
          if (p[j] < t0) take = true;
          else if (p[j] == t0) { take = my0 < r0; ++my0; }
        }
        if (take) mine += 1u;
      } else if (c[j] == SM_NEG) {
        if (mode1 == SM_TAKE_ALL) take = true;
        else if (mode1 == SM_TAKE_SOME) {
          if (p[j] < t1) take = true;
          else if (p[j] == t1) { take = my1 < r1; ++my1; }
        }
        if (take) mine += 1u << 16;
      }
      chosen |= take ? (1u << j) : 0u;
    }
    const uint32_t ex = lmv_select_scan<SM_WAVES>(mine, wt[parity][1], lane, wave, &total);
    int at0 = out0 + (int)(ex & 0xffffu), at1 = n_pos + out1 + (int)(ex >> 16);
    out0 += (int)(total & 0xffffu); out1 += (int)(total >> 16);
    if (e0 < a.M) {
      uint32_t mw[SM_VEC / 4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < SM_VEC; ++j) {
        if ((chosen >> j) & 1u) {
          int& at = c[j] == SM_POS ? at0 : at1;
          if (at < a.num) inds[at] = (int64_t)(e0 + j);          // (always: n_pos + n_neg <= num)
          ++at;
          mw[j >> 2] |= (uint32_t)c[j] << (8 * (j & 3));
        }
      }
      if (mask) {
        uint8_t* m = mask + e0;
        if (e0 + SM_VEC <= a.M && (((uintptr_t)m) & 15u) == 0) *reinterpret_cast<uint4*>(m) = make_uint4(mw[0], mw[1], mw[2], mw[3]);
        else {
#pragma unroll
          for (int j = 0; j < SM_VEC; ++j)
            if (e0 + j < a.M) m[j] = (uint8_t)((mw[j >> 2] >> (8 * (j & 3))) & 0xffu);
        }
      }
    }
  }
  for (int s = n_pos + n_neg + tid; s < a.num; s += SM_T2) inds[s] = -1;
  if (tid == 0) { a.num_pos[b] = n_pos; a.num_neg[b] = n_neg; }
}

struct GaArgs {
  const int64_t* inds; int num;
  const float* boxes; int box_stride; int64_t box_batch; int N, k;
  const float* gts; int gt_stride; int Gmax, off;
  const int64_t* gt_inds; const int64_t* gt_labels; const int32_t* gt_counts; int64_t bg_label;
  float* rois; int64_t* s_gt_inds; int64_t* s_labels;
};

template <int K>
__global__ __launch_bounds__(256) void sample_gather_kernel(GaArgs a) {
  const int s = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (s >= a.num) return;
  const int64_t o = (int64_t)b * a.num + s;
  const int64_t e = a.inds[o];
  const int count = a.gt_counts ? min(max(a.gt_counts[b], 0), a.Gmax) : a.Gmax;
  float row[1 + K];
  row[0] = -1.f;
#pragma unroll
  for (int i = 0; i < K; ++i) row[1 + i] = 0.f;
  int64_t gi = -1, label = -1;
  const float* src = nullptr;          // (a row that names no candidate reads nothing and is padding)
  if (e >= 0 && e < (int64_t)a.off) {
    if (e < (int64_t)count) { src = a.gts + ((int64_t)b * a.Gmax + e) * a.gt_stride; gi = e + 1; }
  } else if (e >= (int64_t)a.off && e < (int64_t)a.off + a.N) {
    const int64_t n = e - a.off, g = a.gt_inds[(int64_t)b * a.N + n];
    if (g >= 0) { src = a.boxes + b * a.box_batch + n * a.box_stride; gi = g; }
  }
  if (src) {
    row[0] = (float)b;
#pragma unroll
    for (int i = 0; i < K; ++i) row[1 + i] = src[i];
    label = gi == 0 ? a.bg_label : (a.gt_labels && gi <= (int64_t)a.Gmax) ? a.gt_labels[(int64_t)b * a.Gmax + (gi - 1)] : -1;
  }
  float* r = a.rois + o * (1 + K);
#pragma unroll
  for (int i = 0; i < 1 + K; ++i) r[i] = row[i];
  a.s_gt_inds[o] = gi;
  if (a.s_labels) a.s_labels[o] = label;
}

// what both entry points refuse about their sizes; `fn` names the caller in the message
int sm_sizes(const char* fn, int N, int B, int Gmax, int add_gt, int num) {
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH) LMV_FAIL(LMV_ERR_SHAPE, "%s: B = %d images outside 1 .. %d", fn, B, LMV_ASSIGN_MAX_BATCH);
  if (N < 0 || Gmax < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: N = %d boxes, Gmax = %d ground truths (a negative size)", fn, N, Gmax);
  if (add_gt != 0 && add_gt != 1) LMV_FAIL(LMV_ERR_SHAPE, "%s: add_gt = %d is neither 0 nor 1", fn, add_gt);
  if (N > LMV_OBB_MAX_BOXES || Gmax > LMV_OBB_MAX_BOXES || (add_gt ? Gmax : 0) + N > LMV_OBB_MAX_BOXES)
    LMV_FAIL(LMV_ERR_SHAPE, "%s: M = %lld elements (N = %d boxes%s), at most %d", fn, (long long)(add_gt ? Gmax : 0) + N, N, add_gt ? " and Gmax ground truths" : "", LMV_OBB_MAX_BOXES);
  if (num < 1 || num > LMV_SAMPLE_MAX_NUM) LMV_FAIL(LMV_ERR_SHAPE, "%s: num = %d samples per image outside 1 .. %d", fn, num, LMV_SAMPLE_MAX_NUM);
  return LMV_OK;
}

}  // namespace

extern "C" size_t lmv_random_sample_workspace_bytes(int B, int M) {
  if (B < 1 || B > LMV_ASSIGN_MAX_BATCH || M < 0 || M > LMV_OBB_MAX_BOXES) return 0;
  return (size_t)B * (SM_HIST_BYTES + (size_t)sm_padded(M) * 5);
}

extern "C" int lmv_random_sample(const int64_t* gt_inds, int N, int B, const int32_t* gt_counts, int Gmax, int add_gt, int num, int P, float neg_pos_ub,
                                 const uint32_t* priorities, const uint32_t* key, void* workspace, size_t workspace_bytes, int64_t* inds, int32_t* num_pos,
                                 int32_t* num_neg, uint8_t* mask, void* stream) {
  const char* fn = "random_sample";
  if (int rc = sm_sizes(fn, N, B, Gmax, add_gt, num)) return rc;
  if (P < 0 || P > num) LMV_FAIL(LMV_ERR_SHAPE, "%s: P = %d positives expected outside 0 .. num = %d", fn, P, num);
  if (neg_pos_ub != neg_pos_ub) LMV_FAIL(LMV_ERR_SHAPE, "%s: neg_pos_ub is NaN (negative: no bound)", fn);
  if (!priorities && !key) LMV_FAIL(LMV_ERR_SHAPE, "%s: neither priorities nor a key (two 32-bit words in device memory)", fn);
  const int M = (add_gt ? Gmax : 0) + N;
  if (N > 0 && !gt_inds) LMV_FAIL(LMV_ERR_SHAPE, "%s: null gt_inds", fn);
  if (!inds || !num_pos || !num_neg) LMV_FAIL(LMV_ERR_SHAPE, "%s: null inds / num_pos / num_neg", fn);
  if ((((uintptr_t)gt_inds) & 7u) || (((uintptr_t)inds) & 7u) || (((uintptr_t)gt_counts) & 3u) || (((uintptr_t)priorities) & 3u) || (((uintptr_t)key) & 3u) ||
      (((uintptr_t)num_pos) & 3u) || (((uintptr_t)num_neg) & 3u) || (((uintptr_t)workspace) & 15u))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer (the workspace: 16 bytes)", fn);
  const size_t need = lmv_random_sample_workspace_bytes(B, M);
  if (workspace_bytes < need || !workspace) LMV_FAIL(LMV_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (lmv_random_sample_workspace_bytes)", fn, workspace_bytes, need);
  if (M == 0) return LMV_OK;
  hipStream_t st = (hipStream_t)stream;
  SmArgs a;
  a.gt_inds = gt_inds; a.gt_counts = gt_counts; a.priorities = priorities; a.key = key;
  a.N = N; a.Gmax = Gmax; a.off = add_gt ? Gmax : 0; a.M = M; a.Mp = sm_padded(M);
  a.num = num; a.P = P; a.ub = neg_pos_ub;
  a.hist = reinterpret_cast<uint32_t*>(workspace);
  a.prio = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(workspace) + (size_t)B * SM_HIST_BYTES);
  a.cls = reinterpret_cast<uint8_t*>(a.prio + (size_t)B * a.Mp);
  a.inds = inds; a.num_pos = num_pos; a.num_neg = num_neg; a.mask = mask;
  if (hipMemsetAsync(workspace, 0, (size_t)B * SM_HIST_BYTES, st) != hipSuccess) LMV_FAIL(LMV_ERR_LAUNCH, "%s: cannot clear the histograms", fn);
  hipLaunchKernelGGL(sample_classify_kernel, dim3((unsigned)((a.Mp + SM_CHUNK - 1) / SM_CHUNK), (unsigned)B), dim3(SM_T1), 0, st, a);
  LMV_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(sample_select_kernel, dim3((unsigned)B), dim3(SM_T2), 0, st, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}

extern "C" int lmv_sample_gather(const int64_t* inds, int num, const float* boxes, int box_stride, int64_t box_batch_stride, int N, int k, const float* gts,
                                 int gt_stride, int B, int Gmax, const int64_t* gt_inds, const int64_t* gt_labels, const int32_t* gt_counts, int add_gt,
                                 int64_t bg_label, float* rois, int64_t* s_gt_inds, int64_t* s_labels, void* stream) {
  const char* fn = "sample_gather";
  if (k != 4 && k != 5) LMV_FAIL(LMV_ERR_SHAPE, "%s: k = %d box columns (4: x1, y1, x2, y2; 5: cx, cy, w, h, theta)", fn, k);
  if (int rc = sm_sizes(fn, N, B, Gmax, add_gt, num)) return rc;
  if (box_stride < k || gt_stride < k) LMV_FAIL(LMV_ERR_SHAPE, "%s: row strides of %d (boxes) and %d (ground truths) floats, at least %d", fn, box_stride, gt_stride, k);
  if (box_batch_stride < 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: a negative batch stride of the boxes (0: one set shared by all images)", fn);
  if (N > 0 && (!boxes || !gt_inds)) LMV_FAIL(LMV_ERR_SHAPE, "%s: null boxes / gt_inds", fn);
  if (add_gt && Gmax > 0 && !gts) LMV_FAIL(LMV_ERR_SHAPE, "%s: null ground truths with add_gt", fn);
  if (!inds || !rois || !s_gt_inds) LMV_FAIL(LMV_ERR_SHAPE, "%s: null inds / rois / s_gt_inds", fn);
  if (s_labels && !gt_labels && Gmax > 0) LMV_FAIL(LMV_ERR_SHAPE, "%s: s_labels without gt_labels (only with Gmax = 0)", fn);
  if ((((uintptr_t)boxes) & 3u) || (((uintptr_t)gts) & 3u) || (((uintptr_t)gt_counts) & 3u) || (((uintptr_t)rois) & 3u) || (((uintptr_t)inds) & 7u) ||
      (((uintptr_t)gt_inds) & 7u) || (((uintptr_t)gt_labels) & 7u) || (((uintptr_t)s_gt_inds) & 7u) || (((uintptr_t)s_labels) & 7u))
    LMV_FAIL(LMV_ERR_SHAPE, "%s: misaligned buffer", fn);
  GaArgs a;
  a.inds = inds; a.num = num; a.boxes = boxes; a.box_stride = box_stride; a.box_batch = box_batch_stride; a.N = N; a.k = k;
  a.gts = gts; a.gt_stride = gt_stride; a.Gmax = Gmax; a.off = add_gt ? Gmax : 0;
  a.gt_inds = gt_inds; a.gt_labels = gt_labels; a.gt_counts = gt_counts; a.bg_label = bg_label;
  a.rois = rois; a.s_gt_inds = s_gt_inds; a.s_labels = s_labels;
  const dim3 grid((unsigned)((num + 255) / 256), (unsigned)B);
  if (k == 4) hipLaunchKernelGGL(sample_gather_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(sample_gather_kernel<5>, grid, dim3(256), 0, (hipStream_t)stream, a);
  LMV_CHECK_LAUNCH(fn);
  return LMV_OK;
}
